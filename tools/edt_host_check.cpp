// Host check of the kernel bodies of tobac_flow_amd/csrc/edt_kernels.h: the same text compiled for the CPU, run lane
// after lane on exactly-sized heap buffers against brute force, meant for AddressSanitizer + UBSan:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/edt_host_check.cpp -o edt_host_check
//   ./edt_host_check
//
// Lanes run one after the other (all of a workgroup's loads of sq[] before its scans, as the barrier orders them), so
// the atomics are plain read-modify-writes.  Checked: every load and store inside its buffer, the squared distances
// against the brute-force minimum over all features of the frame, the reported feature against the documented rule
// (smallest |x' - x|, then the left one, then the upper one), the cylinder minimum with its earliest-frame rule, the
// envelope along t (its pruned scan against the plain minimum over all frames, with the nearer-then-earlier frame on equal
// keys, and the distance in SciPy's summation order) and the per-label minimum at every alignment and tail form.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <type_traits>
#include <vector>

#define __host__
#define __device__
#define __forceinline__ inline
#define __restrict__
struct int4 { int32_t x, y, z, w; };
struct float4 { float x, y, z, w; };
struct double2 { double x, y; };
struct uchar4 { uint8_t x, y, z, w; };
template <typename T> static T atomicAdd(T *p, T v) { T o = *p; *p = o + v; return o; }
static unsigned long long atomicMin(unsigned long long *p, unsigned long long v) { unsigned long long o = *p; *p = std::min(o, v); return o; }
static unsigned long long atomicMax(unsigned long long *p, unsigned long long v) { unsigned long long o = *p; *p = std::max(o, v); return o; }

#include "../tobac_flow_amd/csrc/edt_kernels.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures < 20) printf("FAILED %s (line %d)\n", #c, __LINE__); failures++; } } while (0)

template <typename E> struct Buf {                                 // exactly-sized copy, `shift` elements past a 16-byte boundary
    std::vector<E> store; E *p;
    Buf(const std::vector<E> &v, int shift) : store(v.size() + shift), p(nullptr) { if (!v.empty()) std::memcpy(store.data() + shift, v.data(), v.size() * sizeof(E)); p = store.data() + shift; }
};

// the volumes of tests/validation_cases.py in spirit: labelled boxes with two empty frames; features in the corners and
// along the borders of a row longer than a workgroup; one feature in a corner and a frame of features; degenerate axes
static std::vector<int32_t> volume(int kind, int64_t T, int64_t H, int64_t W)
{
    std::vector<int32_t> v((size_t)(T * H * W), 0);
    auto at = [&](int64_t t, int64_t y, int64_t x) -> int32_t & { return v[(size_t)((t * H + y) * W + x)]; };
    std::mt19937 rng(7 + kind);
    if (kind == 0) {
        for (int64_t t = 0; t < T; t++) {
            if (t == 2 || t == 5) continue;
            for (int b = 0; b < 4; b++) {
                const int64_t y0 = rng() % H, x0 = rng() % W, h = 1 + rng() % 6, w = 1 + rng() % 9;
                for (int64_t y = y0; y < std::min(H, y0 + h); y++) for (int64_t x = x0; x < std::min(W, x0 + w); x++) at(t, y, x) = b + 1;
            }
        }
    } else if (kind == 1) {
        for (int64_t t = 0; t < T; t++) {
            at(t, 0, 0) = 1; at(t, 0, W - 1) = 2; at(t, H - 1, 0) = 3; at(t, H - 1, W - 1) = 4;
            if (t & 1) for (int64_t x = 0; x < W; x += 7) at(t, 0, x) = 5;
            if (t & 2) for (int64_t y = 0; y < H; y += 5) at(t, y, W - 1) = 6;
        }
    } else if (kind == 2) {
        at(0, H - 1, W - 1) = 9;
        if (T > 1) for (int64_t i = 0; i < H * W; i++) v[(size_t)(H * W + i)] = -1;
    } else {
        for (int64_t i = 0; i < T * H * W; i++) v[(size_t)i] = rng() % 23 == 0;
    }
    return v;
}

// brute force, once per volume: the squared distance and the feature the documented rule picks
struct Truth {
    std::vector<int32_t> vi, d2, nearest;
    Truth(int kind, int64_t T, int64_t H, int64_t W) : vi(volume(kind, T, H, W)), d2(vi.size()), nearest(vi.size())
    {
        const int64_t hw = H * W;
        for (int64_t t = 0; t < T; t++) for (int64_t y = 0; y < H; y++) for (int64_t x = 0; x < W; x++) {
            int64_t best = EDT_NONE, bi = -1;
            auto better = [&](int64_t d, int64_t yy, int64_t xx) {
                if (d != best) return d < best;
                const int64_t by = bi / W, bx = bi % W, a = std::llabs(xx - x), c = std::llabs(bx - x);
                if (a != c) return a < c;
                if (xx != bx) return xx < bx;
                return yy < by;
            };
            for (int64_t yy = 0; yy < H; yy++) for (int64_t xx = 0; xx < W; xx++) {
                if (!vi[(size_t)(t * hw + yy * W + xx)]) continue;
                const int64_t d = (yy - y) * (yy - y) + (xx - x) * (xx - x);
                if (bi < 0 || better(d, yy, xx)) { best = d; bi = yy * W + xx; }
            }
            d2[(size_t)(t * hw + y * W + x)] = (int32_t)best;
            nearest[(size_t)(t * hw + y * W + x)] = (int32_t)bi;
        }
    }
};

template <typename E>
static void edt_case(const Truth &truth, int64_t T, int64_t H, int64_t W, bool want_nearest, bool sq_in_workspace, int64_t tm)
{
    const std::vector<int32_t> &vi = truth.vi;
    std::vector<E> ve(vi.size());
    for (size_t i = 0; i < vi.size(); i++) ve[i] = (E)vi[i];
    if constexpr (std::is_floating_point<E>::value) for (size_t i = 0; i < vi.size(); i += 97) if (vi[i]) ve[i] = (E)NAN;   // NaN is a feature
    const int64_t hw = H * W, n = T * hw;
    std::vector<int32_t> fy((size_t)n), d2((size_t)n), nearest(want_nearest ? (size_t)n : 0);
    std::vector<uint32_t> sq((size_t)(sq_in_workspace ? n : W));
    const int64_t x_blocks = (W + 255) / 256;
    for (int64_t b = 0; b < T * x_blocks; b++) for (int tid = 0; tid < 256; tid++)
        edt_cols_body<E>((b % x_blocks) * 256 + tid, b / x_blocks, ve.data(), H, W, fy.data());
    for (int64_t row = 0; row < T * H; row++) {
        uint32_t *s = sq.data() + (sq_in_workspace ? row * W : 0);
        bool any = false;                                          // the workgroup's __syncthreads_or
        for (int tid = 0; tid < 256; tid++) any |= edt_row_load_body(tid, 256, fy.data() + row * W, (int32_t)(row % H), W, s);
        int32_t *near_row = want_nearest ? nearest.data() + row * W : nullptr;
        for (int tid = 0; tid < 256; tid++) {
            if (any) edt_row_scan_body(tid, 256, s, fy.data() + row * W, W, d2.data() + row * W, near_row);
            else edt_row_empty_body(tid, 256, W, d2.data() + row * W, near_row);
        }
    }
    CHECK(d2 == truth.d2);
    if (want_nearest) CHECK(nearest == truth.nearest);
    std::vector<double> dist((size_t)n);
    std::vector<int64_t> src(want_nearest ? (size_t)n : 0);
    for (int64_t i = 0; i < (n + 255) / 256 * 256; i++)
        edt_cyl_body(i, T, hw, std::min(tm, T), d2.data(), want_nearest ? nearest.data() : nullptr, dist.data(), want_nearest ? src.data() : nullptr);
    for (int64_t t = 0; t < T; t++) for (int64_t p = 0; p < hw; p++) {
        int64_t best = EDT_NONE, bt = -1;
        for (int64_t k = std::max<int64_t>(t - tm, 0); k <= std::min(t + tm, T - 1); k++)
            if (d2[(size_t)(k * hw + p)] < best) { best = d2[(size_t)(k * hw + p)]; bt = k; }
        const size_t i = (size_t)(t * hw + p);
        CHECK(bt < 0 ? std::isinf(dist[i]) && dist[i] > 0 : dist[i] == std::sqrt((double)best));
        if (want_nearest) CHECK(src[i] == (bt < 0 ? -1 : bt * hw + nearest[(size_t)(bt * hw + p)]));
    }
    // the envelope along t against the plain rule: over ALL frames the smallest key, then the nearer frame, then the earlier
    if (tm) return;                                                // once per volume and element type
    for (double s : {10.0 / 3.0, 1.0, 3.0, 0.3, 1e9, 1e200}) {
        std::fill(dist.begin(), dist.end(), -1.0);
        std::fill(src.begin(), src.end(), (int64_t)-7);
        for (int64_t p = 0; p < (hw + 255) / 256 * 256; p++)
            edt_env_body(p, T, hw, (int32_t)W, s, d2.data(), want_nearest ? nearest.data() : nullptr, dist.data(), want_nearest ? src.data() : nullptr);
        for (int64_t t = 0; t < T; t++) for (int64_t p = 0; p < hw; p++) {
            double best = INFINITY; int64_t bk = -1;
            for (int64_t k = 0; k < T; k++) {
                const int32_t v = d2[(size_t)(k * hw + p)];
                if (v == EDT_NONE) continue;
                const double a = (double)(k - t) * s, key = a * a + (double)v;
                const bool nearer = std::llabs(k - t) < std::llabs(bk - t) || (std::llabs(k - t) == std::llabs(bk - t) && k < bk);
                if (bk < 0 || key < best || (key == best && nearer)) { best = key; bk = k; }
            }
            const size_t i = (size_t)(t * hw + p);
            if (bk < 0) { CHECK(std::isinf(dist[i]) && dist[i] > 0); if (want_nearest) CHECK(src[i] == -1); continue; }
            if (!want_nearest) { CHECK(dist[i] == std::sqrt(best)); continue; }
            const int64_t n = nearest[(size_t)(bk * hw + p)];
            const double a = (double)(bk - t) * s, dy = (double)(n / W - p / W), dx = (double)(n % W - p % W);
            CHECK(src[i] == bk * hw + n);
            CHECK(dist[i] == std::sqrt((a * a + dy * dy) + dx * dx));
        }
    }
}

template <typename F>
static void nanmin_case(int64_t n, int shift, unsigned seed)
{
    const int64_t n_labels = 9;
    std::mt19937 rng(seed);
    std::vector<int32_t> lab((size_t)n);
    std::vector<F> x((size_t)n);
    constexpr bool floating = std::is_floating_point<F>::value;
    for (int64_t i = 0; i < n; i++) {
        lab[(size_t)i] = ((i / 37) % 3 == 0) ? 0 : (int32_t)((i / 53) % 12) - 1;      // runs; ids -1 .. 10: some beyond n_labels, 9 rare
        const int r = rng() % 50;
        x[(size_t)i] = floating ? (F)((int)(rng() % 64) - 20) / (F)8 : (F)(rng() % 2);
        if constexpr (floating) {
            if (r == 0) x[(size_t)i] = (F)NAN; else if (r == 1) x[(size_t)i] = (F)INFINITY; else if (r == 2) x[(size_t)i] = (F)-0.0;
            if (lab[(size_t)i] == 4) x[(size_t)i] = (F)NAN;                            // a label whose values are all NaN
            if (lab[(size_t)i] == 5) x[(size_t)i] = (F)INFINITY;                       // ... and one lying over inf
        }
        if (lab[(size_t)i] == 7) lab[(size_t)i] = 0;                                    // ... and one that is absent
    }
    Buf<int32_t> L(lab, shift ? 1 : 0); Buf<F> X(x, shift ? 1 : 0);
    const bool vec = lr_aligned16(L.p) && lr_aligned16(X.p);
    std::vector<unsigned long long> acc((size_t)n_labels * LM_REC);
    const std::vector<int64_t> ids = {3, 7, 1, 12, 4, 5, 9, 2, 0, 6, 8};
    std::vector<double> mn(ids.size());
    std::vector<int64_t> cnt(ids.size());
    for (int64_t l = 0; l < 256; l++) lm_init_body(l, n_labels, acc.data());
    for (int64_t b = 0; b < (n + LR_BLOCK - 1) / LR_BLOCK; b++) for (int t = 0; t < 256; t++) lm_pass_body<F>(b, t, L.p, X.p, n, vec, n_labels, acc.data());
    for (int64_t k = 0; k < 256; k++) lm_finish_body(k, (int64_t)ids.size(), ids.data(), n_labels, acc.data(), mn.data(), cnt.data());
    for (size_t k = 0; k < ids.size(); k++) {
        double want = NAN; int64_t all = 0, good = 0;
        for (int64_t i = 0; i < n; i++) {
            if (lab[(size_t)i] != ids[k] || ids[k] < 1 || ids[k] > n_labels) continue;
            all++;
            const double v = (double)x[(size_t)i];
            if (v != v) continue;
            good++;
            if (std::isnan(want) || v < want) want = v;
        }
        CHECK(cnt[k] == (all ? good : -1));
        CHECK(good ? mn[k] == want : std::isnan(mn[k]));
    }
}

int main()
{
    struct { int kind; int64_t T, H, W; } shapes[] = {{0, 6, 37, 70}, {1, 4, 33, 300}, {2, 3, 70, 37}, {3, 2, 1, 130}, {3, 2, 65, 1}, {3, 1, 1, 1}, {1, 2, 3, 520}};
    for (auto &s : shapes) {
        const Truth truth(s.kind, s.T, s.H, s.W);
        for (int nearest = 0; nearest < 2; nearest++)
            for (int64_t tm : {(int64_t)0, (int64_t)2, s.T + 3}) {
                edt_case<int32_t>(truth, s.T, s.H, s.W, nearest, false, tm);
                if (tm) continue;
                edt_case<uint8_t>(truth, s.T, s.H, s.W, nearest, true, tm);
                edt_case<float>(truth, s.T, s.H, s.W, nearest, false, tm);
                edt_case<double>(truth, s.T, s.H, s.W, nearest, true, tm);
            }
    }
    unsigned seed = 1;
    for (int64_t n : {(int64_t)5 * 33 * 67, (int64_t)4099, (int64_t)1, (int64_t)4096, (int64_t)21, (int64_t)2 * 8192 + 5})
        for (int shift = 0; shift < 2; shift++) {
            nanmin_case<float>(n, shift, seed++);
            nanmin_case<double>(n, shift, seed++);
            nanmin_case<uint8_t>(n, shift, seed++);
        }
    // the largest frame the entry point admits: the arithmetic of the scan stays inside its types
    const int64_t side = 32768;
    CHECK((side - 1) * (side - 1) * 2 < (1ll << 31) && (uint64_t)(side - 1) * (side - 1) + (uint32_t)EDT_NONE < (1ull << 32));
    CHECK(lr_key(INFINITY) < LM_ALLNAN && LM_ALLNAN < LR_NONE);
    printf(failures ? "%d FAILURES\n" : "edt host check: all equal (%d failures)\n", failures);
    return failures != 0;
}
