// Host check of the kernel bodies of tobac_flow_amd/csrc/wstats_kernels.h and of the raveled walker of label_runs.h under
// them: the same text compiled for the CPU, run lane after lane on exactly-sized heap buffers against plain loops, meant
// for AddressSanitizer + UBSan:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/wstats_host_check.cpp -o wstats_host_check
//   ./wstats_host_check
//
// Lanes run one after the other, so the atomics are plain read-modify-writes; what is checked is indexing (every load and
// store inside its buffer, at every alignment / tail / plane-straddle form) and the arithmetic of the three stages.  The
// last part feeds raveled indices beyond 2^32 through the index arithmetic alone (no buffer of that size exists here).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
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

#include "../tobac_flow_amd/csrc/wstats_kernels.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s (line %d)\n", #c, __LINE__); failures++; } } while (0)

static bool same(double a, double b, double rtol)
{
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    if (std::isinf(a) || std::isinf(b)) return a == b;
    return std::fabs(a - b) <= rtol * std::fabs(b);
}

// exactly-sized copy whose start is `shift` elements past a 16-byte boundary (shift != 0: the element-load form)
template <typename E> struct Buf {
    std::vector<E> store; E *p;
    Buf(const std::vector<E> &v, int shift) : store(v.size() + shift), p(nullptr) { if (!v.empty()) std::memcpy(store.data() + shift, v.data(), v.size() * sizeof(E)); p = store.data() + shift; }
};

template <typename F>
static void stats_case(int64_t T, int64_t hw, bool plane, bool with_e, int shift, unsigned seed)
{
    const int64_t n = T * hw, n_labels = 9;
    std::mt19937 rng(seed);
    std::vector<int32_t> lab(n);
    std::vector<F> x(n), e(n), w(plane ? hw : n);
    for (int64_t i = 0; i < n; i++) {
        const int r = rng() % 100;
        lab[i] = ((i / 37) % 3 == 0) ? 0 : (int32_t)((i / 53) % 12) - 1;      // runs; ids -1 .. 10: some beyond n_labels
        x[i] = (F)(200 + (int)(rng() % 64)) / (F)8;                               // ties on purpose
        if (r == 0) x[i] = NAN; else if (r == 1) x[i] = INFINITY; else if (r == 2) x[i] = -INFINITY; else if (r == 3) x[i] = (F)-0.0;
        e[i] = (F)(1 + rng() % 9) / (F)16;
    }
    for (auto &v : w) v = (rng() % 5 == 0) ? (F)0 : (F)(1 + rng() % 7) / (F)4;
    for (int64_t i = 0; i < n; i++) if (lab[i] == 4) { w[plane ? i % hw : i] = NAN; break; }   // one label poisoned
    Buf<int32_t> L(lab, shift ? 1 : 0); Buf<F> X(x, shift ? 1 : 0), E(e, shift ? 1 : 0), W(w, shift ? 1 : 0);
    const F *ep = with_e ? E.p : nullptr;
    const bool vec = lr_aligned16(L.p) && lr_aligned16(X.p) && (!ep || lr_aligned16(ep));
    const bool vec_w = lr_aligned16(W.p) && (!plane || hw % LR_VEC == 0);
    std::vector<double> acc((size_t)n_labels * WS_REC), out((size_t)n_labels * WS_OUT);
    const int64_t blocks = (n + LR_BLOCK - 1) / LR_BLOCK;
    for (int64_t l = 0; l < (n_labels + 255) / 256 * 256; l++) ws_init_body(l, n_labels, acc.data());
    for (int64_t b = 0; b < blocks; b++) for (int t = 0; t < 256; t++) ws_pass1_body<F>(b, t, L.p, X.p, ep, W.p, n, hw, plane, vec, vec_w, n_labels, acc.data());
    for (int64_t b = 0; b < blocks; b++) for (int t = 0; t < 256; t++) ws_pass2_body<F>(b, t, L.p, X.p, W.p, n, hw, plane, vec, vec_w, n_labels, acc.data());
    for (int64_t l = 0; l < (n_labels + 255) / 256 * 256; l++) ws_finish_body<F>(l, n_labels, acc.data(), X.p, ep, n, out.data());
    for (int64_t id = 1; id <= n_labels; id++) {
        double cnt = 0, sw = 0, sww = 0, swx = 0, swe = 0, mn = INFINITY, mx = -INFINITY; int64_t imin = -1, imax = -1;
        for (int64_t i = 0; i < n; i++) {
            if (lab[i] != id || !std::isfinite((double)x[i])) continue;
            const double wd = w[plane ? i % hw : i], xd = x[i];
            cnt++; sw += wd; sww += wd * wd; swx += wd * xd; swe += wd * wd * ((double)e[i] * (double)e[i]);
            if (xd < mn) { mn = xd; imin = i; }
            if (xd > mx) { mx = xd; imax = i; }
        }
        double want[WS_OUT]; for (double &v : want) v = NAN;
        want[0] = cnt; want[1] = sw;
        if (cnt > 0 && sw > 0) {
            const double mean = swx / sw; double sv = 0;
            for (int64_t i = 0; i < n; i++) if (lab[i] == id && std::isfinite((double)x[i])) sv += (double)w[plane ? i % hw : i] * (((double)x[i] - mean) * ((double)x[i] - mean));
            const double c = 1 - sww / (sw * sw), sd = c >= 0 ? std::sqrt(sv / sw / c) : NAN;
            want[2] = mean; want[3] = sd; want[4] = mn; want[5] = mx;
            if (with_e) { const double un = std::sqrt(swe) / sw; want[6] = un; want[7] = std::sqrt(sd / std::sqrt(cnt) * (sd / std::sqrt(cnt)) + un * un); want[8] = e[imin]; want[9] = e[imax]; }
        }
        for (int k = 0; k < WS_OUT; k++) {
            const bool exact = k == 0 || k == 4 || k == 5 || k == 8 || k == 9;
            if (!same(out[(id - 1) * WS_OUT + k], want[k], exact ? 0 : 1e-12)) {
                printf("stats T=%lld hw=%lld plane=%d e=%d shift=%d id=%lld slot %d: %.17g != %.17g\n", (long long)T, (long long)hw, plane, with_e, shift, (long long)id, k, out[(id - 1) * WS_OUT + k], want[k]);
                failures++;
            }
        }
    }
}

static void proportions_case(int64_t T, int64_t hw, bool plane, int shift, unsigned seed)
{
    const int64_t n = T * hw, n_labels = 7;
    WpFlags fl; fl.k = 3; std::memset(fl.v, 0, sizeof fl.v); fl.v[0] = 2; fl.v[1] = -1; fl.v[2] = 40;     // 40 never occurs
    std::mt19937 rng(seed);
    std::vector<int32_t> lab(n), flag(n); std::vector<float> w(plane ? hw : n);
    for (int64_t i = 0; i < n; i++) { lab[i] = ((i / 29) % 4 == 0) ? 0 : (int32_t)((i / 61) % 10) - 1; flag[i] = (int32_t)((i / 3) % 4) - 1; }
    for (auto &v : w) { const int r = rng() % 20; v = r == 0 ? NAN : r == 1 ? 0.f : (float)(1 + rng() % 7) / 4.f; }
    for (int64_t i = 0; i < n; i++) if (lab[i] == 3) w[plane ? i % hw : i] = 0.f;                           // a label without weight
    Buf<int32_t> L(lab, shift ? 1 : 0), G(flag, shift ? 1 : 0); Buf<float> W(w, shift ? 1 : 0);
    const bool vec = lr_aligned16(L.p) && lr_aligned16(G.p), vec_w = lr_aligned16(W.p) && (!plane || hw % LR_VEC == 0);
    std::vector<double> acc((size_t)n_labels * (1 + fl.k), 0.0), out((size_t)n_labels * fl.k);
    for (int64_t b = 0; b < (n + LR_BLOCK - 1) / LR_BLOCK; b++) for (int t = 0; t < 256; t++) wp_pass_body(b, t, L.p, G.p, W.p, n, hw, plane, vec, vec_w, n_labels, fl, acc.data());
    for (int64_t l = 0; l < 256; l++) wp_finish_body(l, n_labels, fl.k, acc.data(), out.data());
    for (int64_t id = 1; id <= n_labels; id++) {
        double tot = 0, part[3] = {0, 0, 0};
        for (int64_t i = 0; i < n; i++) {
            const float wf = w[plane ? i % hw : i];
            if (lab[i] != id || std::isnan(wf)) continue;
            tot += wf;
            for (int k = 0; k < 3; k++) if (flag[i] == fl.v[k]) part[k] += wf;
        }
        for (int k = 0; k < 3; k++) CHECK(same(out[(id - 1) * 3 + k], tot > 0 ? part[k] / tot : NAN, 1e-12));
    }
}

int main()
{
    // shapes: a tail that is no multiple of 4 or 16, several workgroups, a plane whose size is no multiple of 4 (the four
    // voxels of a lane straddle its end), one voxel, exactly one workgroup
    const int64_t shapes[][2] = {{5, 33 * 67}, {6, 40 * 50}, {3, 4099}, {1, 1}, {1, 4096}, {7, 3}, {2, 8192 + 5}};
    unsigned seed = 1;
    for (auto &s : shapes)
        for (int plane = 0; plane < 2; plane++)
            for (int with_e = 0; with_e < 2; with_e++)
                for (int shift = 0; shift < 2; shift++) {
                    stats_case<float>(s[0], s[1], plane, with_e, shift, seed++);
                    stats_case<double>(s[0], s[1], plane, with_e, shift, seed++);
                    if (with_e) proportions_case(s[0], s[1], plane, shift, seed++);
                }
    // indices beyond 2^32 through the index arithmetic only: 160 x 5424^2 = 4.7e9 voxels (144 frames, one day of full-disk
    // images, are 4.24e9: beyond int32, just short of 2^32)
    const int64_t hw = 5424ll * 5424, n = 160 * hw, blocks = (n + LR_BLOCK - 1) / LR_BLOCK;
    CHECK(n > (1ll << 32) && blocks <= 0x7fffffffll);
    CHECK(lr_first_voxel(0, 0, 0) == 0 && lr_first_voxel(0, 63, 0) == 252 && lr_first_voxel(0, 0, 1) == 256 && lr_first_voxel(0, 64, 0) == 1024);
    CHECK(lr_first_voxel(blocks - 1, 255, LR_ITERS - 1) == (blocks - 1) * 4096 + 4092);
    CHECK(lr_first_voxel(blocks - 1, 0, 0) < n && lr_first_voxel(blocks, 0, 0) >= n);
    {   // every voxel of a range around 2^32 and around the end of the volume is covered exactly once
        for (int64_t b : {(int64_t)((1ll << 32) / LR_BLOCK - 1), (int64_t)((1ll << 32) / LR_BLOCK), blocks - 1}) {
            std::vector<int> hit(LR_BLOCK, 0);
            for (int t = 0; t < 256; t++) for (int k = 0; k < LR_ITERS; k++) {
                const int64_t i = lr_first_voxel(b, t, k);
                CHECK(i % LR_VEC == 0 && i >= b * LR_BLOCK && i + LR_VEC <= (b + 1) * LR_BLOCK);
                for (int j = 0; j < LR_VEC; j++) hit[i + j - b * LR_BLOCK]++;
                CHECK(i % hw == (int64_t)((unsigned long long)i % (unsigned long long)hw));
            }
            CHECK(std::all_of(hit.begin(), hit.end(), [](int h) { return h == 1; }));
        }
        unsigned long long slot = LR_NONE;                          // the index minimum is a 64-bit one
        atomicMin(&slot, (unsigned long long)(n - 1)); atomicMin(&slot, (1ull << 32) + 5); atomicMin(&slot, (1ull << 33));
        CHECK(slot == (1ull << 32) + 5);
    }
    // keys: order-preserving over finite doubles, one key for both zeros
    const double vals[] = {-1e300, -2.5, -1e-310, -0.0, 0.0, 1e-310, 1.0, 3.5, 1e300};
    for (size_t a = 0; a + 1 < sizeof vals / sizeof *vals; a++)
        CHECK(vals[a] == vals[a + 1] ? lr_key(vals[a]) == lr_key(vals[a + 1]) : lr_key(vals[a]) < lr_key(vals[a + 1]));
    CHECK(lr_key(-1e300) > 0 && lr_key(1e300) < LR_NONE);
    printf(failures ? "%d FAILURES\n" : "wstats host check: all equal (%d failures)\n", failures);
    return failures != 0;
}
