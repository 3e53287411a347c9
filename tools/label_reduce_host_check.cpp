// Host check of the kernel bodies of tobac_flow_amd/csrc/label_reduce_kernels.h (tf_label_reduce, tf_label_order) and of
// the span form of the raveled walker of label_runs.h under them: the same text compiled for the CPU, run lane after lane
// on exactly-sized heap buffers against plain loops, meant for AddressSanitizer + UBSan:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/label_reduce_host_check.cpp -o label_reduce_host_check
//   ./label_reduce_host_check
//
// Lanes run one after the other, so the atomics are plain read-modify-writes; what is checked is indexing (every load and
// store inside its buffer, at every alignment / tail / plane-straddle / per-frame form, for spans that start below 1) and
// the arithmetic of the passes.  The last part feeds raveled indices beyond 2^32 through the index arithmetic alone (no
// buffer of that size exists here).
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
template <typename T> static T atomicAdd(T *p, T v) { T o = *p; *p = o + v; return o; }
static unsigned long long atomicMin(unsigned long long *p, unsigned long long v) { unsigned long long o = *p; *p = std::min(o, v); return o; }
static unsigned long long atomicMax(unsigned long long *p, unsigned long long v) { unsigned long long o = *p; *p = std::max(o, v); return o; }

#include "../tobac_flow_amd/csrc/label_reduce_kernels.h"

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

template <typename E> static E draw(std::mt19937 &rng)
{
    const int r = rng() % 64;
    if (std::is_floating_point<E>::value) {
        if (r == 0) return (E)NAN;
        if (r == 1) return (E)INFINITY;
        if (r == 2) return (E)-INFINITY;
        if (r == 3) return (E)-0.0;
        return (E)((int)(rng() % 129) - 64) / (E)8;                    // ties, zeros and both signs
    }
    if (std::is_same<E, uint8_t>::value) return (E)(rng() % 3);
    if (r == 0) return (E)INT32_MIN;
    if (r == 1) return (E)INT32_MAX;
    return (E)((int)(rng() % 9) - 4);
}

// the field value of voxel i in a layout
template <typename E> static E at(const std::vector<E> &f, int64_t i, int64_t hw, int layout)
{
    return f[layout == LRD_VOLUME ? i : layout == LRD_PLANE ? i % hw : i / hw];
}

template <typename E>
static void reduce_case(int64_t T, int64_t hw, int layout, int shift, int64_t lo, int64_t hi, unsigned seed)
{
    typedef typename LrdSum<E>::type S;
    typedef typename LroKey<E>::type K;
    const int64_t n = T * hw, span = hi - lo + 1;
    const int32_t none = (int32_t)(lo - 1);
    std::mt19937 rng(seed);
    std::vector<int32_t> lab(n);
    std::vector<E> f(layout == LRD_VOLUME ? n : layout == LRD_PLANE ? hw : T);
    for (int64_t i = 0; i < n; i++) lab[i] = ((i / 37) % 3 == 0) ? 0 : (int32_t)((i / 5) % (span + 4)) + (int32_t)lo - 2;   // runs; ids on both sides of the span
    for (auto &v : f) v = draw<E>(rng);
    for (int64_t i = 0; i < n; i++) if (lab[i] == lo + 1 && std::is_floating_point<E>::value && layout == LRD_VOLUME) f[i] = (E)NAN;   // an all-NaN id
    Buf<int32_t> L(lab, shift ? 1 : 0); Buf<E> F(f, shift ? 1 : 0);
    const bool vec = lr_aligned16(L.p), vec_f = lr_aligned16(F.p) && (layout != LRD_PLANE || hw % LR_VEC == 0);
    std::vector<unsigned long long> rec((size_t)span * LRD_REC);
    std::vector<double> mean(span);
    const int64_t blocks = (n + LR_BLOCK - 1) / LR_BLOCK, id_lanes = (span + 1 + 255) / 256 * 256;
    for (int64_t l = 0; l < id_lanes; l++) lrd_init_body(l, span, rec.data());
    for (int64_t b = 0; b < blocks; b++) for (int t = 0; t < 256; t++) lrd_pass1_body<E>(b, t, L.p, F.p, n, hw, layout, vec, vec_f, lo, hi, none, rec.data());
    for (int64_t l = 0; l < id_lanes; l++) lrd_mean_body<E>(l, span, rec.data(), mean.data());
    for (int64_t b = 0; b < blocks; b++) for (int t = 0; t < 256; t++) lrd_pass2_body<E>(b, t, L.p, F.p, n, hw, layout, vec, vec_f, lo, hi, none, mean.data(), rec.data());
    // tf_label_order on the same operands
    std::vector<uint32_t> count(span + 1), offset(span + 1), cursor(span);
    for (int64_t l = 0; l < id_lanes; l++) lro_counts_body(l, span, rec.data(), count.data());
    uint32_t run = 0;
    for (int64_t l = 0; l <= span; l++) { offset[l] = run; run += count[l]; }
    const int64_t n_keys = offset[span];
    for (int64_t l = 0; l < id_lanes; l++) lro_clamp_body(l, span, offset.data(), n_keys);      // changes nothing here
    std::copy(offset.begin(), offset.begin() + span, cursor.begin());
    std::vector<K> keys(n_keys);
    std::vector<double> mid(2 * span);
    for (int64_t b = 0; b < blocks; b++) for (int t = 0; t < 256; t++) lro_scatter_body<E>(b, t, L.p, F.p, n, hw, layout, vec, vec_f, lo, hi, none, offset.data(), cursor.data(), keys.data(), n_keys);
    for (int64_t l = 0; l < span; l++) { CHECK(cursor[l] == offset[l + 1]); std::sort(keys.begin() + offset[l], keys.begin() + offset[l + 1]); }
    for (int64_t l = 0; l < id_lanes; l++) lro_pick_body<E>(l, span, offset.data(), keys.data(), n_keys, mid.data());

    for (int64_t id = lo; id <= hi; id++) {
        long long cnt = 0, nn = 0, nz = 0; S sum = 0; double mn = INFINITY, mx = -INFINITY;
        std::vector<double> vals;
        for (int64_t i = 0; i < n; i++) {
            if (lab[i] != id) continue;
            const E x = at(f, i, hw, layout);
            cnt++; nz += x != (E)0;
            if (x != x) continue;
            nn++; sum += (S)x; mn = std::min(mn, (double)x); mx = std::max(mx, (double)x); vals.push_back((double)x);
        }
        const unsigned long long *r = rec.data() + LRD_REC * (id - lo);
        S got_sum; std::memcpy(&got_sum, r + 3, 8);
        double got_sv; std::memcpy(&got_sv, r + 6, 8);
        bool ok = r[0] == (unsigned long long)cnt && r[1] == (unsigned long long)nn && r[2] == (unsigned long long)nz && r[7] == 0;
        ok = ok && (std::is_floating_point<E>::value ? same((double)got_sum, (double)sum, 1e-12) : got_sum == sum);
        ok = ok && (nn ? lrd_unkey(r[4]) == mn && lrd_unkey(r[5]) == mx : r[4] == LR_NONE && r[5] == 0);
        double sv = 0;
        const double m = nn ? (double)sum / (double)nn : NAN;
        for (double x : vals) sv += (x - m) * (x - m);
        ok = ok && same(got_sv, sv, 1e-12) && same(mean[id - lo], m, 1e-12);
        std::sort(vals.begin(), vals.end());
        const double a = nn ? vals[(nn - 1) / 2] : NAN, b = nn ? vals[nn / 2] : NAN;
        ok = ok && same(mid[2 * (id - lo)], a, 0) && same(mid[2 * (id - lo) + 1], b, 0);
        if (!ok) {
            printf("T=%lld hw=%lld layout=%d shift=%d span=[%lld, %lld] id=%lld size %zu differs\n", (long long)T, (long long)hw, layout, shift, (long long)lo, (long long)hi, (long long)id, sizeof(E));
            failures++;
        }
    }
}

int main()
{
    // shapes: a tail that is no multiple of 4 or 16, several workgroups, a plane whose size is no multiple of 4 (the four
    // voxels of a lane straddle its end) or below 4 (they pass several frames), one voxel, exactly one workgroup
    const int64_t shapes[][2] = {{5, 33 * 67}, {3, 4099}, {1, 1}, {1, 4096}, {7, 3}, {2, 8192 + 5}, {5, 1}};
    const int64_t spans[][2] = {{1, 9}, {-2, 6}, {0, 0}, {3, 3}};
    unsigned seed = 1;
    for (auto &s : shapes)
        for (auto &sp : spans)
            for (int layout = 0; layout < 3; layout++)
                for (int shift = 0; shift < 2; shift++) {
                    reduce_case<uint8_t>(s[0], s[1], layout, shift, sp[0], sp[1], seed++);
                    reduce_case<int32_t>(s[0], s[1], layout, shift, sp[0], sp[1], seed++);
                    reduce_case<float>(s[0], s[1], layout, shift, sp[0], sp[1], seed++);
                    reduce_case<double>(s[0], s[1], layout, shift, sp[0], sp[1], seed++);
                }
    // indices beyond 2^32 through the index arithmetic only: 160 x 5424^2 = 4.7e9 voxels.  The per-frame and the plane
    // form are asked for the voxels around 2^32 and around the end of the volume; the plane is a one-element stand-in
    // (hw = 1 would need a real plane), so what is checked there is i % hw through lr_load_weights' own expression
    const int64_t hw = 5424ll * 5424, T = 160, n = T * hw;
    CHECK(n > (1ll << 32) && (n + LR_BLOCK - 1) / LR_BLOCK <= 0x7fffffffll);
    std::vector<float> frames(T);
    for (int64_t t = 0; t < T; t++) frames[t] = (float)t;
    const int64_t two32 = (int64_t)1 << 32;
    for (int64_t i : std::vector<int64_t>{two32 - 4, two32, (two32 / hw + 1) * hw - 2, n - 4, n - 1}) {
        float xv[LR_VEC];
        const int m = n - i < LR_VEC ? (int)(n - i) : LR_VEC;
        lrd_load_field<float>(frames.data(), i, m, m == LR_VEC, hw, LRD_FRAME, false, xv);
        for (int j = 0; j < m; j++) CHECK(xv[j] == (float)((i + j) / hw));
        CHECK(i % hw == (int64_t)((unsigned long long)i % (unsigned long long)hw));
    }
    // keys: order-preserving, one key for both zeros, the infinities at the ends, and back
    const double vals[] = {-INFINITY, -1e300, -2.5, -1e-310, -0.0, 0.0, 1e-310, 1.0, 3.5, 1e300, INFINITY};
    for (size_t a = 0; a + 1 < sizeof vals / sizeof *vals; a++) {
        CHECK(vals[a] == vals[a + 1] ? lr_key(vals[a]) == lr_key(vals[a + 1]) : lr_key(vals[a]) < lr_key(vals[a + 1]));
        CHECK(lrd_unkey(lr_key(vals[a])) == vals[a] && !std::signbit(lrd_unkey(lr_key(-0.0))));
        const float fa = (float)vals[a], fb = (float)vals[a + 1];
        CHECK(fa == fb ? lro_key(fa) == lro_key(fb) : lro_key(fa) < lro_key(fb));
        CHECK(lro_value(lro_key(fa), 0.f) == (double)fa);
    }
    CHECK(lr_key(-INFINITY) > 0 && lr_key(INFINITY) < LR_NONE);
    for (int32_t v : {INT32_MIN, -1, 0, 1, INT32_MAX}) CHECK(lro_value(lro_key(v), (int32_t)0) == (double)v);
    CHECK(lro_key(INT32_MIN) < lro_key(-1) && lro_key(-1) < lro_key(0) && lro_key(0) < lro_key(INT32_MAX));
    printf(failures ? "%d FAILURES\n" : "label reduce host check: all equal (%d failures)\n", failures);
    return failures != 0;
}
