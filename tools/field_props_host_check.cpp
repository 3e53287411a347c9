// Host check of the kernel bodies of tobac_flow_amd/csrc/field_props_kernels.h (tf_flux_cre, tf_quality_weights,
// tf_label_wstats_multi) and of the raveled walker of label_runs.h under them: the same text compiled for the CPU, run
// lane after lane on exactly-sized heap buffers against plain loops, meant for AddressSanitizer + UBSan:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/field_props_host_check.cpp -o field_props_host_check
//   ./field_props_host_check
//
// Lanes run one after the other, so the atomics are plain read-modify-writes; what is checked is indexing (every load and
// store inside its buffer, at every alignment / tail / plane-straddle form), the derivation trees bit for bit against the
// expressions written out again here, and -- the one thing fusion can get wrong -- that every field of a set keeps its
// own finite mask.  Every set, both field types and both weight types, on the shapes of tests/field_props_cases.py.
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
template <typename T> static T atomicAdd(T *p, T v) { T o = *p; *p = o + v; return o; }
static unsigned long long atomicMin(unsigned long long *p, unsigned long long v) { unsigned long long o = *p; *p = std::min(o, v); return o; }
static unsigned long long atomicMax(unsigned long long *p, unsigned long long v) { unsigned long long o = *p; *p = std::max(o, v); return o; }

#include "../tobac_flow_amd/csrc/field_props_kernels.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s (line %d)\n", #c, __LINE__); failures++; } } while (0)

static bool same(double a, double b, double rtol)
{
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    if (std::isinf(a) || std::isinf(b)) return a == b;
    return std::fabs(a - b) <= rtol * std::fabs(b);
}
// equal as values of F with NaN == NaN and the sign of a zero told apart
template <typename F> static bool same_bits(F a, F b)
{
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    return a == b && std::signbit(a) == std::signbit(b);
}

// exactly-sized copy whose start is `shift` elements past a 16-byte boundary (shift != 0: the element-load form)
template <typename E> struct Buf {
    std::vector<E> store; E *p;
    Buf(const std::vector<E> &v, int shift) : store(v.size() + shift), p(nullptr) { if (!v.empty()) std::memcpy(store.data() + shift, v.data(), v.size() * sizeof(E)); p = store.data() + shift; }
};

// signed flux-like values with the special cases planted: NaN, +-inf (inf - inf in a derived field), -0.0, ties
template <typename F> static std::vector<F> plane_values(int64_t n, std::mt19937 &rng)
{
    std::vector<F> v(n);
    for (int64_t i = 0; i < n; i++) {
        const int r = rng() % 60;
        v[i] = (F)((int)(rng() % 4001) - 2000) / (F)7;
        if (r == 0) v[i] = NAN; else if (r == 1) v[i] = INFINITY; else if (r == 2) v[i] = -INFINITY; else if (r == 3) v[i] = (F)-0.0; else if (r < 12) v[i] = (F)(r - 8);
    }
    return v;
}

// the derived fields written out again (NOT through fp_toa_fields / fp_boa_fields): the reference's trees
template <typename F> static void toa_restated(const F *in, F *out)
{
    const F swdn = in[0], swup = in[1], swup_clr = in[2], lwup = in[3], lwup_clr = in[4];
    const F swup_cre = swup - swup_clr, lwup_cre = lwup - lwup_clr;
    const F net = swdn - (swup + lwup), net_cre = -(swup_cre + lwup_cre);
    const F all[7] = {swdn, swup, swup_cre, lwup, lwup_cre, net, net_cre};
    std::copy(all, all + 7, out);
}
template <typename F> static void boa_restated(const F *in, F *out)
{
    const F swdn = in[0], swup = in[1], lwdn = in[2], lwup = in[3];
    const F swdn_cre = swdn - in[4], swup_cre = swup - in[5], lwdn_cre = lwdn - in[6], lwup_cre = lwup - in[7];
    const F net = swdn + lwdn - (swup + lwup), net_cre = swdn_cre + lwdn_cre - (swup_cre + lwup_cre);
    const F all[10] = {swdn, swdn_cre, swup, swup_cre, lwdn, lwdn_cre, lwup, lwup_cre, net, net_cre};
    std::copy(all, all + 10, out);
}

template <typename F> static void cre_case(int64_t n, int shift, unsigned seed)
{
    std::mt19937 rng(seed);
    std::vector<Buf<F>> in, out;
    for (int k = 0; k < FP_CRE_IN; k++) in.emplace_back(plane_values<F>(n, rng), shift ? 1 : 0);
    for (int k = 0; k < FP_CRE_OUT; k++) out.emplace_back(std::vector<F>(n, (F)12345), shift ? 1 : 0);
    FpCrePlanes p; bool vec = true;
    for (int k = 0; k < FP_CRE_IN; k++) { p.in[k] = in[k].p; vec = vec && lr_aligned16(p.in[k]); }
    for (int k = 0; k < FP_CRE_OUT; k++) { p.out[k] = out[k].p; vec = vec && lr_aligned16(p.out[k]); }
    const int64_t lanes = ((n + LR_VEC - 1) / LR_VEC + 255) / 256 * 256;
    for (int64_t l = 0; l < lanes; l++) fp_cre_body<F>(l, n, vec, p);
    for (int64_t i = 0; i < n; i++) {
        F ti[5], bi[8], t[7], b[10];
        for (int k = 0; k < 5; k++) ti[k] = in[k].p[i];
        for (int k = 0; k < 8; k++) bi[k] = in[5 + k].p[i];
        toa_restated(ti, t); boa_restated(bi, b);
        const F want[FP_CRE_OUT] = {t[2], t[4], b[1], b[3], b[5], b[7], t[5], t[6], b[8], b[9]};
        for (int k = 0; k < FP_CRE_OUT; k++)
            if (!same_bits(out[k].p[i], want[k])) { printf("cre n=%lld shift=%d i=%lld out %d: %.9g != %.9g\n", (long long)n, shift, (long long)i, k, (double)out[k].p[i], (double)want[k]); failures++; }
    }
}

template <typename W, typename C> static void quality_case(int64_t T, int64_t hw, bool plane, int shift, unsigned seed)
{
    const int64_t n = T * hw;
    std::mt19937 rng(seed);
    std::vector<W> w(plane ? hw : n); std::vector<int32_t> q(n); std::vector<C> cth(n), cot(n);
    for (auto &v : w) { const int r = rng() % 12; v = r == 0 ? (W)NAN : r == 1 ? (W)INFINITY : r == 2 ? (W)0 : (W)(1 + rng() % 9) / (W)4; }
    for (int64_t i = 0; i < n; i++) {
        q[i] = (rng() % 4 == 0) ? (int32_t)(rng() % 5) - 2 : 0;
        const int r = rng() % 10;
        cth[i] = r == 0 ? (C)NAN : r == 1 ? (C)30 : (C)(rng() % 45);
        cot[i] = (rng() % 6 == 0) ? (C)NAN : (rng() % 9 == 0) ? (C)INFINITY : (C)(rng() % 100) / (C)8;
    }
    Buf<W> Wb(w, shift ? 1 : 0), O(std::vector<W>(n, (W)777), shift ? 1 : 0); Buf<int32_t> Q(q, shift ? 1 : 0); Buf<C> H(cth, shift ? 1 : 0), Tb(cot, shift ? 1 : 0);
    const bool vec = lr_aligned16(Q.p) && lr_aligned16(H.p) && lr_aligned16(Tb.p), vec_w = lr_aligned16(Wb.p) && (!plane || hw % LR_VEC == 0);
    const int64_t lanes = ((n + LR_VEC - 1) / LR_VEC + 255) / 256 * 256;
    for (int64_t l = 0; l < lanes; l++) fp_quality_body<W, C>(l, Wb.p, Q.p, H.p, Tb.p, n, hw, plane, vec, vec_w, lr_aligned16(O.p), O.p);
    for (int64_t i = 0; i < n; i++) {
        const W a = q[i] == 0 ? (W)1 : (W)0, b = cth[i] < (C)30 ? (W)1 : (W)0, c = std::isfinite((double)cot[i]) ? (W)1 : (W)0;
        const W want = w[plane ? i % hw : i] * a * b * c;
        if (!same_bits(O.p[i], want)) { printf("quality T=%lld hw=%lld plane=%d shift=%d i=%lld: %.9g != %.9g\n", (long long)T, (long long)hw, plane, shift, (long long)i, (double)O.p[i], (double)want); failures++; }
    }
}

// S: the field set; nf: planes in use (FpPlain) -- every second one of them then has an errors plane
template <typename S, typename F, typename W>
static void multi_case(const char *name, int nf_planes, int64_t T, int64_t hw, bool plane, int shift, unsigned seed)
{
    const int64_t n = T * hw, n_labels = 9;
    const int n_fields = S::PLAIN ? nf_planes : S::FIELDS;
    std::mt19937 rng(seed);
    std::vector<int32_t> lab(n);
    for (int64_t i = 0; i < n; i++) lab[i] = ((i / 37) % 3 == 0) ? 0 : (int32_t)((i / 53) % 12) - 1;     // runs; ids -1 .. 10
    std::vector<std::vector<F>> x, e;
    for (int p = 0; p < nf_planes; p++) { x.push_back(plane_values<F>(n, rng)); e.emplace_back(n); for (auto &v : e.back()) v = (F)(1 + rng() % 9) / (F)16; }
    if (n > 60) for (int64_t i = 0; i < n; i++) if (lab[i] == 2) x[nf_planes - 1][i] = NAN;              // a label all-NaN in one plane only
    std::vector<W> w(plane ? hw : n);
    for (auto &v : w) v = (rng() % 5 == 0) ? (W)0 : (W)(1 + rng() % 7) / (W)4;
    for (int64_t i = 0; i < n; i++) if (lab[i] == 4) { w[plane ? i % hw : i] = NAN; break; }              // one label poisoned
    Buf<int32_t> L(lab, shift ? 1 : 0); Buf<W> Wb(w, shift ? 1 : 0);
    std::vector<Buf<F>> X, E;
    for (int p = 0; p < nf_planes; p++) { X.emplace_back(x[p], shift ? 1 : 0); E.emplace_back(e[p], shift ? 1 : 0); }
    FpPlanes pl; pl.nf = n_fields;
    bool vec = lr_aligned16(L.p);
    for (int p = 0; p < FP_MAX_PLANES; p++) {
        pl.x[p] = p < nf_planes ? X[p].p : nullptr;
        pl.e[p] = (S::PLAIN && p < nf_planes && p % 2 == 0) ? E[p].p : nullptr;
        if (p < nf_planes) vec = vec && lr_aligned16(pl.x[p]);
    }
    const bool vec_w = lr_aligned16(Wb.p) && (!plane || hw % LR_VEC == 0);
    const int64_t records = n_fields * n_labels, blocks = (n + LR_BLOCK - 1) / LR_BLOCK, id_lanes = (records + 255) / 256 * 256;
    std::vector<double> acc((size_t)records * WS_REC), out((size_t)records * WS_OUT);
    for (int64_t l = 0; l < id_lanes; l++) ws_init_body(l, records, acc.data());
    for (int64_t b = 0; b < blocks; b++) for (int t = 0; t < 256; t++) fp_pass1_body<S, F, W>(b, t, L.p, pl, Wb.p, n, hw, plane, vec, vec_w, n_labels, acc.data());
    for (int64_t b = 0; b < blocks; b++) for (int t = 0; t < 256; t++) fp_pass2_body<S, F, W>(b, t, L.p, pl, Wb.p, n, hw, plane, vec, vec_w, n_labels, acc.data());
    for (int64_t l = 0; l < id_lanes; l++) fp_finish_body<S, F>(l, n_labels, acc.data(), pl, n, out.data());
    // the fields as volumes, by the restated trees
    std::vector<std::vector<F>> fld(n_fields, std::vector<F>(n));
    for (int64_t i = 0; i < n; i++) {
        F in[FP_MAX_PLANES], o[FP_BOA_FIELDS];
        for (int p = 0; p < nf_planes; p++) in[p] = x[p][i];
        if (S::PLAIN) std::copy(in, in + nf_planes, o); else if (S::FIELDS == FP_TOA_FIELDS) toa_restated(in, o); else boa_restated(in, o);
        for (int f = 0; f < n_fields; f++) fld[f][i] = o[f];
    }
    for (int f = 0; f < n_fields; f++) for (int64_t id = 1; id <= n_labels; id++) {
        const bool with_e = S::PLAIN && pl.e[f] != nullptr;
        const std::vector<F> &xs = fld[f];
        double cnt = 0, sw = 0, sww = 0, swx = 0, swax = 0, swe = 0, mn = INFINITY, mx = -INFINITY; int64_t imin = -1, imax = -1;
        for (int64_t i = 0; i < n; i++) {
            if (lab[i] != id || !std::isfinite((double)xs[i])) continue;
            const double wd = w[plane ? i % hw : i], xd = xs[i];
            cnt++; sw += wd; sww += wd * wd; swx += wd * xd; swax += std::fabs(wd * xd);
            if (with_e) swe += wd * wd * ((double)e[f][i] * (double)e[f][i]);
            if (xd < mn) { mn = xd; imin = i; }
            if (xd > mx) { mx = xd; imax = i; }
        }
        double want[WS_OUT]; for (double &v : want) v = NAN;
        want[0] = cnt; want[1] = sw;
        if (cnt > 0 && sw > 0) {
            const double mean = swx / sw; double sv = 0;
            for (int64_t i = 0; i < n; i++) if (lab[i] == id && std::isfinite((double)xs[i])) sv += (double)w[plane ? i % hw : i] * (((double)xs[i] - mean) * ((double)xs[i] - mean));
            const double c = 1 - sww / (sw * sw), sd = c >= 0 ? std::sqrt(sv / sw / c) : NAN;
            want[2] = mean; want[3] = sd; want[4] = mn; want[5] = mx;
            if (with_e) { const double un = std::sqrt(swe) / sw; want[6] = un; want[7] = std::sqrt(sd / std::sqrt(cnt) * (sd / std::sqrt(cnt)) + un * un); want[8] = e[f][imin]; want[9] = e[f][imax]; }
        }
        for (int k = 0; k < WS_OUT; k++) {
            const bool exact = k == 0 || k == 4 || k == 5 || k == 8 || k == 9;
            const double got = out[((int64_t)f * n_labels + id - 1) * WS_OUT + k];
            // the mean of signed terms can cancel: its error is relative to sum |w x| / sum w, not to the mean
            const bool ok = k == 2 && std::isfinite(got) && std::isfinite(want[k]) ? std::fabs(got - want[k]) <= 1e-12 * swax / sw : same(got, want[k], exact ? 0 : 1e-9);
            if (!ok) {
                printf("%s F%zu W%zu T=%lld hw=%lld plane=%d shift=%d field %d id=%lld slot %d: %.17g != %.17g\n", name, sizeof(F), sizeof(W), (long long)T, (long long)hw, plane, shift, f, (long long)id, k, got, want[k]);
                failures++;
            }
        }
    }
}

template <typename F, typename W> static void multi_cases(int64_t T, int64_t hw, bool plane, int shift, unsigned &seed)
{
    multi_case<FpToa, F, W>("TOA", FP_TOA_PLANES, T, hw, plane, shift, seed++);
    multi_case<FpBoa, F, W>("BOA", FP_BOA_PLANES, T, hw, plane, shift, seed++);
    multi_case<FpPlain<4>, F, W>("PLAIN4", 3, T, hw, plane, shift, seed++);
    multi_case<FpPlain<4>, F, W>("PLAIN4", 1, T, hw, plane, shift, seed++);
    multi_case<FpPlain<FP_MAX_PLANES>, F, W>("PLAIN8", 8, T, hw, plane, shift, seed++);
    multi_case<FpPlain<FP_MAX_PLANES>, F, W>("PLAIN8", 5, T, hw, plane, shift, seed++);
}

int main()
{
    // the shapes of tests/field_props_cases.py: one voxel, exactly one workgroup (2 x 32 x 64 = 4096), several workgroups
    // with an odd plane (37 x 41 = 1517: a lane's four voxels straddle the plane's end, the tail is no multiple of 4),
    // aligned everywhere (5 x 64 x 96)
    const int64_t shapes[][2] = {{1, 1}, {2, 32 * 64}, {3, 37 * 41}, {5, 64 * 96}};
    unsigned seed = 1;
    for (auto &s : shapes)
        for (int shift = 0; shift < 2; shift++) {
            cre_case<float>(s[0] * s[1], shift, seed++);
            cre_case<double>(s[0] * s[1], shift, seed++);
            for (int plane = 0; plane < 2; plane++) {
                quality_case<float, float>(s[0], s[1], plane, shift, seed++);
                quality_case<float, double>(s[0], s[1], plane, shift, seed++);
                quality_case<double, float>(s[0], s[1], plane, shift, seed++);
                quality_case<double, double>(s[0], s[1], plane, shift, seed++);
                multi_cases<float, float>(s[0], s[1], plane, shift, seed);
                multi_cases<float, double>(s[0], s[1], plane, shift, seed);
                multi_cases<double, float>(s[0], s[1], plane, shift, seed);
                multi_cases<double, double>(s[0], s[1], plane, shift, seed);
            }
        }
    // the key and its inverse: every finite value comes back, both zeros as one that equals either
    const double vals[] = {-1e300, -2.5, -1e-310, -0.0, 0.0, 1e-310, 1.0, 3.5, 1e300};
    for (double v : vals) CHECK(fp_unkey(lr_key(v)) == v);
    // the offset of pass 2: a lane's voxels lie within LR_BLOCK of the workgroup's first, also beyond 2^32
    const int64_t b = (1ll << 33) / LR_BLOCK + 3;
    for (int t = 0; t < 256; t++) for (int k = 0; k < LR_ITERS; k++) {
        const int64_t off = lr_first_voxel(b, t, k) + LR_VEC - 1 - b * LR_BLOCK;
        CHECK(off >= 0 && off < LR_BLOCK && (uint32_t)off != FP_NO_OFFSET);
    }
    printf(failures ? "%d FAILURES\n" : "field props host check: all equal (%d failures)\n", failures);
    return failures != 0;
}
