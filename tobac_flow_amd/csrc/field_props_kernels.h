// Kernel bodies of field_props.hip (tf_flux_cre, tf_quality_weights, tf_label_wstats_multi).  Kept apart from the entry
// points so that the same text compiles for the host: tools/field_props_host_check.cpp supplies the vector types and the
// atomics and runs the bodies lane after lane.  Nothing here touches the HIP runtime.
// The work layout and the run walker are label_runs.h's; the record per (field, label) and its finish are those of
// wstats_kernels.h (WS_REC, WS_OUT, ws_init_body): tf_label_wstats_multi is tf_label_wstats with the per-field state
// arrayed over a field set, so that labels, weights and every input plane are read once per pass for the whole set.
#pragma once
#include <stdint.h>
#include "label_runs.h"
#include "wstats_kernels.h"

// ---- the derived fluxes (tobac_flow/postprocess.py:29-99, get_cre / add_cre_to_dataset) -------------------------------------
// THE derivation: tf_flux_cre, the TOA / BOA field sets and the host check all call these two.  Every operation is an
// addition, a subtraction or a negation rounded in F, in the reference's tree (a regrouped tree rounds differently).
// TOA planes: 0 swdn  1 swup  2 swup_clr  3 lwup  4 lwup_clr
// TOA fields: 0 swdn  1 swup  2 swup_cre  3 lwup  4 lwup_cre  5 net  6 net_cre
#define FP_TOA_PLANES 5
#define FP_TOA_FIELDS 7
template <typename F>
__host__ __device__ __forceinline__ void fp_toa_fields(const F in[FP_TOA_PLANES], F out[FP_TOA_FIELDS])
{
    const F swup_cre = in[1] - in[2], lwup_cre = in[3] - in[4];
    out[0] = in[0]; out[1] = in[1]; out[2] = swup_cre; out[3] = in[3]; out[4] = lwup_cre;
    out[5] = in[0] - (in[1] + in[3]);
    out[6] = -(swup_cre + lwup_cre);
}

// BOA planes: 0 swdn  1 swup  2 lwdn  3 lwup  4 swdn_clr  5 swup_clr  6 lwdn_clr  7 lwup_clr
// BOA fields: 0 swdn  1 swdn_cre  2 swup  3 swup_cre  4 lwdn  5 lwdn_cre  6 lwup  7 lwup_cre  8 net  9 net_cre
#define FP_BOA_PLANES 8
#define FP_BOA_FIELDS 10
template <typename F>
__host__ __device__ __forceinline__ void fp_boa_fields(const F in[FP_BOA_PLANES], F out[FP_BOA_FIELDS])
{
    const F swdn_cre = in[0] - in[4], swup_cre = in[1] - in[5], lwdn_cre = in[2] - in[6], lwup_cre = in[3] - in[7];
    out[0] = in[0]; out[1] = swdn_cre; out[2] = in[1]; out[3] = swup_cre;
    out[4] = in[2]; out[5] = lwdn_cre; out[6] = in[3]; out[7] = lwup_cre;
    out[8] = in[0] + in[2] - (in[1] + in[3]);
    out[9] = swdn_cre + lwdn_cre - (swup_cre + lwup_cre);
}

// four consecutive elements out: one 16-byte store (float) or two (double) when `vec`, else the first m by element
__host__ __device__ inline void fp_vstore(float *p, const float v[LR_VEC])
{
    float4 q;
    q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
    *(float4 *)p = q;
}
__host__ __device__ inline void fp_vstore(double *p, const double v[LR_VEC])
{
    double2 a, b;
    a.x = v[0]; a.y = v[1]; b.x = v[2]; b.y = v[3];
    ((double2 *)p)[0] = a;
    ((double2 *)p)[1] = b;
}
template <typename E>
__host__ __device__ __forceinline__ void fp_store4(E *__restrict__ p, int64_t i, int m, bool vec, const E v[LR_VEC])
{
    if (vec) { fp_vstore(p + i, v); return; }
#pragma unroll
    for (int j = 0; j < LR_VEC; j++) if (j < m) p[i + j] = v[j];
}

// ---- tf_flux_cre ---------------------------------------------------------------------------------------------------------
// in: the 5 TOA planes, then the 8 BOA planes (orders above).  out, the reference's order of insertion:
//   0 toa_swup_cre  1 toa_lwup_cre  2 boa_swdn_cre  3 boa_swup_cre  4 boa_lwdn_cre  5 boa_lwup_cre  6 toa_net
//   7 toa_net_cre   8 boa_net       9 boa_net_cre
#define FP_CRE_IN (FP_TOA_PLANES + FP_BOA_PLANES)
#define FP_CRE_OUT 10
struct FpCrePlanes { const void *in[FP_CRE_IN]; void *out[FP_CRE_OUT]; };

// lane `lane` of the launch takes the elements 4 lane .. 4 lane + 3; vec: all 23 planes are 16-byte aligned
template <typename F>
__device__ inline void fp_cre_body(int64_t lane, int64_t n, bool vec, const FpCrePlanes &p)
{
    const int64_t i = lane * LR_VEC;
    if (i >= n) return;
    const int m = n - i < LR_VEC ? (int)(n - i) : LR_VEC;
    const bool v4 = vec && m == LR_VEC;
    F xv[FP_CRE_IN][LR_VEC], ov[FP_CRE_OUT][LR_VEC];
#pragma unroll
    for (int k = 0; k < FP_CRE_IN; k++) lr_load4<F>((const F *)p.in[k], i, m, v4, xv[k], (F)0);
#pragma unroll
    for (int j = 0; j < LR_VEC; j++) {
        F toa_in[FP_TOA_PLANES], boa_in[FP_BOA_PLANES], toa[FP_TOA_FIELDS], boa[FP_BOA_FIELDS];
#pragma unroll
        for (int k = 0; k < FP_TOA_PLANES; k++) toa_in[k] = xv[k][j];
#pragma unroll
        for (int k = 0; k < FP_BOA_PLANES; k++) boa_in[k] = xv[FP_TOA_PLANES + k][j];
        fp_toa_fields<F>(toa_in, toa);
        fp_boa_fields<F>(boa_in, boa);
        ov[0][j] = toa[2]; ov[1][j] = toa[4];
        ov[2][j] = boa[1]; ov[3][j] = boa[3]; ov[4][j] = boa[5]; ov[5][j] = boa[7];
        ov[6][j] = toa[5]; ov[7][j] = toa[6]; ov[8][j] = boa[8]; ov[9][j] = boa[9];
    }
#pragma unroll
    for (int k = 0; k < FP_CRE_OUT; k++) fp_store4<F>((F *)p.out[k], i, m, v4, ov[k]);
}

// ---- tf_quality_weights ----------------------------------------------------------------------------------------------------
// out = w * (qcflag == 0) * (cth < 30) * isfinite(cot), the three factors 0 or 1 (exact in any float type), multiplied in
// the script's order in the weights' type: a NaN or infinite weight times 0 is NaN, a NaN cth compares false.
template <typename W, typename C>
__device__ inline void fp_quality_body(int64_t lane, const W *__restrict__ w, const int32_t *__restrict__ q, const C *__restrict__ cth,
                                       const C *__restrict__ cot, int64_t n, int64_t hw, bool plane, bool vec, bool vec_w,
                                       bool vec_out, W *__restrict__ out)
{
    const int64_t i = lane * LR_VEC;
    if (i >= n) return;
    const int m = n - i < LR_VEC ? (int)(n - i) : LR_VEC;
    const bool full = m == LR_VEC;
    W wv[LR_VEC], ov[LR_VEC]; int32_t qv[LR_VEC]; C hv[LR_VEC], tv[LR_VEC];
    lr_load_weights<W>(w, i, m, full, hw, plane, vec_w, wv);
    lr_load4<int32_t>(q, i, m, vec && full, qv, 0);
    lr_load4<C>(cth, i, m, vec && full, hv, (C)0);
    lr_load4<C>(cot, i, m, vec && full, tv, (C)0);
#pragma unroll
    for (int j = 0; j < LR_VEC; j++)
        ov[j] = wv[j] * (W)(qv[j] == 0 ? 1 : 0) * (W)(hv[j] < (C)30 ? 1 : 0) * (W)(lr_finite((double)tv[j]) ? 1 : 0);
    fp_store4<W>(out, i, m, vec_out && full, ov);
}

// ---- tf_label_wstats_multi -------------------------------------------------------------------------------------------------
// A field set is a policy: PLANES input planes, FIELDS fields, `fields(in, out)` the values of one voxel in the field
// type.  FpPlain<N> takes up to N planes as they are (`nf` of them are used), each with an optional errors plane.
#define FP_MAX_PLANES 8
struct FpPlanes { const void *x[FP_MAX_PLANES]; const void *e[FP_MAX_PLANES]; int nf; };

template <int N>
struct FpPlain {
    static constexpr int PLANES = N, FIELDS = N;
    static constexpr bool PLAIN = true;
    template <typename F> static __host__ __device__ __forceinline__ void fields(const F in[N], F out[N])
    {
#pragma unroll
        for (int k = 0; k < N; k++) out[k] = in[k];
    }
};
struct FpToa {
    static constexpr int PLANES = FP_TOA_PLANES, FIELDS = FP_TOA_FIELDS;
    static constexpr bool PLAIN = false;
    template <typename F> static __host__ __device__ __forceinline__ void fields(const F in[PLANES], F out[FIELDS]) { fp_toa_fields<F>(in, out); }
};
struct FpBoa {
    static constexpr int PLANES = FP_BOA_PLANES, FIELDS = FP_BOA_FIELDS;
    static constexpr bool PLAIN = false;
    template <typename F> static __host__ __device__ __forceinline__ void fields(const F in[PLANES], F out[FIELDS]) { fp_boa_fields<F>(in, out); }
};

// the value the order-preserving key k stands for (lr_key's inverse; both zeros come back as +0.0, which equals either)
__host__ __device__ inline double fp_unkey(unsigned long long k)
{
    union { double d; unsigned long long u; } c;
    c.u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return c.d;
}

// Record of (field f, label id): acc + WS_REC * (f * n_labels + id - 1), the slots of wstats_kernels.h.  Every field keeps
// its OWN finite mask: its n, sums, extremes and indices see the voxels at which ITS value is finite and no others.
// Pass 1.  A lane's open run keeps, per field, n (<= 16), the three sums (four with errors) and the extremes as values of
// F; the keys are formed at the close.  The errors (FpPlain only) are read by element under labelled voxels.
template <typename S, typename F, typename W>
struct FpPass1 {
    static constexpr int NP = S::PLANES, NF = S::FIELDS;
    const FpPlanes &pl; const W *__restrict__ w;
    int64_t hw, n_labels; bool plane, vec, vec_w; double *acc;
    uint32_t cnt[NF];
    F xmin[NF], xmax[NF];
    double sw[NF], sww[NF], swx[NF], swe[S::PLAIN ? NF : 1];
    F xv[NP][LR_VEC]; W wv[LR_VEC];

    __device__ __forceinline__ bool used(int f) const { return !S::PLAIN || f < pl.nf; }
    __device__ __forceinline__ void load(int64_t i, int m, bool full)
    {
#pragma unroll
        for (int p = 0; p < NP; p++) if (used(p)) lr_load4<F>((const F *)pl.x[p], i, m, vec && full, xv[p], (F)0);
        lr_load_weights<W>(w, i, m, full, hw, plane, vec_w, wv);
    }
    __device__ __forceinline__ bool ends(int) const { return false; }
    __device__ __forceinline__ void open(int32_t, bool, int)
    {
#pragma unroll
        for (int f = 0; f < NF; f++) {
            cnt[f] = 0; sw[f] = sww[f] = swx[f] = 0;
            xmin[f] = (F)__builtin_inf(); xmax[f] = -(F)__builtin_inf();
            if (S::PLAIN) swe[f] = 0;
        }
    }
    __device__ __forceinline__ void add(int64_t i, int j)
    {
        F in[NP], x[NF];
#pragma unroll
        for (int p = 0; p < NP; p++) in[p] = used(p) ? xv[p][j] : (F)0;
        S::template fields<F>(in, x);
        const double wd = (double)wv[j], w2 = wd * wd;
#pragma unroll
        for (int f = 0; f < NF; f++) {
            if (!used(f)) continue;
            const double xd = (double)x[f];
            if (!lr_finite(xd)) continue;
            cnt[f]++;
            sw[f] += wd; sww[f] += w2; swx[f] += wd * xd;
            if (S::PLAIN && pl.e[f]) { const double ed = (double)((const F *)pl.e[f])[i + j]; swe[f] += w2 * (ed * ed); }
            xmin[f] = x[f] < xmin[f] ? x[f] : xmin[f];
            xmax[f] = x[f] > xmax[f] ? x[f] : xmax[f];
        }
    }
    __device__ __forceinline__ void close(int32_t cur)
    {
#pragma unroll
        for (int f = 0; f < NF; f++) {
            if (!used(f) || !cnt[f]) continue;                    // cur is in [1, n_labels] whenever a count is not 0
            double *r = acc + WS_REC * ((int64_t)f * n_labels + (int64_t)(cur - 1));
            unsigned long long *u = (unsigned long long *)r;
            atomicAdd(u, (unsigned long long)cnt[f]);
            if (sw[f] != 0) atomicAdd(r + 1, sw[f]);              // NaN != 0: a NaN weight reaches the sum and poisons the label
            if (sww[f] != 0) atomicAdd(r + 2, sww[f]);
            if (swx[f] != 0) atomicAdd(r + 3, swx[f]);
            if (S::PLAIN && pl.e[f] && swe[f] != 0) atomicAdd(r + 4, swe[f]);
            const unsigned long long kmin = lr_key((double)xmin[f]), kmax = lr_key((double)xmax[f]);
            if (u[5] > kmin) atomicMin(u + 5, kmin);              // a stale read only costs a redundant atomic
            if (u[6] < kmax) atomicMax(u + 6, kmax);
            cnt[f] = 0;
        }
    }
    __device__ __forceinline__ void last(int, int32_t cur) { close(cur); }
};

template <typename S, typename F, typename W>
__device__ inline void fp_pass1_body(int64_t block, int tid, const int32_t *__restrict__ labels, const FpPlanes &pl,
                                     const W *__restrict__ w, int64_t n, int64_t hw, bool plane, bool vec, bool vec_w,
                                     int64_t n_labels, double *acc)
{
    FpPass1<S, F, W> v{pl, w, hw, n_labels, plane, vec, vec_w, acc};
#pragma unroll
    for (int f = 0; f < S::FIELDS; f++) v.cnt[f] = 0;
    lr_walk(block, tid, labels, n, vec, n_labels, v);
}

// Pass 2.  Per field the mean and the two extremes pass 1 left, the sum of weighted squared deviations, and the smallest
// index at each extreme as an offset from the workgroup's first voxel (a lane's voxels lie within LR_BLOCK of it).
#define FP_NO_OFFSET 0xffffffffu
template <typename S, typename F, typename W>
struct FpPass2 {
    static constexpr int NP = S::PLANES, NF = S::FIELDS;
    const FpPlanes &pl; const W *__restrict__ w;
    int64_t hw, n_labels, base; bool plane, vec, vec_w; double *acc;
    bool valid[NF];
    double mean[NF], sv[NF];
    F xmin[NF], xmax[NF];
    uint32_t imin[NF], imax[NF];
    F xv[NP][LR_VEC]; W wv[LR_VEC];

    __device__ __forceinline__ bool used(int f) const { return !S::PLAIN || f < pl.nf; }
    __device__ __forceinline__ void load(int64_t i, int m, bool full)
    {
#pragma unroll
        for (int p = 0; p < NP; p++) if (used(p)) lr_load4<F>((const F *)pl.x[p], i, m, vec && full, xv[p], (F)0);
        lr_load_weights<W>(w, i, m, full, hw, plane, vec_w, wv);
    }
    __device__ __forceinline__ bool ends(int) const { return false; }
    __device__ __forceinline__ void open(int32_t l, bool in, int)
    {
#pragma unroll
        for (int f = 0; f < NF; f++) {
            valid[f] = false; sv[f] = 0; imin[f] = imax[f] = FP_NO_OFFSET;
            if (in && used(f)) {                                  // what pass 1 left for this label (a finished kernel's writes)
                const double *r = acc + WS_REC * ((int64_t)f * n_labels + (int64_t)(l - 1));
                const unsigned long long *u = (const unsigned long long *)r;
                const double tw = r[1];
                valid[f] = u[0] > 0 && tw > 0;                    // false for a NaN sum: the label is NaN throughout
                mean[f] = r[3] / tw; xmin[f] = (F)fp_unkey(u[5]); xmax[f] = (F)fp_unkey(u[6]);
            }
        }
    }
    __device__ __forceinline__ void add(int64_t i, int j)
    {
        F in[NP], x[NF];
#pragma unroll
        for (int p = 0; p < NP; p++) in[p] = used(p) ? xv[p][j] : (F)0;
        S::template fields<F>(in, x);
        const double wd = (double)wv[j];
        const uint32_t at = (uint32_t)(i + j - base);
#pragma unroll
        for (int f = 0; f < NF; f++) {
            if (!valid[f]) continue;
            const double xd = (double)x[f];
            if (!lr_finite(xd)) continue;
            const double d = xd - mean[f];
            sv[f] += wd * (d * d);
            if (x[f] == xmin[f] && at < imin[f]) imin[f] = at;
            if (x[f] == xmax[f] && at < imax[f]) imax[f] = at;
        }
    }
    __device__ __forceinline__ void close(int32_t cur)
    {
#pragma unroll
        for (int f = 0; f < NF; f++) {
            if (!valid[f]) continue;                              // cur is in [1, n_labels] whenever a field is valid
            double *r = acc + WS_REC * ((int64_t)f * n_labels + (int64_t)(cur - 1));
            unsigned long long *u = (unsigned long long *)r;
            if (sv[f] != 0) atomicAdd(r + 8, sv[f]);
            if (imin[f] != FP_NO_OFFSET) { const unsigned long long at = (unsigned long long)base + imin[f]; if (at < u[9]) atomicMin(u + 9, at); }
            if (imax[f] != FP_NO_OFFSET) { const unsigned long long at = (unsigned long long)base + imax[f]; if (at < u[10]) atomicMin(u + 10, at); }
            valid[f] = false;
        }
    }
    __device__ __forceinline__ void last(int, int32_t cur) { close(cur); }
};

template <typename S, typename F, typename W>
__device__ inline void fp_pass2_body(int64_t block, int tid, const int32_t *__restrict__ labels, const FpPlanes &pl,
                                     const W *__restrict__ w, int64_t n, int64_t hw, bool plane, bool vec, bool vec_w,
                                     int64_t n_labels, double *acc)
{
    FpPass2<S, F, W> v{pl, w, hw, n_labels, block * LR_BLOCK, plane, vec, vec_w, acc};
#pragma unroll
    for (int f = 0; f < S::FIELDS; f++) v.valid[f] = false;
    lr_walk(block, tid, labels, n, vec, n_labels, v);
}

// field f of the set at voxel `at`, through the set's own derivation
template <typename S, typename F>
__device__ __forceinline__ F fp_field_at(const FpPlanes &pl, int f, int64_t at)
{
    F in[S::PLANES], x[S::FIELDS];
#pragma unroll
    for (int p = 0; p < S::PLANES; p++) in[p] = (!S::PLAIN || p < pl.nf) ? ((const F *)pl.x[p])[at] : (F)0;
    S::template fields<F>(in, x);
    F v = (F)0;
#pragma unroll
    for (int k = 0; k < S::FIELDS; k++) v = k == f ? x[k] : v;    // a select, not an indexed read of a register array
    return v;
}

// out[(f * n_labels + id - 1) * WS_OUT + ..]: the ten columns of ws_finish_body, one lane per (field, label)
template <typename S, typename F>
__device__ inline void fp_finish_body(int64_t r_index, int64_t n_labels, const double *__restrict__ acc, const FpPlanes &pl,
                                      int64_t n, double *__restrict__ out)
{
    const int nf = S::PLAIN ? pl.nf : S::FIELDS;
    if (r_index >= (int64_t)nf * n_labels) return;
    const int f = (int)(r_index / n_labels);
    const double *r = acc + WS_REC * r_index;
    const unsigned long long *u = (const unsigned long long *)r;
    double *o = out + WS_OUT * r_index;
    const double nan = __builtin_nan("");
    const double cnt = (double)u[0], sw = r[1];
    o[0] = cnt; o[1] = sw;
#pragma unroll
    for (int k = 2; k < WS_OUT; k++) o[k] = nan;
    if (!(u[0] > 0 && sw > 0)) return;
    const unsigned long long imin = u[9], imax = u[10];
    if (imin >= (unsigned long long)n || imax >= (unsigned long long)n) return;   // cannot happen: pass 2 met both extremes
    const double var = r[8] / sw;
    const double c = 1.0 - r[2] / (sw * sw);                      // Bessel's correction for reliability weights
    const double sd = c >= 0 ? sqrt(var / c) : nan;               // 0 / 0 -> NaN, a / 0 -> inf, as numpy's scalars
    o[2] = r[3] / sw;
    o[3] = sd;
    o[4] = (double)fp_field_at<S, F>(pl, f, (int64_t)imin);
    o[5] = (double)fp_field_at<S, F>(pl, f, (int64_t)imax);
    if (!S::PLAIN) return;
    const F *e = nullptr;
#pragma unroll
    for (int k = 0; k < (S::PLAIN ? S::FIELDS : 0); k++) e = k == f ? (const F *)pl.e[k] : e;
    if (!e) return;
    const double un = sqrt(r[4]) / sw, se = sd / sqrt(cnt);
    o[6] = un;
    o[7] = sqrt(se * se + un * un);
    o[8] = (double)e[imin];
    o[9] = (double)e[imax];
}
