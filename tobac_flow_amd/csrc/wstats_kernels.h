// Kernel bodies of wstats.hip (tf_label_wstats, tf_label_proportions).  Kept apart from the entry points so that the same
// text compiles for the host: tools/wstats_host_check.cpp supplies blockIdx / threadIdx / the vector types / the atomics
// and runs the bodies lane after lane under AddressSanitizer.  Nothing here touches the HIP runtime.
// The work layout and the walk over a lane's runs of equal labels are label_runs.h's (the raveled walker, lr_walk); what is
// here are the records and, per pass, the visitor that says what a run gathers and how it reaches its record.
#pragma once
#include <stdint.h>
#include "label_runs.h"

// ---- tf_label_wstats -------------------------------------------------------------------------------------------------
// Workspace record per label id (WS_REC doubles = 128 B, id - 1 indexes it):
//   pass 1:  0 n (uint64)   1 sum w   2 sum w^2   3 sum w x   4 sum w^2 e^2   5 key of min x (uint64)   6 key of max x
//   pass 2:  8 sum w (x - mean)^2   9 smallest raveled index with key(x) == key of min (uint64)   10 the same for max
// all over F = the label's voxels with finite x.  Slots 5, 9, 10 start at LR_NONE, everything else at 0.
#define WS_REC 16
#define WS_OUT 10

__device__ inline void ws_init_body(int64_t l, int64_t n_labels, double *acc)
{
    if (l >= n_labels) return;
    unsigned long long *r = (unsigned long long *)(acc + WS_REC * l);
#pragma unroll
    for (int k = 0; k < WS_REC; k++) r[k] = (k == 5 || k == 9 || k == 10) ? LR_NONE : 0ull;   // +0.0 and 0 share their bits
}

// weights: a (T, hw) volume, or with `plane` one (hw,) plane that every frame shares (lr_load_weights)
template <typename F>
struct WsPass1 {
    const F *__restrict__ x, *__restrict__ e, *__restrict__ w;
    int64_t hw; bool plane, vec, vec_w; double *acc;
    unsigned long long cnt = 0, kmin = LR_NONE, kmax = 0;
    double sw = 0, sww = 0, swx = 0, swe = 0;
    F xv[LR_VEC], wv[LR_VEC], ev[LR_VEC];

    __device__ __forceinline__ void load(int64_t i, int m, bool full)
    {
        lr_load4<F>(x, i, m, vec && full, xv, (F)0);
        lr_load_weights<F>(w, i, m, full, hw, plane, vec_w, wv);
        if (e) lr_load4<F>(e, i, m, vec && full, ev, (F)0);
    }
    __device__ __forceinline__ bool ends(int) const { return false; }
    __device__ __forceinline__ void open(int32_t, bool, int) { cnt = 0; kmin = LR_NONE; kmax = 0; sw = sww = swx = swe = 0; }
    __device__ __forceinline__ void add(int64_t, int j)
    {
        const double xd = (double)xv[j];
        if (!lr_finite(xd)) return;
        const double wd = (double)wv[j], w2 = wd * wd;
        cnt++;
        sw += wd; sww += w2; swx += wd * xd;
        if (e) { const double ed = (double)ev[j]; swe += w2 * (ed * ed); }
        const unsigned long long k = lr_key(xd);
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
    }
    __device__ __forceinline__ void close(int32_t cur)
    {
        if (!cnt) return;                                         // cur is in [1, n_labels] whenever cnt != 0
        double *r = acc + WS_REC * (int64_t)(cur - 1);
        unsigned long long *u = (unsigned long long *)r;
        atomicAdd(u, cnt);
        if (sw != 0) atomicAdd(r + 1, sw);                        // NaN != 0: a NaN weight reaches the sum and poisons the label
        if (sww != 0) atomicAdd(r + 2, sww);
        if (swx != 0) atomicAdd(r + 3, swx);
        if (e && swe != 0) atomicAdd(r + 4, swe);
        if (u[5] > kmin) atomicMin(u + 5, kmin);                  // a stale read only costs a redundant atomic
        if (u[6] < kmax) atomicMax(u + 6, kmax);
        cnt = 0;
    }
    __device__ __forceinline__ void last(int, int32_t cur) { close(cur); }
};

template <typename F>
__device__ inline void ws_pass1_body(int64_t block, int tid, const int32_t *__restrict__ labels, const F *__restrict__ x,
                                     const F *__restrict__ e, const F *__restrict__ w, int64_t n, int64_t hw, bool plane,
                                     bool vec, bool vec_w, int64_t n_labels, double *acc)
{
    WsPass1<F> v{x, e, w, hw, plane, vec, vec_w, acc};
    lr_walk(block, tid, labels, n, vec, n_labels, v);
}

template <typename F>
struct WsPass2 {
    const F *__restrict__ x, *__restrict__ w;
    int64_t hw; bool plane, vec, vec_w; double *acc;
    bool valid = false;
    double mean = 0, sv = 0;
    unsigned long long kmin = 0, kmax = 0, imin = LR_NONE, imax = LR_NONE;
    F xv[LR_VEC], wv[LR_VEC];

    __device__ __forceinline__ void load(int64_t i, int m, bool full)
    {
        lr_load4<F>(x, i, m, vec && full, xv, (F)0);
        lr_load_weights<F>(w, i, m, full, hw, plane, vec_w, wv);
    }
    __device__ __forceinline__ bool ends(int) const { return false; }
    __device__ __forceinline__ void open(int32_t l, bool in, int)
    {
        valid = false; sv = 0; imin = imax = LR_NONE;
        if (in) {                                                 // what pass 1 left for this label (a finished kernel's writes)
            const double *r = acc + WS_REC * (int64_t)(l - 1);
            const unsigned long long *u = (const unsigned long long *)r;
            const double tw = r[1];
            valid = u[0] > 0 && tw > 0;                           // false for a NaN sum: the label is NaN throughout
            mean = r[3] / tw; kmin = u[5]; kmax = u[6];
        }
    }
    __device__ __forceinline__ void add(int64_t i, int j)
    {
        if (!valid) return;
        const double xd = (double)xv[j];
        if (!lr_finite(xd)) return;
        const double d = xd - mean;
        sv += (double)wv[j] * (d * d);
        const unsigned long long k = lr_key(xd), at = (unsigned long long)(i + j);
        if (k == kmin && at < imin) imin = at;
        if (k == kmax && at < imax) imax = at;
    }
    __device__ __forceinline__ void close(int32_t cur)
    {
        if (!valid) return;                                       // cur is in [1, n_labels] whenever valid
        double *r = acc + WS_REC * (int64_t)(cur - 1);
        unsigned long long *u = (unsigned long long *)r;
        if (sv != 0) atomicAdd(r + 8, sv);
        if (imin < u[9]) atomicMin(u + 9, imin);
        if (imax < u[10]) atomicMin(u + 10, imax);
        valid = false;
    }
    __device__ __forceinline__ void last(int, int32_t cur) { close(cur); }
};

template <typename F>
__device__ inline void ws_pass2_body(int64_t block, int tid, const int32_t *__restrict__ labels, const F *__restrict__ x,
                                     const F *__restrict__ w, int64_t n, int64_t hw, bool plane, bool vec, bool vec_w,
                                     int64_t n_labels, double *acc)
{
    WsPass2<F> v{x, w, hw, plane, vec, vec_w, acc};
    lr_walk(block, tid, labels, n, vec, n_labels, v);
}

// out[(id - 1) * WS_OUT + ..] = n, sum w, mean, std, min, max, uncertainty, combined error, error at min, error at max
template <typename F>
__device__ inline void ws_finish_body(int64_t l, int64_t n_labels, const double *__restrict__ acc, const F *__restrict__ x,
                                      const F *__restrict__ e, int64_t n, double *__restrict__ out)
{
    if (l >= n_labels) return;
    const double *r = acc + WS_REC * l;
    const unsigned long long *u = (const unsigned long long *)r;
    double *o = out + WS_OUT * l;
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
    o[4] = (double)x[imin];
    o[5] = (double)x[imax];
    if (!e) return;
    const double un = sqrt(r[4]) / sw, se = sd / sqrt(cnt);
    o[6] = un;
    o[7] = sqrt(se * se + un * un);
    o[8] = (double)e[imin];
    o[9] = (double)e[imax];
}

// ---- tf_label_proportions ----------------------------------------------------------------------------------------------
// Record per label id: 1 + K doubles -- the sum of the label's non-NaN weights, then that sum restricted to flag ==
// values[k].  One pass; a lane keeps one open run of equal (label, flag) pairs and adds it to at most two doubles.
#define WP_MAX_FLAGS 64
struct WpFlags { int32_t k; int32_t v[WP_MAX_FLAGS]; };

// A run of an id outside [1, n_labels] gathers nothing (s stays 0), so neither does its close issue anything; only its
// slot search is skipped.
struct WpPass {
    const int32_t *__restrict__ flags; const float *__restrict__ w;
    int64_t hw; bool plane, vec, vec_w; const WpFlags &fl; double *acc;
    int32_t cur_flag = 0;
    int slot = -1;
    double s = 0;
    int32_t fv[LR_VEC]; float wv[LR_VEC];

    __device__ __forceinline__ void load(int64_t i, int m, bool full)
    {
        lr_load4<int32_t>(flags, i, m, vec && full, fv, 0);
        lr_load_weights<float>(w, i, m, full, hw, plane, vec_w, wv);
    }
    __device__ __forceinline__ bool ends(int j) const { return fv[j] != cur_flag; }
    __device__ __forceinline__ void open(int32_t, bool in, int j)
    {
        cur_flag = fv[j]; s = 0; slot = -1;
        if (!in) return;
        for (int k = 0; k < fl.k; k++) if (fl.v[k] == cur_flag) slot = k;             // the values are distinct
    }
    __device__ __forceinline__ void add(int64_t, int j)
    {
        const float wf = wv[j];
        if (wf == wf) s += (double)wf;                            // np.nansum: a NaN weight counts nowhere
    }
    __device__ __forceinline__ void close(int32_t cur)
    {
        if (s == 0) return;                                       // cur is in [1, n_labels] whenever s != 0
        double *r = acc + (int64_t)(1 + fl.k) * (int64_t)(cur - 1);
        atomicAdd(r, s);
        if (slot >= 0) atomicAdd(r + 1 + slot, s);
        s = 0;
    }
    __device__ __forceinline__ void last(int, int32_t cur) { close(cur); }
};

__device__ inline void wp_pass_body(int64_t block, int tid, const int32_t *__restrict__ labels, const int32_t *__restrict__ flags,
                                    const float *__restrict__ w, int64_t n, int64_t hw, bool plane, bool vec, bool vec_w,
                                    int64_t n_labels, const WpFlags &fl, double *acc)
{
    WpPass v{flags, w, hw, plane, vec, vec_w, fl, acc};
    lr_walk(block, tid, labels, n, vec, n_labels, v);
}

__device__ inline void wp_finish_body(int64_t l, int64_t n_labels, int K, const double *__restrict__ acc, double *__restrict__ out)
{
    if (l >= n_labels) return;
    const double *r = acc + (int64_t)(1 + K) * l;
    const double total = r[0];
    for (int k = 0; k < K; k++) out[(int64_t)K * l + k] = total > 0 ? r[1 + k] / total : __builtin_nan("");
}
