// Kernel bodies of wstats.hip (tf_label_wstats, tf_label_proportions).  Kept apart from the entry points so that the same
// text compiles for the host: tools/wstats_host_check.cpp supplies blockIdx / threadIdx / the vector types / the atomics
// and runs the bodies lane after lane under AddressSanitizer.  Nothing here touches the HIP runtime.
#pragma once
#include <stdint.h>

// ---- work layout -----------------------------------------------------------------------------------------------------
// A workgroup of 256 lanes takes WS_BLOCK = 4096 consecutive voxels of the raveled volume, each of its four waves 1024 of
// them in WS_ITERS = 4 steps of 256: in step k lane j holds the WS_VEC = 4 voxels from wave base + 256 k + 4 j, so one
// load instruction of a wave reads 64 adjacent 16-byte pieces of the labels (and of a float32 operand; a float64 operand
// is two adjacent 16-byte pieces per lane).  A lane keeps ONE open run -- label id and its partial sums -- across its 16
// voxels, which need not be neighbours for that: labels are coherent down the rows as well as along them, and a sum does
// not care.  It issues one set of atomics when the id changes and one at the end; a lane whose four labels are all
// background loads nothing else.  Runs are not merged across the wave (see profiles/weighted_stats_notes.txt).
#define WS_VEC 4
#define WS_ITERS 4
#define WS_WAVE_SPAN (64 * WS_VEC * WS_ITERS)
#define WS_BLOCK (4 * WS_WAVE_SPAN)
#define WS_NONE 0xffffffffffffffffull

// first voxel of (workgroup, lane, step); everything that indexes the volume is 64-bit: 144 x 5424^2 = 4.2e9 voxels
// are beyond int32 and a longer run is beyond 2^32
__host__ __device__ inline int64_t ws_first_voxel(int64_t block, int tid, int step)
{
    return block * WS_BLOCK + (int64_t)(tid >> 6) * WS_WAVE_SPAN + (int64_t)step * (64 * WS_VEC) + (int64_t)(tid & 63) * WS_VEC;
}

// Order-preserving key of a FINITE value: a < b  <=>  key(a) < key(b) as unsigned; -0.0 and +0.0 share a key (x + 0.0
// is +0.0 for both under round-to-nearest), as np.argmin / np.argmax see them.  float -> double is exact.
__host__ __device__ inline unsigned long long ws_key(double x)
{
    union { double d; unsigned long long u; } c;
    c.d = x + 0.0;
    return (c.u >> 63) ? ~c.u : (c.u | 0x8000000000000000ull);
}

__host__ __device__ inline bool ws_finite(double x) { return x - x == 0; }        // false for NaN and +-inf

// four consecutive elements: one 16-byte load (int32, float) or two adjacent ones (double)
__host__ __device__ inline void ws_vload(const int32_t *p, int32_t v[WS_VEC])
{
    const int4 q = *(const int4 *)p;
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__host__ __device__ inline void ws_vload(const float *p, float v[WS_VEC])
{
    const float4 q = *(const float4 *)p;
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__host__ __device__ inline void ws_vload(const uint8_t *p, uint8_t v[WS_VEC])      // tf_label_nanmin's bool field: one 4-byte load
{
    const uchar4 q = *(const uchar4 *)p;
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__host__ __device__ inline void ws_vload(const double *p, double v[WS_VEC])
{
    const double2 a = ((const double2 *)p)[0], b = ((const double2 *)p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}

// elements i .. i + m - 1 of p (m <= 4): vector loads when `vec` (the caller guarantees that p + i is 16-byte aligned
// and m == 4), element loads otherwise; the rest of v is `fill`
template <typename E>
__host__ __device__ inline void ws_load4(const E *__restrict__ p, int64_t i, int m, bool vec, E v[WS_VEC], E fill)
{
    if (vec) { ws_vload(p + i, v); return; }
#pragma unroll
    for (int j = 0; j < WS_VEC; j++) v[j] = j < m ? p[i + j] : fill;
}

// ---- tf_label_wstats -------------------------------------------------------------------------------------------------
// Workspace record per label id (WS_REC doubles = 128 B, id - 1 indexes it):
//   pass 1:  0 n (uint64)   1 sum w   2 sum w^2   3 sum w x   4 sum w^2 e^2   5 key of min x (uint64)   6 key of max x
//   pass 2:  8 sum w (x - mean)^2   9 smallest raveled index with key(x) == key of min (uint64)   10 the same for max
// all over F = the label's voxels with finite x.  Slots 5, 9, 10 start at WS_NONE, everything else at 0.
#define WS_REC 16
#define WS_OUT 10

__device__ inline void ws_init_body(int64_t l, int64_t n_labels, double *acc)
{
    if (l >= n_labels) return;
    unsigned long long *r = (unsigned long long *)(acc + WS_REC * l);
#pragma unroll
    for (int k = 0; k < WS_REC; k++) r[k] = (k == 5 || k == 9 || k == 10) ? WS_NONE : 0ull;   // +0.0 and 0 share their bits
}

// weights: a (T, hw) volume, or with `plane` one (hw,) plane that every frame shares (index i % hw; never materialised)
template <typename F>
__device__ inline void ws_pass1_body(int64_t block, int tid, const int32_t *__restrict__ labels, const F *__restrict__ x,
                                     const F *__restrict__ e, const F *__restrict__ w, int64_t n, int64_t hw, bool plane,
                                     bool vec, bool vec_w, int64_t n_labels, double *acc)
{
    int32_t cur = 0;
    unsigned long long cnt = 0, kmin = WS_NONE, kmax = 0;
    double sw = 0, sww = 0, swx = 0, swe = 0;
    auto flush = [&]() {
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
    };
#pragma unroll
    for (int step = 0; step < WS_ITERS; step++) {
        const int64_t i = ws_first_voxel(block, tid, step);
        if (i >= n) break;
        const int m = n - i < WS_VEC ? (int)(n - i) : WS_VEC;
        const bool full = m == WS_VEC;
        int32_t lv[WS_VEC];
        ws_load4<int32_t>(labels, i, m, vec && full, lv, 0);
        bool any = false;
#pragma unroll
        for (int j = 0; j < WS_VEC; j++) any |= lv[j] >= 1 && lv[j] <= n_labels;
        if (!any) { flush(); cur = 0; cnt = 0; continue; }        // background costs nothing more
        F xv[WS_VEC], wv[WS_VEC], ev[WS_VEC];
        ws_load4<F>(x, i, m, vec && full, xv, (F)0);
        const int64_t iw = plane ? i % hw : i;
        if (plane && iw + m > hw) {                               // the four voxels straddle the end of the plane
#pragma unroll
            for (int j = 0; j < WS_VEC; j++) wv[j] = j < m ? w[(iw + j) % hw] : (F)0;
        } else
            ws_load4<F>(w, iw, m, vec_w && full, wv, (F)0);
        if (e) ws_load4<F>(e, i, m, vec && full, ev, (F)0);
#pragma unroll
        for (int j = 0; j < WS_VEC; j++) {
            const int32_t l = lv[j];
            if (l != cur) {
                flush();
                cur = l; cnt = 0; kmin = WS_NONE; kmax = 0; sw = sww = swx = swe = 0;
            }
            if (l < 1 || l > n_labels) continue;
            const double xd = (double)xv[j];
            if (!ws_finite(xd)) continue;
            const double wd = (double)wv[j], w2 = wd * wd;
            cnt++;
            sw += wd; sww += w2; swx += wd * xd;
            if (e) { const double ed = (double)ev[j]; swe += w2 * (ed * ed); }
            const unsigned long long k = ws_key(xd);
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
        }
    }
    flush();
}

template <typename F>
__device__ inline void ws_pass2_body(int64_t block, int tid, const int32_t *__restrict__ labels, const F *__restrict__ x,
                                     const F *__restrict__ w, int64_t n, int64_t hw, bool plane, bool vec, bool vec_w,
                                     int64_t n_labels, double *acc)
{
    int32_t cur = 0;
    bool valid = false;
    double mean = 0, sv = 0;
    unsigned long long kmin = 0, kmax = 0, imin = WS_NONE, imax = WS_NONE;
    auto flush = [&]() {
        if (!valid) return;
        double *r = acc + WS_REC * (int64_t)(cur - 1);
        unsigned long long *u = (unsigned long long *)r;
        if (sv != 0) atomicAdd(r + 8, sv);
        if (imin < u[9]) atomicMin(u + 9, imin);
        if (imax < u[10]) atomicMin(u + 10, imax);
    };
#pragma unroll
    for (int step = 0; step < WS_ITERS; step++) {
        const int64_t i = ws_first_voxel(block, tid, step);
        if (i >= n) break;
        const int m = n - i < WS_VEC ? (int)(n - i) : WS_VEC;
        const bool full = m == WS_VEC;
        int32_t lv[WS_VEC];
        ws_load4<int32_t>(labels, i, m, vec && full, lv, 0);
        bool any = false;
#pragma unroll
        for (int j = 0; j < WS_VEC; j++) any |= lv[j] >= 1 && lv[j] <= n_labels;
        if (!any) { flush(); cur = 0; valid = false; continue; }
        F xv[WS_VEC], wv[WS_VEC];
        ws_load4<F>(x, i, m, vec && full, xv, (F)0);
        const int64_t iw = plane ? i % hw : i;
        if (plane && iw + m > hw) {
#pragma unroll
            for (int j = 0; j < WS_VEC; j++) wv[j] = j < m ? w[(iw + j) % hw] : (F)0;
        } else
            ws_load4<F>(w, iw, m, vec_w && full, wv, (F)0);
#pragma unroll
        for (int j = 0; j < WS_VEC; j++) {
            const int32_t l = lv[j];
            if (l != cur) {
                flush();
                cur = l; valid = false; sv = 0; imin = imax = WS_NONE;
                if (l >= 1 && l <= n_labels) {                    // what pass 1 left for this label (a finished kernel's writes)
                    const double *r = acc + WS_REC * (int64_t)(l - 1);
                    const unsigned long long *u = (const unsigned long long *)r;
                    const double tw = r[1];
                    valid = u[0] > 0 && tw > 0;                   // false for a NaN sum: the label is NaN throughout
                    mean = r[3] / tw; kmin = u[5]; kmax = u[6];
                }
            }
            if (!valid) continue;
            const double xd = (double)xv[j];
            if (!ws_finite(xd)) continue;
            const double d = xd - mean;
            sv += (double)wv[j] * (d * d);
            const unsigned long long k = ws_key(xd), at = (unsigned long long)(i + j);
            if (k == kmin && at < imin) imin = at;
            if (k == kmax && at < imax) imax = at;
        }
    }
    flush();
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

__device__ inline void wp_pass_body(int64_t block, int tid, const int32_t *__restrict__ labels, const int32_t *__restrict__ flags,
                                    const float *__restrict__ w, int64_t n, int64_t hw, bool plane, bool vec, bool vec_w,
                                    int64_t n_labels, const WpFlags &fl, double *acc)
{
    const int64_t rec = 1 + fl.k;
    int32_t cur = 0, cur_flag = 0;
    int slot = -1;
    bool open = false;
    double s = 0;
    auto flush = [&]() {
        if (!open || s == 0) return;
        double *r = acc + rec * (int64_t)(cur - 1);
        atomicAdd(r, s);
        if (slot >= 0) atomicAdd(r + 1 + slot, s);
    };
#pragma unroll
    for (int step = 0; step < WS_ITERS; step++) {
        const int64_t i = ws_first_voxel(block, tid, step);
        if (i >= n) break;
        const int m = n - i < WS_VEC ? (int)(n - i) : WS_VEC;
        const bool full = m == WS_VEC;
        int32_t lv[WS_VEC], fv[WS_VEC];
        ws_load4<int32_t>(labels, i, m, vec && full, lv, 0);
        bool any = false;
#pragma unroll
        for (int j = 0; j < WS_VEC; j++) any |= lv[j] >= 1 && lv[j] <= n_labels;
        if (!any) { flush(); open = false; cur = 0; continue; }
        float wv[WS_VEC];
        ws_load4<int32_t>(flags, i, m, vec && full, fv, 0);
        const int64_t iw = plane ? i % hw : i;
        if (plane && iw + m > hw) {
#pragma unroll
            for (int j = 0; j < WS_VEC; j++) wv[j] = j < m ? w[(iw + j) % hw] : 0.f;
        } else
            ws_load4<float>(w, iw, m, vec_w && full, wv, 0.f);
#pragma unroll
        for (int j = 0; j < WS_VEC; j++) {
            const int32_t l = lv[j];
            if (l < 1 || l > n_labels) { flush(); open = false; cur = 0; continue; }
            if (!open || l != cur || fv[j] != cur_flag) {
                flush();
                open = true; cur = l; cur_flag = fv[j]; s = 0; slot = -1;
                for (int k = 0; k < fl.k; k++) if (fl.v[k] == cur_flag) slot = k;     // the values are distinct
            }
            const float wf = wv[j];
            if (wf == wf) s += (double)wf;                        // np.nansum: a NaN weight counts nowhere
        }
    }
    flush();
}

__device__ inline void wp_finish_body(int64_t l, int64_t n_labels, int K, const double *__restrict__ acc, double *__restrict__ out)
{
    if (l >= n_labels) return;
    const double *r = acc + (int64_t)(1 + K) * l;
    const double total = r[0];
    for (int k = 0; k < K; k++) out[(int64_t)K * l + k] = total > 0 ? r[1 + k] / total : __builtin_nan("");
}
