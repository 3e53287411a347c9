// Kernel body of binning.hip (tf_bin_points).  Kept apart from the entry point so that the same text compiles for the
// host: tools/bin_host_check.cpp supplies the vector types and the atomics and runs the body lane after lane under
// AddressSanitizer.  Nothing here touches the HIP runtime.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/tobac_flow_hip.h"
#include "label_runs.h"                                           // the raveled work layout, lr_load4, lr_aligned16

// ---- work layout -----------------------------------------------------------------------------------------------------
// The raveled layout of label_runs.h with points for voxels: a workgroup of 256 lanes takes LR_BLOCK = 4096 consecutive
// points, lane j of a wave the LR_VEC = 4 points from wave base + 256 k + 4 j in step k (lr_first_voxel).  A lane keeps
// ONE open run -- the (frame range, bin) of its last kept point and the partial count / sums -- across its 16 points and
// issues one set of atomics per frame of the range when the key changes and at the end.  Neighbouring pixels of a swath
// mostly share a bin; scattered points do not, and then every point costs its atomics (profiles/point_binning.txt).

// four consecutive int64: two adjacent 16-byte loads (little endian)
__host__ __device__ inline void bn_load4_i64(const int64_t *__restrict__ p, int64_t i, int m, bool vec, int64_t v[LR_VEC])
{
    if (vec) {
        const int4 a = ((const int4 *)(p + i))[0], b = ((const int4 *)(p + i))[1];
        v[0] = (int64_t)(((uint64_t)(uint32_t)a.y << 32) | (uint32_t)a.x);
        v[1] = (int64_t)(((uint64_t)(uint32_t)a.w << 32) | (uint32_t)a.z);
        v[2] = (int64_t)(((uint64_t)(uint32_t)b.y << 32) | (uint32_t)b.x);
        v[3] = (int64_t)(((uint64_t)(uint32_t)b.w << 32) | (uint32_t)b.z);
        return;
    }
#pragma unroll
    for (int j = 0; j < LR_VEC; j++) v[j] = j < m ? p[i + j] : 0;
}

// np.around(v, decimals) in the type of v: multiply by 10^d, rint, divide for d > 0; divide, rint, multiply for d < 0
// (`scale` = 10^|d|, which NumPy converts to the array's type first).  Every operation rounds once: -ffp-contract=off.
__host__ __device__ inline double bn_around(double v, int decimals, double scale)
{
    if (decimals > 0) return rint(v * scale) / scale;
    if (decimals < 0) return rint(v / scale) * scale;
    return rint(v);
}
__host__ __device__ inline float bn_around(float v, int decimals, double scale)
{
    const float s = (float)scale;
    if (decimals > 0) return rintf(v * s) / s;
    if (decimals < 0) return rintf(v / s) * s;
    return rintf(v);
}

// np.searchsorted(a, t, side="right") of a non-decreasing int64 array
__host__ __device__ inline int64_t bn_upper_bound(const int64_t *__restrict__ a, int64_t n, int64_t t)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// what a lane needs of one axis: read once from the edge array
struct BnAxis { const double *e; int64_t ne; double e0, el, inv; int decimals; double scale; };

__host__ __device__ inline BnAxis bn_axis(const TfBinPoints &p, int d)
{
    BnAxis a;
    a.e = p.edges[d]; a.ne = p.n_edges[d];
    a.e0 = a.e[0]; a.el = a.e[a.ne - 1];
    a.inv = (double)(a.ne - 1) / (a.el - a.e0);                    // only a guess is made from it: any value will do
    a.decimals = p.decimals[d]; a.scale = p.round_scale[d];
    return a;
}

// The bin of one coordinate: k = searchsorted(e, v, side="right") - 1 where 0 <= k < ne - 1, with the last-edge rule of
// `rule`; -1 for a point that the axis drops (below e[0], beyond the last edge, NaN).  For e[0] <= v < e[ne - 1] the
// answer is THE k with e[k] <= v < e[k + 1] (unique for non-decreasing edges, zero-width bins included): a guess from
// the mean step is moved by up to two bins and kept only if it satisfies that; otherwise the binary search decides.
// Every index stays inside [0, ne - 1] whatever the edges hold: v >= e[0] stops the walk down, v < e[ne - 1] the walk up.
// `differ` is set where the SciPy rule and NumPy's disagree about the point.
template <typename C>
__host__ __device__ inline int64_t bn_axis_bin(C vc, const BnAxis &a, int rule, bool &differ)
{
    const double v = (double)vc;                                  // float -> double is exact, as np.searchsorted widens
    if (!(v >= a.e0)) return -1;                                  // below the first edge, -inf, NaN
    if (v >= a.el) {
        if (rule == TF_BIN_RULE_NUMPY) return v == a.el ? a.ne - 2 : -1;
        // SciPy rounds the point and the edge in the SAMPLE's type (it casts the edges to float32 for float32 samples)
        const bool kept = bn_around(vc, a.decimals, a.scale) == bn_around((C)a.el, a.decimals, a.scale);
        differ = differ || kept != (v == a.el);
        return kept ? a.ne - 2 : -1;
    }
    const double g = (v - a.e0) * a.inv;
    int64_t k = g >= 0 && g < (double)(a.ne - 1) ? (int64_t)g : 0;
    if (k > a.ne - 2) k = a.ne - 2;
    for (int s = 0; s < 2 && v < a.e[k]; s++) k--;
    for (int s = 0; s < 2 && v >= a.e[k + 1]; s++) k++;
    if (a.e[k] <= v && v < a.e[k + 1]) return k;
    int64_t lo = 0, hi = a.ne;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a.e[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

__host__ __device__ inline void bn_load4_real(const void *__restrict__ p, int dtype, int64_t i, int m, bool vec, float f[LR_VEC],
                                              double d[LR_VEC])
{
    if (dtype == TF_F32) {
        lr_load4<float>((const float *)p, i, m, vec, f, 0.f);
#pragma unroll
        for (int j = 0; j < LR_VEC; j++) d[j] = (double)f[j];
    } else {
        lr_load4<double>((const double *)p, i, m, vec, d, 0.0);
#pragma unroll
        for (int j = 0; j < LR_VEC; j++) f[j] = 0.f;
    }
}

// C: the coordinates' type.  Every output is accumulated into; flat indices are 64-bit (144 x 5424^2 bins > 2^32).
template <typename C>
__device__ inline void bn_points_body(int64_t block, int tid, const TfBinPoints &p)
{
    const int nd = p.n_dims;
    const int64_t n = p.n_points;
    BnAxis ax[TF_BIN_MAX_DIMS];
    int64_t n_bins = 1;
    bool vec_c = true;
#pragma unroll
    for (int d = 0; d < TF_BIN_MAX_DIMS; d++) {                    // unrolled with a guard: ax[] and cv[] stay in registers
        if (d >= nd) continue;
        ax[d] = bn_axis(p, d);
        n_bins *= ax[d].ne - 1;
        vec_c = vec_c && lr_aligned16(p.coord[d]);
    }
    const bool scipy = p.rule == TF_BIN_RULE_SCIPY, finite_value = (p.flags & TF_BIN_FINITE_VALUE) != 0;
    const bool want_value = p.count_v || p.sum_w || p.sum_wv;
    const bool f32_product = p.value && p.value_dtype == TF_F32 && !(p.weight && p.weight_dtype == TF_F64);
    const bool vec_keep = lr_aligned16(p.keep), vec_kv = lr_aligned16(p.keep_value), vec_t = lr_aligned16(p.time);
    const bool vec_v = lr_aligned16(p.value), vec_w = lr_aligned16(p.weight);

    int64_t cur_bin = -1, cur_f0 = 0, cur_f1 = 0;
    int32_t cnt = 0, cnt_v = 0;
    double sw = 0, swv = 0;
    uint32_t status = 0;
    auto flush = [&]() {
        if (cur_bin < 0 || (cnt == 0 && cnt_v == 0)) return;
        for (int64_t f = cur_f0; f < cur_f1; f++) {
            const int64_t at = f * n_bins + cur_bin;
            if (p.count && cnt) atomicAdd(p.count + at, cnt);
            if (!cnt_v) continue;
            if (p.count_v) atomicAdd(p.count_v + at, cnt_v);
            if (p.sum_w) atomicAdd(p.sum_w + at, sw);
            if (p.sum_wv) atomicAdd(p.sum_wv + at, swv);
        }
    };
#pragma unroll 1
    for (int step = 0; step < LR_ITERS; step++) {
        const int64_t i = lr_first_voxel(block, tid, step);
        if (i >= n) break;
        const int m = n - i < LR_VEC ? (int)(n - i) : LR_VEC;
        const bool full = m == LR_VEC;
        uint8_t kp[LR_VEC] = {1, 1, 1, 1}, kv[LR_VEC] = {1, 1, 1, 1};
        if (p.keep) {
            lr_load4<uint8_t>(p.keep, i, m, vec_keep && full, kp, (uint8_t)0);
            if (!(kp[0] | kp[1] | kp[2] | kp[3])) continue;       // nothing kept: the open run stays open
        }
        C cv[TF_BIN_MAX_DIMS][LR_VEC];
#pragma unroll
        for (int d = 0; d < TF_BIN_MAX_DIMS; d++)
            if (d < nd) lr_load4<C>((const C *)p.coord[d], i, m, vec_c && full, cv[d], (C)0);
        int64_t tv[LR_VEC] = {0, 0, 0, 0};
        if (p.time) bn_load4_i64(p.time, i, m, vec_t && full, tv);
        float vf[LR_VEC] = {0.f, 0.f, 0.f, 0.f}, wf[LR_VEC] = {1.f, 1.f, 1.f, 1.f};
        double vd[LR_VEC] = {0, 0, 0, 0}, wd[LR_VEC] = {1, 1, 1, 1};
        if (want_value) {
            if (p.keep_value) lr_load4<uint8_t>(p.keep_value, i, m, vec_kv && full, kv, (uint8_t)0);
            if (p.value) bn_load4_real(p.value, p.value_dtype, i, m, vec_v && full, vf, vd);
            if (p.weight) bn_load4_real(p.weight, p.weight_dtype, i, m, vec_w && full, wf, wd);
        }
#pragma unroll
        for (int j = 0; j < LR_VEC; j++) {
            if (j >= m || !kp[j]) continue;
            int64_t f0 = 0, f1 = 1;
            if (p.time) {                                         // win_start[f] <= t < win_end[f]: a contiguous range of frames
                f0 = bn_upper_bound(p.win_end, p.n_frames, tv[j]);
                f1 = bn_upper_bound(p.win_start, p.n_frames, tv[j]);
                if (f0 >= f1) continue;
            }
            int64_t bin = 0;
            bool inside = true, finite = true, differ = false;
#pragma unroll
            for (int d = 0; d < TF_BIN_MAX_DIMS; d++) {
                if (d >= nd) continue;
                const C c = cv[d][j];
                finite = finite && (c - c == 0);
                const int64_t k = bn_axis_bin<C>(c, ax[d], p.rule, differ);
                inside = inside && k >= 0;
                const int64_t nb = ax[d].ne - 1;
                bin = bin * nb + (k < 0 ? 0 : ((p.flip_mask >> d) & 1) ? nb - 1 - k : k);
            }
            bool with_value = want_value && kv[j];
            if (with_value && p.value && !lr_finite(vd[j])) {
                if (finite_value) with_value = false;
                else if (scipy) { status |= TF_BIN_STATUS_VALUE; continue; }
            }
            if (!p.count && !with_value) continue;                // nothing left that this point could add to
            if (scipy && !finite) { status |= TF_BIN_STATUS_COORD; continue; }
            if (differ) status |= TF_BIN_STATUS_RULES_DIFFER;
            if (!inside) continue;
            if (bin != cur_bin || f0 != cur_f0 || f1 != cur_f1) {
                flush();
                cur_bin = bin; cur_f0 = f0; cur_f1 = f1; cnt = cnt_v = 0; sw = swv = 0;
            }
            cnt++;
            if (with_value) {
                cnt_v++;
                sw += wd[j];
                // the product in NumPy's result type of the two operands: float32 * float32 rounds in float32
                swv += f32_product ? (double)(vf[j] * wf[j]) : vd[j] * wd[j];
            }
        }
    }
    flush();
    if (status && p.status) atomicOr(p.status, status);
}
