// Kernel bodies of fields.hip (tf_stripe_deviation, tf_prepare_fields): the array-level field preparation under the
// reference's loaders (tobac_flow/dataloader.py:234-321, 588-688, 833-958).  Nothing here touches the HIP runtime.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/tobac_flow_hip.h"

#define FK_THREADS 256
#define FK_VEC 8                                                  // voxels per lane of k_prepare_fields
#define FK_COL_VEC 16                                             // columns per lane of k_stripe_columns: one 16-byte load
#define FK_COL_SPAN (64 * FK_COL_VEC)                             // columns per workgroup: every wave covers all of them
#define FK_COL_ROWS 256                                           // rows per workgroup, 64 per wave

__device__ inline bool fk_aligned(const void *p, uintptr_t bytes) { return (((uintptr_t)p) & (bytes - 1)) == 0; }

// one stored 8-bit DQF value as an integer, and whether it is the plane's fill
__device__ inline int fk_dqf_value(uint8_t raw, bool is_signed) { return is_signed ? (int)(int8_t)raw : (int)raw; }

// ---- stripe rows, pass 1: exact column counts and sums------------------------------------------------------------------
// Workgroup (bx, by, t) takes columns [1024 bx, +1024) and rows [256 by, +256) of frame t: lane l of every wave holds
// the 16 columns from 1024 bx + 16 l, wave w the rows 256 by + w, + 4, ...  The count and the sum of the valid elements
// are int32 per lane, combined over the four waves by LDS atomics and added to the (T, W) int64 tables with one 64-bit
// integer atomic per column and table: exact, whatever the order.
struct FkColumns {
    const uint8_t *data; int64_t frame_stride, row_stride; int is_signed, has_fill, fill;
    int64_t H, W;
    unsigned long long *cnt, *sum;                                // (T, W) each, zeroed by the entry point
};

__device__ inline void fk_stripe_columns_body(const FkColumns &p, int bx, int by, int64_t t, int tid, int32_t *sh /* [2][FK_COL_SPAN] */)
{
    for (int i = tid; i < 2 * FK_COL_SPAN; i += FK_THREADS) sh[i] = 0;
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t x0 = (int64_t)bx * FK_COL_SPAN + (int64_t)lane * FK_COL_VEC;
    const int64_t y_begin = (int64_t)by * FK_COL_ROWS, y_end = y_begin + FK_COL_ROWS < p.H ? y_begin + FK_COL_ROWS : p.H;
    if (x0 < p.W) {
        const uint8_t *base = p.data + t * p.frame_stride + x0;
        const int m = p.W - x0 < FK_COL_VEC ? (int)(p.W - x0) : FK_COL_VEC;
        const bool vec = m == FK_COL_VEC && fk_aligned(base, 16) && (p.row_stride & 15) == 0;
        int32_t n[FK_COL_VEC], s1[FK_COL_VEC];
#pragma unroll
        for (int j = 0; j < FK_COL_VEC; j++) n[j] = s1[j] = 0;
        for (int64_t y = y_begin + wave; y < y_end; y += 4) {
            const uint8_t *row = base + y * p.row_stride;
            uint32_t q[4] = {0, 0, 0, 0};
            if (vec) {
                const uint4 v = *(const uint4 *)row;
                q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < FK_COL_VEC; j++)
                    if (j < m) q[j >> 2] |= (uint32_t)row[j] << (8 * (j & 3));
            }
#pragma unroll
            for (int j = 0; j < FK_COL_VEC; j++) {
                const int d = fk_dqf_value((uint8_t)(q[j >> 2] >> (8 * (j & 3))), p.is_signed);
                const bool ok = j < m && !(p.has_fill && d == p.fill);
                n[j] += ok ? 1 : 0;
                s1[j] += ok ? d : 0;
            }
        }
#pragma unroll
        for (int j = 0; j < FK_COL_VEC; j++) {
            if (j >= m || n[j] == 0) continue;
            const int c = lane * FK_COL_VEC + j;
            atomicAdd(&sh[c], n[j]);
            atomicAdd(&sh[FK_COL_SPAN + c], s1[j]);
        }
    }
    __syncthreads();
    for (int c = tid; c < FK_COL_SPAN; c += FK_THREADS) {
        const int64_t x = (int64_t)bx * FK_COL_SPAN + c;
        if (x >= p.W || sh[c] == 0) continue;
        const int64_t at = t * p.W + x;
        atomicAdd(p.cnt + at, (unsigned long long)(int64_t)sh[c]);
        atomicAdd(p.sum + at, (unsigned long long)(int64_t)sh[FK_COL_SPAN + c]);       // two's complement: a negative sum wraps back
    }
}

// ---- stripe rows, pass 2: mean and standard deviation of every column ------------------------------------------------
// mean = sum / n from the exact integers: np.nanmean's value bit for bit, since its float64 sum of small integers is
// exact as well.  The variance is np.nanstd's own second pass, restated operation for operation: (D - mean)^2 rounded
// twice (-ffp-contract=off) and added down the column in row order, which is the order NumPy reduces a middle axis in,
// then / n, sqrt, + 1e-8.  One lane per column; the loads of a batch of rows are independent, the additions are not.
// ((n sum D^2 - (sum D)^2) / n^2 from integer moments is the more accurate value, and for that reason not NumPy's: on a
// 1030-row plane the deviations of the two differ by 2e-14, five times what the order of the row sum accounts for.)
// NaN for an empty column.
struct FkVariance {
    const uint8_t *data; int64_t frame_stride, row_stride; int is_signed, has_fill, fill;
    int64_t H, W, n_cols;                                         // n_cols = T W
    const unsigned long long *cnt, *sum;
    double *mean, *denom;                                         // (T, W)
};

__device__ inline void fk_stripe_variance_body(const FkVariance &p, int64_t i)
{
    if (i >= p.n_cols) return;
    const int64_t n = (int64_t)p.cnt[i];
    if (n == 0) { p.mean[i] = p.denom[i] = (double)NAN; return; }
    const int64_t t = i / p.W, x = i - t * p.W;
    const double dn = (double)n, mean = (double)(int64_t)p.sum[i] / dn;
    const uint8_t *col = p.data + t * p.frame_stride + x;
    double acc = 0;
#pragma unroll 8
    for (int64_t y = 0; y < p.H; y++) {
        const int d = fk_dqf_value(col[y * p.row_stride], p.is_signed);
        const double diff = (double)d - mean, sqr = diff * diff;
        if (!(p.has_fill && d == p.fill)) acc += sqr;             // NumPy adds 0.0 for a NaN element: the same sum
    }
    p.mean[i] = mean;
    p.denom[i] = sqrt(acc / dn) + 1e-8;
}

// ---- stripe rows, pass 3: the deviation of one row -------------------------------------------------------------------
// One workgroup per (t, y).  Lane l sums the terms (D - mean[x]) / denom[x] of x = 4 l .. 4 l + 3, then + 1024, ... in
// that order in float64, the 256 partial sums meet in a fixed tree: the same value in every run.
struct FkRows {
    const uint8_t *data; int64_t frame_stride, row_stride; int is_signed, has_fill, fill;
    int64_t H, W;
    const double *mean, *denom;                                   // (T, W)
    double threshold;
    double *dev; uint8_t *row_flags;                              // (T, H), optional each
};

__device__ inline void fk_stripe_rows_body(const FkRows &p, int64_t row_id, int tid, double *sh_sum, int32_t *sh_cnt)
{
    const int64_t t = row_id / p.H, y = row_id - t * p.H;
    const uint8_t *row = p.data + t * p.frame_stride + y * p.row_stride;
    const double *mean = p.mean + t * p.W, *denom = p.denom + t * p.W;
    const bool vec = fk_aligned(row, 4);
    double acc = 0;
    int32_t cnt = 0;
    for (int64_t x = (int64_t)tid * 4; x < p.W; x += FK_THREADS * 4) {
        const int m = p.W - x < 4 ? (int)(p.W - x) : 4;
        uint32_t q = 0;
        if (vec && m == 4) q = *(const uint32_t *)(row + x);
        else
            for (int j = 0; j < m; j++) q |= (uint32_t)row[x + j] << (8 * j);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (j >= m) continue;
            const int d = fk_dqf_value((uint8_t)(q >> (8 * j)), p.is_signed);
            if (p.has_fill && d == p.fill) continue;
            const double term = ((double)d - mean[x + j]) / denom[x + j];    // a valid element: its column is not empty
            acc += term;
            cnt++;
        }
    }
    sh_sum[tid] = acc; sh_cnt[tid] = cnt;
    __syncthreads();
    for (int s = FK_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) { sh_sum[tid] += sh_sum[tid + s]; sh_cnt[tid] += sh_cnt[tid + s]; }
        __syncthreads();
    }
    if (tid != 0) return;
    const double dev = sh_cnt[0] ? fabs(sh_sum[0] / (double)sh_cnt[0]) : (double)NAN;
    if (p.dev) p.dev[row_id] = dev;
    if (p.row_flags && dev > p.threshold) p.row_flags[row_id] = 1;
}

// ---- the fused preparation -------------------------------------------------------------------------------------------
// Workgroup b of output frame k takes 2048 voxels of the frame, lane l the eight from 8 (256 b + l) - e, where
// e = (k H W) mod 4: the eight are 16-byte aligned in the contiguous outputs whatever H W is.  A group may straddle rows
// (odd W) and is clipped at both ends of the frame; an input is read with vector loads (16 bytes of a packed channel,
// 2 x 16 of a float32 one, 8 of a DQF plane) where the eight voxels lie in one row and their address is aligned, element
// by element otherwise.  Everything that indexes the stack is 64-bit.

// where a lane's voxels lie in the input frame: (y, x) per voxel, `here` for those inside the frame; `row`: all eight
// are there and share the row y[0]
struct FkGroup { int32_t y[FK_VEC], x[FK_VEC]; bool here[FK_VEC], row; };

__device__ inline int64_t fk_at(const TfFieldPlane &c, int64_t src, const FkGroup &g, int j)
{
    return src * c.frame_stride + (int64_t)g.y[j] * c.row_stride + g.x[j];
}

// eight decoded values of one channel of input frame `src`
template <bool PACKED>
__device__ inline void fk_load_channel(const TfFieldPlane &c, int64_t src, const FkGroup &g, float v[FK_VEC])
{
    if (PACKED) {
        const uint16_t *p = (const uint16_t *)c.data;
        uint32_t raw[FK_VEC];
        if (g.row && fk_aligned(p + fk_at(c, src, g, 0), 16)) {
            const uint4 q = *(const uint4 *)(p + fk_at(c, src, g, 0));
            raw[0] = q.x & 0xffffu; raw[1] = q.x >> 16; raw[2] = q.y & 0xffffu; raw[3] = q.y >> 16;
            raw[4] = q.z & 0xffffu; raw[5] = q.z >> 16; raw[6] = q.w & 0xffffu; raw[7] = q.w >> 16;
        } else {
#pragma unroll
            for (int j = 0; j < FK_VEC; j++) raw[j] = g.here[j] ? p[fk_at(c, src, g, j)] : 0;
        }
#pragma unroll
        for (int j = 0; j < FK_VEC; j++) {
            const int stored = c.is_unsigned ? (int)raw[j] : (int)(int16_t)raw[j];
            const float x = (float)stored * c.scale + c.offset;   // two roundings: -ffp-contract=off
            v[j] = c.has_fill && stored == c.fill ? NAN : x;
        }
    } else {
        const float *p = (const float *)c.data;
        if (g.row && fk_aligned(p + fk_at(c, src, g, 0), 16)) {
            const float4 q0 = ((const float4 *)(p + fk_at(c, src, g, 0)))[0], q1 = ((const float4 *)(p + fk_at(c, src, g, 0)))[1];
            v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w; v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
        } else {
#pragma unroll
            for (int j = 0; j < FK_VEC; j++) v[j] = g.here[j] ? p[fk_at(c, src, g, j)] : NAN;
        }
    }
}

// OR of "flagged or fill" over the eight voxels of one DQF plane
__device__ inline void fk_load_dqf(const TfFieldPlane &c, int64_t src, const FkGroup &g, bool bad[FK_VEC])
{
    const uint8_t *p = (const uint8_t *)c.data;
    uint32_t q[2] = {0, 0};
    if (g.row && fk_aligned(p + fk_at(c, src, g, 0), 8)) {
        const uint2 v = *(const uint2 *)(p + fk_at(c, src, g, 0));
        q[0] = v.x; q[1] = v.y;
    } else {
#pragma unroll
        for (int j = 0; j < FK_VEC; j++) q[j >> 2] |= (g.here[j] ? (uint32_t)p[fk_at(c, src, g, j)] : 0u) << (8 * (j & 3));
    }
    // non-zero covers a fill as well unless the fill is 0: np.any is true for the NaN a fill decodes to
#pragma unroll
    for (int j = 0; j < FK_VEC; j++) {
        const int d = fk_dqf_value((uint8_t)(q[j >> 2] >> (8 * (j & 3))), c.dtype == TF_I8);
        bad[j] = bad[j] || d != 0 || (c.has_fill && d == c.fill);
    }
}

template <bool PACKED, bool HAS_DQF>
__device__ inline void fk_prepare_body(const TfFieldPrep &p, int64_t k, int64_t block, int tid, int32_t *sh_cnt)
{
    const int64_t HW = p.H * p.W;
    const int e = (int)(((k & 3) * (HW & 3)) & 3);
    const int64_t lo = FK_VEC * (block * FK_THREADS + tid) - e;   // first voxel of the lane within the frame, may be < 0
    const int64_t out_at = k * HW + lo;
    const int64_t src = p.src[k] < p.T ? p.src[k] : -1;           // a frame that is not there is a NaN frame, never a read
    FkGroup g;
#pragma unroll
    for (int j = 0; j < FK_VEC; j++) g.here[j] = lo + j >= 0 && lo + j < HW;
    const bool full = g.here[0] && g.here[FK_VEC - 1];
    int masked = 0;
    float out[TF_FIELD_MAX_RECIPES][FK_VEC];
    bool bad[FK_VEC];
#pragma unroll
    for (int j = 0; j < FK_VEC; j++) bad[j] = src < 0;
    const bool copy = (p.flags & TF_FIELD_COPY) != 0;
    if (src >= 0 && lo < HW && lo + FK_VEC > 0) {
        // (y, x) of every voxel: one division, then a walk
        const int32_t first = lo < 0 ? 0 : (int32_t)lo, W = (int32_t)p.W;
        int32_t y = first / W, x = first - y * W;
#pragma unroll
        for (int j = 0; j < FK_VEC; j++) {
            g.y[j] = y; g.x[j] = x;
            if (lo + j >= 0) { x++; if (x == W) { x = 0; y++; } }
        }
        g.row = full && g.y[0] == g.y[FK_VEC - 1];
        float a[FK_VEC], b[FK_VEC];
#pragma unroll
        for (int r = 0; r < TF_FIELD_MAX_RECIPES; r++) {
            if (r >= p.n_recipes) continue;
            const TfFieldRecipe &rc = p.recipe[r];
            fk_load_channel<PACKED>(p.channel[rc.a], src, g, a);
            if (rc.b >= 0) fk_load_channel<PACKED>(p.channel[rc.b], src, g, b);
#pragma unroll
            for (int j = 0; j < FK_VEC; j++) {
                float v = rc.b >= 0 ? a[j] - b[j] : a[j];
                if (rc.has_floor) v = v < rc.floor ? rc.floor : v;        // np.maximum(v, floor): NaN stays NaN
                out[r][j] = v;
                bad[j] = bad[j] || (!copy && !(v - v == 0));      // NaN, +inf, -inf
            }
        }
        if (HAS_DQF) {
            for (int d = 0; d < p.n_dqf; d++) fk_load_dqf(p.dqf[d], src, g, bad);
            if (p.row_flags) {
                const uint8_t *flags = p.row_flags + src * p.H;
                if (g.row) {
                    const bool stripe = flags[g.y[0]] != 0;
#pragma unroll
                    for (int j = 0; j < FK_VEC; j++) bad[j] = bad[j] || stripe;
                } else {
#pragma unroll
                    for (int j = 0; j < FK_VEC; j++)
                        if (g.here[j] && flags[g.y[j]]) bad[j] = true;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < FK_VEC; j++) masked += g.here[j] && bad[j] ? 1 : 0;
#pragma unroll
    for (int r = 0; r < TF_FIELD_MAX_RECIPES; r++) {
        if (r >= p.n_recipes) continue;
        float *o = p.recipe[r].out + out_at;
        float v[FK_VEC];
#pragma unroll
        for (int j = 0; j < FK_VEC; j++) v[j] = bad[j] ? NAN : out[r][j];
        if (full && fk_aligned(o, 16)) {
            ((float4 *)o)[0] = make_float4(v[0], v[1], v[2], v[3]);
            ((float4 *)o)[1] = make_float4(v[4], v[5], v[6], v[7]);
        } else {
#pragma unroll
            for (int j = 0; j < FK_VEC; j++)
                if (g.here[j]) o[j] = v[j];
        }
    }
    // one integer atomic per workgroup
    for (int s = 32; s > 0; s >>= 1) masked += __shfl_down(masked, s, 64);
    if ((tid & 63) == 0) sh_cnt[tid >> 6] = masked;
    __syncthreads();
    if (tid == 0 && p.n_masked) {
        const int total = sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
        if (total) atomicAdd(p.n_masked + k, total);
    }
}
