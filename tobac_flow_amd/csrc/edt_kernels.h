// Kernel bodies of edt.hip (tf_edt2d_frames, tf_edt_cylinder, tf_edt_time_envelope, tf_label_nanmin).  Kept apart from the
// entry points so that the same text compiles for the host: tools/edt_host_check.cpp supplies the vector types and the
// atomics and runs the bodies lane after lane under AddressSanitizer.  Nothing here touches the HIP runtime.
#pragma once
#include <stdint.h>
#include "label_runs.h"                                           // lr_key, the raveled work layout and its walker

// ---- tf_edt2d_frames ---------------------------------------------------------------------------------------------------
// Exact squared Euclidean distance to the nearest feature (voxel != 0; NaN != 0, so NaN is one) of the same frame, in
// integers throughout.  Two passes over a chunk of frames:
//   columns  one lane per (frame, x): down the rows, then up; fy[y][x] = row of the nearest feature of column x (the upper
//            one where the one above and the one below are equally far), -1 where the column has none
//   rows     one workgroup per (frame, y): sq[x] = (y - fy[y][x])^2 (EDT_NONE for -1) goes to LDS; the lane of output x
//            starts from best = sq[x] and walks dx = 1, 2, .. outward, x - dx before x + dx, taking a candidate only where
//            dx^2 + sq[x -+ dx] < best, until dx^2 >= best (nothing further out can be nearer) or both sides are outside
// The scan order fixes which of several equally near features is returned: the one with the smallest |x' - x|, of two at
// the same |x' - x| the left one, and within a column the upper one.
// (H - 1)^2 + (W - 1)^2 < 2^31 is required, so every distance fits int32 and dx^2 + sq fits uint32; 2^31 - 1 is prime and
// = 3 mod 4, hence no sum of two squares: EDT_NONE is no distance.
#define EDT_NONE 0x7fffffff
#define EDT_LDS_MAX_W 16384                                       // 64 KiB of sq[] per workgroup; wider rows keep sq[] in the workspace

template <typename E>
__device__ inline void edt_cols_body(int64_t x, int64_t t, const E *__restrict__ vol, int64_t H, int64_t W, int32_t *__restrict__ fy)
{
    if (x >= W) return;
    const E *v = vol + t * H * W + x;
    int32_t *f = fy + t * H * W + x;
    int32_t last = -1;
#pragma unroll 8
    for (int64_t y = 0; y < H; y++) {
        if (v[y * W] != (E)0) last = (int32_t)y;
        f[y * W] = last;
    }
    int32_t next = -1;
    for (int64_t y = H - 1; y >= 0; y--) {
        const int32_t up = f[y * W];
        if (up == (int32_t)y) next = up;                          // a feature
        else if (next >= 0 && (up < 0 || next - (int32_t)y < (int32_t)y - up)) f[y * W] = next;
    }
}

// returns whether this lane met a column with a feature.  No lane of the row's workgroup does exactly when the FRAME has no
// feature (fy is -1 down a whole column or nowhere in it): the row is then filled by edt_row_empty_body, not scanned --
// the scan would walk every pixel to the end of its row and find nothing
__device__ inline bool edt_row_load_body(int tid, int lanes, const int32_t *__restrict__ fy_row, int32_t y, int64_t W, uint32_t *sq)
{
    bool any = false;
    for (int64_t x = tid; x < W; x += lanes) {
        const int32_t f = fy_row[x];
        any |= f >= 0;
        sq[x] = f < 0 ? (uint32_t)EDT_NONE : (uint32_t)((y - f) * (y - f));
    }
    return any;
}

__device__ inline void edt_row_empty_body(int tid, int lanes, int64_t W, int32_t *__restrict__ d2_row, int32_t *__restrict__ nearest_row)
{
    for (int64_t x = tid; x < W; x += lanes) {
        d2_row[x] = EDT_NONE;
        if (nearest_row) nearest_row[x] = -1;
    }
}

// nearest_row may be null.  Reads all of sq[], writes d2_row[x] and nearest_row[x] of this lane's x only.
__device__ inline void edt_row_scan_body(int tid, int lanes, const uint32_t *sq, const int32_t *__restrict__ fy_row, int64_t W,
                                         int32_t *__restrict__ d2_row, int32_t *__restrict__ nearest_row)
{
    const int32_t w = (int32_t)W;
    for (int32_t x = tid; x < w; x += lanes) {
        uint32_t best = sq[x];
        int32_t bx = x;
        const int32_t reach = x > w - 1 - x ? x : w - 1 - x;
        for (int32_t dx = 1; dx <= reach; dx++) {
            const uint32_t dd = (uint32_t)dx * (uint32_t)dx;
            if (dd >= best) break;
            if (x - dx >= 0) {
                const uint32_t c = dd + sq[x - dx];
                if (c < best) { best = c; bx = x - dx; }
            }
            if (x + dx < w) {
                const uint32_t c = dd + sq[x + dx];
                if (c < best) { best = c; bx = x + dx; }
            }
        }
        d2_row[x] = (int32_t)best;
        if (nearest_row) nearest_row[x] = best == (uint32_t)EDT_NONE ? -1 : (int32_t)((int64_t)fy_row[bx] * W + bx);
    }
}

// ---- tf_edt_cylinder ---------------------------------------------------------------------------------------------------
// tobac_flow/validation.py:52-104: per voxel the smallest d2 over the frames t - tm .. t + tm, the earliest frame where
// several hold it (np.nanargmin returns the first), its square root as a double, and with `src` the raveled index into
// the volume of that frame's nearest feature.  0 <= tm <= T (the entry point clamps it).
__device__ inline void edt_cyl_body(int64_t i, int64_t T, int64_t hw, int64_t tm, const int32_t *__restrict__ d2,
                                    const int32_t *__restrict__ nearest, double *__restrict__ dist, int64_t *__restrict__ src)
{
    if (i >= T * hw) return;
    const int64_t t = i / hw, p = i - t * hw;
    const int64_t lo = t - tm > 0 ? t - tm : 0, hi = t + tm < T - 1 ? t + tm : T - 1;
    int32_t best = EDT_NONE;
    int64_t bt = -1;
    for (int64_t k = lo; k <= hi; k++) {
        const int32_t v = d2[k * hw + p];
        if (v < best) { best = v; bt = k; }
    }
    dist[i] = bt < 0 ? (double)__builtin_inf() : sqrt((double)best);
    if (src) src[i] = bt < 0 ? -1 : bt * hw + (int64_t)nearest[bt * hw + p];
}

// ---- tf_edt_time_envelope ----------------------------------------------------------------------------------------------
// scipy.ndimage.distance_transform_edt(..., sampling=(s, 1, 1)) of a (T, H, W) volume from the per-frame transform: the
// squared distance (s dt)^2 + dy^2 + dx^2 is smallest, for a fixed frame, at that frame's nearest in-plane feature, so the
// 3-D transform is the lower envelope along t of (s dt)^2 + d2[k].  In float64, for output voxel (t, y, x) and frame k:
//   a = fl((double)(k - t) * s), A = fl(a * a), key_k = fl(A + (double)d2[k][p])
// The winner is the k of the smallest key; of equal keys the one with the smaller |k - t|, then the earlier frame.  The
// distance is SciPy's own expression for the winner's feature (the axis differences times their sampling, squared, summed in
// axis order, one square root): sqrt(fl(fl(A + dy * dy) + dx * dx)).  Without `nearest` there is no (dy, dx) and the
// distance is sqrt(key), which is NOT SciPy's summation order.  No product or sum here may be contracted into an FMA (the
// library is built with -ffp-contract=off).
// One lane per pixel p, looping over t: per t it looks at dt = 0, -1, +1, -2, +2, .. and stops at the first |dt| whose A is
// no smaller than the best key (key_k >= A_k, and A does not decrease with |dt|) or that leaves the volume on both sides.
// A wave re-reads its own T x 256 B of d2 from cache; `nearest` is read at the winners only.  hw = H * W < 2^31.
__device__ inline void edt_env_body(int64_t p, int64_t T, int64_t hw, int32_t W, double s, const int32_t *__restrict__ d2,
                                    const int32_t *__restrict__ nearest, double *__restrict__ dist, int64_t *__restrict__ src)
{
    if (p >= hw) return;
    const int32_t y = (int32_t)(p / W), x = (int32_t)(p - (int64_t)y * W);
    const int32_t *col = d2 + p;
    for (int64_t t = 0; t < T; t++) {
        double best = (double)__builtin_inf();
        int64_t bk = -1;
        const int32_t v0 = col[t * hw];
        if (v0 != EDT_NONE) { best = (double)v0; bk = t; }        // A = 0: the key is d2 itself
        const int64_t reach = t > T - 1 - t ? t : T - 1 - t;
        for (int64_t d = 1; d <= reach; d++) {
            const double a = (double)d * s, A = a * a;            // (-d * s)^2 is the same number
            if (bk >= 0 && A >= best) break;
            const int64_t lo = t - d, hi = t + d;
            const int32_t vl = lo >= 0 ? col[lo * hw] : EDT_NONE, vh = hi < T ? col[hi * hw] : EDT_NONE;
            if (vl != EDT_NONE) {
                const double key = A + (double)vl;
                if (bk < 0 || key < best) { best = key; bk = lo; }    // bk < 0: a key that overflowed to inf still is a feature
            }
            if (vh != EDT_NONE) {
                const double key = A + (double)vh;
                if (bk < 0 || key < best) { best = key; bk = hi; }
            }
        }
        const int64_t i = t * hw + p;
        if (bk < 0) {
            dist[i] = (double)__builtin_inf();
            if (src) src[i] = -1;
        } else if (!nearest) {
            dist[i] = sqrt(best);
        } else {
            const int32_t n = nearest[bk * hw + p], fy = n / W, fx = n - fy * W;
            const double a = (double)(bk - t) * s, dy = (double)(fy - y), dx = (double)(fx - x);
            dist[i] = sqrt((a * a + dy * dy) + dx * dx);
            if (src) src[i] = bk * hw + (int64_t)n;
        }
    }
}

// ---- tf_label_nanmin ---------------------------------------------------------------------------------------------------
// Record per label id (id - 1 indexes it): [0] the smallest lr_key of the label's non-NaN values, LM_ALLNAN where it has
// voxels and all are NaN, LR_NONE where it has none; [1] the number of its non-NaN voxels.  The work layout is the
// raveled one of label_runs.h, walked by its lr_walk: a lane keeps one open run over its 16 voxels and issues one
// atomicMin (skipped where the record already holds a smaller key) and one atomicAdd per run that ends inside them; the
// runs still open at the end are combined across the wave where its lanes agree on the label (lm_flush_wave).  Every real
// key, +inf's included, is below LM_ALLNAN.
#define LM_REC 2
#define LM_ALLNAN (LR_NONE - 1)

__device__ inline void lm_init_body(int64_t l, int64_t n_labels, unsigned long long *acc)
{
    if (l >= n_labels) return;
    acc[LM_REC * l] = LR_NONE;
    acc[LM_REC * l + 1] = 0;
}

__device__ inline void lm_flush(int32_t cur, unsigned long long kmin, unsigned long long cnt, unsigned long long *acc)
{
    if (kmin == LR_NONE) return;                                  // cur is in [1, n_labels] whenever a voxel was met
    unsigned long long *r = acc + LM_REC * (int64_t)(cur - 1);
    if (r[0] > kmin) atomicMin(r, kmin);                          // a stale read only costs a redundant atomic
    if (cnt) atomicAdd(r + 1, cnt);
}

// The run a lane still holds after its 16 voxels.  Inside a region every lane of a wave ends with the same label: the
// wave then combines its 64 runs (minimum of the keys, sum of the counts, both independent of order) and lane 0 issues
// the two atomics for all of them.  Where the lanes' labels differ each lane flushes its own run.  Every lane of the
// workgroup reaches this call (the body has no early return).  The host build has no wave: each lane flushes.
__device__ inline void lm_flush_wave(int tid, int32_t cur, unsigned long long kmin, unsigned long long cnt, unsigned long long *acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const bool has = kmin != LR_NONE;
    int32_t top = has ? cur : 0;                                  // labels are >= 1
    for (int o = 32; o; o >>= 1) {
        const int32_t v = __shfl_xor(top, o);
        top = v > top ? v : top;
    }
    if (top && __all(!has || cur == top)) {
        if (!has) cnt = 0;
        for (int o = 32; o; o >>= 1) {
            const unsigned long long k = __shfl_xor(kmin, o), c = __shfl_xor(cnt, o);
            kmin = k < kmin ? k : kmin;
            cnt += c;
        }
        if (tid & 63) return;
        cur = top;
    }
#endif
    lm_flush(cur, kmin, cnt, acc);
}

template <typename F>
struct LmPass {
    const F *__restrict__ x; bool vec; unsigned long long *acc;
    unsigned long long cnt = 0, kmin = LR_NONE;
    F xv[LR_VEC];

    __device__ __forceinline__ void load(int64_t i, int m, bool full) { lr_load4<F>(x, i, m, vec && full, xv, (F)0); }
    __device__ __forceinline__ bool ends(int) const { return false; }
    __device__ __forceinline__ void open(int32_t, bool, int) { cnt = 0; kmin = LR_NONE; }
    __device__ __forceinline__ void add(int64_t, int j)
    {
        const double xd = (double)xv[j];
        unsigned long long k = LM_ALLNAN;
        if (xd == xd) { k = lr_key(xd); cnt++; }
        kmin = k < kmin ? k : kmin;
    }
    __device__ __forceinline__ void close(int32_t cur) { lm_flush(cur, kmin, cnt, acc); cnt = 0; kmin = LR_NONE; }
    __device__ __forceinline__ void last(int tid, int32_t cur) { lm_flush_wave(tid, cur, kmin, cnt, acc); }
};

template <typename F>
__device__ inline void lm_pass_body(int64_t block, int tid, const int32_t *__restrict__ labels, const F *__restrict__ x, int64_t n,
                                    bool vec, int64_t n_labels, unsigned long long *acc)
{
    LmPass<F> v{x, vec, acc};
    lr_walk(block, tid, labels, n, vec, n_labels, v);
}

// For the k-th requested id: out_min[k] = the minimum, NaN where the label has no non-NaN voxel; out_count[k] = the
// number of its non-NaN voxels, -1 where the label has no voxel at all (or the id lies outside [1, n_labels]).
__device__ inline void lm_finish_body(int64_t k, int64_t n_ids, const int64_t *__restrict__ ids, int64_t n_labels,
                                      const unsigned long long *__restrict__ acc, double *__restrict__ out_min,
                                      int64_t *__restrict__ out_count)
{
    if (k >= n_ids) return;
    const int64_t id = ids[k];
    double mn = __builtin_nan("");
    int64_t count = -1;
    if (id >= 1 && id <= n_labels) {
        const unsigned long long key = acc[LM_REC * (id - 1)];
        if (key != LR_NONE) {
            count = (int64_t)acc[LM_REC * (id - 1) + 1];
            if (key != LM_ALLNAN) {
                union { double d; unsigned long long u; } c;
                c.u = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
                mn = c.d;
            }
        }
    }
    out_min[k] = mn;
    out_count[k] = count;
}
