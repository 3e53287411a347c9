// What the per-label reduction kernels share: the work layouts, the vector loads, and the two walkers that take a lane
// through its voxels as runs of equal labels.  Users: wstats_kernels.h, field_props_kernels.h, edt_kernels.h (tf_label_nanmin), props.hip,
// label_reduce_kernels.h (the span form of the raveled walker);
// label_filter.hip takes the row-chunk layout and its launch geometry and keeps its own loop (see there); bin_kernels.h
// and subseg.hip take the loads and the alignment predicate only.  The same text compiles
// for the host (tools/*_host_check.cpp supply blockIdx-free bodies, the vector types and the atomics).  Nothing here
// touches the HIP runtime.
#pragma once
#include <stdint.h>

// ---- the raveled work layout -----------------------------------------------------------------------------------------
// A workgroup of 256 lanes takes LR_BLOCK = 4096 consecutive voxels of the raveled volume, each of its four waves 1024 of
// them in LR_ITERS = 4 steps of 256: in step k lane j holds the LR_VEC = 4 voxels from wave base + 256 k + 4 j, so one
// load instruction of a wave reads 64 adjacent 16-byte pieces of the labels (and of a float32 operand; a float64 operand
// is two adjacent 16-byte pieces per lane).  A lane keeps ONE open run -- label id and its partial results -- across its
// 16 voxels, which need not be neighbours for that: labels are coherent down the rows as well as along them, and a sum
// does not care.  It issues one set of atomics when the id changes and one at the end; a lane whose four labels are all
// background loads nothing else.
// Runs are merged per lane, not across the wave (profiles/weighted_stats_notes.txt): a merge across the lanes saves
// atomics only for regions wider than a lane's voxels and costs a segmented scan of every partial result on every wave,
// labelled or not.  The one exception is a visitor's own `last` (tf_label_nanmin combines the runs still open at the end).
#define LR_VEC 4
#define LR_ITERS 4
#define LR_WAVE_SPAN (64 * LR_VEC * LR_ITERS)
#define LR_BLOCK (4 * LR_WAVE_SPAN)
#define LR_NONE 0xffffffffffffffffull

// ---- the row-chunk work layout ---------------------------------------------------------------------------------------
// Where a kernel needs (t, y, x) of a voxel, one lane takes LR_ROW_RUN consecutive voxels of ONE row (a run never
// straddles a row: y and the plane index change there); most lanes see background only and leave after their loads.
#define LR_ROW_RUN 16

// first voxel of (workgroup, lane, step); everything that indexes the volume is 64-bit: 144 x 5424^2 = 4.2e9 voxels
// are beyond int32 and a longer run is beyond 2^32
__host__ __device__ inline int64_t lr_first_voxel(int64_t block, int tid, int step)
{
    return block * LR_BLOCK + (int64_t)(tid >> 6) * LR_WAVE_SPAN + (int64_t)step * (64 * LR_VEC) + (int64_t)(tid & 63) * LR_VEC;
}

__host__ __device__ inline bool lr_aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

// Order-preserving key of a FINITE value: a < b  <=>  key(a) < key(b) as unsigned; -0.0 and +0.0 share a key (x + 0.0
// is +0.0 for both under round-to-nearest), as np.argmin / np.argmax see them.  float -> double is exact.
__host__ __device__ inline unsigned long long lr_key(double x)
{
    union { double d; unsigned long long u; } c;
    c.d = x + 0.0;
    return (c.u >> 63) ? ~c.u : (c.u | 0x8000000000000000ull);
}

__host__ __device__ inline bool lr_finite(double x) { return x - x == 0; }        // false for NaN and +-inf

// four consecutive elements: one 16-byte load (int32, float) or two adjacent ones (double)
__host__ __device__ inline void lr_vload(const int32_t *p, int32_t v[LR_VEC])
{
    const int4 q = *(const int4 *)p;
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__host__ __device__ inline void lr_vload(const float *p, float v[LR_VEC])
{
    const float4 q = *(const float4 *)p;
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
// a bool field (tf_label_nanmin, tf_bin_points' masks): ONE 4-byte load, little endian -- as a uchar4 the load can come
// out as two 2-byte ones once v is a member of a visitor
__host__ __device__ inline void lr_vload(const uint8_t *p, uint8_t v[LR_VEC])
{
    const uint32_t q = *(const uint32_t *)p;
    v[0] = (uint8_t)q; v[1] = (uint8_t)(q >> 8); v[2] = (uint8_t)(q >> 16); v[3] = (uint8_t)(q >> 24);
}
__host__ __device__ inline void lr_vload(const double *p, double v[LR_VEC])
{
    const double2 a = ((const double2 *)p)[0], b = ((const double2 *)p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}

// elements i .. i + m - 1 of p (m <= 4): vector loads when `vec` (the caller guarantees that p + i is 16-byte aligned
// and m == 4), element loads otherwise; the rest of v is `fill`
template <typename E>
__host__ __device__ inline void lr_load4(const E *__restrict__ p, int64_t i, int m, bool vec, E v[LR_VEC], E fill)
{
    if (vec) { lr_vload(p + i, v); return; }
#pragma unroll
    for (int j = 0; j < LR_VEC; j++) v[j] = j < m ? p[i + j] : fill;
}

// the weights of voxels i .. i + m - 1: a volume like the labels, or with `plane` one (hw,) plane that every frame shares
// (index i % hw; never materialised).  vec_w: w is 16-byte aligned and, for a plane, hw % 4 == 0 (then i % hw keeps the
// alignment of i).  The element arm takes (iw + j) % hw per voxel: four voxels wrap more than once where hw < 4.
template <typename F>
__host__ __device__ __forceinline__ void lr_load_weights(const F *__restrict__ w, int64_t i, int m, bool full, int64_t hw,
                                                         bool plane, bool vec_w, F wv[LR_VEC])
{
    const int64_t iw = plane ? i % hw : i;
    if (plane && iw + m > hw) {                                   // the four voxels straddle the end of the plane
#pragma unroll
        for (int j = 0; j < LR_VEC; j++) wv[j] = j < m ? w[(iw + j) % hw] : (F)0;
    } else
        lr_load4<F>(w, iw, m, vec_w && full, wv, (F)0);
}

// ---- the run loop ----------------------------------------------------------------------------------------------------
// N labels of one lane in their order, `cur` the id of the lane's open run (0: none yet).  A visitor V holds the run's
// partial results and supplies
//   bool ends(j)        the run also ends before voxel j although the id stays (tf_label_proportions: the flag changes)
//   void close(id)      issue the run's atomics, if it gathered anything, and leave it empty
//   void open(l, in, j) start a run of id l at voxel j; `in`: l is in [1, n_labels].  Called for other ids too: such a run
//                       gathers nothing, so its close issues nothing
//   void add(i, j)      voxel j of the step (raveled index i + j), called for ids in [1, n_labels] only
// The ids that count are those of the span [lo, hi] (lr_runs: [1, n_labels]); every other id is background.
template <int N, typename V, typename Lo>
__device__ __forceinline__ void lr_runs_span(const int32_t (&lv)[N], int64_t i, Lo lo, int64_t hi, int32_t &cur, V &v)
{
#pragma unroll
    for (int j = 0; j < N; j++) {
        const int32_t l = lv[j];
        const bool in = l >= lo && l <= hi;
        if (l != cur || v.ends(j)) {
            v.close(cur);
            cur = l;
            v.open(l, in, j);
        }
        if (in) v.add(i, j);
    }
}

template <int N, typename V>
__device__ __forceinline__ void lr_runs(const int32_t (&lv)[N], int64_t i, int64_t n_labels, int32_t &cur, V &v)
{
    lr_runs_span<N>(lv, i, 1, n_labels, cur, v);                  // lo as the int it is: the code of before the span form
}

// ---- the raveled walker ----------------------------------------------------------------------------------------------
// One lane's 16 voxels of the raveled layout above.  Besides the hooks of lr_runs the visitor supplies
//   void load(i, m, full)  the other operands of the step's voxels i .. i + m - 1 (full: m == 4), called only for steps
//                          that hold an id in [1, n_labels]
//   void last(tid, id)     the run still open after the last step (a plain close for all but tf_label_nanmin)
// vec: `labels` is 16-byte aligned.  Every lane of the workgroup reaches `last` (no early return).
// lr_walk_span: the ids of the span [lo, hi] count instead (tf_label_reduce: 0 and negative ids are regions like any
// other there); `none` is an id OUTSIDE the span that stands for "no open run".
template <typename V, typename Lo>
__device__ __forceinline__ void lr_walk_span(int64_t block, int tid, const int32_t *__restrict__ labels, int64_t n, bool vec,
                                             Lo lo, int64_t hi, int32_t none, V &v)
{
    int32_t cur = none;
#pragma unroll
    for (int step = 0; step < LR_ITERS; step++) {
        const int64_t i = lr_first_voxel(block, tid, step);
        if (i >= n) break;
        const int m = n - i < LR_VEC ? (int)(n - i) : LR_VEC;
        const bool full = m == LR_VEC;
        int32_t lv[LR_VEC];
        lr_load4<int32_t>(labels, i, m, vec && full, lv, none);
        bool any = false;
#pragma unroll
        for (int j = 0; j < LR_VEC; j++) any |= lv[j] >= lo && lv[j] <= hi;
        if (!any) { v.close(cur); cur = none; continue; }         // background costs nothing more
        v.load(i, m, full);
        lr_runs_span<LR_VEC>(lv, i, lo, hi, cur, v);
    }
    v.last(tid, cur);
}

template <typename V>
__device__ __forceinline__ void lr_walk(int64_t block, int tid, const int32_t *__restrict__ labels, int64_t n, bool vec,
                                        int64_t n_labels, V &v)
{
    lr_walk_span(block, tid, labels, n, vec, 1, n_labels, 0, v);
}

// ---- the row-chunk walker --------------------------------------------------------------------------------------------
// Chunk c of the row-chunk layout above: LR_ROW_RUN voxels from x0 of row t * H + y.  ALIGNED: `labels` is 16-byte
// aligned and W % 4 == 0, so every full chunk is four 16-byte loads.  A lane that sees background only returns before
// the visitor is touched; otherwise the visitor's begin(t, y, x0) comes first (what depends on the row), then the hooks
// of lr_runs with i = the raveled index of the chunk's first voxel, then a close.
template <bool ALIGNED, typename V>
__device__ __forceinline__ void lr_walk_row(int64_t c, const int32_t *__restrict__ labels, int64_t n_chunks, int H, int W,
                                            int chunks_per_row, int64_t n_labels, V &v)
{
    if (c >= n_chunks) return;
    const int64_t row = c / chunks_per_row;                       // = t * H + y
    const int x0 = (int)(c - row * chunks_per_row) * LR_ROW_RUN;
    const int t = (int)(row / H), y = (int)(row - (int64_t)t * H);
    const int m = W - x0 < LR_ROW_RUN ? W - x0 : LR_ROW_RUN;
    const int64_t base = row * W + x0;
    const int32_t *L = labels + base;
    int32_t lv[LR_ROW_RUN];
    if (ALIGNED && m == LR_ROW_RUN) {
#pragma unroll
        for (int q = 0; q < LR_ROW_RUN / LR_VEC; q++) lr_vload(L + LR_VEC * q, lv + LR_VEC * q);
    } else {
#pragma unroll
        for (int j = 0; j < LR_ROW_RUN; j++) lv[j] = j < m ? L[j] : 0;
    }
    int32_t any = 0;
#pragma unroll
    for (int j = 0; j < LR_ROW_RUN; j++) any |= lv[j];
    if (any == 0) return;                                         // background costs nothing
    v.begin(t, y, x0);
    int32_t cur = 0;
    lr_runs<LR_ROW_RUN>(lv, base, n_labels, cur, v);
    v.close(cur);
}

// launch geometry of a row-chunk kernel (256 lanes per workgroup); returns null, or what is wrong with the shape
struct LrRowGrid { int64_t n_chunks; int chunks_per_row; unsigned blocks; bool aligned; };

inline const char *lr_row_grid(const int32_t *labels, int64_t T, int64_t H, int64_t W, LrRowGrid *g)
{
    if (!(T > 0 && T < 65536 && H > 0 && W > 0 && H <= 0x7fffffff && W <= 0x7fffffff - LR_ROW_RUN)) return "bad shape";
    const int64_t cpr = (W + LR_ROW_RUN - 1) / LR_ROW_RUN, n_chunks = T * H * cpr, blocks = (n_chunks + 255) / 256;
    if (blocks > 0x7fffffffll) return "volume too large for one launch";
    *g = LrRowGrid{n_chunks, (int)cpr, (unsigned)blocks, lr_aligned16(labels) && W % 4 == 0};
    return nullptr;
}
