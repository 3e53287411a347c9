// Label filters of the detection recipes on gfx950.
//
//   tf_label_filter      tobac_flow/analysis.py:15-201 -- find_object_lengths, mask_labels and the filter_labels_by_* family:
//                        per label the first / last leading index and, for up to eight criteria at once, whether some voxel
//                        of the label satisfies the criterion -- as ONE read of the label volume
//
// A criterion is a byte mask ("non-zero") or a float32 / float64 field compared with a threshold, so that the recipes'
// `field >= upper` volumes never exist.  Criterion operands are read only under labelled voxels, and only while the
// label's bit for that criterion is still clear.
#include "tf_common.h"
#include "label_runs.h"
#include <math.h>

// The row-chunk layout of label_runs.h, as k_label_props: one lane takes LR_ROW_RUN consecutive voxels of ONE row, most
// lanes see background only and leave after their loads, and the others flush once per run of equal labels.  No merge
// across the wave, for the reason given there.  The kernel keeps its own loop over the chunk and does not go through
// lr_walk_row: on that walker it measured 7.5 % slower with three criteria, with the same loads and atomics in the code
// object (profiles/label_runs.txt; the cause was not found).  Only the launch geometry (lr_row_grid) is shared.
// Record per label id: {tmin, tmax, hits, 0} = 16 B, so four labels share a 64-B line and one label's atomics fall into
// one line.  At the start of a run the lane reads the record once: a criterion whose bit is set already is not evaluated
// for the run, and an atomic is issued only where the value read would change.  Bits are only ever set, tmin only falls
// and tmax only rises, so a stale read costs a redundant evaluation or atomic, never a wrong answer.
#define LF_MAX 8

struct LfCrit { const void *data; int dtype, op; float th32; double th64; };
struct LfArgs { LfCrit c[LF_MAX]; int n; };

__global__ void __launch_bounds__(256)
k_label_filter_init(int4 *__restrict__ rec, int64_t n_ids)
{
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l < n_ids) rec[l] = make_int4(0x7fffffff, -1, 0, 0);
}

template <typename T>
__device__ __forceinline__ bool lf_cmp(T v, T th, int op)          // every comparison with a NaN is false
{
    return op == TF_CMP_GE ? v >= th : op == TF_CMP_GT ? v > th : op == TF_CMP_LE ? v <= th : v < th;
}

__device__ __forceinline__ bool lf_eval(const LfCrit &c, int64_t i)
{
    if (c.dtype == TF_U8) return ((const uint8_t *)c.data)[i] != 0;
    if (c.dtype == TF_F32) return lf_cmp(((const float *)c.data)[i], c.th32, c.op);
    return lf_cmp(((const double *)c.data)[i], c.th64, c.op);
}

template <bool ALIGNED>
__global__ void __launch_bounds__(256)
k_label_filter(const int32_t *__restrict__ labels, int64_t n_chunks, int H, int W, int chunks_per_row, int64_t n_labels,
               LfArgs a, int32_t *rec)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const int64_t row = c / chunks_per_row;                       // = t * H + y
    const int x0 = (int)(c - row * chunks_per_row) * LR_ROW_RUN;
    const int t = (int)(row / H);
    const int m = min(LR_ROW_RUN, W - x0);
    const int64_t base = row * W + x0;
    const int32_t *L = labels + base;
    int32_t v[LR_ROW_RUN];
    if (ALIGNED && m == LR_ROW_RUN) {
#pragma unroll
        for (int q = 0; q < LR_ROW_RUN / 4; q++) {
            const int4 w4 = ((const int4 *)L)[q];
            v[4 * q] = w4.x; v[4 * q + 1] = w4.y; v[4 * q + 2] = w4.z; v[4 * q + 3] = w4.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < LR_ROW_RUN; j++) v[j] = j < m ? L[j] : 0;
    }
    int32_t any = 0;
#pragma unroll
    for (int j = 0; j < LR_ROW_RUN; j++) any |= v[j];
    if (any == 0) return;                                         // background costs nothing

    const int all = (1 << a.n) - 1;
    int32_t cur = 0; bool live = false;
    int seen_min = 0, seen_max = 0, known = 0, found = 0;
    auto flush = [&]() {
        if (!live) return;                                        // cur is in [1, n_labels] whenever live
        int32_t *r = rec + 4 * (int64_t)cur;
        if (seen_min > t) atomicMin(&r[0], t);
        if (seen_max < t) atomicMax(&r[1], t);
        if (found & ~known) atomicOr(&r[2], found);
    };
#pragma unroll
    for (int j = 0; j < LR_ROW_RUN; j++) {
        const int32_t l = v[j];
        if (l != cur) {
            flush();
            cur = l; live = l >= 1 && l <= n_labels; found = 0;
            if (live) {
                const int4 r = *(const int4 *)(rec + 4 * (int64_t)l);
                seen_min = r.x; seen_max = r.y; known = r.z;
            }
        }
        if (!live || ((known | found) & all) == all) continue;
        const int64_t i = base + j;
#pragma unroll
        for (int k = 0; k < LF_MAX; k++)
            if (k < a.n && !(((known | found) >> k) & 1) && lf_eval(a.c[k], i)) found |= 1 << k;
    }
    flush();
}

extern "C" int tf_label_filter(const int32_t *labels, int64_t T, int64_t H, int64_t W, int64_t n_labels,
                               const tf_label_criterion *criteria, int n_criteria, int32_t *records, void *stream)
{
    TF_REQUIRE(labels && records, "tf_label_filter: null pointer");
    TF_REQUIRE(lr_aligned16(records), "tf_label_filter: records must be 16-byte aligned");
    TF_REQUIRE(n_labels >= 0 && n_labels < 0x7fffffffll, "tf_label_filter: n_labels out of range");
    TF_REQUIRE(n_criteria >= 0 && n_criteria <= LF_MAX, "tf_label_filter: 0 to 8 criteria");
    TF_REQUIRE(criteria || n_criteria == 0, "tf_label_filter: null criteria");
    LrRowGrid g;
    if (const char *bad = lr_row_grid(labels, T, H, W, &g)) { tf_set_error("tf_label_filter: %s", bad); return TF_EINVAL; }
    LfArgs a;
    a.n = n_criteria;
    for (int k = 0; k < LF_MAX; k++) a.c[k] = LfCrit{nullptr, TF_U8, TF_CMP_GE, 0.0f, 0.0};
    for (int k = 0; k < n_criteria; k++) {
        const tf_label_criterion &q = criteria[k];
        TF_REQUIRE(q.data, "tf_label_filter: a criterion without data");
        TF_REQUIRE(q.dtype == TF_U8 || q.dtype == TF_F32 || q.dtype == TF_F64, "tf_label_filter: a criterion is TF_U8, TF_F32 or TF_F64");
        if (q.dtype == TF_U8) { a.c[k].data = q.data; continue; } // op and threshold ignored: "non-zero"
        TF_REQUIRE(q.op >= TF_CMP_GE && q.op <= TF_CMP_LT, "tf_label_filter: unknown comparison");
        TF_REQUIRE(!isnan(q.threshold), "tf_label_filter: NaN threshold");
        a.c[k] = LfCrit{q.data, q.dtype, q.op, (float)q.threshold, q.threshold};
    }
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_ids = n_labels + 1;
    hipLaunchKernelGGL(k_label_filter_init, dim3((unsigned)((n_ids + 255) / 256)), dim3(256), 0, s, (int4 *)records, n_ids);
    TF_CHECK_LAUNCH();
    if (n_labels == 0) return TF_OK;
    hipLaunchKernelGGL(g.aligned ? k_label_filter<true> : k_label_filter<false>, dim3(g.blocks), dim3(256), 0, s, labels, g.n_chunks,
                       (int)H, (int)W, g.chunks_per_row, n_labels, a, records);
    TF_CHECK_LAUNCH();
    return TF_OK;
}
