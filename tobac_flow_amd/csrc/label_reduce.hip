// The generic per-label reductions on gfx950: what tobac_flow/utils/label_utils.py:8-55 labeled_comprehension and :58-140
// apply_func_to_labels compute when `func` is one of NumPy's plain reducers.
//
//   tf_label_reduce  one 64-byte record per label id of a span: counts, sum, extremes and (on request, a second read)
//                    the squared deviations about the mean -- every sum / mean / var / std / min / max / ptp / any / all /
//                    count_nonzero / size is a host-side expression of it
// (tf_label_order, the order statistics on the same operands, is label_order.hip.)
//
// The reference sorts the whole label volume per call and runs a Python function per label; here nothing of the volume is
// sorted.  The field is a volume, one plane shared by every frame
// or one value per frame, never materialised.  The kernel bodies are in label_reduce_kernels.h, the work layout and the
// run walker they use in label_runs.h.
#include "tf_common.h"
#include "label_reduce_kernels.h"

__global__ void __launch_bounds__(256)
k_lreduce_init(int64_t span, unsigned long long *rec)
{
    lrd_init_body((int64_t)blockIdx.x * blockDim.x + threadIdx.x, span, rec);
}

template <typename E>
__global__ void __launch_bounds__(256)
k_lreduce_pass1(const int32_t *__restrict__ labels, const E *__restrict__ f, int64_t n, int64_t hw, int layout, bool vec,
                bool vec_f, int64_t lo, int64_t hi, int32_t none, unsigned long long *rec)
{
    lrd_pass1_body<E>((int64_t)blockIdx.x, (int)threadIdx.x, labels, f, n, hw, layout, vec, vec_f, lo, hi, none, rec);
}

template <typename E>
__global__ void __launch_bounds__(256)
k_lreduce_mean(int64_t span, const unsigned long long *__restrict__ rec, double *__restrict__ mean)
{
    lrd_mean_body<E>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, span, rec, mean);
}

template <typename E>
__global__ void __launch_bounds__(256)
k_lreduce_pass2(const int32_t *__restrict__ labels, const E *__restrict__ f, int64_t n, int64_t hw, int layout, bool vec,
                bool vec_f, int64_t lo, int64_t hi, int32_t none, const double *__restrict__ mean, unsigned long long *rec)
{
    lrd_pass2_body<E>((int64_t)blockIdx.x, (int)threadIdx.x, labels, f, n, hw, layout, vec, vec_f, lo, hi, none, mean, rec);
}

extern "C" size_t tf_label_reduce_workspace_bytes(int64_t id_lo, int64_t id_hi)
{
    if (id_lo > id_hi || id_hi - id_lo >= LRD_MAX_SPAN) return 0;
    return tf_align_up((size_t)(id_hi - id_lo + 1) * sizeof(double), 256) + 256;
}

template <typename E>
static int lrd_run(const int32_t *labels, const E *f, int layout, int64_t hw, int64_t lo, int64_t hi, int want,
                   const LrdShape &g, unsigned long long *rec, double *mean, hipStream_t s)
{
    const dim3 grid((unsigned)g.blocks), ids((unsigned)g.id_blocks), lanes(256);
    hipLaunchKernelGGL(k_lreduce_init, ids, lanes, 0, s, g.span, rec);
    TF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_lreduce_pass1<E>, grid, lanes, 0, s, labels, f, g.n, hw, layout, g.vec, g.vec_f, lo, hi, g.none, rec);
    TF_CHECK_LAUNCH();
    if (!(want & LRD_WANT_VAR)) return TF_OK;
    hipLaunchKernelGGL(k_lreduce_mean<E>, ids, lanes, 0, s, g.span, (const unsigned long long *)rec, mean);
    TF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_lreduce_pass2<E>, grid, lanes, 0, s, labels, f, g.n, hw, layout, g.vec, g.vec_f, lo, hi, g.none, (const double *)mean, rec);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

extern "C" int tf_label_reduce(const int32_t *labels, const void *field, int dtype, int layout, int64_t T, int64_t hw,
                               int64_t id_lo, int64_t id_hi, int want, void *records, void *ws, size_t ws_bytes, void *stream)
{
    LrdShape g;
    const char *bad = lrd_shape(labels, field, dtype, layout, T, hw, id_lo, id_hi, &g);
    if (bad) { tf_set_error("tf_label_reduce: %s", bad); return TF_EINVAL; }
    TF_REQUIRE(records && (want & ~LRD_WANT_VAR) == 0, "tf_label_reduce: bad arguments");
    double *mean = nullptr;
    if (want & LRD_WANT_VAR) {
        TfArena ar(ws, ws_bytes);
        mean = ar.take<double>((size_t)g.span);
        if (!ar.ok()) { tf_set_error("tf_label_reduce: workspace too small"); return TF_ENOMEM; }
    }
    unsigned long long *rec = (unsigned long long *)records;
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
    case TF_U8: return lrd_run<uint8_t>(labels, (const uint8_t *)field, layout, hw, id_lo, id_hi, want, g, rec, mean, s);
    case TF_I32: return lrd_run<int32_t>(labels, (const int32_t *)field, layout, hw, id_lo, id_hi, want, g, rec, mean, s);
    case TF_F32: return lrd_run<float>(labels, (const float *)field, layout, hw, id_lo, id_hi, want, g, rec, mean, s);
    default: return lrd_run<double>(labels, (const double *)field, layout, hw, id_lo, id_hi, want, g, rec, mean, s);
    }
}
