// The order statistics of the generic per-label reductions on gfx950 (np.median / np.nanmedian through
// tobac_flow/utils/label_utils.py:8-55 labeled_comprehension and :58-140 apply_func_to_labels).
//
//   tf_label_order   the two middle values of every label's non-NaN values: slot-1 counts of tf_label_reduce's records ->
//                    exclusive scan -> scatter of order keys into per-label segments (one atomic cursor per label) ->
//                    rocPRIM segmented radix sort -> pick
//
// Only the labelled voxels' keys are sorted, never the volume.  Operands, layouts and the span are tf_label_reduce's
// (label_reduce.hip); the kernel bodies are in label_reduce_kernels.h.  Kept in a file of its own: rocPRIM's sort is most
// of the compile time.
#include "tf_common.h"
#include "tf_prim.h"
#include "label_reduce_kernels.h"

__global__ void __launch_bounds__(256)
k_lorder_counts(int64_t span, const unsigned long long *__restrict__ rec, uint32_t *__restrict__ count)
{
    lro_counts_body((int64_t)blockIdx.x * blockDim.x + threadIdx.x, span, rec, count);
}

__global__ void __launch_bounds__(256)
k_lorder_clamp(int64_t span, uint32_t *offset, int64_t n_keys)
{
    lro_clamp_body((int64_t)blockIdx.x * blockDim.x + threadIdx.x, span, offset, n_keys);
}

template <typename E>
__global__ void __launch_bounds__(256)
k_lorder_scatter(const int32_t *__restrict__ labels, const E *__restrict__ f, int64_t n, int64_t hw, int layout, bool vec,
                 bool vec_f, int64_t lo, int64_t hi, int32_t none, const uint32_t *__restrict__ offset, uint32_t *cursor,
                 typename LroKey<E>::type *keys, int64_t n_keys)
{
    lro_scatter_body<E>((int64_t)blockIdx.x, (int)threadIdx.x, labels, f, n, hw, layout, vec, vec_f, lo, hi, none, offset, cursor, keys, n_keys);
}

template <typename E>
__global__ void __launch_bounds__(256)
k_lorder_pick(int64_t span, const uint32_t *__restrict__ offset, const typename LroKey<E>::type *__restrict__ sorted,
              int64_t n_keys, double *__restrict__ out)
{
    lro_pick_body<E>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, span, offset, sorted, n_keys, out);
}

// workspace: count, offset (span + 1 each), cursor (span), two key buffers of n_keys, rocPRIM's scratch (scan and sort use
// it one after the other)
template <typename K>
static hipError_t lro_prim_bytes(int64_t span, int64_t n_keys, size_t *bytes)
{
    size_t a = 0, b = 0;
    hipError_t e = tf_exclusive_sum(nullptr, a, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)span + 1);
    if (e != hipSuccess) return e;
    e = rocprim::segmented_radix_sort_keys(nullptr, b, (const K *)nullptr, (K *)nullptr, (unsigned)n_keys, (unsigned)span,
                                           (const uint32_t *)nullptr, (const uint32_t *)nullptr);
    *bytes = a > b ? a : b;
    return e;
}

static bool lro_sizes_ok(int64_t id_lo, int64_t id_hi, int64_t n_keys)
{
    return id_lo <= id_hi && id_hi - id_lo < LRD_MAX_SPAN && n_keys >= 0 && n_keys <= 0x7fffffffll;
}

extern "C" size_t tf_label_order_workspace_bytes(int64_t id_lo, int64_t id_hi, int64_t n_keys, int dtype)
{
    if (!lro_sizes_ok(id_lo, id_hi, n_keys)) return 0;
    const int64_t span = id_hi - id_lo + 1;
    const size_t key = dtype == TF_F64 ? 8 : 4;
    size_t prim = 0;
    if ((dtype == TF_F64 ? lro_prim_bytes<unsigned long long>(span, n_keys, &prim) : lro_prim_bytes<uint32_t>(span, n_keys, &prim)) != hipSuccess) return 0;
    return 3 * (tf_align_up((size_t)(span + 1) * 4, 256) + 256) + 2 * (tf_align_up((size_t)(n_keys + 1) * key, 256) + 256) + tf_align_up(prim + 1, 256) + 512;
}

template <typename E>
static int lro_run(const int32_t *labels, const E *f, int layout, int64_t hw, int64_t lo, int64_t hi, const LrdShape &g,
                   const unsigned long long *rec, int64_t n_keys, double *out, void *ws, size_t ws_bytes, hipStream_t s)
{
    typedef typename LroKey<E>::type K;
    size_t prim = 0;
    TF_CHECK_HIP(lro_prim_bytes<K>(g.span, n_keys, &prim));
    TfArena ar(ws, ws_bytes);
    uint32_t *count = ar.take<uint32_t>((size_t)g.span + 1), *offset = ar.take<uint32_t>((size_t)g.span + 1);
    uint32_t *cursor = ar.take<uint32_t>((size_t)g.span);
    K *keys = ar.take<K>((size_t)n_keys + 1), *sorted = ar.take<K>((size_t)n_keys + 1);
    char *tmp = ar.take<char>(prim + 1);
    if (!ar.ok()) { tf_set_error("tf_label_order: workspace too small"); return TF_ENOMEM; }
    const dim3 grid((unsigned)g.blocks), ids((unsigned)g.id_blocks), lanes(256);
    hipLaunchKernelGGL(k_lorder_counts, ids, lanes, 0, s, g.span, rec, count);
    TF_CHECK_LAUNCH();
    size_t bytes = prim;
    TF_CHECK_HIP(tf_exclusive_sum(tmp, bytes, (const uint32_t *)count, offset, (size_t)g.span + 1, s));
    hipLaunchKernelGGL(k_lorder_clamp, ids, lanes, 0, s, g.span, offset, n_keys);
    TF_CHECK_LAUNCH();
    if (n_keys > 0) {
        TF_CHECK_HIP(hipMemcpyAsync(cursor, offset, (size_t)g.span * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_lorder_scatter<E>, grid, lanes, 0, s, labels, f, g.n, hw, layout, g.vec, g.vec_f, lo, hi, g.none,
                           (const uint32_t *)offset, cursor, keys, n_keys);
        TF_CHECK_LAUNCH();
        bytes = prim;
        TF_CHECK_HIP(rocprim::segmented_radix_sort_keys(tmp, bytes, (const K *)keys, sorted, (unsigned)n_keys, (unsigned)g.span,
                                                        (const uint32_t *)offset, (const uint32_t *)offset + 1, 0, 8 * sizeof(K), s));
    }
    hipLaunchKernelGGL(k_lorder_pick<E>, ids, lanes, 0, s, g.span, (const uint32_t *)offset, (const K *)sorted, n_keys, out);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

extern "C" int tf_label_order(const int32_t *labels, const void *field, int dtype, int layout, int64_t T, int64_t hw,
                              int64_t id_lo, int64_t id_hi, const void *records, int64_t n_keys, double *out, void *ws,
                              size_t ws_bytes, void *stream)
{
    LrdShape g;
    const char *bad = lrd_shape(labels, field, dtype, layout, T, hw, id_lo, id_hi, &g);
    if (bad) { tf_set_error("tf_label_order: %s", bad); return TF_EINVAL; }
    TF_REQUIRE(records && out && lro_sizes_ok(id_lo, id_hi, n_keys), "tf_label_order: bad arguments (n_keys is 0 .. 2^31 - 1)");
    const unsigned long long *rec = (const unsigned long long *)records;
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
    case TF_U8: return lro_run<uint8_t>(labels, (const uint8_t *)field, layout, hw, id_lo, id_hi, g, rec, n_keys, out, ws, ws_bytes, s);
    case TF_I32: return lro_run<int32_t>(labels, (const int32_t *)field, layout, hw, id_lo, id_hi, g, rec, n_keys, out, ws, ws_bytes, s);
    case TF_F32: return lro_run<float>(labels, (const float *)field, layout, hw, id_lo, id_hi, g, rec, n_keys, out, ws, ws_bytes, s);
    default: return lro_run<double>(labels, (const double *)field, layout, hw, id_lo, id_hi, g, rec, n_keys, out, ws, ws_bytes, s);
    }
}
