// Per-label weighted statistics, their uncertainties and flag proportions of the post-processing scripts on gfx950.
//
//   tf_label_wstats       tobac_flow/utils/stats_utils.py:33-154 weighted_stats / weighted_stats_and_uncertainties applied
//                         to every label by tobac_flow/utils/label_utils.py:58-140 apply_func_to_labels
//                         (tobac_flow/postprocess.py:102-242): two reads of the volume and a finish per label
//   tf_label_proportions  stats_utils.py:157-168 get_weighted_proportions (postprocess.py:245-310): one read and a finish
//
// The reference sorts the whole label volume (bincount + argsort) per call and runs a Python function per label; here a
// call reads labels, field and weights twice (once for the proportions), the errors only under labelled voxels, and
// writes a record per label.  Weights that the scripts build with np.repeat(area[None], T, 0) stay one (H, W) plane.
// The kernel bodies are in wstats_kernels.h, the work layout and the run walker they use in label_runs.h.
#include "tf_common.h"
#include "wstats_kernels.h"

__global__ void __launch_bounds__(256)
k_wstats_init(int64_t n_labels, double *acc)
{
    ws_init_body((int64_t)blockIdx.x * blockDim.x + threadIdx.x, n_labels, acc);
}

template <typename F>
__global__ void __launch_bounds__(256)
k_wstats_pass1(const int32_t *__restrict__ labels, const F *__restrict__ x, const F *__restrict__ e, const F *__restrict__ w,
               int64_t n, int64_t hw, bool plane, bool vec, bool vec_w, int64_t n_labels, double *acc)
{
    ws_pass1_body<F>((int64_t)blockIdx.x, (int)threadIdx.x, labels, x, e, w, n, hw, plane, vec, vec_w, n_labels, acc);
}

template <typename F>
__global__ void __launch_bounds__(256)
k_wstats_pass2(const int32_t *__restrict__ labels, const F *__restrict__ x, const F *__restrict__ w, int64_t n, int64_t hw,
               bool plane, bool vec, bool vec_w, int64_t n_labels, double *acc)
{
    ws_pass2_body<F>((int64_t)blockIdx.x, (int)threadIdx.x, labels, x, w, n, hw, plane, vec, vec_w, n_labels, acc);
}

template <typename F>
__global__ void __launch_bounds__(256)
k_wstats_finish(int64_t n_labels, const double *__restrict__ acc, const F *__restrict__ x, const F *__restrict__ e, int64_t n,
                double *__restrict__ out)
{
    ws_finish_body<F>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, n_labels, acc, x, e, n, out);
}

__global__ void __launch_bounds__(256)
k_wprop_pass(const int32_t *__restrict__ labels, const int32_t *__restrict__ flags, const float *__restrict__ w, int64_t n,
             int64_t hw, bool plane, bool vec, bool vec_w, int64_t n_labels, WpFlags fl, double *acc)
{
    wp_pass_body((int64_t)blockIdx.x, (int)threadIdx.x, labels, flags, w, n, hw, plane, vec, vec_w, n_labels, fl, acc);
}

__global__ void __launch_bounds__(256)
k_wprop_finish(int64_t n_labels, int K, const double *__restrict__ acc, double *__restrict__ out)
{
    wp_finish_body((int64_t)blockIdx.x * blockDim.x + threadIdx.x, n_labels, K, acc, out);
}

extern "C" size_t tf_label_wstats_workspace_bytes(int64_t n_labels)
{
    if (n_labels <= 0) return 0;
    return tf_align_up((size_t)n_labels * WS_REC * sizeof(double), 256) + 256;
}

template <typename F>
static int ws_run(const int32_t *labels, const F *x, const F *e, const F *w, int64_t n, int64_t hw, bool plane,
                  int64_t n_labels, double *out, double *acc, hipStream_t s)
{
    const int64_t blocks = (n + LR_BLOCK - 1) / LR_BLOCK, id_blocks = (n_labels + 255) / 256;
    TF_REQUIRE(blocks <= 0x7fffffffll && id_blocks <= 0x7fffffffll, "tf_label_wstats: volume too large for one launch");
    const bool vec = lr_aligned16(labels) && lr_aligned16(x) && (!e || lr_aligned16(e));
    const bool vec_w = lr_aligned16(w) && (!plane || hw % LR_VEC == 0);      // then i % hw keeps the alignment of i
    hipLaunchKernelGGL(k_wstats_init, dim3((unsigned)id_blocks), dim3(256), 0, s, n_labels, acc);
    TF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_wstats_pass1<F>, dim3((unsigned)blocks), dim3(256), 0, s, labels, x, e, w, n, hw, plane, vec, vec_w, n_labels, acc);
    TF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_wstats_pass2<F>, dim3((unsigned)blocks), dim3(256), 0, s, labels, x, w, n, hw, plane, vec, vec_w, n_labels, acc);
    TF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_wstats_finish<F>, dim3((unsigned)id_blocks), dim3(256), 0, s, n_labels, (const double *)acc, x, e, n, out);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

extern "C" int tf_label_wstats(const int32_t *labels, const void *field, const void *errors, const void *weights, int dtype,
                               int64_t T, int64_t hw, int weights_plane, int64_t n_labels, double *out, void *ws,
                               size_t ws_bytes, void *stream)
{
    TF_REQUIRE(labels && field && weights && out && n_labels > 0, "tf_label_wstats: bad arguments");
    TF_REQUIRE(dtype == TF_F32 || dtype == TF_F64, "tf_label_wstats: the field, errors and weights are float32 or float64");
    TF_REQUIRE(T > 0 && hw > 0 && n_labels <= 0x7fffffffll && T <= 0x7fffffffffffffffll / hw, "tf_label_wstats: bad shape");
    TfArena ar(ws, ws_bytes);
    double *acc = ar.take<double>((size_t)n_labels * WS_REC);
    if (!ar.ok()) { tf_set_error("tf_label_wstats: workspace too small"); return TF_ENOMEM; }
    hipStream_t s = (hipStream_t)stream;
    if (dtype == TF_F32)
        return ws_run<float>(labels, (const float *)field, (const float *)errors, (const float *)weights, T * hw, hw,
                             weights_plane != 0, n_labels, out, acc, s);
    return ws_run<double>(labels, (const double *)field, (const double *)errors, (const double *)weights, T * hw, hw,
                          weights_plane != 0, n_labels, out, acc, s);
}

extern "C" size_t tf_label_proportions_workspace_bytes(int64_t n_labels, int n_flags)
{
    if (n_labels <= 0 || n_flags < 0 || n_flags > WP_MAX_FLAGS) return 0;
    return tf_align_up((size_t)n_labels * (size_t)(1 + n_flags) * sizeof(double), 256) + 256;
}

extern "C" int tf_label_proportions(const int32_t *labels, const int32_t *flags, const float *weights, int64_t T, int64_t hw,
                                    int weights_plane, int64_t n_labels, const int32_t *flag_values_host, int n_flags,
                                    double *out, void *ws, size_t ws_bytes, void *stream)
{
    TF_REQUIRE(labels && flags && weights && out && flag_values_host && n_labels > 0, "tf_label_proportions: bad arguments");
    TF_REQUIRE(n_flags >= 1 && n_flags <= WP_MAX_FLAGS, "tf_label_proportions: 1 to 64 flag values");
    TF_REQUIRE(T > 0 && hw > 0 && n_labels <= 0x7fffffffll && T <= 0x7fffffffffffffffll / hw, "tf_label_proportions: bad shape");
    WpFlags fl;
    fl.k = n_flags;
    for (int k = 0; k < WP_MAX_FLAGS; k++) fl.v[k] = k < n_flags ? flag_values_host[k] : 0;
    for (int k = 1; k < n_flags; k++)
        for (int j = 0; j < k; j++) TF_REQUIRE(fl.v[j] != fl.v[k], "tf_label_proportions: the flag values must be distinct");
    TfArena ar(ws, ws_bytes);
    const size_t cells = (size_t)n_labels * (size_t)(1 + n_flags);
    double *acc = ar.take<double>(cells);
    if (!ar.ok()) { tf_set_error("tf_label_proportions: workspace too small"); return TF_ENOMEM; }
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = T * hw, blocks = (n + LR_BLOCK - 1) / LR_BLOCK, id_blocks = (n_labels + 255) / 256;
    TF_REQUIRE(blocks <= 0x7fffffffll, "tf_label_proportions: volume too large for one launch");
    const bool plane = weights_plane != 0;
    const bool vec = lr_aligned16(labels) && lr_aligned16(flags);
    const bool vec_w = lr_aligned16(weights) && (!plane || hw % LR_VEC == 0);
    TF_CHECK_HIP(hipMemsetAsync(acc, 0, cells * sizeof(double), s));
    hipLaunchKernelGGL(k_wprop_pass, dim3((unsigned)blocks), dim3(256), 0, s, labels, flags, weights, n, hw, plane, vec, vec_w, n_labels, fl, acc);
    TF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_wprop_finish, dim3((unsigned)id_blocks), dim3(256), 0, s, n_labels, n_flags, (const double *)acc, out);
    TF_CHECK_LAUNCH();
    return TF_OK;
}
