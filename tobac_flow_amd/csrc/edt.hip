// GLM validation of the detected cores and anvils on gfx950 (tobac_flow/validation.py, scripts/dcc_validation.py:145-250).
//
//   tf_edt2d_frames  scipy.ndimage.distance_transform_edt of every frame of a volume (validation.py:24-36, 52-104), as exact
//                    int32 squared distances and the raveled index of a nearest feature: a column pass and a row pass
//   tf_edt_cylinder  validation.py:52-104 get_marker_distance_cylinder: the minimum over +- time_margin frames, the
//                    earliest frame on ties, its square root as a double and the source voxel
//   tf_edt_time_envelope  validation.py:39-49 get_marker_distance_ellipse: SciPy's 3-D transform with sampling (s, 1, 1) as the
//                    lower envelope along t of (s dt)^2 + d2, evaluated in SciPy's summation order (edt_kernels.h)
//   tf_label_nanmin  np.nanmin applied to every label by tobac_flow/utils/label_utils.py:58-140 apply_func_to_labels
//                    (validation.py:13-21, 144-152): one read of labels and field, a finish per requested id
//
// The reference runs SciPy's transform on the CPU for every frame, six times per file.  Everything here is integer
// arithmetic followed by one square root, so the results equal the reference's bit for bit; which of several equally
// near features is reported is fixed by the scan order (edt_kernels.h).  The kernel bodies are in edt_kernels.h.
#include "tf_common.h"
#include "edt_kernels.h"

template <typename E>
__global__ void __launch_bounds__(256)
k_edt_cols(const E *__restrict__ vol, int64_t H, int64_t W, int64_t x_blocks, int32_t *__restrict__ fy)
{
    const int64_t t = (int64_t)blockIdx.x / x_blocks, xb = (int64_t)blockIdx.x - t * x_blocks;
    edt_cols_body<E>(xb * blockDim.x + threadIdx.x, t, vol, H, W, fy);
}

// one workgroup per row of the chunk; sq_rows == nullptr: sq[] in LDS (W words), else in the workspace
__global__ void __launch_bounds__(256)
k_edt_rows(const int32_t *__restrict__ fy, int64_t H, int64_t W, uint32_t *sq_rows, int32_t *__restrict__ d2,
           int32_t *__restrict__ nearest)
{
    extern __shared__ uint32_t edt_lds[];
    const int64_t row = (int64_t)blockIdx.x;
    uint32_t *sq = sq_rows ? sq_rows + row * W : edt_lds;
    const int32_t *fy_row = fy + row * W;
    const bool mine = edt_row_load_body((int)threadIdx.x, (int)blockDim.x, fy_row, (int32_t)(row % H), W, sq);
    int32_t *near_row = nearest ? nearest + row * W : nullptr;
    if (__syncthreads_or(mine)) edt_row_scan_body((int)threadIdx.x, (int)blockDim.x, sq, fy_row, W, d2 + row * W, near_row);
    else edt_row_empty_body((int)threadIdx.x, (int)blockDim.x, W, d2 + row * W, near_row);
}

__global__ void __launch_bounds__(256)
k_edt_cylinder(int64_t T, int64_t hw, int64_t tm, const int32_t *__restrict__ d2, const int32_t *__restrict__ nearest,
               double *__restrict__ dist, int64_t *__restrict__ src)
{
    edt_cyl_body((int64_t)blockIdx.x * blockDim.x + threadIdx.x, T, hw, tm, d2, nearest, dist, src);
}

__global__ void __launch_bounds__(256)
k_edt_envelope(int64_t T, int64_t hw, int32_t W, double s, const int32_t *__restrict__ d2, const int32_t *__restrict__ nearest,
               double *__restrict__ dist, int64_t *__restrict__ src)
{
    edt_env_body((int64_t)blockIdx.x * blockDim.x + threadIdx.x, T, hw, W, s, d2, nearest, dist, src);
}

__global__ void __launch_bounds__(256)
k_label_nanmin_init(int64_t n_labels, unsigned long long *acc)
{
    lm_init_body((int64_t)blockIdx.x * blockDim.x + threadIdx.x, n_labels, acc);
}

template <typename F>
__global__ void __launch_bounds__(256)
k_label_nanmin_pass(const int32_t *__restrict__ labels, const F *__restrict__ x, int64_t n, bool vec, int64_t n_labels,
                    unsigned long long *acc)
{
    lm_pass_body<F>((int64_t)blockIdx.x, (int)threadIdx.x, labels, x, n, vec, n_labels, acc);
}

__global__ void __launch_bounds__(256)
k_label_nanmin_finish(int64_t n_ids, const int64_t *__restrict__ ids, int64_t n_labels, const unsigned long long *__restrict__ acc,
                      double *__restrict__ out_min, int64_t *__restrict__ out_count)
{
    lm_finish_body((int64_t)blockIdx.x * blockDim.x + threadIdx.x, n_ids, ids, n_labels, acc, out_min, out_count);
}

// ---- tf_edt2d_frames ---------------------------------------------------------------------------------------------------
#define EDT_WS_TARGET ((size_t)1 << 30)                           // the chunk of frames whose fy[] (and sq[]) fit 1 GiB; at least one

static bool edt_shape_ok(int64_t T, int64_t H, int64_t W)
{
    return T > 0 && H > 0 && W > 0 && H <= 46341 && W <= 46341 && (H - 1) * (H - 1) + (W - 1) * (W - 1) < ((int64_t)1 << 31) &&
           T <= 0x7fffffffffffffffll / (H * W);
}

static size_t edt_frame_bytes(int64_t H, int64_t W) { return (size_t)(H * W) * sizeof(int32_t) * (W > EDT_LDS_MAX_W ? 2 : 1); }

static int64_t edt_chunk_frames(int64_t T, int64_t H, int64_t W)
{
    const int64_t fit = (int64_t)(EDT_WS_TARGET / edt_frame_bytes(H, W));
    return fit < 1 ? 1 : (fit < T ? fit : T);
}

extern "C" size_t tf_edt2d_frames_workspace_bytes(int64_t T, int64_t H, int64_t W)
{
    if (!edt_shape_ok(T, H, W)) return 0;
    return tf_align_up((size_t)edt_chunk_frames(T, H, W) * edt_frame_bytes(H, W), 256) + 512;
}

template <typename E>
static int edt_run(const E *vol, int64_t T, int64_t H, int64_t W, int32_t *d2, int32_t *nearest, int32_t *fy, uint32_t *sq,
                   int64_t chunk, hipStream_t s)
{
    const int64_t x_blocks = (W + 255) / 256;
    const size_t lds = sq ? 0 : (size_t)W * sizeof(uint32_t);
    for (int64_t t0 = 0; t0 < T; t0 += chunk) {
        const int64_t nt = T - t0 < chunk ? T - t0 : chunk, off = t0 * H * W;
        hipLaunchKernelGGL(k_edt_cols<E>, dim3((unsigned)(nt * x_blocks)), dim3(256), 0, s, vol + off, H, W, x_blocks, fy);
        TF_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_edt_rows, dim3((unsigned)(nt * H)), dim3(256), lds, s, (const int32_t *)fy, H, W, sq, d2 + off,
                           nearest ? nearest + off : nullptr);
        TF_CHECK_LAUNCH();
    }
    return TF_OK;
}

extern "C" int tf_edt2d_frames(const void *vol, int dtype, int64_t T, int64_t H, int64_t W, int32_t *d2, int32_t *nearest,
                               void *ws, size_t ws_bytes, void *stream)
{
    TF_REQUIRE(vol && d2, "tf_edt2d_frames: bad arguments");
    TF_REQUIRE(dtype == TF_U8 || dtype == TF_I32 || dtype == TF_F32 || dtype == TF_F64,
               "tf_edt2d_frames: the volume is uint8, int32, float32 or float64");
    TF_REQUIRE(edt_shape_ok(T, H, W), "tf_edt2d_frames: bad shape ((H - 1)^2 + (W - 1)^2 < 2^31 is required)");
    const int64_t chunk = edt_chunk_frames(T, H, W);
    TF_REQUIRE(chunk * ((W + 255) / 256) <= 0x7fffffffll && chunk * H <= 0x7fffffffll, "tf_edt2d_frames: frame too large for one launch");
    TfArena ar(ws, ws_bytes);
    int32_t *fy = ar.take<int32_t>((size_t)(chunk * H * W));
    uint32_t *sq = W > EDT_LDS_MAX_W ? ar.take<uint32_t>((size_t)(chunk * H * W)) : nullptr;
    if (!ar.ok()) { tf_set_error("tf_edt2d_frames: workspace too small"); return TF_ENOMEM; }
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
    case TF_U8: return edt_run<uint8_t>((const uint8_t *)vol, T, H, W, d2, nearest, fy, sq, chunk, s);
    case TF_I32: return edt_run<int32_t>((const int32_t *)vol, T, H, W, d2, nearest, fy, sq, chunk, s);
    case TF_F32: return edt_run<float>((const float *)vol, T, H, W, d2, nearest, fy, sq, chunk, s);
    default: return edt_run<double>((const double *)vol, T, H, W, d2, nearest, fy, sq, chunk, s);
    }
}

// ---- tf_edt_cylinder ---------------------------------------------------------------------------------------------------
extern "C" int tf_edt_cylinder(const int32_t *d2, const int32_t *nearest, int64_t T, int64_t hw, int64_t time_margin,
                               double *dist, int64_t *src, void *stream)
{
    TF_REQUIRE(d2 && dist && (!src || nearest), "tf_edt_cylinder: bad arguments (src needs nearest)");
    TF_REQUIRE(T > 0 && hw > 0 && T <= 0x7fffffffffffffffll / hw && time_margin >= 0, "tf_edt_cylinder: bad shape or time margin");
    const int64_t n = T * hw, blocks = (n + 255) / 256;
    TF_REQUIRE(blocks <= 0x7fffffffll, "tf_edt_cylinder: volume too large for one launch");
    hipLaunchKernelGGL(k_edt_cylinder, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, T, hw,
                       time_margin < T ? time_margin : T, d2, nearest, dist, src);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

// ---- tf_edt_time_envelope ----------------------------------------------------------------------------------------------
extern "C" int tf_edt_time_envelope(const int32_t *d2, const int32_t *nearest, int64_t T, int64_t H, int64_t W, double sampling_t,
                                    double *dist, int64_t *src, void *stream)
{
    TF_REQUIRE(d2 && dist && (!src || nearest), "tf_edt_time_envelope: bad arguments (src needs nearest)");
    TF_REQUIRE(edt_shape_ok(T, H, W), "tf_edt_time_envelope: bad shape ((H - 1)^2 + (W - 1)^2 < 2^31 is required)");
    TF_REQUIRE(sampling_t > 0 && sampling_t <= 1.7976931348623157e308, "tf_edt_time_envelope: sampling_t must be finite and > 0");
    const int64_t hw = H * W, blocks = (hw + 255) / 256;        // one lane per pixel, looping over t; hw < 2^31 by edt_shape_ok
    hipLaunchKernelGGL(k_edt_envelope, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, T, hw, (int32_t)W, sampling_t, d2,
                       nearest, dist, src);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

// ---- tf_label_nanmin ---------------------------------------------------------------------------------------------------
extern "C" size_t tf_label_nanmin_workspace_bytes(int64_t n_labels)
{
    if (n_labels <= 0) return 0;
    return tf_align_up((size_t)n_labels * LM_REC * sizeof(unsigned long long), 256) + 256;
}

template <typename F>
static int lm_run(const int32_t *labels, const F *x, int64_t n, int64_t n_labels, const int64_t *ids, int64_t n_ids,
                  double *out_min, int64_t *out_count, unsigned long long *acc, hipStream_t s)
{
    const int64_t blocks = (n + LR_BLOCK - 1) / LR_BLOCK, id_blocks = (n_ids + 255) / 256;
    TF_REQUIRE(blocks <= 0x7fffffffll && id_blocks <= 0x7fffffffll, "tf_label_nanmin: volume too large for one launch");
    hipLaunchKernelGGL(k_label_nanmin_init, dim3((unsigned)((n_labels + 255) / 256)), dim3(256), 0, s, n_labels, acc);
    TF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_label_nanmin_pass<F>, dim3((unsigned)blocks), dim3(256), 0, s, labels, x, n,
                       lr_aligned16(labels) && lr_aligned16(x), n_labels, acc);
    TF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_label_nanmin_finish, dim3((unsigned)id_blocks), dim3(256), 0, s, n_ids, ids, n_labels,
                       (const unsigned long long *)acc, out_min, out_count);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

extern "C" int tf_label_nanmin(const int32_t *labels, const void *field, int dtype, int64_t n, int64_t n_labels,
                               const int64_t *ids, int64_t n_ids, double *out_min, int64_t *out_count, void *ws,
                               size_t ws_bytes, void *stream)
{
    TF_REQUIRE(labels && field && ids && out_min && out_count, "tf_label_nanmin: bad arguments");
    TF_REQUIRE(dtype == TF_U8 || dtype == TF_F32 || dtype == TF_F64, "tf_label_nanmin: the field is uint8, float32 or float64");
    TF_REQUIRE(n > 0 && n_ids > 0 && n_labels > 0 && n_labels <= 0x7fffffffll, "tf_label_nanmin: bad shape");
    TfArena ar(ws, ws_bytes);
    unsigned long long *acc = ar.take<unsigned long long>((size_t)n_labels * LM_REC);
    if (!ar.ok()) { tf_set_error("tf_label_nanmin: workspace too small"); return TF_ENOMEM; }
    hipStream_t s = (hipStream_t)stream;
    if (dtype == TF_U8) return lm_run<uint8_t>(labels, (const uint8_t *)field, n, n_labels, ids, n_ids, out_min, out_count, acc, s);
    if (dtype == TF_F32) return lm_run<float>(labels, (const float *)field, n, n_labels, ids, n_ids, out_min, out_count, acc, s);
    return lm_run<double>(labels, (const double *)field, n, n_labels, ids, n_ids, out_min, out_count, acc, s);
}
