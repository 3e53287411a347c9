// The fifth stage of the post-processing scripts on gfx950: cloud and flux properties per object.
//
//   tf_flux_cre            tobac_flow/postprocess.py:29-99 get_cre / add_cre_to_dataset: the ten derived flux planes from the
//                          thirteen raw ones in one launch
//   tf_quality_weights     scripts/postprocess_seviri_nat_dcc.py:181-186: weights * (qcflag == 0) * (cth < 30) * isfinite(cot)
//   tf_label_wstats_multi  tf_label_wstats (wstats.hip) for a whole field set over ONE walk of the label volume per pass:
//                          the scripts' loop `for var in (...): for dim in (...): add_weighted_stats_to_dataset(...)`
//                          (postprocess_seviri_nat_dcc.py:190-205, 274-298) reads the label volume twice per variable; here
//                          twice per set, and the derived fluxes of the TOA / BOA sets are formed in registers.
// The kernel bodies are in field_props_kernels.h, the work layout and the run walker in label_runs.h.
#include "tf_common.h"
#include "field_props_kernels.h"

template <typename F>
__global__ void __launch_bounds__(256)
k_flux_cre(int64_t n, bool vec, FpCrePlanes p)
{
    fp_cre_body<F>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, n, vec, p);
}

template <typename W, typename C>
__global__ void __launch_bounds__(256)
k_quality_weights(const W *__restrict__ w, const int32_t *__restrict__ q, const C *__restrict__ cth, const C *__restrict__ cot,
                  int64_t n, int64_t hw, bool plane, bool vec, bool vec_w, bool vec_out, W *__restrict__ out)
{
    fp_quality_body<W, C>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, w, q, cth, cot, n, hw, plane, vec, vec_w, vec_out, out);
}

__global__ void __launch_bounds__(256)
k_fp_init(int64_t n_records, double *acc)
{
    ws_init_body((int64_t)blockIdx.x * blockDim.x + threadIdx.x, n_records, acc);
}

template <typename S, typename F, typename W>
__global__ void __launch_bounds__(256)
k_fp_pass1(const int32_t *__restrict__ labels, FpPlanes pl, const W *__restrict__ w, int64_t n, int64_t hw, bool plane, bool vec,
           bool vec_w, int64_t n_labels, double *acc)
{
    fp_pass1_body<S, F, W>((int64_t)blockIdx.x, (int)threadIdx.x, labels, pl, w, n, hw, plane, vec, vec_w, n_labels, acc);
}

template <typename S, typename F, typename W>
__global__ void __launch_bounds__(256)
k_fp_pass2(const int32_t *__restrict__ labels, FpPlanes pl, const W *__restrict__ w, int64_t n, int64_t hw, bool plane, bool vec,
           bool vec_w, int64_t n_labels, double *acc)
{
    fp_pass2_body<S, F, W>((int64_t)blockIdx.x, (int)threadIdx.x, labels, pl, w, n, hw, plane, vec, vec_w, n_labels, acc);
}

template <typename S, typename F>
__global__ void __launch_bounds__(256)
k_fp_finish(int64_t n_labels, const double *__restrict__ acc, FpPlanes pl, int64_t n, double *__restrict__ out)
{
    fp_finish_body<S, F>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, n_labels, acc, pl, n, out);
}

static bool fp_type_ok(int dtype) { return dtype == TF_F32 || dtype == TF_F64; }

extern "C" int tf_flux_cre(const void *const *planes_host, void *const *out_host, int dtype, int64_t n, void *stream)
{
    TF_REQUIRE(planes_host && out_host && n > 0, "tf_flux_cre: bad arguments");
    TF_REQUIRE(fp_type_ok(dtype), "tf_flux_cre: the planes are float32 or float64");
    FpCrePlanes p;
    bool vec = true;
    for (int k = 0; k < FP_CRE_IN; k++) {
        TF_REQUIRE(planes_host[k], "tf_flux_cre: thirteen input planes");
        p.in[k] = planes_host[k]; vec = vec && lr_aligned16(p.in[k]);
    }
    for (int k = 0; k < FP_CRE_OUT; k++) {
        TF_REQUIRE(out_host[k], "tf_flux_cre: ten output planes");
        p.out[k] = out_host[k]; vec = vec && lr_aligned16(p.out[k]);
    }
    const int64_t lanes = (n + LR_VEC - 1) / LR_VEC, blocks = (lanes + 255) / 256;
    TF_REQUIRE(blocks <= 0x7fffffffll, "tf_flux_cre: too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == TF_F32) hipLaunchKernelGGL(k_flux_cre<float>, dim3((unsigned)blocks), dim3(256), 0, s, n, vec, p);
    else hipLaunchKernelGGL(k_flux_cre<double>, dim3((unsigned)blocks), dim3(256), 0, s, n, vec, p);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

template <typename W, typename C>
static int fp_quality_run(const void *w, const int32_t *q, const void *cth, const void *cot, int64_t n, int64_t hw, bool plane,
                          void *out, hipStream_t s)
{
    const int64_t lanes = (n + LR_VEC - 1) / LR_VEC, blocks = (lanes + 255) / 256;
    TF_REQUIRE(blocks <= 0x7fffffffll, "tf_quality_weights: too large for one launch");
    const bool vec = lr_aligned16(q) && lr_aligned16(cth) && lr_aligned16(cot);
    const bool vec_w = lr_aligned16(w) && (!plane || hw % LR_VEC == 0);
    hipLaunchKernelGGL((k_quality_weights<W, C>), dim3((unsigned)blocks), dim3(256), 0, s, (const W *)w, q, (const C *)cth,
                       (const C *)cot, n, hw, plane, vec, vec_w, lr_aligned16(out), (W *)out);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

extern "C" int tf_quality_weights(const void *weights, int weight_dtype, int weights_plane, const int32_t *qcflag, const void *cth,
                                  const void *cot, int field_dtype, int64_t T, int64_t hw, void *out, void *stream)
{
    TF_REQUIRE(weights && qcflag && cth && cot && out, "tf_quality_weights: bad arguments");
    TF_REQUIRE(fp_type_ok(weight_dtype) && fp_type_ok(field_dtype), "tf_quality_weights: weights, cth and cot are float32 or float64");
    TF_REQUIRE(T > 0 && hw > 0 && T <= 0x7fffffffffffffffll / hw, "tf_quality_weights: bad shape");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = T * hw;
    const bool plane = weights_plane != 0;
    if (weight_dtype == TF_F32)
        return field_dtype == TF_F32 ? fp_quality_run<float, float>(weights, qcflag, cth, cot, n, hw, plane, out, s)
                                     : fp_quality_run<float, double>(weights, qcflag, cth, cot, n, hw, plane, out, s);
    return field_dtype == TF_F32 ? fp_quality_run<double, float>(weights, qcflag, cth, cot, n, hw, plane, out, s)
                                 : fp_quality_run<double, double>(weights, qcflag, cth, cot, n, hw, plane, out, s);
}

// fields of a set; 0 for an unknown set or a plane count the set does not take
static int fp_set_fields(int set, int n_planes)
{
    if (set == TF_FIELDS_PLAIN) return n_planes >= 1 && n_planes <= FP_MAX_PLANES ? n_planes : 0;
    if (set == TF_FIELDS_TOA) return n_planes == FP_TOA_PLANES ? FP_TOA_FIELDS : 0;
    if (set == TF_FIELDS_BOA) return n_planes == FP_BOA_PLANES ? FP_BOA_FIELDS : 0;
    return 0;
}

extern "C" size_t tf_label_wstats_multi_workspace_bytes(int set, int n_planes, int64_t n_labels)
{
    const int nf = fp_set_fields(set, n_planes);
    if (n_labels <= 0 || nf == 0) return 0;
    return tf_align_up((size_t)nf * (size_t)n_labels * WS_REC * sizeof(double), 256) + 256;
}

template <typename S, typename F, typename W>
static int fp_run(const int32_t *labels, const FpPlanes &pl, int nf, const void *w, int64_t n, int64_t hw, bool plane,
                  int64_t n_labels, double *out, double *acc, hipStream_t s)
{
    const int64_t records = (int64_t)nf * n_labels;
    const int64_t blocks = (n + LR_BLOCK - 1) / LR_BLOCK, id_blocks = (records + 255) / 256;
    TF_REQUIRE(blocks <= 0x7fffffffll && id_blocks <= 0x7fffffffll, "tf_label_wstats_multi: volume too large for one launch");
    bool vec = lr_aligned16(labels);
    for (int p = 0; p < S::PLANES; p++) if (!S::PLAIN || p < nf) vec = vec && lr_aligned16(pl.x[p]);
    const bool vec_w = lr_aligned16(w) && (!plane || hw % LR_VEC == 0);      // then i % hw keeps the alignment of i
    hipLaunchKernelGGL(k_fp_init, dim3((unsigned)id_blocks), dim3(256), 0, s, records, acc);
    TF_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_fp_pass1<S, F, W>), dim3((unsigned)blocks), dim3(256), 0, s, labels, pl, (const W *)w, n, hw, plane, vec, vec_w, n_labels, acc);
    TF_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_fp_pass2<S, F, W>), dim3((unsigned)blocks), dim3(256), 0, s, labels, pl, (const W *)w, n, hw, plane, vec, vec_w, n_labels, acc);
    TF_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_fp_finish<S, F>), dim3((unsigned)id_blocks), dim3(256), 0, s, n_labels, (const double *)acc, pl, n, out);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

template <typename S>
static int fp_run_types(int field_dtype, int weight_dtype, const int32_t *labels, const FpPlanes &pl, int nf, const void *w,
                        int64_t n, int64_t hw, bool plane, int64_t n_labels, double *out, double *acc, hipStream_t s)
{
    if (field_dtype == TF_F32)
        return weight_dtype == TF_F32 ? fp_run<S, float, float>(labels, pl, nf, w, n, hw, plane, n_labels, out, acc, s)
                                      : fp_run<S, float, double>(labels, pl, nf, w, n, hw, plane, n_labels, out, acc, s);
    return weight_dtype == TF_F32 ? fp_run<S, double, float>(labels, pl, nf, w, n, hw, plane, n_labels, out, acc, s)
                                  : fp_run<S, double, double>(labels, pl, nf, w, n, hw, plane, n_labels, out, acc, s);
}

extern "C" int tf_label_wstats_multi(const int32_t *labels, int set, const void *const *planes_host, const void *const *errors_host,
                                     int n_planes, const void *weights, int field_dtype, int weight_dtype, int64_t T, int64_t hw,
                                     int weights_plane, int64_t n_labels, double *out, void *ws, size_t ws_bytes, void *stream)
{
    TF_REQUIRE(labels && planes_host && weights && out && n_labels > 0, "tf_label_wstats_multi: bad arguments");
    const int nf = fp_set_fields(set, n_planes);
    TF_REQUIRE(nf > 0, "tf_label_wstats_multi: TF_FIELDS_PLAIN takes 1 to 8 planes, TF_FIELDS_TOA 5, TF_FIELDS_BOA 8");
    TF_REQUIRE(set == TF_FIELDS_PLAIN || !errors_host, "tf_label_wstats_multi: only TF_FIELDS_PLAIN takes errors planes");
    TF_REQUIRE(fp_type_ok(field_dtype) && fp_type_ok(weight_dtype), "tf_label_wstats_multi: fields and weights are float32 or float64");
    TF_REQUIRE(T > 0 && hw > 0 && n_labels <= 0x7fffffffll && T <= 0x7fffffffffffffffll / hw, "tf_label_wstats_multi: bad shape");
    FpPlanes pl;
    pl.nf = nf;
    for (int p = 0; p < FP_MAX_PLANES; p++) {
        pl.x[p] = p < n_planes ? planes_host[p] : nullptr;
        pl.e[p] = (p < n_planes && errors_host) ? errors_host[p] : nullptr;
        TF_REQUIRE(p >= n_planes || pl.x[p], "tf_label_wstats_multi: a NULL input plane");
    }
    TfArena ar(ws, ws_bytes);
    double *acc = ar.take<double>((size_t)nf * (size_t)n_labels * WS_REC);
    if (!ar.ok()) { tf_set_error("tf_label_wstats_multi: workspace too small"); return TF_ENOMEM; }
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = T * hw;
    const bool plane = weights_plane != 0;
    if (set == TF_FIELDS_TOA) return fp_run_types<FpToa>(field_dtype, weight_dtype, labels, pl, nf, weights, n, hw, plane, n_labels, out, acc, s);
    if (set == TF_FIELDS_BOA) return fp_run_types<FpBoa>(field_dtype, weight_dtype, labels, pl, nf, weights, n, hw, plane, n_labels, out, acc, s);
    if (nf <= 4) return fp_run_types<FpPlain<4>>(field_dtype, weight_dtype, labels, pl, nf, weights, n, hw, plane, n_labels, out, acc, s);
    return fp_run_types<FpPlain<FP_MAX_PLANES>>(field_dtype, weight_dtype, labels, pl, nf, weights, n, hw, plane, n_labels, out, acc, s);
}
