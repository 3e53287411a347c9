// bt, wvd and swd from raw channel stacks on gfx950: the array-level work under the reference's loaders.
//
//   tf_stripe_deviation   get_stripe_deviation of tobac_flow/dataloader.py:234-237 for one DQF plane, with xarray's skipna
//                         rule: exact integer column counts and sums, np.nanstd's own second pass down every column, then one
//                         float64 row sum in a fixed order
//   tf_prepare_fields     the channel differences, the joint non-finite / DQF / stripe mask of load_mcmip (:260-313),
//                         seviri_dataloader (:640-653) and seviri_nat_dataloader (:875-884), the sort of :316-317, the
//                         dropped frames of goes_dataloader:78-94 and the NaN frames of fill_time_gap_nan (:341-357) in
//                         one pass: output frame k is written from input frame src[k]
//
// The kernel bodies and the work layouts are in field_kernels.h.
#include "tf_common.h"
#include "field_kernels.h"

__global__ void __launch_bounds__(FK_THREADS)
k_stripe_columns(const FkColumns p)
{
    __shared__ int32_t sh[2 * FK_COL_SPAN];
    fk_stripe_columns_body(p, (int)blockIdx.x, (int)blockIdx.y, (int64_t)blockIdx.z, (int)threadIdx.x, sh);
}

__global__ void __launch_bounds__(FK_THREADS)
k_stripe_variance(const FkVariance p)
{
    fk_stripe_variance_body(p, (int64_t)blockIdx.x * FK_THREADS + threadIdx.x);
}

__global__ void __launch_bounds__(FK_THREADS)
k_stripe_rows(const FkRows p)
{
    __shared__ double sh_sum[FK_THREADS];
    __shared__ int32_t sh_cnt[FK_THREADS];
    fk_stripe_rows_body(p, (int64_t)blockIdx.x, (int)threadIdx.x, sh_sum, sh_cnt);
}

template <bool PACKED, bool HAS_DQF>
__global__ void __launch_bounds__(FK_THREADS)
k_prepare_fields(const TfFieldPrep p, int64_t k0)
{
    __shared__ int32_t sh_cnt[4];
    fk_prepare_body<PACKED, HAS_DQF>(p, k0 + (int64_t)blockIdx.y, (int64_t)blockIdx.x, (int)threadIdx.x, sh_cnt);
}

// ---- argument checks -------------------------------------------------------------------------------------------------
static bool fk_shape_ok(int64_t T, int64_t H, int64_t W)
{
    // H < 2^24 keeps a column's count and sum exact in the tables and in float64; H W < 2^31 keeps a frame inside one grid
    return T >= 1 && H >= 1 && W >= 1 && H < (1ll << 24) && W < (1ll << 31) && H * W < (1ll << 31) && T < (1ll << 31) &&
           T <= 0x7fffffffffffffffll / (H * W);
}

// a plane whose rows do not overlap and whose elements are aligned to their size
static bool fk_plane_ok(const TfFieldPlane &c, int64_t T, int64_t H, int64_t W, bool dqf)
{
    if (!c.data) return false;
    const bool type_ok = dqf ? (c.dtype == TF_I8 || c.dtype == TF_U8) : (c.dtype == TF_F32 || c.dtype == TF_I16);
    if (!type_ok) return false;
    const uintptr_t size = c.dtype == TF_F32 ? 4 : c.dtype == TF_I16 ? 2 : 1;
    if (((uintptr_t)c.data) % size) return false;
    if (c.row_stride < W || (H > 1 && c.frame_stride < c.row_stride) || (T > 1 && c.frame_stride < 1)) return false;
    if (c.frame_stride < 0 || c.frame_stride > 0x7fffffffffffffffll / (T * 8)) return false;
    if (c.has_fill) {
        if (c.dtype == TF_I16 && (c.is_unsigned ? (c.fill < 0 || c.fill > 65535) : (c.fill < -32768 || c.fill > 32767))) return false;
        if (c.dtype == TF_I8 && (c.fill < -128 || c.fill > 127)) return false;
        if (c.dtype == TF_U8 && (c.fill < 0 || c.fill > 255)) return false;
    }
    return true;
}

// ---- tf_stripe_deviation ---------------------------------------------------------------------------------------------
extern "C" size_t tf_stripe_workspace_bytes(int64_t T, int64_t H, int64_t W)
{
    if (!fk_shape_ok(T, H, W)) return 0;
    return 4 * tf_align_up((size_t)(T * W) * 8, 256);             // count, sum (int64); mean, denominator (double)
}

extern "C" int tf_stripe_deviation(const TfFieldPlane *dqf, int64_t T, int64_t H, int64_t W, double threshold, double *dev,
                                   uint8_t *row_flags, void *ws, size_t ws_bytes, void *stream)
{
    TF_REQUIRE(dqf && ws, "tf_stripe_deviation: bad arguments");
    TF_REQUIRE(fk_shape_ok(T, H, W), "tf_stripe_deviation: T, H, W >= 1, H < 2^24, H W < 2^31");
    TF_REQUIRE(T <= 65535 && T * H < (1ll << 31), "tf_stripe_deviation: at most 65535 frames and 2^31 - 1 rows per call");
    TF_REQUIRE(fk_plane_ok(*dqf, T, H, W, true), "tf_stripe_deviation: the plane is int8 or uint8 with row_stride >= W, frame_stride >= row_stride and a fill inside its type");
    TF_REQUIRE(threshold == threshold, "tf_stripe_deviation: the threshold is NaN");
    if (ws_bytes < tf_stripe_workspace_bytes(T, H, W)) { tf_set_error("tf_stripe_deviation: workspace too small"); return TF_ENOMEM; }
    TfArena arena(ws, ws_bytes);
    const size_t n = (size_t)(T * W);
    unsigned long long *cnt = arena.take<unsigned long long>(n), *sum = arena.take<unsigned long long>(n);
    double *mean = arena.take<double>(n), *denom = arena.take<double>(n);
    if (!arena.ok()) { tf_set_error("tf_stripe_deviation: workspace too small"); return TF_ENOMEM; }
    hipStream_t s = (hipStream_t)stream;
    const double plane_bytes = (double)T * (double)H * (double)W;
    {
        TfProfScope ps(TFK_STRIPE_COLUMNS, 2.0 * plane_bytes + 32.0 * (double)n, s);
        TF_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)((char *)(sum + n) - (char *)cnt), s));     // both tables and the padding between them
        FkColumns c{(const uint8_t *)dqf->data, dqf->frame_stride, dqf->row_stride, dqf->dtype == TF_I8, dqf->has_fill, dqf->fill, H, W, cnt, sum};
        const dim3 grid((unsigned)((W + FK_COL_SPAN - 1) / FK_COL_SPAN), (unsigned)((H + FK_COL_ROWS - 1) / FK_COL_ROWS), (unsigned)T);
        hipLaunchKernelGGL(k_stripe_columns, grid, dim3(FK_THREADS), 0, s, c);
        TF_CHECK_LAUNCH();
        FkVariance v{(const uint8_t *)dqf->data, dqf->frame_stride, dqf->row_stride, dqf->dtype == TF_I8, dqf->has_fill, dqf->fill, H, W, (int64_t)n,
                     cnt, sum, mean, denom};
        hipLaunchKernelGGL(k_stripe_variance, dim3((unsigned)((n + FK_THREADS - 1) / FK_THREADS)), dim3(FK_THREADS), 0, s, v);
        TF_CHECK_LAUNCH();
    }
    {
        TfProfScope ps(TFK_STRIPE_ROWS, plane_bytes + 16.0 * (double)n + (dev ? 8.0 : 0.0) * (double)(T * H), s);
        FkRows r{(const uint8_t *)dqf->data, dqf->frame_stride, dqf->row_stride, dqf->dtype == TF_I8, dqf->has_fill, dqf->fill, H, W, mean, denom,
                 threshold, dev, row_flags};
        hipLaunchKernelGGL(k_stripe_rows, dim3((unsigned)(T * H)), dim3(FK_THREADS), 0, s, r);
        TF_CHECK_LAUNCH();
    }
    return TF_OK;
}

// ---- tf_prepare_fields -----------------------------------------------------------------------------------------------
extern "C" int tf_prepare_fields(const TfFieldPrep *params_host, void *stream)
{
    TF_REQUIRE(params_host, "tf_prepare_fields: bad arguments");
    const TfFieldPrep p = *params_host;
    TF_REQUIRE(fk_shape_ok(p.T, p.H, p.W), "tf_prepare_fields: T, H, W >= 1, H < 2^24, H W < 2^31");
    TF_REQUIRE(p.T_out >= 1 && p.T_out < (1ll << 31) && p.T_out <= 0x7fffffffffffffffll / (p.H * p.W * 4), "tf_prepare_fields: bad number of output frames");
    TF_REQUIRE(p.src, "tf_prepare_fields: the frame table is missing");
    TF_REQUIRE((p.flags & ~TF_FIELD_COPY) == 0, "tf_prepare_fields: unknown flag");
    TF_REQUIRE(!(p.flags & TF_FIELD_COPY) || (p.n_dqf == 0 && !p.row_flags && !p.n_masked), "tf_prepare_fields: TF_FIELD_COPY takes no DQF plane, no row flags and counts nothing");
    TF_REQUIRE(p.n_channels >= 1 && p.n_channels <= TF_FIELD_MAX_CHANNELS, "tf_prepare_fields: 1 to 8 channels");
    TF_REQUIRE(p.n_dqf >= 0 && p.n_dqf <= TF_FIELD_MAX_DQF, "tf_prepare_fields: at most 8 DQF planes");
    TF_REQUIRE(p.n_recipes >= 1 && p.n_recipes <= TF_FIELD_MAX_RECIPES, "tf_prepare_fields: 1 to 4 outputs");
    for (int c = 0; c < p.n_channels; c++) {
        TF_REQUIRE(fk_plane_ok(p.channel[c], p.T, p.H, p.W, false), "tf_prepare_fields: a channel is float32 or packed int16 with row_stride >= W, frame_stride >= row_stride and a fill inside its type");
        TF_REQUIRE(p.channel[c].dtype == p.channel[0].dtype, "tf_prepare_fields: the channels are all float32 or all packed");
    }
    for (int d = 0; d < p.n_dqf; d++)
        TF_REQUIRE(fk_plane_ok(p.dqf[d], p.T, p.H, p.W, true), "tf_prepare_fields: a DQF plane is int8 or uint8 with row_stride >= W, frame_stride >= row_stride and a fill inside its type");
    for (int r = 0; r < p.n_recipes; r++) {
        const TfFieldRecipe &rc = p.recipe[r];
        TF_REQUIRE(rc.a >= 0 && rc.a < p.n_channels && rc.b >= -1 && rc.b < p.n_channels, "tf_prepare_fields: a recipe names a channel that is not there");
        TF_REQUIRE(rc.out && ((uintptr_t)rc.out & 3) == 0, "tf_prepare_fields: an output is missing");
        TF_REQUIRE(!rc.has_floor || rc.floor == rc.floor, "tf_prepare_fields: a floor is NaN");
    }
    hipStream_t s = (hipStream_t)stream;
    const bool packed = p.channel[0].dtype == TF_I16, has_dqf = p.n_dqf > 0 || p.row_flags;
    // algorithmic bytes: every operand of every recipe once, the DQF planes, the outputs
    double in_px = 0;
    for (int r = 0; r < p.n_recipes; r++) in_px += (p.recipe[r].b >= 0 ? 2.0 : 1.0) * (packed ? 2.0 : 4.0);
    const double voxels = (double)p.T_out * (double)p.H * (double)p.W;
    TfProfScope ps(TFK_PREPARE_FIELDS, voxels * (in_px + (double)p.n_dqf + 4.0 * p.n_recipes), s);
    if (p.n_masked) TF_CHECK_HIP(hipMemsetAsync(p.n_masked, 0, (size_t)p.T_out * sizeof(int32_t), s));
    const int64_t blocks = (p.H * p.W + 3 + FK_VEC * FK_THREADS - 1) / (FK_VEC * FK_THREADS);
    for (int64_t k0 = 0; k0 < p.T_out; k0 += 65535) {
        const dim3 grid((unsigned)blocks, (unsigned)(p.T_out - k0 < 65535 ? p.T_out - k0 : 65535));
        if (packed && has_dqf) hipLaunchKernelGGL((k_prepare_fields<true, true>), grid, dim3(FK_THREADS), 0, s, p, k0);
        else if (packed) hipLaunchKernelGGL((k_prepare_fields<true, false>), grid, dim3(FK_THREADS), 0, s, p, k0);
        else if (has_dqf) hipLaunchKernelGGL((k_prepare_fields<false, true>), grid, dim3(FK_THREADS), 0, s, p, k0);
        else hipLaunchKernelGGL((k_prepare_fields<false, false>), grid, dim3(FK_THREADS), 0, s, p, k0);
        TF_CHECK_LAUNCH();
    }
    return TF_OK;
}
