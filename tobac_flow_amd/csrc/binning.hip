// Point observations onto a grid on gfx950: the array-level binning under the reference's GLM, NEXRAD and flux gridding.
//
//   tf_bin_points   np.histogram2d per frame of tobac_flow/glm.py:77-145, the two np.histogram2d and the
//                   scipy.stats.binned_statistic_dd per site and frame of tobac_flow/nexrad.py:80-231, the two
//                   binned_statistic_2d sums per variable of scripts/grid_flux.py:65-112
//
// The libraries run a bincount over all (H + 2) (W + 2) bins per call and re-mask all points per frame; here one pass over
// the points writes counts, masked counts and both sums of every frame.  The kernel body and the work layout are in
// bin_kernels.h.
#include "tf_common.h"
#include "bin_kernels.h"

template <typename C>
__global__ void __launch_bounds__(256)
k_bin_points(const TfBinPoints p)
{
    bn_points_body<C>((int64_t)blockIdx.x, (int)threadIdx.x, p);
}

static bool bn_real(int dtype) { return dtype == TF_F32 || dtype == TF_F64; }

extern "C" int tf_bin_points(const TfBinPoints *params_host, void *stream)
{
    TF_REQUIRE(params_host, "tf_bin_points: bad arguments");
    const TfBinPoints p = *params_host;
    TF_REQUIRE(p.n_dims >= 1 && p.n_dims <= TF_BIN_MAX_DIMS, "tf_bin_points: 1 to 3 coordinate arrays");
    TF_REQUIRE(bn_real(p.coord_dtype), "tf_bin_points: the coordinates are float32 or float64");
    TF_REQUIRE(p.rule == TF_BIN_RULE_NUMPY || p.rule == TF_BIN_RULE_SCIPY, "tf_bin_points: unknown last-edge rule");
    TF_REQUIRE((p.flags & ~TF_BIN_FINITE_VALUE) == 0, "tf_bin_points: unknown flag");
    TF_REQUIRE(p.n_points >= 0 && p.n_points < 0x80000000ll, "tf_bin_points: fewer than 2^31 points per call");
    TF_REQUIRE(p.flip_mask >= 0 && p.flip_mask < (1 << p.n_dims), "tf_bin_points: flip_mask names an axis that is not there");
    TF_REQUIRE(p.n_frames >= 1, "tf_bin_points: bad number of frames");
    const bool windows = p.time || p.win_start || p.win_end;
    TF_REQUIRE(!windows || ((p.time || p.n_points == 0) && p.win_start && p.win_end), "tf_bin_points: time, win_start and win_end go together");
    TF_REQUIRE(windows || p.n_frames == 1, "tf_bin_points: several frames need time windows");
    int64_t cells = p.n_frames;
    for (int d = 0; d < p.n_dims; d++) {
        TF_REQUIRE((p.coord[d] || p.n_points == 0) && p.edges[d], "tf_bin_points: a coordinate or edge array is missing");
        TF_REQUIRE(p.n_edges[d] >= 2, "tf_bin_points: an axis needs at least 2 edges");
        TF_REQUIRE(p.n_edges[d] - 1 <= 0x7fffffffffffffffll / cells, "tf_bin_points: the grid is too large");
        cells *= p.n_edges[d] - 1;
        TF_REQUIRE(p.rule != TF_BIN_RULE_SCIPY || (p.round_scale[d] >= 1 && p.round_scale[d] - p.round_scale[d] == 0),
                   "tf_bin_points: round_scale is 10^|decimals|");
    }
    TF_REQUIRE(!p.value || bn_real(p.value_dtype), "tf_bin_points: the values are float32 or float64");
    TF_REQUIRE(!p.weight || bn_real(p.weight_dtype), "tf_bin_points: the weights are float32 or float64");
    TF_REQUIRE(!p.sum_wv || p.value || p.n_points == 0, "tf_bin_points: sum_wv needs values");
    TF_REQUIRE(p.count || p.count_v || p.sum_w || p.sum_wv, "tf_bin_points: no output");
    if (p.n_points == 0) return TF_OK;
    const int64_t blocks = (p.n_points + LR_BLOCK - 1) / LR_BLOCK;
    hipStream_t s = (hipStream_t)stream;
    if (p.coord_dtype == TF_F32)
        hipLaunchKernelGGL(k_bin_points<float>, dim3((unsigned)blocks), dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL(k_bin_points<double>, dim3((unsigned)blocks), dim3(256), 0, s, p);
    TF_CHECK_LAUNCH();
    return TF_OK;
}
