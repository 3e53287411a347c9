// The per-voxel passes of subsegment_labels on gfx950 (tobac_flow/label.py:13-80): what lies between the integer distance
// transform (tf_edt2d_frames) and the per-frame flood (tf_watershed).
//
//   tf_subseg_prepare  label.py:52-56: dist_mask = distance to the region's edge / radius of the circle of the region's area,
//                      and the shrunk markers dist_mask > shrink_factor, from one read of the labels and squared distances
//   tf_subseg_rank     the flood's key: the rank of -dist_mask among the frame's distinct values, as float32
//
// The reference floods float64 -dist_mask; tf_watershed floods float32.  Rounding -dist_mask to float32 makes values of
// different regions equal that float64 keeps apart, and the heap's arrangement changes with them; the flood only COMPARES
// keys, so the rank -- strictly order-preserving, exact in float32 up to 2^24 distinct values -- gives the float64 flood.
// dist_mask itself has to equal numpy's bit for bit (it is thresholded, and its equal values are the peak candidates'
// ties): one correctly rounded square root of the integer d2, one of count / pi, one division, each written as such and
// compiled with -ffp-contract=off and without fast-math (no reciprocal, no fused step).
#include "tf_common.h"
#include "label_runs.h"                                           // lr_aligned16

#define SUBSEG_PI 3.141592653589793                              // np.pi
#define SUBSEG_MAX_BLOCKS ((int64_t)1 << 20)                     // grid-stride beyond that
#define SUBSEG_MAX_KEYS ((int64_t)1 << 24)                       // ranks 0 .. 2^24 - 1 are exact in float32

// ids outside [0, n_labels] have no count: they are written as background (0, 0)
__device__ __forceinline__ double subseg_dist(int32_t label, int32_t d2, const int64_t *__restrict__ counts, int64_t n_labels)
{
    if (label < 0 || (int64_t)label > n_labels) return 0.0;
    const double radius = sqrt((double)counts[label] / SUBSEG_PI);
    return sqrt((double)d2) / radius;
}

// four voxels per lane where every array is 16-byte aligned (vec), one otherwise; the last n % 4 voxels one per lane
__global__ void __launch_bounds__(256)
k_subseg_prepare(const int32_t *__restrict__ labels, const int32_t *__restrict__ d2, const int64_t *__restrict__ counts,
                 int64_t n_labels, int64_t n, bool vec, double shrink, double *__restrict__ dist, uint8_t *__restrict__ shrunk)
{
    const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = (int64_t)gridDim.x * blockDim.x;
    const int64_t groups = vec ? n / 4 : 0;
    for (int64_t g = lane; g < groups; g += lanes) {
        const int4 l = ((const int4 *)labels)[g], q = ((const int4 *)d2)[g];
        const double a = subseg_dist(l.x, q.x, counts, n_labels), b = subseg_dist(l.y, q.y, counts, n_labels);
        const double c = subseg_dist(l.z, q.z, counts, n_labels), d = subseg_dist(l.w, q.w, counts, n_labels);
        ((double2 *)dist)[2 * g] = make_double2(a, b);
        ((double2 *)dist)[2 * g + 1] = make_double2(c, d);
        ((uchar4 *)shrunk)[g] = make_uchar4(a > shrink, b > shrink, c > shrink, d > shrink);
    }
    for (int64_t i = groups * 4 + lane; i < n; i += lanes) {
        const double a = subseg_dist(labels[i], d2[i], counts, n_labels);
        dist[i] = a;
        shrunk[i] = a > shrink;
    }
}

// rank[i] = n_keys - 1 - (index of values[i] in keys): keys ascending and distinct, so this is the rank of -values[i]
// among the ascending distinct -keys.  A value that is not a key (the caller's mistake; NaN) gets the rank of the first key
// that is not below it, clamped to the array: every read stays inside keys[0 .. n_keys - 1].
__global__ void __launch_bounds__(256)
k_subseg_rank(const double *__restrict__ values, int64_t n, const double *__restrict__ keys, int64_t n_keys, float *__restrict__ rank)
{
    const int64_t lanes = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += lanes) {
        const double v = values[i];
        int64_t lo = 0, hi = n_keys - 1;                         // the answer lies in [lo, hi]
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (keys[mid] < v) lo = mid + 1;
            else hi = mid;
        }
        rank[i] = (float)(n_keys - 1 - lo);
    }
}

static unsigned subseg_blocks(int64_t work)
{
    const int64_t blocks = (work + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : (blocks < SUBSEG_MAX_BLOCKS ? blocks : SUBSEG_MAX_BLOCKS));
}

extern "C" int tf_subseg_prepare(const int32_t *labels, const int32_t *d2, const int64_t *counts, int64_t n_labels, int64_t n,
                                 double shrink_factor, double *dist_mask, uint8_t *shrunk, void *stream)
{
    TF_REQUIRE(labels && d2 && counts && dist_mask && shrunk, "tf_subseg_prepare: bad arguments");
    TF_REQUIRE(n > 0 && n_labels >= 0 && n_labels <= 0x7fffffffll, "tf_subseg_prepare: bad shape or label count");
    TF_REQUIRE(shrink_factor == shrink_factor, "tf_subseg_prepare: shrink_factor is NaN");
    const bool vec = lr_aligned16(labels) && lr_aligned16(d2) && lr_aligned16(dist_mask) && (((uintptr_t)shrunk) & 3) == 0;
    hipLaunchKernelGGL(k_subseg_prepare, dim3(subseg_blocks(vec ? (n + 3) / 4 : n)), dim3(256), 0, (hipStream_t)stream, labels, d2,
                       counts, n_labels, n, vec, shrink_factor, dist_mask, shrunk);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

extern "C" int tf_subseg_rank(const double *values, int64_t n, const double *sorted_keys, int64_t n_keys, float *rank, void *stream)
{
    TF_REQUIRE(values && sorted_keys && rank && n > 0 && n_keys > 0, "tf_subseg_rank: bad arguments");
    if (n_keys > SUBSEG_MAX_KEYS) {
        tf_set_error("tf_subseg_rank: %lld distinct keys in one frame; a float32 rank is exact up to 2^24 of them", (long long)n_keys);
        return TF_EINVAL;
    }
    hipLaunchKernelGGL(k_subseg_rank, dim3(subseg_blocks(n)), dim3(256), 0, (hipStream_t)stream, values, n, sorted_keys, n_keys, rank);
    TF_CHECK_LAUNCH();
    return TF_OK;
}
