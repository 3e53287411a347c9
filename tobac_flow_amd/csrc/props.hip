// Per-label properties and coverage maps of the detection output files on gfx950.
//
//   tf_label_props       tobac_flow/dataset.py:705-1595 calculate_label_properties: everything that function asks of one
//                        label volume -- np.bincount, labeled_comprehension(area, np.nansum), labeled_comprehension(t,
//                        np.nanmin / np.nanmax) and the four np.average(..., weights=area) of x, y, lat, lon -- as ONE
//                        read of the volume
//   tf_unique_along_t    tobac_flow/utils/stats_utils.py:23-30 n_unique_along_axis(a, 0) and np.count_nonzero(a, 0)
//   tf_unique_per_frame  n_unique_along_axis(a.reshape(T, -1), 1) and np.count_nonzero(a, (1, 2)) (analysis.py:245-290)
//
// Every operand of the properties except the labels varies with (y, x) only (area, lat, lon), with x or y only, or with t
// only, so nothing of the volume's size is read besides the labels (4 B per voxel) and nothing of that size is allocated:
// the reference's np.repeat stacks never exist.  The (H, W) planes are read only under labelled voxels.
#include "tf_common.h"
#include "label_runs.h"
#include <algorithm>

// ---- tf_label_props ------------------------------------------------------------------------------------------------
// The row-chunk layout and walker of label_runs.h (lr_walk_row): one lane takes LR_ROW_RUN consecutive voxels of one row
// and issues one set of atomics per run of equal labels inside them; why runs are not merged across the wave is said
// there (here the scan would carry seven doubles per lane).
// Record per label id (PR_REC doubles = 64 B, so one label's atomics fall into one 64-B line):
//   0 count (int64)  1 sum area (NaN skipped)  2 sum area  3 sum area*x  4 sum area*y  5 sum area*lat  6 sum area*lon
//   7 {tmin, tmax} (two int32)
#define PR_REC 8

struct PrIn { const double *area, *x, *y, *lat, *lon; const int32_t *t_rank; };

__global__ void __launch_bounds__(256)
k_props_init(double *__restrict__ acc, int64_t n_ids)
{
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_ids) return;
    double *r = acc + PR_REC * l;
    for (int k = 0; k < 7; k++) r[k] = 0.0;                      // +0.0 and int64 0 share their bits
    int *tm = (int *)(r + 7);
    tm[0] = 0x7fffffff; tm[1] = -1;
}

struct PrRun {
    const PrIn in; int W; double *acc;
    bool has_loc; int64_t p0; int x0, rank; double yv;         // of the chunk: p0 = its first pixel of the (H, W) planes
    unsigned long long cnt = 0;
    double an = 0, sw = 0, sx = 0, sy = 0, slat = 0, slon = 0;

    __device__ __forceinline__ void begin(int t, int y, int x0_)
    {
        has_loc = in.x || in.y || in.lat || in.lon;
        x0 = x0_; p0 = (int64_t)y * W + x0_;
        yv = in.y ? in.y[y] : 0.0;
        rank = in.t_rank ? in.t_rank[t] : 0;
    }
    __device__ __forceinline__ bool ends(int) const { return false; }
    __device__ __forceinline__ void open(int32_t, bool, int) { cnt = 0; an = sw = sx = sy = slat = slon = 0; }
    __device__ __forceinline__ void add(int64_t, int j)
    {
        cnt++;
        if (!in.area) return;
        const int64_t p = p0 + j;
        const double a = in.area[p];
        if (!(a != a)) an += a;
        sw += a;
        if (has_loc) {
            if (in.x) sx += a * in.x[x0 + j];
            if (in.y) sy += a * yv;
            if (in.lat) slat += a * in.lat[p];
            if (in.lon) slon += a * in.lon[p];
        }
    }
    __device__ __forceinline__ void close(int32_t cur)
    {
        if (!cnt) return;                                         // cur is in [1, n_labels] whenever cnt != 0
        double *r = acc + PR_REC * (int64_t)cur;
        atomicAdd((unsigned long long *)r, cnt);
        if (in.area) {
            if (an != 0) atomicAdd(r + 1, an);
            if (sw != 0) atomicAdd(r + 2, sw);                    // NaN != 0: it propagates
            if (in.x && sx != 0) atomicAdd(r + 3, sx);
            if (in.y && sy != 0) atomicAdd(r + 4, sy);
            if (in.lat && slat != 0) atomicAdd(r + 5, slat);
            if (in.lon && slon != 0) atomicAdd(r + 6, slon);
        }
        if (in.t_rank) {
            int *tm = (int *)(r + 7);                             // a stale read only costs a redundant atomic
            if (tm[0] > rank) atomicMin(&tm[0], rank);
            if (tm[1] < rank) atomicMax(&tm[1], rank);
        }
        cnt = 0;
    }
};

template <bool ALIGNED>
__global__ void __launch_bounds__(256)
k_label_props(const int32_t *__restrict__ labels, int64_t n_chunks, int H, int W, int chunks_per_row, int64_t n_labels,
              PrIn in, double *acc)
{
    PrRun v{in, W, acc};
    lr_walk_row<ALIGNED>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, labels, n_chunks, H, W, chunks_per_row, n_labels, v);
}

extern "C" int tf_label_props(const int32_t *labels, int64_t T, int64_t H, int64_t W, int64_t n_labels,
                              const double *area, const double *x, const double *y, const double *lat, const double *lon,
                              const int32_t *t_rank, double *acc, void *stream)
{
    TF_REQUIRE(labels && acc && n_labels >= 0, "tf_label_props: bad arguments");
    LrRowGrid g;
    if (const char *bad = lr_row_grid(labels, T, H, W, &g)) { tf_set_error("tf_label_props: %s", bad); return TF_EINVAL; }
    TF_REQUIRE(area || !(x || y || lat || lon), "tf_label_props: x, y, lat and lon are weighted by area");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_ids = n_labels + 1;
    hipLaunchKernelGGL(k_props_init, dim3((unsigned)((n_ids + 255) / 256)), dim3(256), 0, s, acc, n_ids);
    TF_CHECK_LAUNCH();
    const PrIn in{area, x, y, lat, lon, t_rank};
    hipLaunchKernelGGL(g.aligned ? k_label_props<true> : k_label_props<false>, dim3(g.blocks), dim3(256), 0, s, labels, g.n_chunks,
                       (int)H, (int)W, g.chunks_per_row, n_labels, in, acc);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

// ---- tf_unique_along_t ---------------------------------------------------------------------------------------------
// One lane per pixel, consecutive lanes on consecutive pixels (coalesced reads of every frame).  The lane walks t, skips
// zeros and repeats of the value just seen, and otherwise searches the set of distinct values it has met so far,
// appending on a miss.  The set has room for T values per pixel, so it cannot overflow.  It is laid out [k][lane]: in LDS
// (stride = lanes of the workgroup, conflict-free) while T * 4 B * lanes fits the CU's 160 KiB, in the caller's scratch
// (stride = H * W, coalesced) beyond that.
#define UT_LDS_BYTES 163840

static int ut_lanes(int64_t T)                                    // pixels per workgroup of the LDS form; 0 = scratch form
{
    for (int lanes = 256; lanes >= 64; lanes >>= 1)
        if (T * 4 * lanes <= UT_LDS_BYTES) return lanes;
    return 0;
}

template <bool IN_LDS>
__global__ void __launch_bounds__(256)
k_unique_along_t(const int32_t *__restrict__ vol, int T, int64_t hw, int32_t *__restrict__ scratch,
                 int32_t *__restrict__ uniq, int32_t *__restrict__ nonzero)
{
    extern __shared__ int32_t ut_lds[];
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= hw) return;
    int32_t *set; int64_t stride;
    if (IN_LDS) { set = ut_lds + threadIdx.x; stride = blockDim.x; }
    else { set = scratch + p; stride = hw; }
    int n = 0, nz = 0; int32_t prev = 0;
    for (int t = 0; t < T; t++) {
        const int32_t v = vol[(int64_t)t * hw + p];
        if (v == 0) { prev = 0; continue; }
        nz++;
        if (v == prev) continue;
        prev = v;
        int k = 0;
        while (k < n && set[k * stride] != v) k++;
        if (k == n) { set[n * stride] = v; n++; }                 // n <= number of frames walked <= T
    }
    uniq[p] = n; nonzero[p] = nz;
}

extern "C" size_t tf_unique_along_t_workspace_bytes(int64_t T, int64_t H, int64_t W)
{
    if (T <= 0 || H <= 0 || W <= 0) return 0;
    return ut_lanes(T) ? 0 : (size_t)T * (size_t)H * (size_t)W * 4;
}

extern "C" int tf_unique_along_t(const int32_t *vol, int64_t T, int64_t H, int64_t W, int32_t *unique, int32_t *nonzero,
                                 int *lanes_host, void *ws, size_t ws_bytes, void *stream)
{
    TF_REQUIRE(vol && unique && nonzero, "tf_unique_along_t: null pointer");
    TF_REQUIRE(T > 0 && T < 65536 && H > 0 && W > 0, "tf_unique_along_t: bad shape");
    hipStream_t s = (hipStream_t)stream;
    const int64_t hw = H * W;
    const int lanes = ut_lanes(T);
    if (lanes_host) *lanes_host = lanes;
    if (lanes) {
        const size_t lds = (size_t)T * 4 * lanes;
        {
            static TfDeviceOnce once;                             // function attributes are per device
            TfDeviceOnce::Guard guard(once);
            if (guard.first) {
                TF_CHECK_HIP(hipFuncSetAttribute((const void *)k_unique_along_t<true>, hipFuncAttributeMaxDynamicSharedMemorySize, UT_LDS_BYTES));
                guard.done();
            }
        }
        const int64_t blocks = (hw + lanes - 1) / lanes;
        TF_REQUIRE(blocks <= 0x7fffffffll, "tf_unique_along_t: frame too large for one launch");
        hipLaunchKernelGGL(k_unique_along_t<true>, dim3((unsigned)blocks), dim3(lanes), lds, s, vol, (int)T, hw, (int32_t *)nullptr, unique, nonzero);
    } else {
        if (!ws || ws_bytes < (size_t)T * (size_t)hw * 4) { tf_set_error("tf_unique_along_t: workspace too small"); return TF_ENOMEM; }
        const int64_t blocks = (hw + 255) / 256;
        TF_REQUIRE(blocks <= 0x7fffffffll, "tf_unique_along_t: frame too large for one launch");
        hipLaunchKernelGGL(k_unique_along_t<false>, dim3((unsigned)blocks), dim3(256), 0, s, vol, (int)T, hw, (int32_t *)ws, unique, nonzero);
    }
    TF_CHECK_LAUNCH();
    return TF_OK;
}

// ---- tf_unique_per_frame -------------------------------------------------------------------------------------------
// A stamp per label id; the frames are launched one after the other on the stream, frame t stamping t + 1: the lane whose
// exchange returns another value is the first of frame t to meet that label and counts it.  Exchanges are issued at the
// start of a run of equal labels inside a lane's 8 consecutive voxels only, and not at all where a plain read already
// shows this frame's stamp (a stale read costs a redundant exchange, never a miscount).
#define UF_RUN 8
__global__ void __launch_bounds__(256)
k_unique_frame(const int32_t *__restrict__ frame, int64_t hw, int64_t n_labels, int *stamp, int mark,
               int32_t *__restrict__ uniq, unsigned long long *__restrict__ nonzero)
{
    __shared__ unsigned part[2][4];
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * UF_RUN;
    unsigned first = 0, nz = 0;
    int32_t prev = 0;
    for (int j = 0; j < UF_RUN && i0 + j < hw; j++) {
        const int32_t l = frame[i0 + j];
        nz += l != 0;
        if (l != prev && l >= 1 && l <= n_labels && stamp[l] != mark) first += atomicExch(&stamp[l], mark) != mark;
        prev = l;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { first += __shfl_down(first, d); nz += __shfl_down(nz, d); }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = first; part[1][threadIdx.x >> 6] = nz; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned f = part[0][0] + part[0][1] + part[0][2] + part[0][3], z = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        if (f) atomicAdd(uniq, (int32_t)f);
        if (z) atomicAdd(nonzero, (unsigned long long)z);
    }
}

extern "C" size_t tf_unique_per_frame_workspace_bytes(int64_t n_labels)
{
    if (n_labels < 0) return 0;
    return tf_align_up((size_t)(n_labels + 1) * 4, 256) + 256;
}

extern "C" int tf_unique_per_frame(const int32_t *vol, int64_t T, int64_t hw, int64_t n_labels, int32_t *unique,
                                   int64_t *nonzero, void *ws, size_t ws_bytes, void *stream)
{
    TF_REQUIRE(vol && unique && nonzero && ws && n_labels >= 0, "tf_unique_per_frame: bad arguments");
    TF_REQUIRE(T > 0 && T < 65536 && hw > 0, "tf_unique_per_frame: bad shape");
    hipStream_t s = (hipStream_t)stream;
    TfArena ar(ws, ws_bytes);
    int *stamp = ar.take<int>(n_labels + 1);
    if (!ar.ok()) { tf_set_error("tf_unique_per_frame: workspace too small"); return TF_ENOMEM; }
    const int64_t blocks = (hw + 256 * UF_RUN - 1) / (256 * UF_RUN);
    TF_REQUIRE(blocks <= 0x7fffffffll, "tf_unique_per_frame: frame too large for one launch");
    TF_CHECK_HIP(hipMemsetAsync(stamp, 0, (size_t)(n_labels + 1) * 4, s));
    TF_CHECK_HIP(hipMemsetAsync(unique, 0, (size_t)T * sizeof(int32_t), s));
    TF_CHECK_HIP(hipMemsetAsync(nonzero, 0, (size_t)T * sizeof(int64_t), s));
    for (int64_t t = 0; t < T; t++)
        hipLaunchKernelGGL(k_unique_frame, dim3((unsigned)blocks), dim3(256), 0, s, vol + t * hw, hw, n_labels, stamp, (int)(t + 1),
                           unique + t, (unsigned long long *)(nonzero + t));
    TF_CHECK_LAUNCH();
    return TF_OK;
}
