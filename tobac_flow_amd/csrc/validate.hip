// The fourth stage on gfx950: a detection product validated against gridded GLM flashes (tobac_flow/validation.py:107-219
// as scripts/dcc_validation.py:145-250 drives it).  Three pieces that keep the stage from materialising volumes which are
// only read at the few voxels that hold a flash:
//
//   tf_flash_count / tf_flash_list   np.repeat(np.arange(n), grid.astype(int).ravel()): the voxel of every flash, in order.
//                    Phase one sums the truncated counts per tile of FL_TILE voxels, flags a count that np.repeat refuses
//                    and scans the tile sums (integers throughout: the list is the same in every run); the host reads the
//                    total; phase two visits the tiles that hold a flash and fills their part of the list output-driven:
//                    lane j of the tile's flashes searches the tile's prefix sums for its voxel, so one voxel with
//                    thousands of flashes is written by the whole workgroup, not by one lane.
//   tf_edt_cylinder_at   tf_edt_cylinder evaluated at a voxel list: the minimum over the time window, its square root, the
//                    label of the nearest marker, and the number of flashes within the margin (an integer atomic).
//   tf_grid_has_missing / tf_edge_filter   validation.py:173-219 get_edge_filter: the borders in time and space, the frames
//                    the host marks around a time gap, and SciPy's binary_dilation of grid == -1 with the reference's
//                    structure for every margin: a time-window OR, a prefix count along each row, and per output voxel one
//                    span lookup per row of the footprint.
#include "tf_common.h"

#define FL_TILE 2048                                              // voxels per workgroup: 256 lanes x 8
#define FL_LANES 256
#define FL_PER_LANE (FL_TILE / FL_LANES)
#define FL_MAX_COUNT 2147483648.0                                 // a count from here on is refused (the list could not be held)
#define FL_WS_HEAD 2                                              // int64 words in front of the tile offsets: total, bad flag

// the flash count of one voxel: truncated toward zero.  `bad` collects FL_BAD_NEGATIVE where np.repeat refuses the count
// (< 0 or NaN, before truncation) and FL_BAD_HUGE where it is >= 2^31
#define FL_BAD_NEGATIVE 1
#define FL_BAD_HUGE 2
template <typename E>
__device__ __forceinline__ int64_t fl_count(E v, int &bad)
{
    const bool counts = v >= (E)0, fits = (double)v < FL_MAX_COUNT;      // both false for NaN
    bad |= !counts ? FL_BAD_NEGATIVE : (!fits ? FL_BAD_HUGE : 0);
    return counts && fits ? (int64_t)v : 0;
}

// inclusive sum over the workgroup's 256 lanes; `total` = the sum of all of them.  wave_sums: 4 words of LDS
__device__ __forceinline__ int64_t fl_block_scan(int64_t v, int tid, int64_t *wave_sums, int64_t &total)
{
    const int lane = tid & 63, wave = tid >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t up = __shfl_up(v, o);
        if (lane >= o) v += up;
    }
    if (lane == 63) wave_sums[wave] = v;
    __syncthreads();
    int64_t before = 0;
    total = 0;
    for (int w = 0; w < FL_LANES / 64; w++) {
        const int64_t s = wave_sums[w];
        if (w < wave) before += s;
        total += s;
    }
    __syncthreads();                                              // wave_sums may be written again by the next call
    return v + before;
}

template <typename E>
__global__ void __launch_bounds__(FL_LANES)
k_flash_tile_sums(const E *__restrict__ grid, int64_t n, int64_t *__restrict__ head, int64_t *__restrict__ tile_sum)
{
    __shared__ int64_t wave_sums[FL_LANES / 64];
    const int tid = (int)threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * FL_TILE;
    int64_t sum = 0;
    int bad = 0;
#pragma unroll
    for (int k = 0; k < FL_PER_LANE; k++) {                       // striped: consecutive lanes read consecutive voxels
        const int64_t i = base + k * FL_LANES + tid;
        if (i < n) sum += fl_count<E>(grid[i], bad);
    }
    int64_t total;
    fl_block_scan(sum, tid, wave_sums, total);
    const int negative = __syncthreads_or(bad & FL_BAD_NEGATIVE), huge = __syncthreads_or(bad & FL_BAD_HUGE);
    if (tid == 0) {
        tile_sum[blockIdx.x] = total;
        if (negative || huge)
            atomicOr((unsigned long long *)(head + 1), (negative ? (unsigned long long)FL_BAD_NEGATIVE : 0ull) | (huge ? (unsigned long long)FL_BAD_HUGE : 0ull));
    }
}

// exclusive scan of the tile sums in place, by one workgroup; off[n_tiles] and head[0] get the total
__global__ void __launch_bounds__(FL_LANES)
k_flash_scan_tiles(int64_t n_tiles, int64_t *__restrict__ head, int64_t *__restrict__ off)
{
    __shared__ int64_t wave_sums[FL_LANES / 64];
    const int tid = (int)threadIdx.x;
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < n_tiles; b0 += FL_LANES) {
        const int64_t b = b0 + tid;
        const int64_t v = b < n_tiles ? off[b] : 0;
        int64_t total;
        const int64_t incl = fl_block_scan(v, tid, wave_sums, total);
        if (b < n_tiles) off[b] = carry + incl - v;
        carry += total;
    }
    if (tid == 0) { off[n_tiles] = carry; head[0] = carry; }
}

template <typename E>
__global__ void __launch_bounds__(FL_LANES)
k_flash_fill(const E *__restrict__ grid, int64_t n, const int64_t *__restrict__ off, int64_t n_flashes, int64_t *__restrict__ voxel)
{
    __shared__ int64_t wave_sums[FL_LANES / 64];
    __shared__ int64_t pre[FL_TILE + 1];                          // pre[v] = flashes of the tile in front of its voxel v
    const int64_t lo = off[blockIdx.x], hi = off[blockIdx.x + 1];
    if (lo == hi) return;                                         // the same for every lane: a tile without a flash is not read
    const int tid = (int)threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * FL_TILE + (int64_t)tid * FL_PER_LANE;
    int64_t c[FL_PER_LANE], sum = 0;
    int bad = 0;                                                  // judged in phase one; here the counts alone matter
#pragma unroll
    for (int k = 0; k < FL_PER_LANE; k++) {                       // blocked: a lane holds 8 consecutive voxels
        c[k] = base + k < n ? fl_count<E>(grid[base + k], bad) : 0;
        sum += c[k];
    }
    int64_t total;
    int64_t run = fl_block_scan(sum, tid, wave_sums, total) - sum;
    if (tid == 0) pre[0] = 0;
#pragma unroll
    for (int k = 0; k < FL_PER_LANE; k++) {
        run += c[k];
        pre[tid * FL_PER_LANE + k + 1] = run;
    }
    __syncthreads();
    const int64_t count = hi - lo < total ? hi - lo : total;     // equal unless the grid changed between the phases
    for (int64_t j = tid; j < count; j += FL_LANES) {
        int a = 0, b = FL_TILE;                                   // the voxel v with pre[v] <= j < pre[v + 1]
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (pre[mid] <= j) a = mid; else b = mid;
        }
        if (lo + j < n_flashes) voxel[lo + j] = (int64_t)blockIdx.x * FL_TILE + a;
    }
}

static int64_t fl_tiles(int64_t n) { return (n + FL_TILE - 1) / FL_TILE; }

extern "C" int tf_flash_tile(void) { return FL_TILE; }

extern "C" size_t tf_flash_workspace_bytes(int64_t n)
{
    if (n <= 0 || fl_tiles(n) > 0x7fffffffll) return 0;
    return tf_align_up((size_t)(FL_WS_HEAD + fl_tiles(n) + 1) * sizeof(int64_t), 256) + 256;
}

static int fl_args(const void *grid, int dtype, int64_t n, void *ws, size_t ws_bytes, int64_t **head, const char *who)
{
    if (!grid || !(dtype == TF_F32 || dtype == TF_F64 || dtype == TF_I32) || n <= 0 || fl_tiles(n) > 0x7fffffffll) {
        tf_set_error("%s: bad arguments (the grid is float32, float64 or int32, 0 < n, at most 2^31 - 1 tiles)", who);
        return TF_EINVAL;
    }
    TfArena ar(ws, ws_bytes);
    *head = ar.take<int64_t>((size_t)(FL_WS_HEAD + fl_tiles(n) + 1));
    if (!ar.ok()) { tf_set_error("%s: workspace too small", who); return TF_ENOMEM; }
    return TF_OK;
}

extern "C" int tf_flash_count(const void *grid, int dtype, int64_t n, void *ws, size_t ws_bytes, int64_t *total_host, int *bad_host,
                              void *stream)
{
    int64_t *head = nullptr;
    TF_REQUIRE(total_host && bad_host, "tf_flash_count: bad arguments");
    if (const int rc = fl_args(grid, dtype, n, ws, ws_bytes, &head, "tf_flash_count")) return rc;
    hipStream_t s = (hipStream_t)stream;
    const unsigned tiles = (unsigned)fl_tiles(n);
    int64_t *off = head + FL_WS_HEAD;
    TF_CHECK_HIP(hipMemsetAsync(head, 0, FL_WS_HEAD * sizeof(int64_t), s));
    if (dtype == TF_F32) hipLaunchKernelGGL(k_flash_tile_sums<float>, dim3(tiles), dim3(FL_LANES), 0, s, (const float *)grid, n, head, off);
    else if (dtype == TF_F64) hipLaunchKernelGGL(k_flash_tile_sums<double>, dim3(tiles), dim3(FL_LANES), 0, s, (const double *)grid, n, head, off);
    else hipLaunchKernelGGL(k_flash_tile_sums<int32_t>, dim3(tiles), dim3(FL_LANES), 0, s, (const int32_t *)grid, n, head, off);
    TF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_flash_scan_tiles, dim3(1), dim3(FL_LANES), 0, s, (int64_t)tiles, head, off);
    TF_CHECK_LAUNCH();
    int64_t words[FL_WS_HEAD];
    TF_CHECK_HIP(hipMemcpyAsync(words, head, sizeof(words), hipMemcpyDeviceToHost, s));
    TF_CHECK_HIP(hipStreamSynchronize(s));
    *total_host = words[0];
    *bad_host = (int)words[1];
    return TF_OK;
}

extern "C" int tf_flash_list(const void *grid, int dtype, int64_t n, void *ws, size_t ws_bytes, int64_t *voxel, int64_t n_flashes,
                             void *stream)
{
    int64_t *head = nullptr;
    TF_REQUIRE(n_flashes >= 0 && (voxel || n_flashes == 0), "tf_flash_list: bad arguments");
    if (const int rc = fl_args(grid, dtype, n, ws, ws_bytes, &head, "tf_flash_list")) return rc;
    if (n_flashes == 0) return TF_OK;
    hipStream_t s = (hipStream_t)stream;
    const unsigned tiles = (unsigned)fl_tiles(n);
    const int64_t *off = head + FL_WS_HEAD;
    if (dtype == TF_F32) hipLaunchKernelGGL(k_flash_fill<float>, dim3(tiles), dim3(FL_LANES), 0, s, (const float *)grid, n, off, n_flashes, voxel);
    else if (dtype == TF_F64) hipLaunchKernelGGL(k_flash_fill<double>, dim3(tiles), dim3(FL_LANES), 0, s, (const double *)grid, n, off, n_flashes, voxel);
    else hipLaunchKernelGGL(k_flash_fill<int32_t>, dim3(tiles), dim3(FL_LANES), 0, s, (const int32_t *)grid, n, off, n_flashes, voxel);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

// ---- tf_edt_cylinder_at ------------------------------------------------------------------------------------------------
#define CY_NONE 0x7fffffff                                        // tf_edt2d_frames' distance in a frame without a feature

__global__ void __launch_bounds__(256)
k_edt_cylinder_at(const int32_t *__restrict__ d2, const int32_t *__restrict__ nearest, const int32_t *__restrict__ markers, int64_t T,
                  int64_t hw, int64_t tm, const int64_t *__restrict__ voxel, int64_t n, double margin, double *__restrict__ dist,
                  int64_t *__restrict__ closest, unsigned long long *__restrict__ n_within)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool within = false;
    if (i < n) {
        const int64_t v = voxel[i];
        int32_t best = CY_NONE;
        int64_t bt = -1, p = 0;
        if (v >= 0 && v < T * hw) {                               // a voxel outside the volume has no marker near it
            const int64_t t = v / hw;
            p = v - t * hw;
            const int64_t lo = t - tm > 0 ? t - tm : 0, hi = t + tm < T - 1 ? t + tm : T - 1;
            for (int64_t k = lo; k <= hi; k++) {
                const int32_t d = d2[k * hw + p];
                if (d < best) { best = d; bt = k; }               // the earliest frame of the minimum, as np.nanargmin
            }
        }
        const double d = bt < 0 ? (double)__builtin_inf() : sqrt((double)best);
        dist[i] = d;
        within = d <= margin;
        if (closest) {
            int64_t label = 0;
            if (bt >= 0) {
                const int64_t q = (int64_t)nearest[bt * hw + p];
                if (q >= 0 && q < hw) label = (int64_t)markers[bt * hw + q];
            }
            closest[i] = label;
        }
    }
    const unsigned long long votes = __ballot(within);            // one integer atomic per wave: the sum has no order
    if ((threadIdx.x & 63) == 0 && votes) atomicAdd(n_within, (unsigned long long)__popcll(votes));
}

extern "C" int tf_edt_cylinder_at(const int32_t *d2, const int32_t *nearest, const int32_t *markers, int64_t T, int64_t hw,
                                  int64_t time_margin, const int64_t *voxel, int64_t n, double margin, double *dist,
                                  int64_t *closest, int64_t *n_within, void *stream)
{
    TF_REQUIRE(d2 && n_within && n >= 0 && (n == 0 || (voxel && dist)), "tf_edt_cylinder_at: bad arguments");
    TF_REQUIRE(!closest || (nearest && markers), "tf_edt_cylinder_at: closest needs nearest and markers");
    TF_REQUIRE(T > 0 && hw > 0 && T <= 0x7fffffffffffffffll / hw && time_margin >= 0, "tf_edt_cylinder_at: bad shape or time margin");
    const int64_t blocks = (n + 255) / 256;
    TF_REQUIRE(blocks <= 0x7fffffffll, "tf_edt_cylinder_at: list too long for one launch");
    hipStream_t s = (hipStream_t)stream;
    TF_CHECK_HIP(hipMemsetAsync(n_within, 0, sizeof(int64_t), s));
    if (n == 0) return TF_OK;
    hipLaunchKernelGGL(k_edt_cylinder_at, dim3((unsigned)blocks), dim3(256), 0, s, d2, nearest, markers, T, hw,
                       time_margin < T ? time_margin : T, voxel, n, margin, dist, closest, (unsigned long long *)n_within);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

// ---- tf_grid_has_missing / tf_edge_filter ------------------------------------------------------------------------------
#define EF_MAX_MARGIN 4000                                        // the span table of the footprint, 8 B per row, stays in LDS
#define EF_WS_TARGET ((size_t)1 << 30)                            // frames are dilated in chunks whose row counts fit 1 GiB
#define EF_SCAN_BLOCKS 4096

template <typename E>
__global__ void __launch_bounds__(256)
k_grid_has_missing(const E *__restrict__ grid, int64_t n, int32_t *__restrict__ flag)
{
    bool hit = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        hit |= grid[i] == (E)-1;                                  // NaN == -1 is false
    if (__syncthreads_or(hit) && threadIdx.x == 0) atomicOr(flag, 1);
}

extern "C" int tf_grid_has_missing(const void *grid, int dtype, int64_t n, int32_t *flag, void *stream)
{
    TF_REQUIRE(grid && flag && n > 0, "tf_grid_has_missing: bad arguments");
    TF_REQUIRE(dtype == TF_F32 || dtype == TF_F64 || dtype == TF_I32, "tf_grid_has_missing: the grid is float32, float64 or int32");
    hipStream_t s = (hipStream_t)stream;
    const int64_t want = (n + 255) / 256;
    const unsigned blocks = (unsigned)(want < EF_SCAN_BLOCKS ? want : EF_SCAN_BLOCKS);
    TF_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), s));
    if (dtype == TF_F32) hipLaunchKernelGGL(k_grid_has_missing<float>, dim3(blocks), dim3(256), 0, s, (const float *)grid, n, flag);
    else if (dtype == TF_F64) hipLaunchKernelGGL(k_grid_has_missing<double>, dim3(blocks), dim3(256), 0, s, (const double *)grid, n, flag);
    else hipLaunchKernelGGL(k_grid_has_missing<int32_t>, dim3(blocks), dim3(256), 0, s, (const int32_t *)grid, n, flag);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

// one workgroup per row (t0 + blockIdx / H, blockIdx % H): cnt[x + 1] = the number of columns <= x of the row where a frame
// of the time window t - tm .. t + tm holds -1; cnt[0] = 0.  cnt rows are W + 1 words long.
template <typename E>
__global__ void __launch_bounds__(256)
k_ef_row_counts(const E *__restrict__ grid, int64_t T, int64_t H, int64_t W, int64_t tm, int64_t t0, int32_t *__restrict__ cnt)
{
    __shared__ int32_t wave_sums[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = (int64_t)blockIdx.x, t = t0 + row / H, y = row % H;
    const int64_t lo = t - tm > 0 ? t - tm : 0, hi = t + tm < T - 1 ? t + tm : T - 1;
    int32_t *out = cnt + row * (W + 1);
    if (tid == 0) out[0] = 0;
    int32_t carry = 0;
    for (int64_t x0 = 0; x0 < W; x0 += 256) {
        const int64_t x = x0 + tid;
        bool hit = false;
        if (x < W)
            for (int64_t k = lo; k <= hi; k++) hit |= grid[(k * H + y) * W + x] == (E)-1;
        const unsigned long long votes = __ballot(hit);
        const int32_t in_wave = (int32_t)__popcll(votes & ((2ull << lane) - 1));      // lanes <= this one
        if (lane == 63) wave_sums[wave] = in_wave;
        __syncthreads();
        int32_t before = 0, total = 0;
        for (int w = 0; w < 4; w++) {
            const int32_t s = wave_sums[w];
            if (w < wave) before += s;
            total += s;
        }
        __syncthreads();
        if (x < W) out[x + 1] = carry + before + in_wave;
        carry += total;
    }
}

// the mask of the frames t0 .. t0 + nt - 1.  cnt == nullptr: no dilation.  span[] (dynamic LDS, 2 m + 1 entries): for the
// footprint row dy = j - m the columns dx = span[j].x .. span[j].y with (dx + m - 10)^2 + (dy + m - 10)^2 < m^2, |dx| <= m
// (x > y: none).  Output (t, y, x) is cleared where a row y - dy of the window-OR holds a -1 in x - dx over that span.
__global__ void __launch_bounds__(256)
k_ef_mask(int64_t T, int64_t H, int64_t W, int64_t m, int64_t tm, int64_t t0, int64_t nt, const uint8_t *__restrict__ frame_off,
          const int32_t *__restrict__ cnt, uint8_t *__restrict__ out)
{
    extern __shared__ int2 span[];
    if (cnt) {
        const int64_t c = 10 - m;                                 // the footprint's centre relative to the box's
        for (int64_t j = threadIdx.x; j <= 2 * m; j += blockDim.x) {
            const int64_t dy = j - m, r2 = m * m - (dy - c) * (dy - c);
            int2 sp = make_int2(1, 0);
            if (r2 > 0) {
                int64_t w = (int64_t)sqrt((double)(r2 - 1));      // the largest w with w^2 < r2
                while (w * w >= r2) w--;
                while ((w + 1) * (w + 1) < r2) w++;
                const int64_t a = c - w > -m ? c - w : -m, b = c + w < m ? c + w : m;
                sp = make_int2((int)a, (int)b);
            }
            span[j] = sp;
        }
        __syncthreads();
    }
    const int64_t hw = H * W, i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nt * hw) return;
    const int64_t tl = i / hw, t = t0 + tl, p = i - tl * hw, y = p / W, x = p - y * W;
    // NumPy's a[:k] = a[-k:] = False: nothing and everything for k == 0
    bool keep = tm > 0 && m > 0 && t >= tm && t < T - tm && y >= m && y < H - m && x >= m && x < W - m;
    if (keep && frame_off && frame_off[t]) keep = false;
    if (keep && cnt) {
        for (int64_t j = 0; j <= 2 * m && keep; j++) {
            const int2 sp = span[j];
            const int64_t ys = y - (j - m);
            if (sp.x > sp.y || ys < 0 || ys >= H) continue;
            const int32_t *row = cnt + (tl * H + ys) * (W + 1);
            if (row[W] == 0) continue;                            // a row without any -1 in the window
            const int64_t a = x - sp.y > 0 ? x - sp.y : 0, b = x - sp.x < W - 1 ? x - sp.x : W - 1;
            if (a <= b && row[b + 1] - row[a] > 0) keep = false;
        }
    }
    out[t * hw + p] = keep ? 1 : 0;
}

static int64_t ef_chunk_frames(int64_t T, int64_t H, int64_t W)
{
    const int64_t fit = (int64_t)(EF_WS_TARGET / ((size_t)(H * (W + 1)) * sizeof(int32_t)));
    return fit < 1 ? 1 : (fit < T ? fit : T);
}

static bool ef_shape_ok(int64_t T, int64_t H, int64_t W)
{
    return T > 0 && H > 0 && W > 0 && W < 0x7fffffffll && H < 0x7fffffffll && H <= 0x7fffffffffffffffll / (W + 1) / 8 &&
           T <= 0x7fffffffffffffffll / (H * (W + 1)) / 8;
}

extern "C" size_t tf_edge_filter_workspace_bytes(int64_t T, int64_t H, int64_t W, int has_missing)
{
    if (!has_missing || !ef_shape_ok(T, H, W)) return 0;
    return tf_align_up((size_t)(ef_chunk_frames(T, H, W) * H * (W + 1)) * sizeof(int32_t), 256) + 256;
}

template <typename E>
static int ef_dilated(const E *grid, int64_t T, int64_t H, int64_t W, int64_t m, int64_t tm, const uint8_t *frame_off, uint8_t *out,
                      int32_t *cnt, int64_t chunk, hipStream_t s)
{
    const size_t lds = (size_t)(2 * m + 1) * sizeof(int2);
    const int64_t tw = tm < T ? tm : T;
    for (int64_t t0 = 0; t0 < T; t0 += chunk) {
        const int64_t nt = T - t0 < chunk ? T - t0 : chunk, blocks = (nt * H * W + 255) / 256;
        TF_REQUIRE(nt * H <= 0x7fffffffll && blocks <= 0x7fffffffll, "tf_edge_filter: frame too large for one launch");
        hipLaunchKernelGGL(k_ef_row_counts<E>, dim3((unsigned)(nt * H)), dim3(256), 0, s, grid, T, H, W, tw, t0, cnt);
        TF_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_ef_mask, dim3((unsigned)blocks), dim3(256), lds, s, T, H, W, m, tm, t0, nt, frame_off, (const int32_t *)cnt, out);
        TF_CHECK_LAUNCH();
    }
    return TF_OK;
}

extern "C" int tf_edge_filter(const void *grid, int dtype, int64_t T, int64_t H, int64_t W, int64_t margin, int64_t time_margin,
                              const uint8_t *frame_off, int has_missing, uint8_t *out, void *ws, size_t ws_bytes, void *stream)
{
    TF_REQUIRE(out && (grid || !has_missing), "tf_edge_filter: bad arguments");
    TF_REQUIRE(dtype == TF_F32 || dtype == TF_F64 || dtype == TF_I32, "tf_edge_filter: the grid is float32, float64 or int32");
    TF_REQUIRE(ef_shape_ok(T, H, W), "tf_edge_filter: bad shape");
    TF_REQUIRE(margin >= 0 && margin <= EF_MAX_MARGIN && time_margin >= 0, "tf_edge_filter: 0 <= margin <= 4000 and 0 <= time_margin are required");
    hipStream_t s = (hipStream_t)stream;
    // with margin or time_margin 0 the reference's a[-0:] = False clears everything: there is nothing left to dilate
    if (!has_missing || margin == 0 || time_margin == 0) {
        const int64_t blocks = (T * H * W + 255) / 256;
        TF_REQUIRE(blocks <= 0x7fffffffll, "tf_edge_filter: volume too large for one launch");
        hipLaunchKernelGGL(k_ef_mask, dim3((unsigned)blocks), dim3(256), 0, s, T, H, W, margin, time_margin, (int64_t)0, T, frame_off,
                           (const int32_t *)nullptr, out);
        TF_CHECK_LAUNCH();
        return TF_OK;
    }
    const int64_t chunk = ef_chunk_frames(T, H, W);
    TfArena ar(ws, ws_bytes);
    int32_t *cnt = ar.take<int32_t>((size_t)(chunk * H * (W + 1)));
    if (!ar.ok()) { tf_set_error("tf_edge_filter: workspace too small"); return TF_ENOMEM; }
    if (dtype == TF_F32) return ef_dilated<float>((const float *)grid, T, H, W, margin, time_margin, frame_off, out, cnt, chunk, s);
    if (dtype == TF_F64) return ef_dilated<double>((const double *)grid, T, H, W, margin, time_margin, frame_off, out, cnt, chunk, s);
    return ef_dilated<int32_t>((const int32_t *)grid, T, H, W, margin, time_margin, frame_off, out, cnt, chunk, s);
}
