// tf_field_stats: count, mean, standard deviation, median, maximum and minimum of the non-NaN values of a float32 or
// float64 field, over everything, per frame, or per pixel along t -- get_bulk_stats / get_spatial_stats /
// get_temporal_stats of tobac_flow/dataset.py:19-148 (np.nanmean, np.nanstd, np.nanmedian, np.nanmax, np.nanmin).
//
// TF_FIELD_ALL (one slice of T H W values) and TF_FIELD_FRAME (T slices of H W values), all slices in the same launches
// (the slice is the grid's y index).  Reads of the volume: 2 for the moments, 3 (float32) or 6 (float64) for the median.
//   k_fs_moments, stage 0     lane partials of { count, float64 sum, max, min } over a fixed share of the slice, a tree
//                             over the 256 lanes, one partial per workgroup
//   k_fs_finish               the workgroups' partials of a slice: lane l takes partials l, l + 256, ... in that order,
//                             then the same tree; mean = sum / count
//   k_fs_moments, stage 1     the same with (x - mean)^2, the subtraction in float64; k_fs_finish: std = sqrt(m2 / count)
//   k_fs_select_begin         ranks (n - 1) / 2 and n / 2 of the slice's n non-NaN values
//   per digit of the key      k_fs_hist (radix_select.h: the digit's histogram under the one or two key prefixes the two
//                             ranks have so far; counted in LDS, added to the slice's 64-bit counters by integer atomics)
//                             k_fs_resolve (running sums, the two digits; after the last digit the keys are the values)
// Every share and every order of combination is a function of the shape alone and no float atomics are used, so two runs
// give the same bits.
//
// TF_FIELD_TIME: one lane per pixel, the lanes of a wave side by side in x, k_fs_time.  Up to TF_FIELD_STATS_LDS_FRAMES
// frames a workgroup of 256 pixels copies its T x 256 tile to LDS (at most 64 KB: two workgroups per CU) and all five
// statistics come from that one read; a lane only ever touches its own column (addresses of neighbouring lanes are
// consecutive: no bank conflicts, no barriers).  The two middle values of a column of up to FS_RANK_FRAMES values come from
// comparison counts (T^2 compares), of a longer one from a count-based selection over the key bits.  Beyond the LDS limit
// the same body walks the volume itself: 1 read for the moments, 1 for the deviations, one per 2-bit digit of the key
// (16 / 32) and 1 for the upper middle value: 19 reads (float32), 35 (float64).  The moments run in t order.
#include "tf_common.h"
#include "radix_select.h"

#define FS_LANES 256
#define FS_GRID_TARGET 16384           // workgroups of a sweep over all slices: 64 per CU, whether the field is 1 slice or 16
#define FS_MIN_GROUPS 256              // ... but a slice is never cut into fewer pieces than this allows
#define FS_RANK_FRAMES 32              // per-pixel columns up to this length are selected by comparison counts
#define FS_MAX_SLICES 65535            // the slice is the grid's y index

static_assert(FS_LANES == RS_LANES, "the shared histogram scan is written for this workgroup");
static_assert(TF_FIELD_STATS_LDS_FRAMES_F32 * FS_LANES * sizeof(float) <= 65536, "the float32 tile is at most 64 KB");
static_assert(TF_FIELD_STATS_LDS_FRAMES_F64 * FS_LANES * sizeof(double) <= 65536, "the float64 tile is at most 64 KB");

namespace {

typedef unsigned long long u64;

struct FsPartial { double sum, hi, lo; u64 n; };
// per slice: the finished moments, then the state of the select (the two ranks' residuals and key prefixes)
struct FsSlice { u64 n; double sum, mean; u64 resid[2], prefix[2]; int nactive; };

template <typename T> struct FsKey;
template <> struct FsKey<float> { typedef unsigned type; enum { bits = 32 }; };
template <> struct FsKey<double> { typedef u64 type; enum { bits = 64 }; };

__device__ __forceinline__ FsPartial fs_empty() { FsPartial p; p.sum = 0; p.hi = -INFINITY; p.lo = INFINITY; p.n = 0; return p; }
__device__ __forceinline__ FsPartial fs_combine(FsPartial a, const FsPartial &b)
{
    a.sum += b.sum; a.hi = fmax(a.hi, b.hi); a.lo = fmin(a.lo, b.lo); a.n += b.n;
    return a;
}
// s[t] += s[t + o] for o = 128 .. 1
__device__ __forceinline__ FsPartial fs_block_tree(FsPartial p, FsPartial *s)
{
    s[threadIdx.x] = p;
    __syncthreads();
    for (int o = FS_LANES / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] = fs_combine(s[threadIdx.x], s[threadIdx.x + o]);
        __syncthreads();
    }
    return s[0];
}

// numpy's mean of the two middle values: the sum rounded in the field's type, then halved; one value when n is odd
template <typename T> __device__ __forceinline__ double fs_median(T a, T b, u64 n)
{
    if (n == 0) return NAN;
    if (n & 1) return (double)a;
    const T s = a + b;
    return (double)(s / (T)2);
}

// ---- TF_FIELD_ALL, TF_FIELD_FRAME ------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(FS_LANES)
k_fs_moments(const T *__restrict__ x, int64_t N, int stage, const FsSlice *__restrict__ sl, FsPartial *__restrict__ part)
{
    __shared__ FsPartial s[FS_LANES];
    const T *v = x + (int64_t)blockIdx.y * N;
    const double mean = stage ? sl[blockIdx.y].mean : 0.0;
    const int64_t stride = (int64_t)gridDim.x * FS_LANES;
    FsPartial p = fs_empty();
    if (stage == 0) {
#pragma unroll 4
        for (int64_t i = (int64_t)blockIdx.x * FS_LANES + threadIdx.x; i < N; i += stride) {
            const double d = (double)v[i];
            if (d != d) continue;
            p.sum += d; p.hi = fmax(p.hi, d); p.lo = fmin(p.lo, d); p.n++;
        }
    } else {
#pragma unroll 4
        for (int64_t i = (int64_t)blockIdx.x * FS_LANES + threadIdx.x; i < N; i += stride) {
            const double d = (double)v[i];
            if (d != d) continue;
            const double e = d - mean;
            p.sum += e * e;
        }
    }
    const FsPartial total = fs_block_tree(p, s);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// one workgroup per slice.  stats: five planes of S doubles (mean, std, median, max, min)
__global__ void __launch_bounds__(FS_LANES)
k_fs_finish(const FsPartial *__restrict__ part, int parts, int stage, int64_t S, FsSlice *__restrict__ sl,
            int64_t *__restrict__ count, double *__restrict__ stats)
{
    __shared__ FsPartial s[FS_LANES];
    const int64_t k = blockIdx.x;
    FsPartial p = fs_empty();
    for (int i = threadIdx.x; i < parts; i += FS_LANES) p = fs_combine(p, part[(size_t)k * parts + i]);
    const FsPartial total = fs_block_tree(p, s);
    if (threadIdx.x != 0) return;
    if (stage == 0) {
        FsSlice r = {};
        r.n = total.n; r.sum = total.sum;
        r.mean = total.sum / (double)total.n;                       // 0 / 0 = NaN, as np.nanmean
        sl[k] = r;
        count[k] = (int64_t)total.n;
        stats[0 * S + k] = r.mean;
        stats[3 * S + k] = total.n ? total.hi : NAN;
        stats[4 * S + k] = total.n ? total.lo : NAN;
    } else
        stats[1 * S + k] = sqrt(total.sum / (double)sl[k].n);
}

__global__ void __launch_bounds__(FS_LANES)
k_fs_select_begin(int64_t S, FsSlice *__restrict__ sl)
{
    const int64_t k = (int64_t)blockIdx.x * FS_LANES + threadIdx.x;
    if (k >= S) return;
    const u64 n = sl[k].n;
    sl[k].resid[0] = n ? (n - 1) / 2 : 0; sl[k].resid[1] = n / 2;
    sl[k].prefix[0] = sl[k].prefix[1] = 0;
    sl[k].nactive = n ? 1 : 0;
}

// hist: per slice two histograms of RS_BINS 64-bit counters (slot 0: the prefix of the lower rank; slot 1: that of the
// upper rank once they differ).  A lane keeps the counter it hit last and its run length and touches LDS only when the
// counter changes: the values of a field share their leading bits, so the first pass is a few long runs.
template <typename T>
__global__ void __launch_bounds__(FS_LANES)
k_fs_hist(const T *__restrict__ x, int64_t N, int pass, const FsSlice *__restrict__ sl, u64 *__restrict__ hist)
{
    typedef typename FsKey<T>::type K;
    __shared__ unsigned lds_hist[2 * RS_BINS];
    const FsSlice me = sl[blockIdx.y];
    if (me.nactive == 0) return;
    for (int i = threadIdx.x; i < 2 * RS_BINS; i += FS_LANES) lds_hist[i] = 0u;
    __syncthreads();
    const T *v = x + (int64_t)blockIdx.y * N;
    const int bits = rs_digit_bits(FsKey<T>::bits, pass), pshift = rs_prefix_shift(FsKey<T>::bits, pass), dshift = pshift - bits;
    const K dmask = (K)((1u << bits) - 1u), p0 = (K)me.prefix[0], p1 = (K)me.prefix[1];
    const bool two = me.nactive == 2;
    const int64_t stride = (int64_t)gridDim.x * FS_LANES;
    int cur = -1; unsigned run = 0;
    for (int64_t i = (int64_t)blockIdx.x * FS_LANES + threadIdx.x; i < N; i += stride) {
        const T f = v[i];
        if (f != f) continue;
        const K key = rs_key(f);
        const K prefix = pass == 0 ? (K)0 : (K)(key >> pshift);
        const int slot = prefix == p0 ? 0 : (two && prefix == p1) ? 1 : -1;
        if (slot < 0) continue;
        const int at = slot * RS_BINS + (int)((key >> dshift) & dmask);
        if (at != cur) {
            if (run) atomicAdd(&lds_hist[cur], run);
            cur = at; run = 0;
        }
        run++;
    }
    if (run) atomicAdd(&lds_hist[cur], run);
    __syncthreads();
    u64 *h = hist + (size_t)blockIdx.y * 2 * RS_BINS;
    for (int i = threadIdx.x; i < (two ? 2 : 1) * RS_BINS; i += FS_LANES)
        if (lds_hist[i]) atomicAdd(&h[i], (u64)lds_hist[i]);
}

// one workgroup per slice: running sums of the active histograms, the two ranks' digits, the histograms zeroed for the
// next pass; after the last pass the prefixes are the keys of the two middle values
template <typename T>
__global__ void __launch_bounds__(FS_LANES)
k_fs_resolve(int pass, int64_t S, u64 total, FsSlice *__restrict__ sl, u64 *__restrict__ hist, double *__restrict__ stats)
{
    typedef typename FsKey<T>::type K;
    __shared__ u64 part[RS_LANES];
    const int64_t k = blockIdx.x;
    const int tid = threadIdx.x, nactive = sl[k].nactive;
    u64 *h = hist + (size_t)k * 2 * RS_BINS;
    const bool last = pass == rs_passes(FsKey<T>::bits) - 1;
    for (int slot = 0; slot < nactive; slot++) {
        rs_scan_sum(tid, h + slot * RS_BINS, part);
        __syncthreads();
        rs_scan_write(tid, h + slot * RS_BINS, part);
        __syncthreads();
    }
    if (tid == 0) {
        FsSlice r = sl[k];
        if (nactive) {
            const int bits = rs_digit_bits(FsKey<T>::bits, pass);
            const u64 slot0 = r.prefix[0];
            for (int j = 0; j < 2; j++) {
                const u64 *cum = h + (r.prefix[j] == slot0 ? 0 : 1) * RS_BINS;
                const int b = rs_rank_bin(cum, 1 << bits, r.resid[j]);
                r.resid[j] -= cum[b];
                r.prefix[j] = (r.prefix[j] << bits) | (u64)b;
            }
            r.nactive = r.prefix[0] != r.prefix[1] ? 2 : 1;
            sl[k] = r;
        }
        if (last) {
            double m = fs_median<T>(rs_unkey((K)r.prefix[0]), rs_unkey((K)r.prefix[1]), r.n);
            if (total && r.n != total) m = NAN;                      // np.median: any NaN makes the result NaN
            stats[2 * S + k] = m;
        }
    }
    __syncthreads();
    for (int i = tid; i < nactive * RS_BINS; i += FS_LANES) h[i] = 0;
}

// ---- TF_FIELD_TIME -------------------------------------------------------------------------------------------------------
// The two middle values of the n >= 1 non-NaN values of a column, by comparison counts: x is the value of rank r exactly
// when  #(values < x) <= r < #(values <= x).  T^2 comparisons: taken for short columns (FS_RANK_FRAMES), where it is a
// third of the digit sweeps' work.  A NaN compares false both ways and is no candidate.
template <typename T, typename P>
__device__ __forceinline__ void fs_column_by_ranks(P col, int64_t step, int64_t Tn, u64 n, T *mid)
{
    const unsigned r0 = (unsigned)((n - 1) / 2), r1 = (unsigned)(n / 2);
    for (int64_t i = 0; i < Tn; i++) {
        const T v = col[i * step];
        if (v != v) continue;
        unsigned lt = 0, le = 0;
        for (int64_t j = 0; j < Tn; j++) {
            const T w = col[j * step];
            lt += w < v; le += w <= v;
        }
        if (lt <= r0 && r0 < le) mid[0] = v;
        if (lt <= r1 && r1 < le) mid[1] = v;
    }
}

// The same by a count-based selection over the key bits, for columns of any length
template <typename T, typename P>
__device__ __forceinline__ void fs_column_by_digits(P col, int64_t step, int64_t Tn, u64 n, T *mid)
{
    typedef typename FsKey<T>::type K;
    // the key of rank (n - 1) / 2, two bits at a time: how many keys under the prefix continue with 0, 1, 2
    K prefix = 0; u64 r = (n - 1) / 2;
    for (int shift = FsKey<T>::bits - 2; shift >= 0; shift -= 2) {
        u64 c0 = 0, c1 = 0, c2 = 0;
        for (int64_t t = 0; t < Tn; t++) {
            const T f = col[t * step];
            if (f != f) continue;
            const K key = rs_key(f);
            if (shift + 2 < FsKey<T>::bits && (key >> (shift + 2)) != prefix) continue;
            const unsigned d = (unsigned)(key >> shift) & 3u;
            c0 += d == 0; c1 += d == 1; c2 += d == 2;
        }
        unsigned d = 3;
        if (r < c0) d = 0; else if (r < c0 + c1) { d = 1; r -= c0; } else if (r < c0 + c1 + c2) { d = 2; r -= c0 + c1; } else r -= c0 + c1 + c2;
        prefix = (K)(prefix << 2) | (K)d;
    }
    // rank n / 2 is the same value when n is odd or more keys equal it, else the smallest key above
    K upper = prefix;
    if (!(n & 1)) {
        u64 le = 0; K next = ~(K)0;
        for (int64_t t = 0; t < Tn; t++) {
            const T f = col[t * step];
            if (f != f) continue;
            const K key = rs_key(f);
            le += key <= prefix;
            if (key > prefix && key < next) next = key;
        }
        if (le <= n / 2) upper = next;
    }
    mid[0] = rs_unkey(prefix); mid[1] = rs_unkey(upper);
}

// the lane's column: element t at col[t * step]
template <typename T, typename P>
__device__ __forceinline__ void fs_column(P col, int64_t step, int64_t Tn, int64_t S, int64_t k,
                                          int64_t *__restrict__ count, double *__restrict__ stats)
{
    u64 n = 0; double sum = 0, hi = -INFINITY, lo = INFINITY;
    for (int64_t t = 0; t < Tn; t++) {
        const double d = (double)col[t * step];
        if (d != d) continue;
        sum += d; hi = fmax(hi, d); lo = fmin(lo, d); n++;
    }
    const double mean = sum / (double)n;
    double m2 = 0;
    for (int64_t t = 0; t < Tn; t++) {
        const double d = (double)col[t * step];
        if (d != d) continue;
        const double e = d - mean;
        m2 += e * e;
    }
    T mid[2] = {(T)0, (T)0};
    if (n && Tn <= FS_RANK_FRAMES) fs_column_by_ranks<T>(col, step, Tn, n, mid);
    else if (n) fs_column_by_digits<T>(col, step, Tn, n, mid);
    count[k] = (int64_t)n;
    stats[0 * S + k] = mean;
    stats[1 * S + k] = sqrt(m2 / (double)n);
    stats[2 * S + k] = fs_median<T>(mid[0], mid[1], n);
    stats[3 * S + k] = n ? hi : NAN;
    stats[4 * S + k] = n ? lo : NAN;
}

template <typename T, bool LDS>
__global__ void __launch_bounds__(FS_LANES)
k_fs_time(const T *__restrict__ x, int64_t Tn, int64_t HW, int64_t *__restrict__ count, double *__restrict__ stats)
{
    const int64_t k = (int64_t)blockIdx.x * FS_LANES + threadIdx.x;
    if (k >= HW) return;
    if (LDS) {
        extern __shared__ double fs_tile_raw[];
        T *tile = (T *)fs_tile_raw + threadIdx.x;
        for (int64_t t = 0; t < Tn; t++) tile[t * FS_LANES] = x[t * HW + k];
        fs_column<T, const T *>(tile, FS_LANES, Tn, HW, k, count, stats);
    } else
        fs_column<T, const T *>(x + k, HW, Tn, HW, k, count, stats);
}

struct Shape { int64_t S, N; };                                     // slices, values per slice

// workgroups per slice of a sweep whose lanes take `per_lane` elements each where the slice is long enough: a function of
// the shape alone (the partials' order of combination follows from it)
int slice_workgroups(Shape sh, int per_lane)
{
    const int64_t g = (sh.N + FS_LANES * per_lane - 1) / (FS_LANES * per_lane);
    int64_t cap = FS_GRID_TARGET / sh.S; if (cap < FS_MIN_GROUPS) cap = FS_MIN_GROUPS;
    return (int)(g > cap ? cap : g);
}
int moment_workgroups(Shape sh) { return slice_workgroups(sh, 16); }

const char *check_args(int dtype, int64_t T, int64_t H, int64_t W, int over, Shape *shape)
{
    if (dtype != TF_F32 && dtype != TF_F64) return "tf_field_stats: dtype must be TF_F32 or TF_F64";
    if (over != TF_FIELD_ALL && over != TF_FIELD_FRAME && over != TF_FIELD_TIME) return "tf_field_stats: unknown geometry";
    const int64_t lim = (int64_t)1 << 40;
    if (T <= 0 || H <= 0 || W <= 0 || T > lim || H > lim || W > lim || H * W > lim || T > lim / (H * W))
        return "tf_field_stats: bad shape (1 <= T H W <= 2^40)";
    if (over == TF_FIELD_FRAME && T > FS_MAX_SLICES) return "tf_field_stats: at most 65535 frames";
    if (over == TF_FIELD_TIME && (H * W + FS_LANES - 1) / FS_LANES > INT32_MAX) return "tf_field_stats: too many pixels";
    shape->S = over == TF_FIELD_ALL ? 1 : over == TF_FIELD_FRAME ? T : H * W;
    shape->N = over == TF_FIELD_ALL ? T * H * W : over == TF_FIELD_FRAME ? H * W : T;
    return nullptr;
}

struct Layout { FsSlice *sl; FsPartial *part; u64 *hist; bool ok; };

Layout layout(void *ws, size_t ws_bytes, Shape sh)
{
    TfArena a(ws, ws_bytes);
    Layout l = {};
    l.sl = a.take<FsSlice>((size_t)sh.S);
    l.part = a.take<FsPartial>((size_t)sh.S * moment_workgroups(sh));
    l.hist = a.take<u64>((size_t)sh.S * 2 * RS_BINS);
    l.ok = a.ok();
    return l;
}

template <typename T>
int run_slices(const T *x, Shape sh, bool bulk, int64_t *count, double *stats, const Layout &l, hipStream_t s)
{
    const int parts = moment_workgroups(sh);
    const dim3 grid((unsigned)parts, (unsigned)sh.S);
    for (int stage = 0; stage < 2; stage++) {
        hipLaunchKernelGGL(k_fs_moments<T>, grid, dim3(FS_LANES), 0, s, x, sh.N, stage, l.sl, l.part);
        hipLaunchKernelGGL(k_fs_finish, dim3((unsigned)sh.S), dim3(FS_LANES), 0, s, l.part, parts, stage, sh.S, l.sl, count, stats);
    }
    hipLaunchKernelGGL(k_fs_select_begin, dim3((unsigned)((sh.S + FS_LANES - 1) / FS_LANES)), dim3(FS_LANES), 0, s, sh.S, l.sl);
    TF_CHECK_HIP(hipMemsetAsync(l.hist, 0, (size_t)sh.S * 2 * RS_BINS * sizeof(u64), s));
    const int groups = slice_workgroups(sh, 32);
    for (int pass = 0; pass < rs_passes(FsKey<T>::bits); pass++) {
        hipLaunchKernelGGL(k_fs_hist<T>, dim3((unsigned)groups, (unsigned)sh.S), dim3(FS_LANES), 0, s, x, sh.N, pass, l.sl, l.hist);
        hipLaunchKernelGGL(k_fs_resolve<T>, dim3((unsigned)sh.S), dim3(FS_LANES), 0, s, pass, sh.S, bulk ? (u64)sh.N : (u64)0, l.sl,
                           l.hist, stats);
    }
    TF_CHECK_LAUNCH();
    return TF_OK;
}

template <typename T>
int run_time(const T *x, int64_t Tn, int64_t HW, int64_t *count, double *stats, hipStream_t s)
{
    const int lds_frames = sizeof(T) == 4 ? TF_FIELD_STATS_LDS_FRAMES_F32 : TF_FIELD_STATS_LDS_FRAMES_F64;
    const dim3 grid((unsigned)((HW + FS_LANES - 1) / FS_LANES));
    if (Tn <= lds_frames)
        hipLaunchKernelGGL((k_fs_time<T, true>), grid, dim3(FS_LANES), (size_t)Tn * FS_LANES * sizeof(T), s, x, Tn, HW, count, stats);
    else
        hipLaunchKernelGGL((k_fs_time<T, false>), grid, dim3(FS_LANES), 0, s, x, Tn, HW, count, stats);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

}  // namespace

extern "C" size_t tf_field_stats_workspace_bytes(int dtype, int64_t T, int64_t H, int64_t W, int over)
{
    Shape sh;
    if (check_args(dtype, T, H, W, over, &sh)) return 0;
    if (over == TF_FIELD_TIME) return 256;                           // nothing is kept between the sweeps of a column
    return tf_align_up((size_t)sh.S * sizeof(FsSlice), 256) + tf_align_up((size_t)sh.S * moment_workgroups(sh) * sizeof(FsPartial), 256)
           + tf_align_up((size_t)sh.S * 2 * RS_BINS * sizeof(u64), 256);
}

extern "C" int tf_field_stats(const void *field, int dtype, int64_t T, int64_t H, int64_t W, int over, int64_t *count,
                              double *stats, void *ws, size_t ws_bytes, void *stream)
{
    Shape sh;
    if (const char *msg = check_args(dtype, T, H, W, over, &sh)) { tf_set_error("%s", msg); return TF_EINVAL; }
    TF_REQUIRE(field && count && stats, "tf_field_stats: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (over == TF_FIELD_TIME)
        return dtype == TF_F32 ? run_time((const float *)field, T, H * W, count, stats, s)
                               : run_time((const double *)field, T, H * W, count, stats, s);
    TF_REQUIRE(ws, "tf_field_stats: null pointer");
    const Layout l = layout(ws, ws_bytes, sh);
    if (!l.ok || ws_bytes < tf_field_stats_workspace_bytes(dtype, T, H, W, over)) { tf_set_error("tf_field_stats: workspace too small"); return TF_ENOMEM; }
    const bool bulk = over == TF_FIELD_ALL;
    return dtype == TF_F32 ? run_slices((const float *)field, sh, bulk, count, stats, l, s)
                           : run_slices((const double *)field, sh, bulk, count, stats, l, s);
}
