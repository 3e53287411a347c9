// Geodesy on gfx950: what the reference does with pyproj on the host.
//
//   tf_geos_inverse, tf_geos_inverse_points   Proj("geos")(x, y, inverse=True) of abi.get_abi_lat_lon (abi.py:21-39)
//   tf_geos_forward                           Proj("geos")(lon, lat) of abi.get_abi_x_y (abi.py:92-104), with `alt` the
//                                             parallax step of nexrad.map_nexrad_to_goes (nexrad.py:60-77) in the same launch
//   tf_geod_inverse                           Geod.inv
//   tf_grid_spacing                           geo.get_pixel_lengths / get_pixel_area (geo.py:224-246) and their two copies
//   tf_view_angles                            geo.get_sza, get_sza_and_azi, get_satellite_viewing_angles (geo.py:14-221),
//                                             abi.get_abi_zenith_angle (abi.py:68-89)
//   tf_ecef, tf_geos_to_ecef                  the toECEF / fromECEF of the lmatools coordinate systems (_lmatools.py)
//   tf_glm_parallax                           glm.get_glm_parallax_offsets and get_corrected_glm_x_y (glm.py:25-57), fused
//
// The arithmetic of one element is in geodesy_kernels.h (it compiles for the host as well); here are the work layouts.
// No atomics: every output is the same in every run.
#include "tf_common.h"
#include "geodesy_kernels.h"

#define GD_BLOCK 256
#define GD_VEC 4                                                  // consecutive pixels of the raveled grid per lane

static __device__ __forceinline__ void gd_store(double *p, double v) { *p = v; }
static __device__ __forceinline__ void gd_store(float *p, double v) { *p = (float)v; }      // the float64 result rounded once
static __device__ __forceinline__ void gd_store4(double *p, const double v[GD_VEC])
{
    ((double2 *)p)[0] = make_double2(v[0], v[1]);
    ((double2 *)p)[1] = make_double2(v[2], v[3]);
}
static __device__ __forceinline__ void gd_store4(float *p, const double v[GD_VEC])
{
    *(float4 *)p = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}

// The grid is raveled: lane l takes the pixels 4 l .. 4 l + 3, which lie in one row unless the row ends among them, so
// the row's terms are computed once per lane and again only where the row changes; with 16-byte aligned outputs every
// group of four starts on a 16-byte boundary whatever the width, and the ragged tail takes the scalar stores.
template <typename T>
__global__ void __launch_bounds__(GD_BLOCK)
k_geos_inverse_grid(const GdGeos s, const double *__restrict__ x, int64_t W, const double *__restrict__ y, int64_t H,
                    T *__restrict__ lat, T *__restrict__ lon, int vec)
{
    const int64_t n = H * W, k0 = ((int64_t)blockIdx.x * GD_BLOCK + threadIdx.x) * GD_VEC;
    if (k0 >= n) return;
    const int m = n - k0 < GD_VEC ? (int)(n - k0) : GD_VEC;
    int64_t i = k0 / W, j = k0 - i * W;
    double ty, hy, la[GD_VEC], lo[GD_VEC];
    gd_geos_row_terms(s, y[i], ty, hy);
#pragma unroll
    for (int e = 0; e < GD_VEC; e++) {
        if (e >= m) break;
        gd_geos_inverse_one(s, x[j], ty, hy, la[e], lo[e]);
        if (++j == W && e + 1 < m) {
            j = 0;
            i++;
            gd_geos_row_terms(s, y[i], ty, hy);
        }
    }
    if (vec && m == GD_VEC) {
        gd_store4(lat + k0, la);
        gd_store4(lon + k0, lo);
        return;
    }
    for (int e = 0; e < m; e++) { gd_store(lat + k0 + e, la[e]); gd_store(lon + k0 + e, lo[e]); }
}

__global__ void __launch_bounds__(GD_BLOCK)
k_geos_inverse_points(const GdGeos s, const double *__restrict__ x, const double *__restrict__ y, int64_t n,
                      double *__restrict__ lat, double *__restrict__ lon)
{
    const int64_t k = (int64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    if (k >= n) return;
    double ty, hy, la, lo;
    gd_geos_row_terms(s, y[k], ty, hy);
    gd_geos_inverse_one(s, x[k], ty, hy, la, lo);
    lat[k] = la;
    lon[k] = lo;
}

__global__ void __launch_bounds__(GD_BLOCK)
k_geos_forward(const GdGeos s, const double *__restrict__ lat, const double *__restrict__ lon, const double *__restrict__ alt,
               int64_t n, double *__restrict__ x, double *__restrict__ y)
{
    const int64_t k = (int64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    if (k >= n) return;
    double px, py;
    if (alt) gd_geos_forward_alt_one(s, lat[k], lon[k], alt[k], px, py);
    else gd_geos_forward_one(s, lat[k], lon[k], px, py);
    x[k] = px;
    y[k] = py;
}

// the number of lanes of the workgroup with `flag` set, to counts[block] (a tree in LDS; every lane of the block calls)
static __device__ __forceinline__ void gd_block_count(int flag, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t part[GD_BLOCK];
    part[threadIdx.x] = (uint32_t)flag;
    __syncthreads();
    for (int step = GD_BLOCK / 2; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) part[threadIdx.x] += part[threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = part[0];
}

// status[0] = sum of counts[0 .. n): one workgroup
__global__ void __launch_bounds__(GD_BLOCK)
k_sum_counts(const uint32_t *__restrict__ counts, int64_t n, uint32_t *__restrict__ status)
{
    __shared__ uint32_t part[GD_BLOCK];
    uint32_t acc = 0;
    for (int64_t k = threadIdx.x; k < n; k += GD_BLOCK) acc += counts[k];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int step = GD_BLOCK / 2; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) part[threadIdx.x] += part[threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x == 0) status[0] = part[0];
}

// One pair per lane.  The iteration is a plain loop with a break: a lane that has converged waits masked for the slowest
// lane of its wave and does not run again.
__global__ void __launch_bounds__(GD_BLOCK)
k_geod_inverse(double a, double f, const double *__restrict__ lon1, const double *__restrict__ lat1,
               const double *__restrict__ lon2, const double *__restrict__ lat2, int64_t n, double *__restrict__ az12,
               double *__restrict__ az21, double *__restrict__ dist, uint32_t *__restrict__ counts)
{
    const int64_t k = (int64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    int failed = 0;
    if (k < n) {
        const GdInverse r = gd_geod_inverse_one(a, f, lon1[k], lat1[k], lon2[k], lat2[k]);
        if (az12) az12[k] = r.az12;
        if (az21) az21[k] = r.az21;
        if (dist) dist[k] = r.s;
        failed = r.failed;
    }
    gd_block_count(failed, counts);
}

// raw spacings in km of every pixel towards the next row (raw_y) and the next column (raw_x): each computed once
__global__ void __launch_bounds__(GD_BLOCK)
k_spacing_raw(double a, double f, const double *__restrict__ lat, const double *__restrict__ lon, int64_t H, int64_t W,
              double *__restrict__ raw_y, double *__restrict__ raw_x, uint32_t *__restrict__ counts)
{
    const int64_t k = (int64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    int failed = 0;
    if (k < H * W) {
        const int64_t i = k / W, j = k - i * W;
        const double la = lat[k], lo = lon[k];
        if (raw_y) {
            double v = 0.0;
            if (i < H - 1) {
                const GdInverse r = gd_geod_inverse_one(a, f, lo, la, lon[k + W], lat[k + W]);
                v = r.s / 1e3;
                failed += r.failed;
            }
            raw_y[k] = v;
        }
        if (raw_x) {
            double v = 0.0;
            if (j < W - 1) {
                const GdInverse r = gd_geod_inverse_one(a, f, lo, la, lon[k + 1], lat[k + 1]);
                v = r.s / 1e3;
                failed += r.failed;
            }
            raw_x[k] = v;
        }
    }
    gd_block_count(failed, counts);
}

__global__ void __launch_bounds__(GD_BLOCK)
k_spacing_combine(const double *__restrict__ raw_y, const double *__restrict__ raw_x, int64_t H, int64_t W,
                  double *__restrict__ dx, double *__restrict__ dy, double *__restrict__ area)
{
    const int64_t k = (int64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    if (k >= H * W) return;
    const int64_t i = k / W, j = k - i * W;
    double vx = 0.0, vy = 0.0;
    if (raw_y) vy = gd_spacing_rule(i, H, i > 0 ? raw_y[k - W] : 0.0, raw_y[k]);
    if (raw_x) vx = gd_spacing_rule(j, W, j > 0 ? raw_x[k - 1] : 0.0, raw_x[k]);
    if (dx) dx[k] = vx;
    if (dy) dy[k] = vy;
    if (area) area[k] = vx * vy;
}

struct GdScalars { double v[4]; };

__global__ void __launch_bounds__(GD_BLOCK)
k_view_angles(int mode, const GdScalars sc, const double *__restrict__ lat, const double *__restrict__ lon, int64_t n,
              const double *__restrict__ x, const double *__restrict__ y, int64_t W, double *__restrict__ out0,
              double *__restrict__ out1)
{
    const int64_t k = (int64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    if (k >= n) return;
    double sx = 0.0, sy = 0.0, a0, a1;
    if (mode == TF_VIEW_ABI_ZENITH) {
        const int64_t i = k / W;
        sx = x[k - i * W];
        sy = y[i];
    }
    gd_view_angles_one(mode, sc.v, lat[k], lon[k], sx, sy, a0, a1);
    out0[k] = a0;
    if (out1) out1[k] = a1;
}

__global__ void __launch_bounds__(GD_BLOCK)
k_ecef(int mode, double a, double f, const double *__restrict__ in0, const double *__restrict__ in1, const double *__restrict__ in2,
       int64_t n, double *__restrict__ out0, double *__restrict__ out1, double *__restrict__ out2)
{
    const int64_t k = (int64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    if (k >= n) return;
    double o0, o1, o2;
    if (mode == TF_ECEF_FROM_GEODETIC) gd_geodetic_to_ecef_one(a, f, in0[k], in1[k], in2[k], o0, o1, o2);
    else gd_ecef_to_geodetic_one(a, f, in0[k], in1[k], in2[k], o0, o1, o2);
    out0[k] = o0;
    out1[k] = o1;
    out2[k] = o2;
}

__global__ void __launch_bounds__(GD_BLOCK)
k_geos_to_ecef(const GdGeos s, const double *__restrict__ x, const double *__restrict__ y, int64_t n, double *__restrict__ X,
               double *__restrict__ Y, double *__restrict__ Z)
{
    const int64_t k = (int64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    if (k >= n) return;
    double px, py, pz;
    gd_geos_to_ecef_one(s, x[k], y[k], px, py, pz);
    X[k] = px;
    Y[k] = py;
    Z[k] = pz;
}

// One flash per lane: 8 or 16 bytes in and 16 or 32 out against some 400 float64 operations, so the lanes' plain
// consecutive loads and stores are all the memory system is asked for.
template <typename T>
__global__ void __launch_bounds__(GD_BLOCK)
k_glm_parallax(const GdParallax c, const T *__restrict__ lat, const T *__restrict__ lon, int64_t n, double *__restrict__ dlon,
               double *__restrict__ dlat, double *__restrict__ x, double *__restrict__ y)
{
    const int64_t k = (int64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    if (k >= n) return;
    double dlo, dla, px, py, alt;
    gd_glm_parallax_one(c, (double)lat[k], (double)lon[k], dlo, dla, px, py, alt);
    if (dlon) { dlon[k] = dlo; dlat[k] = dla; }
    if (x) { x[k] = px; y[k] = py; }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------
#define GD_MAX_N ((((int64_t)1 << 31) - 1) * GD_BLOCK)

static int gd_check_geos(const TfGeos *g, const char *what)
{
    if (!g) { tf_set_error("%s: bad arguments", what); return TF_EINVAL; }
    if (!(g->lat_0 == 0.0)) { tf_set_error("%s: the geos projection takes lat_0 = 0 only", what); return TF_EINVAL; }
    if (!(g->h > 0.0) || !(g->a > 0.0) || !(g->rf == 0.0 || g->rf > 1.0) || !(g->lon_0 - g->lon_0 == 0.0)) {
        tf_set_error("%s: h and a are positive, rf is 0 (a sphere) or above 1, lon_0 is finite", what);
        return TF_EINVAL;
    }
    if (g->sweep_y != 0 && g->sweep_y != 1) { tf_set_error("%s: sweep_y is 0 (sweep x) or 1", what); return TF_EINVAL; }
    if (g->flags & ~TF_GEOS_INF) { tf_set_error("%s: unknown flag", what); return TF_EINVAL; }
    return TF_OK;
}

static unsigned gd_blocks(int64_t n, int per_block = GD_BLOCK) { return (unsigned)((n + per_block - 1) / per_block); }

extern "C" int tf_geos_inverse(const TfGeos *geos, const double *x, int64_t W, const double *y, int64_t H, void *lat, void *lon,
                               int out_dtype, void *stream)
{
    const int rc = gd_check_geos(geos, "tf_geos_inverse");
    if (rc != TF_OK) return rc;
    TF_REQUIRE(H >= 0 && W >= 0 && (H == 0 || W <= GD_MAX_N / H), "tf_geos_inverse: bad grid size");
    TF_REQUIRE(out_dtype == TF_F32 || out_dtype == TF_F64, "tf_geos_inverse: lat and lon are float32 or float64");
    if (H == 0 || W == 0) return TF_OK;
    TF_REQUIRE(x && y && lat && lon, "tf_geos_inverse: null pointer");
    const GdGeos s = gd_geos_setup(*geos);
    const int vec = (uintptr_t)lat % 16 == 0 && (uintptr_t)lon % 16 == 0;
    const unsigned blocks = gd_blocks(H * W, GD_BLOCK * GD_VEC);
    hipStream_t st = (hipStream_t)stream;
    if (out_dtype == TF_F64)
        hipLaunchKernelGGL(k_geos_inverse_grid<double>, dim3(blocks), dim3(GD_BLOCK), 0, st, s, x, W, y, H, (double *)lat, (double *)lon, vec);
    else
        hipLaunchKernelGGL(k_geos_inverse_grid<float>, dim3(blocks), dim3(GD_BLOCK), 0, st, s, x, W, y, H, (float *)lat, (float *)lon, vec);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

extern "C" int tf_geos_inverse_points(const TfGeos *geos, const double *x, const double *y, int64_t n, double *lat, double *lon,
                                      void *stream)
{
    const int rc = gd_check_geos(geos, "tf_geos_inverse_points");
    if (rc != TF_OK) return rc;
    TF_REQUIRE(n >= 0 && n <= GD_MAX_N, "tf_geos_inverse_points: bad number of points");
    if (n == 0) return TF_OK;
    TF_REQUIRE(x && y && lat && lon, "tf_geos_inverse_points: null pointer");
    hipLaunchKernelGGL(k_geos_inverse_points, dim3(gd_blocks(n)), dim3(GD_BLOCK), 0, (hipStream_t)stream, gd_geos_setup(*geos), x, y, n, lat, lon);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

extern "C" int tf_geos_forward(const TfGeos *geos, const double *lat, const double *lon, const double *alt, int64_t n, double *x,
                               double *y, void *stream)
{
    const int rc = gd_check_geos(geos, "tf_geos_forward");
    if (rc != TF_OK) return rc;
    TF_REQUIRE(n >= 0 && n <= GD_MAX_N, "tf_geos_forward: bad number of points");
    if (n == 0) return TF_OK;
    TF_REQUIRE(lat && lon && x && y, "tf_geos_forward: null pointer");
    hipLaunchKernelGGL(k_geos_forward, dim3(gd_blocks(n)), dim3(GD_BLOCK), 0, (hipStream_t)stream, gd_geos_setup(*geos), lat, lon, alt, n, x, y);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

static bool gd_ellipsoid_ok(double a, double rf) { return a > 0.0 && a - a == 0.0 && (rf == 0.0 || (rf > 1.0 && rf - rf == 0.0)); }

extern "C" size_t tf_geod_inverse_workspace_bytes(int64_t n)
{
    return n > 0 ? tf_align_up((size_t)gd_blocks(n) * sizeof(uint32_t), 256) : 0;
}

extern "C" int tf_geod_inverse(double a, double rf, const double *lon1, const double *lat1, const double *lon2, const double *lat2,
                               int64_t n, double *az12, double *az21, double *dist, uint32_t *status, void *ws, size_t ws_bytes,
                               void *stream)
{
    TF_REQUIRE(gd_ellipsoid_ok(a, rf), "tf_geod_inverse: a is positive and finite, rf is 0 (a sphere) or above 1");
    TF_REQUIRE(n >= 0 && n <= GD_MAX_N, "tf_geod_inverse: bad number of pairs");
    TF_REQUIRE(status, "tf_geod_inverse: null status");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        TF_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(uint32_t), st));
        return TF_OK;
    }
    TF_REQUIRE(lon1 && lat1 && lon2 && lat2, "tf_geod_inverse: null pointer");
    TF_REQUIRE(az12 || az21 || dist, "tf_geod_inverse: no output");
    if (!ws || ws_bytes < tf_geod_inverse_workspace_bytes(n)) { tf_set_error("tf_geod_inverse: workspace too small"); return TF_ENOMEM; }
    const unsigned blocks = gd_blocks(n);
    hipLaunchKernelGGL(k_geod_inverse, dim3(blocks), dim3(GD_BLOCK), 0, st, a, rf != 0.0 ? 1.0 / rf : 0.0, lon1, lat1, lon2, lat2, n,
                       az12, az21, dist, (uint32_t *)ws);
    TF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sum_counts, dim3(1), dim3(GD_BLOCK), 0, st, (const uint32_t *)ws, (int64_t)blocks, status);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

extern "C" size_t tf_grid_spacing_workspace_bytes(int64_t H, int64_t W)
{
    if (H <= 0 || W <= 0) return 0;
    const size_t plane = tf_align_up((size_t)H * (size_t)W * sizeof(double), 256);
    return 2 * plane + tf_geod_inverse_workspace_bytes(H * W);
}

extern "C" int tf_grid_spacing(double a, double rf, const double *lat, const double *lon, int64_t H, int64_t W, double *dx, double *dy,
                               double *area, uint32_t *status, void *ws, size_t ws_bytes, void *stream)
{
    TF_REQUIRE(gd_ellipsoid_ok(a, rf), "tf_grid_spacing: a is positive and finite, rf is 0 (a sphere) or above 1");
    TF_REQUIRE(H >= 0 && W >= 0 && (H == 0 || W <= GD_MAX_N / H), "tf_grid_spacing: bad grid size");
    TF_REQUIRE(status, "tf_grid_spacing: null status");
    hipStream_t st = (hipStream_t)stream;
    if (H == 0 || W == 0) {
        TF_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(uint32_t), st));
        return TF_OK;
    }
    TF_REQUIRE(lat && lon, "tf_grid_spacing: null pointer");
    TF_REQUIRE(dx || dy || area, "tf_grid_spacing: no output");
    if (!ws || ws_bytes < tf_grid_spacing_workspace_bytes(H, W)) { tf_set_error("tf_grid_spacing: workspace too small"); return TF_ENOMEM; }
    TfArena arena(ws, ws_bytes);
    double *raw_y = arena.take<double>((size_t)(H * W)), *raw_x = arena.take<double>((size_t)(H * W));
    const unsigned blocks = gd_blocks(H * W);
    uint32_t *counts = arena.take<uint32_t>(blocks);
    if (!arena.ok()) { tf_set_error("tf_grid_spacing: workspace too small"); return TF_ENOMEM; }
    if (!dy && !area) raw_y = nullptr;
    if (!dx && !area) raw_x = nullptr;
    hipLaunchKernelGGL(k_spacing_raw, dim3(blocks), dim3(GD_BLOCK), 0, st, a, rf != 0.0 ? 1.0 / rf : 0.0, lat, lon, H, W, raw_y, raw_x, counts);
    TF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_spacing_combine, dim3(blocks), dim3(GD_BLOCK), 0, st, (const double *)raw_y, (const double *)raw_x, H, W, dx, dy, area);
    TF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sum_counts, dim3(1), dim3(GD_BLOCK), 0, st, (const uint32_t *)counts, (int64_t)blocks, status);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

extern "C" int tf_view_angles(int mode, const double *scalars, int n_scalars, const double *lat, const double *lon, int64_t n,
                              const double *x, const double *y, int64_t W, double *out0, double *out1, void *stream)
{
    TF_REQUIRE(mode >= TF_VIEW_SZA && mode <= TF_VIEW_ABI_ZENITH, "tf_view_angles: unknown mode");
    const int want = mode == TF_VIEW_ABI_ZENITH ? 2 : 3;
    TF_REQUIRE(scalars && n_scalars == want, "tf_view_angles: the mode's scalars (3; 2 for TF_VIEW_ABI_ZENITH)");
    TF_REQUIRE(n >= 0 && n <= GD_MAX_N, "tf_view_angles: bad number of pixels");
    if (n == 0) return TF_OK;
    TF_REQUIRE(lat && lon && out0, "tf_view_angles: null pointer");
    const bool two = mode == TF_VIEW_SZA_AZI || mode == TF_VIEW_SATELLITE;
    TF_REQUIRE(two ? out1 != nullptr : out1 == nullptr, "tf_view_angles: out1 goes with the two-angle modes");
    if (mode == TF_VIEW_ABI_ZENITH) TF_REQUIRE(x && y && W >= 1 && n % W == 0, "tf_view_angles: x (W), y (n / W) for TF_VIEW_ABI_ZENITH");
    GdScalars sc = {{0, 0, 0, 0}};
    for (int k = 0; k < n_scalars; k++) sc.v[k] = scalars[k];
    hipLaunchKernelGGL(k_view_angles, dim3(gd_blocks(n)), dim3(GD_BLOCK), 0, (hipStream_t)stream, mode, sc, lat, lon, n, x, y, W, out0, out1);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

extern "C" int tf_ecef(int mode, double a, double rf, const double *in0, const double *in1, const double *in2, int64_t n, double *out0,
                       double *out1, double *out2, void *stream)
{
    TF_REQUIRE(mode == TF_ECEF_FROM_GEODETIC || mode == TF_ECEF_TO_GEODETIC, "tf_ecef: unknown mode");
    TF_REQUIRE(gd_ellipsoid_ok(a, rf), "tf_ecef: a is positive and finite, rf is 0 (a sphere) or above 1");
    TF_REQUIRE(n >= 0 && n <= GD_MAX_N, "tf_ecef: bad number of points");
    if (n == 0) return TF_OK;
    TF_REQUIRE(in0 && in1 && in2 && out0 && out1 && out2, "tf_ecef: null pointer");
    hipLaunchKernelGGL(k_ecef, dim3(gd_blocks(n)), dim3(GD_BLOCK), 0, (hipStream_t)stream, mode, a, rf != 0.0 ? 1.0 / rf : 0.0, in0, in1, in2,
                       n, out0, out1, out2);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

extern "C" int tf_geos_to_ecef(const TfGeos *geos, const double *x, const double *y, int64_t n, double *X, double *Y, double *Z,
                               void *stream)
{
    const int rc = gd_check_geos(geos, "tf_geos_to_ecef");
    if (rc != TF_OK) return rc;
    TF_REQUIRE(n >= 0 && n <= GD_MAX_N, "tf_geos_to_ecef: bad number of points");
    if (n == 0) return TF_OK;
    TF_REQUIRE(x && y && X && Y && Z, "tf_geos_to_ecef: null pointer");
    hipLaunchKernelGGL(k_geos_to_ecef, dim3(gd_blocks(n)), dim3(GD_BLOCK), 0, (hipStream_t)stream, gd_geos_setup(*geos), x, y, n, X, Y, Z);
    TF_CHECK_LAUNCH();
    return TF_OK;
}

extern "C" int tf_glm_parallax(const TfGeos *grid, const TfGeos *ltg, double lla_a, double lla_rf, const void *lat, const void *lon,
                               int in_dtype, int64_t n, double *dlon, double *dlat, double *x, double *y, void *stream)
{
    int rc = gd_check_geos(grid, "tf_glm_parallax (grid)");
    if (rc == TF_OK) rc = gd_check_geos(ltg, "tf_glm_parallax (ltg)");
    if (rc != TF_OK) return rc;
    TF_REQUIRE(grid->lon_0 == ltg->lon_0 && grid->sweep_y == ltg->sweep_y, "tf_glm_parallax: ltg shares lon_0 and sweep_y with grid");
    TF_REQUIRE(gd_ellipsoid_ok(lla_a, lla_rf), "tf_glm_parallax: lla_a is positive and finite, lla_rf is 0 (a sphere) or above 1");
    TF_REQUIRE(in_dtype == TF_F32 || in_dtype == TF_F64, "tf_glm_parallax: lat and lon are float32 or float64");
    TF_REQUIRE(n >= 0 && n <= GD_MAX_N, "tf_glm_parallax: bad number of flashes");
    if (n == 0) return TF_OK;
    TF_REQUIRE(lat && lon, "tf_glm_parallax: null pointer");
    TF_REQUIRE((dlon != nullptr) == (dlat != nullptr) && (x != nullptr) == (y != nullptr), "tf_glm_parallax: dlon goes with dlat, x with y");
    TF_REQUIRE(dlon || x, "tf_glm_parallax: no output");
    const GdParallax c = gd_parallax_setup(*grid, *ltg, lla_a, lla_rf);
    if (in_dtype == TF_F64)
        hipLaunchKernelGGL(k_glm_parallax<double>, dim3(gd_blocks(n)), dim3(GD_BLOCK), 0, (hipStream_t)stream, c, (const double *)lat,
                           (const double *)lon, n, dlon, dlat, x, y);
    else
        hipLaunchKernelGGL(k_glm_parallax<float>, dim3(gd_blocks(n)), dim3(GD_BLOCK), 0, (hipStream_t)stream, c, (const float *)lat,
                           (const float *)lon, n, dlon, dlat, x, y);
    TF_CHECK_LAUNCH();
    return TF_OK;
}
