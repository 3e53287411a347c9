// tf_norm8_pair: to_8bit(method(data[i:i+2], **kwargs), 0, 1) for the normalisation methods that
// tobac_flow/flow.py:411-414 of the reference selects by name
// (tobac_flow/utils/normalisation_utils.py:59-116).  The bodies are in norm_kernels.h; this file is
// the workgroup plumbing (LDS, barriers, launch geometry) and the entry point.
//
// Passes over the pair, per pixel pair (two float32 in, two bytes out):
//   every method   reduction                         8 B read
//   z_score        second reduction (deviations)     8 B read
//   linear / log / inverse_log / z_score: map        8 B read + 2 B written
//   local_linear   row filter                        8 B read (the maximum's second read of the row hits L2) + 8 B written
//                  column suffix pass                8 B read + 8 B written
//                  column prefix pass + map          16 B + 8 B read, 2 B written
//   uniform        three histogram passes            3 x 8 B read (plus counters: 8 KB per active key prefix)
//                  digitising map                    8 B read + 2 B written
#include "tf_common.h"
#include "norm_kernels.h"

namespace {

// the partials of a workgroup's lanes, then of the workgroups, combined as one tree: s[t] += s[t + o] for o = 128 .. 1
__device__ __forceinline__ NmPartial nm_block_tree(NmPartial p, NmPartial *s)
{
    s[threadIdx.x] = p;
    __syncthreads();
    for (int o = NM_LANES / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] = nm_combine(s[threadIdx.x], s[threadIdx.x + o]);
        __syncthreads();
    }
    return s[0];
}

__global__ void __launch_bounds__(NM_LANES)
k_nm_reduce(const float *__restrict__ f0, const float *__restrict__ f1, int64_t n, int stage, const NmState *__restrict__ st,
            NmPartial *__restrict__ part)
{
    __shared__ NmPartial s[NM_LANES];
    const double mean = stage ? st->sum / (double)st->n : 0.0;
    const NmPartial p = nm_reduce_lane(f0, f1, n, (int64_t)blockIdx.x * NM_LANES + threadIdx.x, (int64_t)gridDim.x * NM_LANES,
                                       stage != 0, mean);
    const NmPartial total = nm_block_tree(p, s);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

__global__ void __launch_bounds__(NM_LANES)
k_nm_finish(const NmPartial *__restrict__ part, int parts, int method, TfNormParams params, int stage, NmState *__restrict__ st)
{
    __shared__ NmPartial s[NM_LANES];
    NmPartial p = nm_empty();
    for (int i = threadIdx.x; i < parts; i += NM_LANES) p = nm_combine(p, part[i]);
    const NmPartial total = nm_block_tree(p, s);
    if (threadIdx.x == 0) nm_finish(method, params, stage, total, *st);
}

__global__ void __launch_bounds__(NM_LANES)
k_nm_map(const float *__restrict__ f0, const float *__restrict__ f1, int64_t n, int method, const NmState *__restrict__ st,
         uint8_t *__restrict__ o0, uint8_t *__restrict__ o1)
{
    const NmState s = *st;
    nm_map_lane(method, f0, f1, n, (int64_t)blockIdx.x * NM_LANES + threadIdx.x, (int64_t)gridDim.x * NM_LANES, s, o0, o1);
}

// one workgroup per row (grid-stride): the running minimum into rmin, then the running maximum into rmax
__global__ void __launch_bounds__(NM_LANES)
k_nm_row_filter(const float *__restrict__ src0, const float *__restrict__ src1, int H, int W, NmWindow k,
                const NmState *__restrict__ st, float *__restrict__ rmin, float *__restrict__ rmax)
{
    extern __shared__ float lds[];
    float *A = lds, *B = lds + W;
    const float mean = st->mean;
    const int tid = threadIdx.x;
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        const int64_t row = (int64_t)y * W;
        nm_row_load<false>(tid, src0 + row, src1 ? src1 + row : nullptr, W, mean, A);
        __syncthreads();
        nm_row_scan<false>(tid, W, k, A, B);
        __syncthreads();
        nm_row_emit<false>(tid, W, k, A, B, rmin + row);
        __syncthreads();
        nm_row_load<true>(tid, src0 + row, src1 ? src1 + row : nullptr, W, mean, A);
        __syncthreads();
        nm_row_scan<true>(tid, W, k, A, B);
        __syncthreads();
        nm_row_emit<true>(tid, W, k, A, B, rmax + row);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(NM_LANES)
k_nm_col_suffix(int64_t H, int64_t W, NmWindow k, const float *__restrict__ rmin, const float *__restrict__ rmax,
                float *__restrict__ hmin, float *__restrict__ hmax)
{
    nm_col_suffix_lane((int64_t)blockIdx.x * NM_LANES + threadIdx.x, H, W, k, rmin, rmax, hmin, hmax);
}

__global__ void __launch_bounds__(NM_LANES)
k_nm_col_finish(int64_t H, int64_t W, NmWindow k, NmPlanes p0, NmPlanes p1, bool shared, const float *__restrict__ f0,
                const float *__restrict__ f1, const NmState *__restrict__ st, uint8_t *__restrict__ o0, uint8_t *__restrict__ o1)
{
    nm_col_finish_lane((int64_t)blockIdx.x * NM_LANES + threadIdx.x, H, W, k, p0, p1, shared, f0, f1, st->mean, o0, o1);
}

// ---- uniform ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NM_LANES)
k_nm_plan(int Q, const NmState *__restrict__ st, NmSelect sel)
{
    for (int k = threadIdx.x; k <= Q; k += NM_LANES) nm_plan_lane(k, Q, st->n, sel);
}

__global__ void __launch_bounds__(NM_LANES)
k_nm_hist(const float *__restrict__ f0, const float *__restrict__ f1, int64_t n, int pass, NmSelect sel)
{
    __shared__ unsigned active[NM_MAX_RANKS];
    __shared__ unsigned lds_hist[NM_LDS_SLOTS * NM_BINS];
    const int tid = threadIdx.x, nactive = *sel.nactive;
    for (int i = tid; i < nactive; i += NM_LANES) active[i] = sel.active[i];
    for (int i = tid; i < NM_LDS_SLOTS * NM_BINS; i += NM_LANES) lds_hist[i] = 0u;
    __syncthreads();
    nm_hist_lane(f0, f1, n, (int64_t)blockIdx.x * NM_LANES + tid, (int64_t)gridDim.x * NM_LANES, pass, active, nactive, lds_hist, sel.hist);
    __syncthreads();
    nm_hist_flush(tid, nactive, lds_hist, sel.hist);
}

// one workgroup per active slot (the grid is sized for the most there can be)
__global__ void __launch_bounds__(NM_LANES)
k_nm_scan(NmSelect sel)
{
    __shared__ unsigned part[NM_LANES];
    if ((int)blockIdx.x >= *sel.nactive) return;
    unsigned *h = sel.hist + (size_t)blockIdx.x * NM_BINS;
    rs_scan_sum(threadIdx.x, h, part);
    __syncthreads();
    rs_scan_write(threadIdx.x, h, part);
}

__global__ void __launch_bounds__(NM_LANES)
k_nm_resolve(int Q, int pass, NmSelect sel)
{
    __shared__ unsigned newp[NM_MAX_RANKS], cnt[NM_LANES];
    const int tid = threadIdx.x, R = 2 * (Q + 1);
    nm_resolve_digit(tid, R, pass, sel, newp);
    __syncthreads();
    nm_resolve_count(tid, R, newp, cnt);
    __syncthreads();
    nm_resolve_slots(tid, R, sel, newp, cnt);
    if (pass == 2)
        for (int k = tid; k <= Q; k += NM_LANES) nm_edge_lane(k, Q, sel, newp);
}

__global__ void __launch_bounds__(NM_LANES)
k_nm_uniform_map(const float *__restrict__ f0, const float *__restrict__ f1, int64_t n, int Q, const NmState *__restrict__ st,
                 const double *__restrict__ edges_in, uint8_t *__restrict__ o0, uint8_t *__restrict__ o1)
{
    __shared__ double edges[TF_NORM_MAX_QUANTILES + 1];
    for (int k = threadIdx.x; k <= Q; k += NM_LANES) edges[k] = edges_in[k];
    __syncthreads();
    nm_uniform_map_lane(f0, f1, n, (int64_t)blockIdx.x * NM_LANES + threadIdx.x, (int64_t)gridDim.x * NM_LANES, edges, Q + 1,
                        st->lo, st->hi, o0, o1);
}

int reduction_workgroups(int64_t n)
{
    const int64_t g = (2 * n + NM_LANES * 16 - 1) / (NM_LANES * 16);
    return (int)(g < 1 ? 1 : g > NM_MAX_PARTIALS ? NM_MAX_PARTIALS : g);
}

// SciPy's window along the PAIR axis (frames f - size / 2 .. f + (size - 1) / 2, reflected) holds both frames from size 3
// on; size 1 sees the frame itself, size 2 sees {0} from frame 0 and {0, 1} from frame 1
int plane_sets(int64_t size) { return size >= 3 ? 1 : 2; }

struct Layout { NmState *st; NmPartial *part; float *planes[8]; NmSelect sel; bool ok; };

Layout layout(void *ws, size_t ws_bytes, int64_t H, int64_t W, int method, const TfNormParams &p)
{
    TfArena a(ws, ws_bytes);
    Layout l = {};
    l.st = a.take<NmState>(1);
    l.part = a.take<NmPartial>(NM_MAX_PARTIALS);
    if (method == TF_NORM_LOCAL_LINEAR)
        for (int i = 0; i < 4 * plane_sets(p.size); i++) l.planes[i] = a.take<float>((size_t)(H * W));
    if (method == TF_NORM_UNIFORM) {
        const size_t R = 2 * (size_t)(p.quantiles + 1);
        l.sel.resid = a.take<unsigned>(R); l.sel.prefix = a.take<unsigned>(R); l.sel.active = a.take<unsigned>(R);
        l.sel.slot = a.take<int>(R); l.sel.nactive = a.take<int>(1);
        l.sel.gamma = a.take<double>(R / 2); l.sel.edges = a.take<double>(R / 2);
        l.sel.hist = a.take<unsigned>(R * NM_BINS);
    }
    l.ok = a.ok();
    return l;
}

const char *check_args(int64_t H, int64_t W, int method, const TfNormParams *p)
{
    if (!p) return "tf_norm8: params is null";
    if (H <= 0 || W <= 0 || H > INT32_MAX || W > INT32_MAX || H * W > INT32_MAX) return "tf_norm8: bad shape (H * W < 2^31)";
    if (method < TF_NORM_LINEAR || method > TF_NORM_LOCAL_LINEAR) return "tf_norm8: unknown method";
    if (method == TF_NORM_UNIFORM && (p->quantiles < 1 || p->quantiles > TF_NORM_MAX_QUANTILES)) return "tf_norm8: quantiles must be in 1 .. 1024";
    if (method == TF_NORM_UNIFORM && 2 * H * W < 2 * (p->quantiles + 1)) return "tf_norm8: uniform needs at least 2 (quantiles + 1) values";
    if (method == TF_NORM_LOCAL_LINEAR && p->size < 1) return "tf_norm8: size must be >= 1";
    if (method == TF_NORM_LOCAL_LINEAR && W > NM_MAX_ROW) return "tf_norm8: local_linear filters rows of at most 8192 pixels";
    return nullptr;
}

}  // namespace

static_assert(NM_MAX_ROW == TF_NORM_MAX_ROW, "the header's row limit is the kernels'");

extern "C" void tf_norm8_default_params(TfNormParams *p)
{
    if (!p) return;
    p->vmin = 0; p->vmax = 0; p->max_std = 3; p->quantiles = 256; p->size = 100; p->flags = 0;
}

extern "C" size_t tf_norm8_workspace_bytes(int64_t H, int64_t W, int method, const TfNormParams *params)
{
    if (check_args(H, W, method, params)) return 0;
    size_t bytes = tf_align_up(sizeof(NmState), 256) + tf_align_up(NM_MAX_PARTIALS * sizeof(NmPartial), 256);
    if (method == TF_NORM_LOCAL_LINEAR) bytes += 4 * plane_sets(params->size) * tf_align_up((size_t)(H * W) * sizeof(float), 256);
    if (method == TF_NORM_UNIFORM) {
        const size_t R = 2 * (size_t)(params->quantiles + 1);
        bytes += 4 * tf_align_up(R * 4, 256) + 256 + 2 * tf_align_up(R / 2 * 8, 256) + tf_align_up(R * NM_BINS * 4, 256);
    }
    return bytes;
}

extern "C" int tf_norm8_pair(const float *frame0, const float *frame1, int64_t H, int64_t W, int method,
                             const TfNormParams *params, uint8_t *out0, uint8_t *out1, void *ws, size_t ws_bytes, void *stream)
{
    if (const char *msg = check_args(H, W, method, params)) { tf_set_error("%s", msg); return TF_EINVAL; }
    TF_REQUIRE(frame0 && frame1 && out0 && out1 && ws, "tf_norm8_pair: null pointer");
    const Layout l = layout(ws, ws_bytes, H, W, method, *params);
    if (!l.ok || ws_bytes < tf_norm8_workspace_bytes(H, W, method, params)) { tf_set_error("tf_norm8_pair: workspace too small"); return TF_ENOMEM; }
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = H * W;
    const int red = reduction_workgroups(n);
    int64_t blocks = (n + NM_LANES - 1) / NM_LANES; if (blocks > 4096) blocks = 4096;
    const double bytes[] = {18, 18, 18, 26, 42, 66};
    TfProfScope ps(TFK_NORM8, bytes[method] * n, s);
    hipLaunchKernelGGL(k_nm_reduce, dim3(red), dim3(NM_LANES), 0, s, frame0, frame1, n, 0, l.st, l.part);
    hipLaunchKernelGGL(k_nm_finish, dim3(1), dim3(NM_LANES), 0, s, l.part, red, method, *params, 0, l.st);
    if (method == TF_NORM_Z_SCORE) {
        hipLaunchKernelGGL(k_nm_reduce, dim3(red), dim3(NM_LANES), 0, s, frame0, frame1, n, 1, l.st, l.part);
        hipLaunchKernelGGL(k_nm_finish, dim3(1), dim3(NM_LANES), 0, s, l.part, red, method, *params, 1, l.st);
    }
    if (method == TF_NORM_UNIFORM) {
        const int Q = (int)params->quantiles, R = 2 * (Q + 1);
        int64_t groups = (2 * n + NM_LANES * 32 - 1) / (NM_LANES * 32); if (groups > 1024) groups = 1024;
        hipLaunchKernelGGL(k_nm_plan, dim3(1), dim3(NM_LANES), 0, s, Q, l.st, l.sel);
        for (int pass = 0; pass < 3; pass++) {
            TF_CHECK_HIP(hipMemsetAsync(l.sel.hist, 0, (size_t)R * NM_BINS * sizeof(unsigned), s));
            hipLaunchKernelGGL(k_nm_hist, dim3((unsigned)groups), dim3(NM_LANES), 0, s, frame0, frame1, n, pass, l.sel);
            hipLaunchKernelGGL(k_nm_scan, dim3(R), dim3(NM_LANES), 0, s, l.sel);
            hipLaunchKernelGGL(k_nm_resolve, dim3(1), dim3(NM_LANES), 0, s, Q, pass, l.sel);
        }
        hipLaunchKernelGGL(k_nm_uniform_map, dim3((unsigned)blocks), dim3(NM_LANES), 0, s, frame0, frame1, n, Q, l.st, l.sel.edges, out0, out1);
        TF_CHECK_LAUNCH();
        return TF_OK;
    }
    if (method != TF_NORM_LOCAL_LINEAR) {
        hipLaunchKernelGGL(k_nm_map, dim3((unsigned)blocks), dim3(NM_LANES), 0, s, frame0, frame1, n, method, l.st, out0, out1);
        TF_CHECK_LAUNCH();
        return TF_OK;
    }
    const NmWindow kx = nm_window(params->size, W), ky = nm_window(params->size, H);
    const int sets = plane_sets(params->size);
    NmPlanes p[2];
    for (int f = 0; f < sets; f++) {
        float *const *q = l.planes + 4 * f;
        // the frames this set's window holds along the pair axis
        const float *src0 = frame0, *src1 = frame1;
        if (sets == 2 && (params->size == 1 || f == 0)) { src0 = f ? frame1 : frame0; src1 = nullptr; }
        const int rows = (int)(H < 2048 ? H : 2048);
        hipLaunchKernelGGL(k_nm_row_filter, dim3(rows), dim3(NM_LANES), 2 * (size_t)W * sizeof(float), s, src0, src1, (int)H, (int)W,
                           kx, l.st, q[0], q[1]);
        const int64_t lanes = W * ((H + ky.w - 1) / ky.w);
        hipLaunchKernelGGL(k_nm_col_suffix, dim3((unsigned)((lanes + NM_LANES - 1) / NM_LANES)), dim3(NM_LANES), 0, s, H, W, ky,
                           q[0], q[1], q[2], q[3]);
        p[f] = NmPlanes{q[0], q[1], q[2], q[3]};
    }
    if (sets == 1) p[1] = p[0];
    const int64_t lanes = W * nm_col_chunks(H, ky);
    hipLaunchKernelGGL(k_nm_col_finish, dim3((unsigned)((lanes + NM_LANES - 1) / NM_LANES)), dim3(NM_LANES), 0, s, H, W, ky, p[0], p[1],
                       sets == 1, frame0, frame1, l.st, out0, out1);
    TF_CHECK_LAUNCH();
    return TF_OK;
}
