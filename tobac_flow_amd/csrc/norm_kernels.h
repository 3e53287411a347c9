// Kernel bodies of norm_methods.hip (tf_norm8_pair): to_8bit(method(pair, **kw), 0, 1) for the joint normalisations of a
// frame pair other than the argument-free linear one (norm.hip).  Kept apart from the entry point so that the same text
// compiles for the host: tools/norm_host_check.cpp supplies the qualifiers and runs the bodies lane after lane.  Nothing
// here touches the HIP runtime, LDS or the lane index: a body is told which lane / row / chunk it is.
//
// Arithmetic contract: float32 IEEE operations in numpy's order (the library is built with -ffp-contract=off); scalars
// that numpy 2 treats as "weak" Python numbers are rounded to float32 where they meet a float32 value and stay double
// among themselves; the moments and log are evaluated in float64 and rounded to float32 (numpy's float32 pairwise sums
// and float32 log are not reproduced: DESIGN.md, "Normalisation methods").
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/tobac_flow_hip.h"
#include "radix_select.h"

#define NM_LANES 256                   // lanes per workgroup of every kernel here
#define NM_MAX_PARTIALS 1024           // workgroups of a reduction = partials the finish stage combines
#define NM_MAX_ROW 8192                // longest row the row filter holds in LDS (2 x 4 B x W <= 64 KB)

// ---- joint reductions --------------------------------------------------------------------------------------------------
// over the non-NaN values of both frames: minimum, maximum, their number, and one float64 sum -- of the
// values (stage 0) or of their squared deviations from a given mean (stage 1).  Lanes and workgroups keep partials that
// are combined in one fixed order (a tree over the lanes, then over the workgroups): no float atomics, identical bytes
// from run to run.
struct NmPartial { float lo, hi; unsigned long long n; double sum; };

__host__ __device__ inline NmPartial nm_empty() { NmPartial p; p.lo = INFINITY; p.hi = -INFINITY; p.n = 0; p.sum = 0; return p; }

__host__ __device__ inline NmPartial nm_combine(NmPartial a, const NmPartial &b)
{
    a.lo = fminf(a.lo, b.lo); a.hi = fmaxf(a.hi, b.hi); a.n += b.n; a.sum += b.sum;
    return a;
}

// elements first, first + stride, ... of the 2 n values of the pair (frame 0, then frame 1)
__host__ __device__ inline NmPartial nm_reduce_lane(const float *__restrict__ f0, const float *__restrict__ f1, int64_t n,
                                                    int64_t first, int64_t stride, bool deviations, double mean)
{
    NmPartial p = nm_empty();
    for (int64_t i = first; i < 2 * n; i += stride) {
        const float v = i < n ? f0[i] : f1[i - n];
        if (v != v) continue;
        p.lo = fminf(p.lo, v); p.hi = fmaxf(p.hi, v); p.n++;
        const double d = (double)v - mean;
        p.sum += deviations ? d * d : (double)v;
    }
    return p;
}

// ---- the scalars of a method -------------------------------------------------------------------------------------------
struct NmState {
    float lo, hi;                      // np.nanmin / np.nanmax of the pair (NaN when every value is NaN)
    unsigned long long n;              // non-NaN values
    double sum, m2;                    // of the values, of their squared deviations from sum / n
    float mean, sd;                    // np.nanmean, np.nanstd rounded to float32
    float lower, scale;                // linear_norm: (v - lower) * scale
};

// A bound of linear_norm: a float32 value (taken from the data, or given as a float32 scalar) or a weak Python number
struct NmBound { double v; bool weak; };

__host__ __device__ inline float nm_log(float v) { return (float)log((double)v); }

// linear_norm's `factor = 1 / (vmax - vmin) if vmax > vmin else 0` and `array - vmin`: two Python numbers are compared,
// subtracted and inverted as doubles before the result meets the array; with a float32 on either side it is float32
__host__ __device__ inline void nm_linear_scalars(NmBound lower, NmBound upper, NmState &s)
{
    if (lower.weak && upper.weak)
        s.scale = upper.v > lower.v ? (float)(1.0 / (upper.v - lower.v)) : 0.f;
    else {
        const float l = (float)lower.v, u = (float)upper.v;
        s.scale = u > l ? 1.f / (u - l) : 0.f;
    }
    s.lower = (float)lower.v;
}

// stage 0: the reduction of the values is in `total`; stage 1 (z_score only): that of the squared deviations
__host__ __device__ inline void nm_finish(int method, const TfNormParams &p, int stage, const NmPartial &total, NmState &s)
{
    const bool weak = !(p.flags & TF_NORM_F32_SCALARS);
    if (stage == 0) {
        s.n = total.n; s.sum = total.sum;
        s.lo = total.n ? total.lo : NAN; s.hi = total.n ? total.hi : NAN;
        s.mean = (float)(total.sum / (double)total.n);                           // 0 / 0 = NaN, as np.nanmean
        s.m2 = 0; s.sd = 0; s.lower = 0; s.scale = 0;
        const NmBound data_lo = {(double)s.lo, false}, data_hi = {(double)s.hi, false};
        const NmBound vmin = {p.vmin, weak}, vmax = {p.vmax, weak};
        if (method == TF_NORM_LINEAR)
            nm_linear_scalars((p.flags & TF_NORM_HAS_VMIN) ? vmin : data_lo, (p.flags & TF_NORM_HAS_VMAX) ? vmax : data_hi, s);
        else if (method == TF_NORM_LOG) {
            // the data minimum is reused as the lower bound of the LOG values; their maximum is the log of the largest
            // distance (log is monotone), evaluated as the map evaluates it
            const NmBound top = {(double)nm_log((s.hi - s.lo) + 1.f), false};
            nm_linear_scalars(data_lo, (p.flags & TF_NORM_HAS_VMAX) ? vmax : top, s);
        } else if (method == TF_NORM_INVERSE_LOG) {
            const NmBound bottom = {(double)nm_log((s.hi - s.hi) + 1.f), false};
            nm_linear_scalars((p.flags & TF_NORM_HAS_VMIN) ? vmin : bottom, data_hi, s);
        }
    } else {
        s.m2 = total.sum;
        s.sd = (float)sqrt(total.sum / (double)s.n);
        const NmBound lower = {-p.max_std, weak}, upper = {p.max_std, weak};
        nm_linear_scalars(lower, upper, s);
    }
}

// ---- elementwise maps --------------------------------------------------------------------------------------------------
__host__ __device__ inline float nm_clip_unit(float t)
{
    t = (t != t) ? t : fminf(t, 1.f);          // np.minimum(., 1), np.maximum(., 0): NaN propagates
    return (t != t) ? t : fmaxf(t, 0.f);
}

__host__ __device__ inline float nm_value(int method, float x, const NmState &s)
{
    float v = x;
    if (method == TF_NORM_LOG) v = nm_log((x - s.lo) + 1.f);
    else if (method == TF_NORM_INVERSE_LOG) v = nm_log((s.hi - x) + 1.f);
    else if (method == TF_NORM_Z_SCORE) v = (x - s.mean) / s.sd;
    return nm_clip_unit((v - s.lower) * s.scale);
}

// local_linear_norm at one pixel: NaN (and only NaN) was replaced by the mean before the filters ran
__host__ __device__ inline float nm_fill(float x, float mean) { return x != x ? mean : x; }
__host__ __device__ inline float nm_local_value(float x, float mean, float lowest, float highest)
{
    const float span = highest - lowest;
    const float scale = span == 0.f ? 0.f : 1.f / span;
    return (nm_fill(x, mean) - lowest) * scale;
}

// to_8bit(., 0, 1) of the pair's two values at one pixel: x 255 in float32, non-finite -> 127, patched from the other
// frame (frame 0 first, then frame 1), truncated
__host__ __device__ inline void nm_tail(float t0, float t1, uint8_t &b0, uint8_t &b1)
{
    float u0 = (t0 - 0.f) * 255.f, u1 = (t1 - 0.f) * 255.f;
    const bool f0 = u0 - u0 == 0.f, f1 = u1 - u1 == 0.f;          // finite
    if (!f0) u0 = 127.f;
    if (!f1) u1 = 127.f;
    if (!f0) u0 = u1;
    if (!f1) u1 = u0;
    b0 = (uint8_t)(int)u0;
    b1 = (uint8_t)(int)u1;
}

__host__ __device__ inline void nm_map_lane(int method, const float *__restrict__ f0, const float *__restrict__ f1, int64_t n,
                                            int64_t first, int64_t stride, const NmState &s,
                                            uint8_t *__restrict__ o0, uint8_t *__restrict__ o1)
{
    for (int64_t i = first; i < n; i += stride)
        nm_tail(nm_value(method, f0[i], s), nm_value(method, f1[i], s), o0[i], o1[i]);
}

// ---- local_linear: running minimum and maximum over the window clipped to the frame --------------------------------------
// Output i of a filter of `size` sees inputs i - size / 2 .. i + (size - 1) / 2 (SciPy's centre); its "reflect" border
// only repeats values the clipped window already holds.  van Herk / Gil-Werman: the axis is cut into chunks of `size`
// starting at 0; with g the running extreme from a chunk's start forwards and h from its end backwards, the window
// [a, b] (b - a = size - 1) spans at most the end of a's chunk and the start of b's:  out = op(h[a], g[b]).  At the
// borders: a < 0 has no h part (then b lies in chunk 0, whose g starts at 0); b beyond the last element takes g at the
// last element if b's chunk still starts inside the axis, and has no g part otherwise.  Three operations per element
// whatever the size.
struct NmWindow { int w, left, right; };          // chunk length, reach to the left and to the right

// a window that reaches beyond the axis on both sides from every position is the whole axis: `size` is clamped so that
// the index arithmetic stays within int
__host__ __device__ inline NmWindow nm_window(int64_t size, int64_t len)
{
    NmWindow k;
    k.w = (int)(size < 2 * len + 2 ? size : 2 * len + 2);
    k.left = k.w / 2; k.right = (k.w - 1) / 2;
    return k;
}

template <bool MAX> __host__ __device__ inline float nm_op(float a, float b) { return MAX ? fmaxf(a, b) : fminf(a, b); }
template <bool MAX> __host__ __device__ inline float nm_ident() { return MAX ? -INFINITY : INFINITY; }

// Row filter, three phases of one workgroup over one row held in two LDS arrays A and B of W floats (a barrier between
// the phases).  src1 == nullptr: the row of one frame; otherwise the pointwise extreme of the two frames' rows.
template <bool MAX>
__host__ __device__ inline void nm_row_load(int tid, const float *__restrict__ src0, const float *__restrict__ src1, int W, float mean, float *A)
{
    for (int x = tid; x < W; x += NM_LANES) {
        float v = nm_fill(src0[x], mean);
        if (src1) v = nm_op<MAX>(v, nm_fill(src1[x], mean));
        A[x] = v;
    }
}

// B = h (from A backwards), then A = g in place: one lane per chunk
template <bool MAX>
__host__ __device__ inline void nm_row_scan(int tid, int W, NmWindow k, float *A, float *B)
{
    for (int x0 = tid * k.w; x0 < W; x0 += NM_LANES * k.w) {        // (W <= NM_MAX_ROW and w <= 2 W + 2: within int)
        const int x1 = x0 + k.w < W ? x0 + k.w : W;
        float run = nm_ident<MAX>();
        for (int x = x1 - 1; x >= x0; x--) { run = nm_op<MAX>(run, A[x]); B[x] = run; }
        run = nm_ident<MAX>();
        for (int x = x0; x < x1; x++) { run = nm_op<MAX>(run, A[x]); A[x] = run; }
    }
}

template <bool MAX>
__host__ __device__ inline float nm_window_value(int i, int len, NmWindow k, const float *g, const float *h, int64_t step)
{
    const int a = i - k.left, b = i + k.right;
    float v = nm_ident<MAX>();
    if (b / k.w * k.w <= len - 1) v = g[(int64_t)(b < len ? b : len - 1) * step];
    if (a >= 0) v = nm_op<MAX>(v, h[(int64_t)a * step]);
    return v;
}

template <bool MAX>
__host__ __device__ inline void nm_row_emit(int tid, int W, NmWindow k, const float *A, const float *B, float *__restrict__ out)
{
    for (int x = tid; x < W; x += NM_LANES) out[x] = nm_window_value<MAX>(x, W, k, A, B, 1);
}

// Column filter, lanes side by side along x.  Pass 1, lane (x, chunk c): h of the two row-filtered planes, backwards.
__host__ __device__ inline void nm_col_suffix_lane(int64_t lane, int64_t H, int64_t W, NmWindow k,
                                                   const float *__restrict__ rmin, const float *__restrict__ rmax,
                                                   float *__restrict__ hmin, float *__restrict__ hmax)
{
    const int64_t chunks = (H + k.w - 1) / k.w;
    if (lane >= W * chunks) return;
    const int64_t x = lane % W, y0 = lane / W * k.w, y1 = y0 + k.w < H ? y0 + k.w : H;
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t y = y1 - 1; y >= y0; y--) {
        lo = fminf(lo, rmin[y * W + x]); hi = fmaxf(hi, rmax[y * W + x]);
        hmin[y * W + x] = lo; hmax[y * W + x] = hi;
    }
}

// Pass 2, lane (x, chunk c) walks b over its chunk with g in registers and finishes the outputs y = b - right: the
// window's extremes, the map and the 8-bit tail for both frames.  The two frames read the same planes except for
// size < 3, where the window does not cover the pair axis from both of them (see norm_methods.hip).
struct NmPlanes { const float *rmin, *rmax, *hmin, *hmax; };

__host__ __device__ inline int64_t nm_col_chunks(int64_t H, NmWindow k) { return (H - 1 + k.right) / k.w + 1; }

__host__ __device__ inline void nm_col_finish_lane(int64_t lane, int64_t H, int64_t W, NmWindow k, NmPlanes p0, NmPlanes p1,
                                                   bool shared, const float *__restrict__ f0, const float *__restrict__ f1,
                                                   float mean, uint8_t *__restrict__ o0, uint8_t *__restrict__ o1)
{
    if (lane >= W * nm_col_chunks(H, k)) return;
    const int64_t x = lane % W, b0 = lane / W * k.w;
    const int64_t b1 = b0 + k.w - 1 < H - 1 + k.right ? b0 + k.w - 1 : H - 1 + k.right;
    float g[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};       // min, max for frame 0; for frame 1
    for (int64_t b = b0; b <= b1; b++) {
        if (b < H) {
            g[0] = fminf(g[0], p0.rmin[b * W + x]); g[1] = fmaxf(g[1], p0.rmax[b * W + x]);
            if (!shared) { g[2] = fminf(g[2], p1.rmin[b * W + x]); g[3] = fmaxf(g[3], p1.rmax[b * W + x]); }
        }
        const int64_t y = b - k.right, a = b - k.w + 1;
        if (y < 0) continue;
        float e[4] = {g[0], g[1], g[2], g[3]};
        if (a >= 0) {
            e[0] = fminf(e[0], p0.hmin[a * W + x]); e[1] = fmaxf(e[1], p0.hmax[a * W + x]);
            if (!shared) { e[2] = fminf(e[2], p1.hmin[a * W + x]); e[3] = fmaxf(e[3], p1.hmax[a * W + x]); }
        }
        if (shared) { e[2] = e[0]; e[3] = e[1]; }
        const int64_t i = y * W + x;
        nm_tail(nm_local_value(f0[i], mean, e[0], e[1]), nm_local_value(f1[i], mean, e[2], e[3]), o0[i], o1[i]);
    }
}

// ---- uniform: exact order statistics by a multi-rank radix select, then a digitising map -------------------------------
// np.quantile(pair, np.linspace(0, 1, Q + 1)) (method "linear") reads two order statistics per edge: R = 2 (Q + 1) ranks.
// They are found on the order-preserving 32-bit keys in three passes of 11 + 11 + 10 bits (the keys, the digit plan, the
// histogram scan and the rank look-up are radix_select.h's, shared with field_stats.hip).  Every rank carries the key
// prefix found so far and its residual rank among the keys with that prefix; the distinct prefixes of a pass are its
// "active" slots (sorted, at most R), each with a histogram of the pass's digit.  A workgroup counts the first
// NM_LDS_SLOTS slots in LDS and adds them to the global counters at its end -- one slot in the first pass, a handful in
// the second for a field whose values share their leading bits -- and the others, which few keys reach, directly.
#define NM_MAX_RANKS (2 * (TF_NORM_MAX_QUANTILES + 1))
#define NM_BINS RS_BINS
#define NM_LDS_SLOTS 4
#define NM_RANKS_PER_LANE ((NM_MAX_RANKS + NM_LANES - 1) / NM_LANES)

static_assert(NM_LANES == RS_LANES, "the shared histogram scan is written for this workgroup");
#define NM_KEY_BITS 32
__host__ __device__ inline int nm_prefix_shift(int pass) { return rs_prefix_shift(NM_KEY_BITS, pass); }
__host__ __device__ inline int nm_digit_bits(int pass) { return rs_digit_bits(NM_KEY_BITS, pass); }

struct NmSelect {
    unsigned *resid, *prefix, *active;      // per rank: residual rank, key prefix; the sorted distinct prefixes
    int *slot, *nactive;                    // per rank: index of its prefix in `active`; their number
    double *gamma, *edges;                  // per edge: the interpolation weight, the edge
    unsigned *hist;                         // NM_BINS counters per slot
};

// edge k of Q: q = np.linspace(0, 1, Q + 1)[k], virtual index (n - 1) q, its two neighbours and the weight
__host__ __device__ inline void nm_plan_lane(int k, int Q, unsigned long long count, NmSelect s)
{
    if (k > Q) return;
    const double q = k == Q ? 1.0 : (double)k * (1.0 / (double)Q);
    const double v = (double)(count - 1) * q;
    double prev = floor(v), next = prev + 1, gamma = v - prev;
    if (v >= (double)(count - 1)) { prev = next = (double)(count - 1); gamma = 1; }   // numpy takes the last element twice
    s.resid[2 * k] = (unsigned)prev; s.resid[2 * k + 1] = (unsigned)next;
    s.prefix[2 * k] = s.prefix[2 * k + 1] = 0u;
    s.slot[2 * k] = s.slot[2 * k + 1] = 0;
    s.gamma[k] = gamma;
    if (k == 0) { s.active[0] = 0u; *s.nactive = 1; }
}

// one lane's share of a pass's histograms; `active` and `lds_hist` are the workgroup's LDS copies
__host__ __device__ inline void nm_hist_lane(const float *__restrict__ f0, const float *__restrict__ f1, int64_t n, int64_t first,
                                             int64_t stride, int pass, const unsigned *active, int nactive, unsigned *lds_hist,
                                             unsigned *__restrict__ hist)
{
    const int pshift = nm_prefix_shift(pass), dshift = pshift - nm_digit_bits(pass);
    const unsigned dmask = (1u << nm_digit_bits(pass)) - 1u;
    for (int64_t i = first; i < 2 * n; i += stride) {
        const unsigned key = rs_key(i < n ? f0[i] : f1[i - n]);
        const unsigned prefix = (unsigned)((unsigned long long)key >> pshift), digit = (key >> dshift) & dmask;
        int lo = 0, hi = nactive;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (active[mid] < prefix) lo = mid + 1; else hi = mid; }
        if (lo == nactive || active[lo] != prefix) continue;
        if (lo < NM_LDS_SLOTS) atomicAdd(&lds_hist[lo * NM_BINS + digit], 1u);
        else atomicAdd(&hist[(size_t)lo * NM_BINS + digit], 1u);
    }
}

__host__ __device__ inline void nm_hist_flush(int tid, int nactive, const unsigned *lds_hist, unsigned *__restrict__ hist)
{
    const int m = (nactive < NM_LDS_SLOTS ? nactive : NM_LDS_SLOTS) * NM_BINS;
    for (int i = tid; i < m; i += NM_LANES) if (lds_hist[i]) atomicAdd(&hist[i], lds_hist[i]);
}

// Resolve, one workgroup, lane t owns ranks NM_RANKS_PER_LANE t ...: (1) the digit of each rank from its slot's running
// sums -- the last bin that starts at or below the residual rank -- into newp (LDS); (2) the number of ranks in the lane's
// block whose prefix differs from the previous rank's (the ranks ascend, so equal prefixes are neighbours) into cnt (LDS);
// (3) the new slots and the list of active prefixes.
__host__ __device__ inline void nm_resolve_digit(int tid, int R, int pass, NmSelect s, unsigned *newp)
{
    const int bins = 1 << nm_digit_bits(pass);
    for (int j = tid * NM_RANKS_PER_LANE; j < (tid + 1) * NM_RANKS_PER_LANE && j < R; j++) {
        const unsigned *cum = s.hist + (size_t)s.slot[j] * NM_BINS;
        const unsigned r = s.resid[j];
        const int b = rs_rank_bin(cum, bins, r);
        s.resid[j] = r - cum[b];
        newp[j] = (pass == 0 ? 0u : s.prefix[j] << nm_digit_bits(pass)) | (unsigned)b;
    }
}
__host__ __device__ inline void nm_resolve_count(int tid, int R, const unsigned *newp, unsigned *cnt)
{
    unsigned c = 0;
    for (int j = tid * NM_RANKS_PER_LANE; j < (tid + 1) * NM_RANKS_PER_LANE && j < R; j++) c += j == 0 || newp[j] != newp[j - 1];
    cnt[tid] = c;
}
__host__ __device__ inline void nm_resolve_slots(int tid, int R, NmSelect s, const unsigned *newp, const unsigned *cnt)
{
    int at = 0;
    for (int t = 0; t < tid; t++) at += (int)cnt[t];
    for (int j = tid * NM_RANKS_PER_LANE; j < (tid + 1) * NM_RANKS_PER_LANE && j < R; j++) {
        if (j == 0 || newp[j] != newp[j - 1]) s.active[at++] = newp[j];
        s.slot[j] = at - 1;
        s.prefix[j] = newp[j];
        if (j == R - 1) *s.nactive = at;
    }
}

// after the last pass a rank's prefix is its key.  numpy's _lerp: the difference in float32, the rest in float64, from
// the right neighbour when the weight is at least one half; the last edge + 1
__host__ __device__ inline void nm_edge_lane(int k, int Q, NmSelect s, const unsigned *keys)
{
    if (k > Q) return;
    const float a = rs_unkey(keys[2 * k]), b = rs_unkey(keys[2 * k + 1]);
    const double t = s.gamma[k], diff = (double)(b - a);
    double e = t >= 0.5 ? (double)b - diff * (1 - t) : (double)a + diff * t;
    if (k == Q) e = e + 1;
    s.edges[k] = e;
}

// np.digitize(x, edges) for ascending edges: how many are <= x
__host__ __device__ inline int nm_bin(const double *edges, int ne, double x)
{
    int lo = 0, hi = ne;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (edges[mid] <= x) lo = mid + 1; else hi = mid; }
    return lo;
}

// linear_norm of the bins (int64 -> float64) and to_8bit(., 0, 1) in float64; every value is finite
__host__ __device__ inline uint8_t nm_uniform_byte(const double *edges, int ne, float x, int lower, double scale)
{
    double t = (double)(nm_bin(edges, ne, (double)x) - lower) * scale;
    t = fmax(fmin(t, 1.0), 0.0);
    return (uint8_t)(int)((t - 0.0) * 255.0);
}

__host__ __device__ inline void nm_uniform_map_lane(const float *__restrict__ f0, const float *__restrict__ f1, int64_t n, int64_t first,
                                                    int64_t stride, const double *edges, int ne, float lo, float hi,
                                                    uint8_t *__restrict__ o0, uint8_t *__restrict__ o1)
{
    const int lower = nm_bin(edges, ne, (double)lo), upper = nm_bin(edges, ne, (double)hi);
    const double scale = upper > lower ? 1.0 / (double)(upper - lower) : 0.0;
    for (int64_t i = first; i < n; i += stride) {
        o0[i] = nm_uniform_byte(edges, ne, f0[i], lower, scale);
        o1[i] = nm_uniform_byte(edges, ne, f1[i], lower, scale);
    }
}
