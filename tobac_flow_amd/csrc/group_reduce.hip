// Grouped reductions over step records on gfx950: the table side of the third stage.
//
//   tf_group_reduce   tobac_flow/utils/stats_utils.py:171-349 (the *_groupby helpers), utils/filter_utils.py:33-289 and
//                     postprocess.py:313-1170 -- what the reference computes per object with a Python list comprehension
//                     over xarray.groupby, once per variable: a segmented reduction over the step records
//
// One call groups once and evaluates up to sixteen column operations:
//   rank     per record, its group's position in the sorted `coord` by binary search (G for an id that is not there)
//   sort     rocPRIM's stable radix sort of (rank, original position) over the bits G needs: (rank, position) order, so
//            the members of a group stay in the record order of the input -- what xarray's groupby hands to its reducers
//   bounds   start[r] = first sorted slot of rank r, for r = 0 .. G + 1 (rank G collects the orphan records); plain stores
//   walk     every run is walked in that order, once or twice per operation: by ONE LANE where it is shorter than a
//            wavefront, by the WHOLE WAVE in step where it is longer (k_gr_walk)
//
// Why split by length: every reduction is defined as a left-to-right walk (float64 sums in record order, first
// occurrence wins, a three-point gradient), i.e. a dependent chain per group.  The parallelism is across groups: 10^5
// to 10^6 of them, about ten records each, so a lane per group fills the machine and a wavefront per group would idle
// 63 lanes on the chain.  But a lane pays a dependent pair of loads (position, then value) per record, and a wave lasts
// as long as its longest run: with one lane per group throughout, the few runs of some thousand records set the time of
// the whole call (measured: 14 ms of 14.2 at 10^6 records, profiles/group_reduce.txt).  For those the wave gathers 64
// records per column at once and every lane steps through them out of registers: same order, same operations, same bits.
//
// Results are written with plain stores by the lane that owns the group, nothing is accumulated with atomics, and no
// lane waits for another: the same bits from run to run.  The status words are the one exception in form, not in
// value: integer counts, added only where the input is in error.
#include "tf_common.h"
#include "tf_prim.h"
#include <math.h>

struct GrOp { const void *f, *w, *aux; void *out; int op, f_dtype, w_dtype, aux_dtype; };
struct GrArgs { GrOp o[TF_GROUP_MAX_OPS]; int n; };

template <typename I>
__global__ void __launch_bounds__(256)
k_gr_rank(const I *__restrict__ ids, int64_t N, const I *__restrict__ coord, int32_t G, int32_t *__restrict__ rank,
          int32_t *__restrict__ pos)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const I id = ids[i];
    int32_t lo = 0, hi = G;                                       // first slot of coord that is >= id
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (coord[mid] < id) lo = mid + 1; else hi = mid;
    }
    rank[i] = lo < G && coord[lo] == id ? lo : G;
    pos[i] = (int32_t)i;
}

// slot i opens the runs of every rank in (key[i - 1], key[i]]; slot N closes the table: every rank above the last key
// starts at N.  Ranks skipped on the way are groups without a record.  status[0] = orphan records, status[1] = such groups
__global__ void __launch_bounds__(256)
k_gr_bounds(const int32_t *__restrict__ key, int64_t N, int32_t G, int32_t *__restrict__ start, unsigned long long *status)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > N) return;
    const int32_t prev = i > 0 ? key[i - 1] : -1;
    const int32_t cur = i < N ? key[i] : G + 1;
    if (cur == prev) return;
    for (int64_t r = (int64_t)prev + 1; r <= cur; r++) start[r] = (int32_t)i;
    const int64_t top = cur < G ? cur : G;                        // ranks prev + 1 .. top - 1 are groups, and empty
    if (top - 1 > prev) atomicAdd(&status[1], (unsigned long long)(top - 1 - prev));
    if (cur == G) atomicAdd(&status[0], (unsigned long long)(N - i));
}

__device__ __forceinline__ double gr_ld(const void *c, int dtype, int64_t p)
{
    if (dtype == TF_F32) return (double)((const float *)c)[p];
    if (dtype == TF_F64) return ((const double *)c)[p];
    return (double)((const int64_t *)c)[p];
}
__device__ __forceinline__ int64_t gr_ldi(const void *c, int64_t p) { return ((const int64_t *)c)[p]; }
__device__ __forceinline__ bool gr_finite(double x) { return x - x == 0.0; }

// How a walk reads the run.  Column slot k: 0 = f, 1 = w, 2 = aux; i is a slot of the sorted table.
// GrLaneRun: the lane owns the group and gathers record by record -- one dependent pair of loads per step.
struct GrLaneRun {
    const int32_t *perm;
    __device__ __forceinline__ void reset() {}
    __device__ __forceinline__ double ld(int, const void *c, int dtype, int32_t i) { return gr_ld(c, dtype, perm[i]); }
    __device__ __forceinline__ int64_t ldi(int, const void *c, int32_t i) { return gr_ldi(c, perm[i]); }
};
// GrWaveRun: the whole wavefront walks ONE group, every lane the same walk with the same values.  Per column slot the
// wave keeps a window of 64 consecutive records, one per lane, gathered in one go; a step reads its record out of the
// owning lane's register (v_readlane, the index is wave-uniform) and refills the window when the walk leaves it.  The
// order of the walk and every operation of it are those of the lane form, so the bits are too; what changes is that a
// long run pays one memory latency per 64 records and column instead of one per record.
struct GrWaveRun {
    const int32_t *perm; int32_t e; int lane;
    int32_t base[3]; uint64_t bits[3];
    template <typename Load> __device__ __forceinline__ void move(int k, int32_t i, Load load)
    {
        base[k] = i;
        const int32_t j = i + lane;
        bits[k] = j < e ? load(perm[j]) : 0;
    }
    __device__ __forceinline__ void reset() { base[0] = base[1] = base[2] = -0x40000000; }
    __device__ __forceinline__ uint64_t at(int k, int32_t i) const
    {
        const int l = __builtin_amdgcn_readfirstlane(i - base[k]);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bits[k], l);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(bits[k] >> 32), l);
        return ((uint64_t)hi << 32) | lo;
    }
    __device__ __forceinline__ bool outside(int k, int32_t i) const { return i < base[k] || i >= base[k] + 64; }
    __device__ __forceinline__ double ld(int k, const void *c, int dtype, int32_t i)
    {
        if (outside(k, i)) move(k, i, [&](int32_t p) { return (uint64_t)__double_as_longlong(gr_ld(c, dtype, p)); });
        return __longlong_as_double((long long)at(k, i));
    }
    __device__ __forceinline__ int64_t ldi(int k, const void *c, int32_t i)
    {
        if (outside(k, i)) move(k, i, [&](int32_t p) { return (uint64_t)gr_ldi(c, p); });
        return (int64_t)at(k, i);
    }
};

// the extreme of a run in record order: first occurrence wins; with SKIP NaN keys are passed over (xarray's idxmin /
// nanmin), without it the first NaN wins (np.argmin).  Returns the run slot, -1 when nothing qualified
template <bool MAX, bool SKIP, typename T, typename L>
__device__ __forceinline__ int32_t gr_extreme(int32_t b, int32_t e, L load, T *value)
{
    int32_t best = -1; T bx = T(0);
    for (int32_t i = b; i < e; i++) {
        const T x = load(i);
        if (x != x) {
            if (SKIP) continue;
            if (best < 0 || bx == bx) { best = i; bx = x; }
            continue;
        }
        if (best < 0 || (bx == bx && (MAX ? x > bx : x < bx))) { best = i; bx = x; }
    }
    *value = bx;
    return best;
}

// np.gradient(f, t, edge_order=1) of a run, reduced on the fly to its NaN-skipping minimum and the slot of it.  NumPy
// takes the constant-spacing form when every difference of t equals the first, and its a, b, c form otherwise; both
// are evaluated as NumPy writes them (no contraction: the library is built with -ffp-contract=off)
template <typename R>
__device__ __forceinline__ int32_t gr_gradient_min(const GrOp &o, R &run, int32_t b, int32_t e, double *value)
{
    *value = NAN;
    if (e - b < 2) return -1;
    const double t0 = run.ld(2, o.aux, o.aux_dtype, b);
    const double dx0 = run.ld(2, o.aux, o.aux_dtype, b + 1) - t0;
    bool uniform = true;
    double tp = t0;
    for (int32_t i = b + 1; i < e; i++) {                         // walk 1: is the spacing constant?
        const double tc = run.ld(2, o.aux, o.aux_dtype, i);
        if (!(tc - tp == dx0)) uniform = false;
        tp = tc;
    }
    int32_t best = -1; double bg = NAN;
    double fp = 0.0;                                              // record i - 1 (with tp)
    double fc = run.ld(0, o.f, o.f_dtype, b), tc = t0;            // record i
    for (int32_t i = b; i < e; i++) {                             // walk 2
        double fn = 0.0, tn = 0.0;
        if (i + 1 < e) { fn = run.ld(0, o.f, o.f_dtype, i + 1); tn = run.ld(2, o.aux, o.aux_dtype, i + 1); }
        double g;
        if (i == b) g = (fn - fc) / (uniform ? dx0 : tn - tc);
        else if (i + 1 == e) g = (fc - fp) / (uniform ? dx0 : tc - tp);
        else if (uniform) g = (fn - fp) / (2.0 * dx0);
        else {
            const double dx1 = tc - tp, dx2 = tn - tc;
            const double ca = -(dx2) / (dx1 * (dx1 + dx2));
            const double cb = (dx2 - dx1) / (dx1 * dx2);
            const double cc = dx1 / (dx2 * (dx1 + dx2));
            g = ca * fp + cb * fc + cc * fn;
        }
        if (g == g && (best < 0 || g < bg)) { best = i; bg = g; }
        fp = fc; tp = tc; fc = fn; tc = tn;
    }
    *value = bg;
    return best;
}

template <typename R>
__device__ __forceinline__ void gr_eval(const GrOp &o, R &run, const int32_t *__restrict__ perm, int32_t b, int32_t e, int64_t g)
{
    double *od = (double *)o.out + g;
    int64_t *oi = (int64_t *)o.out + g;
    const bool ints = o.f_dtype == TF_I64;
    run.reset();
    auto F = [&](int32_t i) { return run.ld(0, o.f, o.f_dtype, i); };
    auto K = [&](int32_t i) { return run.ldi(0, o.f, i); };
    auto W = [&](int32_t i) { return run.ld(1, o.w, o.w_dtype, i); };
    auto A = [&](int32_t i) { return run.ld(2, o.aux, o.aux_dtype, i); };
    switch (o.op) {
    case TF_GROUP_COUNT: *oi = e - b; break;
    case TF_GROUP_SUM: case TF_GROUP_MEAN: {
        double s = 0.0; int64_t c = 0;
        for (int32_t i = b; i < e; i++) { const double x = F(i); if (x == x) { s += x; c++; } }
        *od = o.op == TF_GROUP_SUM ? s : c ? s / (double)c : NAN;
    } break;
    case TF_GROUP_MIN: case TF_GROUP_MAX: case TF_GROUP_PICK_ARGMIN: case TF_GROUP_PICK_ARGMAX:
    case TF_GROUP_PICK_IDXMIN: case TF_GROUP_PICK_IDXMAX: {
        const bool mx = o.op == TF_GROUP_MAX || o.op == TF_GROUP_PICK_ARGMAX || o.op == TF_GROUP_PICK_IDXMAX;
        const bool skip = o.op != TF_GROUP_PICK_ARGMIN && o.op != TF_GROUP_PICK_ARGMAX;
        const bool value = o.op == TF_GROUP_MIN || o.op == TF_GROUP_MAX;
        int32_t at;
        if (ints) {
            int64_t v = 0;
            at = mx ? gr_extreme<true, true>(b, e, K, &v) : gr_extreme<false, true>(b, e, K, &v);
            if (value) { *oi = at < 0 ? 0 : v; break; }
        } else {
            double v = 0.0;
            at = mx ? (skip ? gr_extreme<true, true>(b, e, F, &v) : gr_extreme<true, false>(b, e, F, &v))
                    : (skip ? gr_extreme<false, true>(b, e, F, &v) : gr_extreme<false, false>(b, e, F, &v));
            if (value) { *od = at < 0 ? NAN : v; break; }
        }
        *oi = at < 0 ? -1 : perm[at];
    } break;
    case TF_GROUP_WEIGHTED_AVERAGE: {
        double sfw = 0.0, sw = 0.0;
        for (int32_t i = b; i < e; i++) { const double w = W(i); sfw += F(i) * w; sw += w; }
        *od = sw == 0.0 ? NAN : sfw / sw;
    } break;
    case TF_GROUP_COMBINED_MEAN: case TF_GROUP_COMBINED_STD: {
        // COMBINED_STD: f = the steps' std, aux = the steps' mean; COMBINED_MEAN: f = the steps' mean
        const bool mean_is_f = o.op == TF_GROUP_COMBINED_MEAN;
        double sma = 0.0, sa = 0.0; bool any = false;
        for (int32_t i = b; i < e; i++) {
            const double m = mean_is_f ? F(i) : A(i), a = W(i);
            if (gr_finite(m) && gr_finite(a)) { sma += m * a; sa += a; any = true; }
        }
        const double cm = any ? sma / sa : NAN;
        if (mean_is_f) { *od = cm; break; }
        double sas = 0.0, sad = 0.0; sa = 0.0; any = false;
        for (int32_t i = b; i < e; i++) {                         // the second walk of the same run
            const double s = F(i), m = A(i), a = W(i);
            if (gr_finite(s) && gr_finite(m) && gr_finite(a)) {
                const double d = m - cm;
                sas += a * s; sad += a * (d * d); sa += a; any = true;
            }
        }
        *od = any ? sqrt((sas + sad) / sa) : NAN;
    } break;
    case TF_GROUP_AVERAGE_UNCERTAINTY: {
        double s2 = 0.0, sw = 0.0;
        for (int32_t i = b; i < e; i++) { const double w = W(i), x = F(i); s2 += (w * w) * (x * x); sw += w; }
        *od = e > b && sw > 0.0 ? sqrt(s2) / sw : NAN;
    } break;
    case TF_GROUP_FIRST_MINUS_LAST: case TF_GROUP_LAST_MINUS_FIRST: {
        const bool fl = o.op == TF_GROUP_FIRST_MINUS_LAST;
        if (e == b) { if (ints) *oi = 0; else *od = NAN; break; }
        if (ints) { const int64_t x0 = K(b), x1 = K(e - 1); *oi = fl ? x0 - x1 : x1 - x0; }
        else { const double x0 = F(b), x1 = F(e - 1); *od = fl ? x0 - x1 : x1 - x0; }
    } break;
    case TF_GROUP_MAX_DIFF: {
        if (ints) {
            int64_t m = 0, xp = 0;
            for (int32_t i = b; i < e; i++) {
                const int64_t x = K(i);
                if (i > b && (i == b + 1 || x - xp > m)) m = x - xp;
                xp = x;
            }
            *oi = m;
        } else {
            double m = 0.0, xp = 0.0; bool nan = false;
            for (int32_t i = b; i < e; i++) {
                const double x = F(i);
                if (i > b) {
                    const double d = x - xp;
                    if (d != d) nan = true; else if (i == b + 1 || d > m) m = d;
                }
                xp = x;
            }
            *od = nan ? NAN : m;
        }
    } break;
    case TF_GROUP_ANY_NAN: {
        int64_t any = 0;
        for (int32_t i = b; i < e; i++) { const double x = F(i); if (x != x) any = 1; }
        *oi = any;
    } break;
    case TF_GROUP_GRADIENT_MIN: case TF_GROUP_GRADIENT_PICK_IDXMIN: {
        double v;
        const int32_t at = gr_gradient_min(o, run, b, e, &v);
        if (o.op == TF_GROUP_GRADIENT_MIN) *od = v; else *oi = at < 0 ? -1 : perm[at];
    } break;
    }
}

// Split by run length.  A lane owns a group and walks it alone while the run is shorter than a wavefront (the common
// case: about ten records).  Runs of GR_WAVE_RUN records and more are left to the second half: the wave goes through its
// 64 groups' long runs one after the other, all lanes on the same run (GrWaveRun).  No lane leaves early -- the window
// reads registers of every lane -- so lanes past G carry an empty run.
#define GR_WAVE_RUN 64
__global__ void __launch_bounds__(256)
k_gr_walk(const int32_t *__restrict__ perm, const int32_t *__restrict__ start, int64_t G, GrArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool mine = g < G;
    const int32_t b = mine ? start[g] : 0, e = mine ? start[g + 1] : 0;
    const bool is_long = e - b >= GR_WAVE_RUN;
    if (mine && !is_long) {
        GrLaneRun run{perm};
        for (int k = 0; k < a.n; k++) gr_eval(a.o[k], run, perm, b, e, g);
    }
    uint64_t todo = __ballot(is_long);
    const int lane = (int)(threadIdx.x & 63);
    const int64_t g0 = g - lane;                                  // the wave's first group
    while (todo) {
        const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1);
        todo &= todo - 1;
        const int64_t gw = g0 + src;
        const int32_t wb = __builtin_amdgcn_readfirstlane(start[gw]), we = __builtin_amdgcn_readfirstlane(start[gw + 1]);
        GrWaveRun run{perm, we, lane};
        for (int k = 0; k < a.n; k++) gr_eval(a.o[k], run, perm, wb, we, gw);
    }
}

static int gr_sort_bits(int64_t G)
{
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) <= G) bits++;         // ranks run 0 .. G
    return bits;
}

static hipError_t gr_sort_bytes(int64_t N, int64_t G, size_t *bytes)
{
    *bytes = 0;
    return tf_sort_pairs_bits(nullptr, *bytes, (const int32_t *)nullptr, (int32_t *)nullptr, (const int32_t *)nullptr,
                              (int32_t *)nullptr, (size_t)N, 0, gr_sort_bits(G));
}

static bool gr_sizes_ok(int64_t N, int64_t G) { return N >= 0 && G >= 0 && N < 0x7fffffffll && G < 0x7ffffffell; }

extern "C" size_t tf_group_reduce_workspace_bytes(int64_t N, int64_t G)
{
    if (!gr_sizes_ok(N, G)) return 0;
    size_t sort = 0;
    if (N > 0 && gr_sort_bytes(N, G, &sort) != hipSuccess) return 0;
    return 4 * (tf_align_up((size_t)N * 4, 256) + 256) + tf_align_up((size_t)(G + 2) * 4, 256) + 256 + tf_align_up(sort, 256) + 256;
}

static bool gr_float(int d) { return d == TF_F32 || d == TF_F64; }
static bool gr_column(int d) { return gr_float(d) || d == TF_I64; }

extern "C" int tf_group_reduce(const void *ids, int id_dtype, int64_t N, const void *coord, int64_t G, const tf_group_op *ops,
                               int n_ops, uint64_t *status, void *workspace, size_t workspace_bytes, void *stream)
{
    TF_REQUIRE(gr_sizes_ok(N, G), "tf_group_reduce: N and G must be in [0, 2^31 - 2)");
    TF_REQUIRE(id_dtype == TF_I32 || id_dtype == TF_I64, "tf_group_reduce: ids are TF_I32 or TF_I64");
    TF_REQUIRE((ids || N == 0) && (coord || G == 0) && status, "tf_group_reduce: null pointer");
    TF_REQUIRE(n_ops >= 0 && n_ops <= TF_GROUP_MAX_OPS, "tf_group_reduce: 0 to 16 operations");
    TF_REQUIRE(ops || n_ops == 0, "tf_group_reduce: null operation table");
    GrArgs a;
    a.n = n_ops;
    for (int k = 0; k < TF_GROUP_MAX_OPS; k++) a.o[k] = GrOp{nullptr, nullptr, nullptr, nullptr, TF_GROUP_COUNT, TF_F64, TF_F64, TF_F64};
    for (int k = 0; k < n_ops; k++) {
        const tf_group_op &q = ops[k];
        TF_REQUIRE(q.op >= TF_GROUP_COUNT && q.op <= TF_GROUP_GRADIENT_PICK_IDXMIN, "tf_group_reduce: unknown operation");
        TF_REQUIRE(q.out || G == 0, "tf_group_reduce: an operation without output");
        const bool takes_int = q.op == TF_GROUP_MIN || q.op == TF_GROUP_MAX || (q.op >= TF_GROUP_PICK_ARGMIN && q.op <= TF_GROUP_PICK_IDXMAX) ||
                               q.op == TF_GROUP_FIRST_MINUS_LAST || q.op == TF_GROUP_LAST_MINUS_FIRST || q.op == TF_GROUP_MAX_DIFF;
        const bool weighted = q.op == TF_GROUP_WEIGHTED_AVERAGE || q.op == TF_GROUP_COMBINED_MEAN || q.op == TF_GROUP_COMBINED_STD ||
                              q.op == TF_GROUP_AVERAGE_UNCERTAINTY;
        const bool third = q.op == TF_GROUP_COMBINED_STD || q.op == TF_GROUP_GRADIENT_MIN || q.op == TF_GROUP_GRADIENT_PICK_IDXMIN;
        if (q.op != TF_GROUP_COUNT) {
            TF_REQUIRE(q.f || N == 0, "tf_group_reduce: an operation without its column");
            TF_REQUIRE(takes_int ? gr_column(q.f_dtype) : gr_float(q.f_dtype), "tf_group_reduce: column dtype not taken by the operation");
        }
        if (weighted) {
            TF_REQUIRE(q.w || N == 0, "tf_group_reduce: a weighted operation without weights");
            TF_REQUIRE(gr_float(q.w_dtype), "tf_group_reduce: weights are TF_F32 or TF_F64");
        }
        if (third) {
            TF_REQUIRE(q.aux || N == 0, "tf_group_reduce: an operation without its third column");
            TF_REQUIRE(q.op == TF_GROUP_COMBINED_STD ? gr_float(q.aux_dtype) : gr_column(q.aux_dtype),
                       "tf_group_reduce: third column dtype not taken by the operation");
        }
        a.o[k] = GrOp{q.f, q.w, q.aux, q.out, q.op, q.f_dtype, q.w_dtype, q.aux_dtype};
    }
    size_t sort_bytes = 0;
    if (N > 0) TF_CHECK_HIP(gr_sort_bytes(N, G, &sort_bytes));
    TfArena arena(workspace, workspace_bytes);
    int32_t *rank = arena.take<int32_t>((size_t)N + 1), *pos = arena.take<int32_t>((size_t)N + 1);
    int32_t *key = arena.take<int32_t>((size_t)N + 1), *perm = arena.take<int32_t>((size_t)N + 1);
    int32_t *start = arena.take<int32_t>((size_t)G + 2);
    void *tmp = arena.take<char>(sort_bytes + 1);
    if (!arena.ok()) { tf_set_error("tf_group_reduce: workspace too small (%zu bytes given)", workspace_bytes); return TF_ENOMEM; }

    hipStream_t s = (hipStream_t)stream;
    TF_CHECK_HIP(hipMemsetAsync(status, 0, 2 * sizeof(uint64_t), s));
    if (N > 0) {
        const dim3 grid((unsigned)((N + 255) / 256));
        if (id_dtype == TF_I32)
            hipLaunchKernelGGL(k_gr_rank<int32_t>, grid, dim3(256), 0, s, (const int32_t *)ids, N, (const int32_t *)coord, (int32_t)G, rank, pos);
        else
            hipLaunchKernelGGL(k_gr_rank<int64_t>, grid, dim3(256), 0, s, (const int64_t *)ids, N, (const int64_t *)coord, (int32_t)G, rank, pos);
        TF_CHECK_LAUNCH();
        TF_CHECK_HIP(tf_sort_pairs_bits(tmp, sort_bytes, rank, key, pos, perm, (size_t)N, 0, gr_sort_bits(G), s));
    }
    hipLaunchKernelGGL(k_gr_bounds, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, s, key, N, (int32_t)G, start,
                       (unsigned long long *)status);
    TF_CHECK_LAUNCH();
    if (G == 0 || n_ops == 0) return TF_OK;
    hipLaunchKernelGGL(k_gr_walk, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s, perm, start, G, a);
    TF_CHECK_LAUNCH();
    return TF_OK;
}
