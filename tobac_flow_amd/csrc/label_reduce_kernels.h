// Kernel bodies of label_reduce.hip (tf_label_reduce) and label_order.hip (tf_label_order).  Kept apart from the entry points so that the same
// text compiles for the host: tools/label_reduce_host_check.cpp supplies the vector types and the atomics and runs the
// bodies lane after lane under AddressSanitizer.  Nothing here touches the HIP runtime.
// The work layout and the walk over a lane's runs of equal labels are label_runs.h's (the raveled walker over an id span,
// lr_walk_span); what is here are the record, the three layouts of the field and, per pass, the visitor.
#pragma once
#include <stdint.h>
#include "label_runs.h"

// ---- the record --------------------------------------------------------------------------------------------------------
// LRD_REC 64-bit words = one 64-byte line per id of the span, id - id_lo indexes it:
//   0 voxels (int64)   1 voxels whose value is not NaN (int64)   2 voxels whose value is != 0, NaN among them (int64)
//   3 sum of the non-NaN values: double for float fields, int64 for integer and bool fields
//   4 key of the smallest non-NaN value (lr_key), LR_NONE where there is none   5 key of the largest, 0 where there is none
//   6 sum of (x - mean)^2 over the non-NaN values (double), pass 2 only   7 spare (0)
#define LRD_REC 8
#define LRD_VOLUME 0        // field (n,)
#define LRD_PLANE 1         // field (hw,): one plane that every frame shares
#define LRD_FRAME 2         // field (T,): one value per frame
#define LRD_WANT_VAR 1

__device__ inline void lrd_init_body(int64_t l, int64_t span, unsigned long long *rec)
{
    if (l >= span) return;
    unsigned long long *r = rec + LRD_REC * l;
#pragma unroll
    for (int k = 0; k < LRD_REC; k++) r[k] = k == 4 ? LR_NONE : 0ull;               // +0.0 and 0 share their bits
}

template <typename E> struct LrdSum { typedef long long type; };                     // integer and bool fields: exact
template <> struct LrdSum<float> { typedef double type; };
template <> struct LrdSum<double> { typedef double type; };

__device__ inline void lrd_add_sum(unsigned long long *slot, double s) { atomicAdd((double *)slot, s); }
__device__ inline void lrd_add_sum(unsigned long long *slot, long long s) { atomicAdd(slot, (unsigned long long)s); }   // two's complement

template <typename E> __host__ __device__ inline bool lrd_is_nan(E) { return false; }
template <> __host__ __device__ inline bool lrd_is_nan<float>(float x) { return x != x; }
template <> __host__ __device__ inline bool lrd_is_nan<double>(double x) { return x != x; }

// lr_key for every non-NaN double: +-inf keep their place at the ends (x + 0.0 leaves them alone)
__host__ __device__ inline double lrd_unkey(unsigned long long k)
{
    union { double d; unsigned long long u; } c;
    c.u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return c.d;
}

// the field values of voxels i .. i + m - 1 in one of the three layouts; vec_f: f is 16-byte aligned and, for a plane,
// hw % 4 == 0.  A frame value is f[(i + j) / hw]: one division per step, then the quotient moves up where a frame ends
// (four voxels can pass several frames where hw < 4).
template <typename E>
__host__ __device__ __forceinline__ void lrd_load_field(const E *__restrict__ f, int64_t i, int m, bool full, int64_t hw,
                                                        int layout, bool vec_f, E xv[LR_VEC])
{
    if (layout == LRD_FRAME) {
        int64_t q = i / hw, r = i - q * hw;
#pragma unroll
        for (int j = 0; j < LR_VEC; j++) {
            xv[j] = j < m ? f[q] : (E)0;
            if (++r == hw) { r = 0; q++; }
        }
        return;
    }
    lr_load_weights<E>(f, i, m, full, hw, layout == LRD_PLANE, vec_f, xv);
}

// ---- pass 1: slots 0 .. 5 ----------------------------------------------------------------------------------------------
template <typename E>
struct LrdPass1 {
    typedef typename LrdSum<E>::type S;
    const E *__restrict__ f;
    int64_t hw, lo; int layout; bool vec_f; unsigned long long *rec;
    uint32_t cnt = 0, nn = 0, nz = 0;                             // a lane holds 16 voxels
    S sum = 0;
    unsigned long long kmin = LR_NONE, kmax = 0;
    E xv[LR_VEC];

    __device__ __forceinline__ void load(int64_t i, int m, bool full) { lrd_load_field<E>(f, i, m, full, hw, layout, vec_f, xv); }
    __device__ __forceinline__ bool ends(int) const { return false; }
    __device__ __forceinline__ void open(int32_t, bool, int) { cnt = nn = nz = 0; sum = 0; kmin = LR_NONE; kmax = 0; }
    __device__ __forceinline__ void add(int64_t, int j)
    {
        const E x = xv[j];
        cnt++;
        nz += x != (E)0;                                          // NaN != 0
        if (lrd_is_nan<E>(x)) return;
        nn++;
        sum += (S)x;
        const unsigned long long k = lr_key((double)x);
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
    }
    __device__ __forceinline__ void close(int32_t cur)
    {
        if (!cnt) return;                                         // cur is in the span whenever cnt != 0
        unsigned long long *u = rec + LRD_REC * ((int64_t)cur - lo);
        atomicAdd(u, (unsigned long long)cnt);
        if (nz) atomicAdd(u + 2, (unsigned long long)nz);
        if (nn) {
            atomicAdd(u + 1, (unsigned long long)nn);
            if (sum != 0) lrd_add_sum(u + 3, sum);                // NaN != 0: inf - inf reaches the sum
            if (u[4] > kmin) atomicMin(u + 4, kmin);              // a stale read only costs a redundant atomic
            if (u[5] < kmax) atomicMax(u + 5, kmax);
        }
        cnt = 0;
    }
    __device__ __forceinline__ void last(int, int32_t cur) { close(cur); }
};

template <typename E>
__device__ inline void lrd_pass1_body(int64_t block, int tid, const int32_t *__restrict__ labels, const E *__restrict__ f,
                                      int64_t n, int64_t hw, int layout, bool vec, bool vec_f, int64_t lo, int64_t hi,
                                      int32_t none, unsigned long long *rec)
{
    LrdPass1<E> v{f, hw, lo, layout, vec_f, rec};
    lr_walk_span(block, tid, labels, n, vec, lo, hi, none, v);
}

// mean[l] = slot 3 / slot 1 (NaN where the id has no non-NaN voxel): one double division, NumPy's for an integer field
template <typename E>
__device__ inline void lrd_mean_body(int64_t l, int64_t span, const unsigned long long *__restrict__ rec, double *__restrict__ mean)
{
    if (l >= span) return;
    typedef typename LrdSum<E>::type S;
    const unsigned long long *r = rec + LRD_REC * l;
    union { unsigned long long u; S s; } c;
    c.u = r[3];
    mean[l] = r[1] ? (double)c.s / (double)r[1] : __builtin_nan("");
}

// ---- pass 2: slot 6, about the mean of pass 1 --------------------------------------------------------------------------
template <typename E>
struct LrdPass2 {
    const E *__restrict__ f;
    int64_t hw, lo; int layout; bool vec_f; const double *__restrict__ mean_of; unsigned long long *rec;
    bool open_ = false;
    double mean = 0, sv = 0;
    E xv[LR_VEC];

    __device__ __forceinline__ void load(int64_t i, int m, bool full) { lrd_load_field<E>(f, i, m, full, hw, layout, vec_f, xv); }
    __device__ __forceinline__ bool ends(int) const { return false; }
    __device__ __forceinline__ void open(int32_t l, bool in, int)
    {
        open_ = in; sv = 0;
        if (in) mean = mean_of[(int64_t)l - lo];                  // a finished kernel's writes
    }
    __device__ __forceinline__ void add(int64_t, int j)
    {
        const E x = xv[j];
        if (lrd_is_nan<E>(x)) return;
        const double d = (double)x - mean;
        sv += d * d;
    }
    __device__ __forceinline__ void close(int32_t cur)
    {
        if (!open_) return;
        if (sv != 0) atomicAdd((double *)(rec + LRD_REC * ((int64_t)cur - lo) + 6), sv);
        open_ = false;
    }
    __device__ __forceinline__ void last(int, int32_t cur) { close(cur); }
};

template <typename E>
__device__ inline void lrd_pass2_body(int64_t block, int tid, const int32_t *__restrict__ labels, const E *__restrict__ f,
                                      int64_t n, int64_t hw, int layout, bool vec, bool vec_f, int64_t lo, int64_t hi,
                                      int32_t none, const double *__restrict__ mean_of, unsigned long long *rec)
{
    LrdPass2<E> v{f, hw, lo, layout, vec_f, mean_of, rec};
    lr_walk_span(block, tid, labels, n, vec, lo, hi, none, v);
}

// ---- tf_label_order ----------------------------------------------------------------------------------------------------
// Order keys: 32 bits for uint8 / int32 / float32, 64 for float64; unsigned order = order of the values, -0.0 and +0.0
// share a key.
template <typename E> struct LroKey { typedef uint32_t type; };
template <> struct LroKey<double> { typedef unsigned long long type; };

__host__ __device__ inline uint32_t lro_key(uint8_t x) { return x; }
__host__ __device__ inline uint32_t lro_key(int32_t x) { return (uint32_t)x ^ 0x80000000u; }
__host__ __device__ inline uint32_t lro_key(float x)
{
    union { float f; uint32_t u; } c;
    c.f = x + 0.0f;
    return (c.u >> 31) ? ~c.u : (c.u | 0x80000000u);
}
__host__ __device__ inline unsigned long long lro_key(double x) { return lr_key(x); }

__host__ __device__ inline double lro_value(uint32_t k, uint8_t) { return (double)k; }
__host__ __device__ inline double lro_value(uint32_t k, int32_t) { return (double)(int32_t)(k ^ 0x80000000u); }
__host__ __device__ inline double lro_value(uint32_t k, float)
{
    union { float f; uint32_t u; } c;
    c.u = (k >> 31) ? (k & 0x7fffffffu) : ~k;
    return (double)c.f;
}
__host__ __device__ inline double lro_value(unsigned long long k, double) { return lrd_unkey(k); }

// count[l] = slot 1 of the record, for l < span; count[span] = 0 (its exclusive sum is the total)
__device__ inline void lro_counts_body(int64_t l, int64_t span, const unsigned long long *__restrict__ rec, uint32_t *__restrict__ count)
{
    if (l > span) return;
    const unsigned long long c = l < span ? rec[LRD_REC * l + 1] : 0ull;
    count[l] = c > 0xffffffffull ? 0xffffffffu : (uint32_t)c;
}

// offsets beyond the key buffers (records that do not belong to these operands) are brought back into them, so that
// neither the sort nor the pick is handed an address outside
__device__ inline void lro_clamp_body(int64_t l, int64_t span, uint32_t *offset, int64_t n_keys)
{
    if (l <= span && (int64_t)offset[l] > n_keys) offset[l] = (uint32_t)n_keys;
}

// every non-NaN voxel of the span puts its key at the next free place of its label's segment [offset[l], offset[l + 1]);
// a place beyond the segment or the buffer (records that do not belong to these operands) is not written
template <typename E>
struct LroScatter {
    typedef typename LroKey<E>::type K;
    const E *__restrict__ f;
    int64_t hw, lo; int layout; bool vec_f; const uint32_t *__restrict__ offset; uint32_t *cursor; K *keys; int64_t n_keys;
    int64_t at = 0;
    E xv[LR_VEC];

    __device__ __forceinline__ void load(int64_t i, int m, bool full) { lrd_load_field<E>(f, i, m, full, hw, layout, vec_f, xv); }
    __device__ __forceinline__ bool ends(int) const { return false; }
    __device__ __forceinline__ void open(int32_t l, bool, int) { at = (int64_t)l - lo; }
    __device__ __forceinline__ void add(int64_t, int j)
    {
        const E x = xv[j];
        if (lrd_is_nan<E>(x)) return;
        const uint32_t place = atomicAdd(cursor + at, 1u);
        if (place < offset[at + 1] && place < n_keys) keys[place] = lro_key(x);
    }
    __device__ __forceinline__ void close(int32_t) {}
    __device__ __forceinline__ void last(int, int32_t) {}
};

template <typename E>
__device__ inline void lro_scatter_body(int64_t block, int tid, const int32_t *__restrict__ labels, const E *__restrict__ f,
                                        int64_t n, int64_t hw, int layout, bool vec, bool vec_f, int64_t lo, int64_t hi,
                                        int32_t none, const uint32_t *__restrict__ offset, uint32_t *cursor,
                                        typename LroKey<E>::type *keys, int64_t n_keys)
{
    LroScatter<E> v{f, hw, lo, layout, vec_f, offset, cursor, keys, n_keys};
    lr_walk_span(block, tid, labels, n, vec, lo, hi, none, v);
}

// out[2 l], out[2 l + 1] = the two middle values of the label's sorted segment (equal for an odd count), NaN for none
template <typename E>
__device__ inline void lro_pick_body(int64_t l, int64_t span, const uint32_t *__restrict__ offset,
                                     const typename LroKey<E>::type *__restrict__ sorted, int64_t n_keys, double *__restrict__ out)
{
    if (l >= span) return;
    const uint32_t a = offset[l], c = offset[l + 1] - a;
    if (!c || (int64_t)a + c > n_keys) {                          // the latter: records that do not belong to these operands
        out[2 * l] = out[2 * l + 1] = __builtin_nan("");
        return;
    }
    out[2 * l] = lro_value(sorted[a + (c - 1) / 2], E());
    out[2 * l + 1] = lro_value(sorted[a + c / 2], E());
}

// ---- what both entry points ask of their operands (host) -------------------------------------------------------------
// returns null, or what is wrong; dtype and layout are the codes of include/tobac_flow_hip.h (TF_F32 0, TF_F64 1, TF_I32 2,
// TF_U8 3)
#define LRD_MAX_SPAN (1ll << 27)

struct LrdShape { int64_t n, span, blocks, id_blocks; int32_t none; bool vec, vec_f; };

inline const char *lrd_shape(const int32_t *labels, const void *field, int dtype, int layout, int64_t T, int64_t hw,
                             int64_t id_lo, int64_t id_hi, LrdShape *g)
{
    if (!labels || !field) return "null pointer";
    if (!(dtype >= 0 && dtype <= 3)) return "the field is uint8 (bool), int32, float32 or float64";
    if (!(layout == LRD_VOLUME || layout == LRD_PLANE || layout == LRD_FRAME)) return "the layout is 0 (volume), 1 (plane) or 2 (one value per frame)";
    if (!(T > 0 && hw > 0 && T <= 0x7fffffffffffffffll / hw)) return "bad shape";
    if (!(id_lo <= id_hi && id_lo > -0x80000000ll && id_hi <= 0x7fffffffll)) return "the span must lie within (INT32_MIN, INT32_MAX]";
    if (id_hi - id_lo >= LRD_MAX_SPAN) return "the span id_hi - id_lo must be below 2^27";
    g->n = T * hw; g->span = id_hi - id_lo + 1;
    g->blocks = (g->n + LR_BLOCK - 1) / LR_BLOCK; g->id_blocks = (g->span + 1 + 255) / 256;
    if (g->blocks > 0x7fffffffll) return "volume too large for one launch";
    g->none = (int32_t)(id_lo - 1);
    g->vec = lr_aligned16(labels);
    g->vec_f = lr_aligned16(field) && (layout != LRD_PLANE || hw % LR_VEC == 0);
    return nullptr;
}
