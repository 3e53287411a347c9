// The steps of the exact radix select that norm_kernels.h (quantile edges of `uniform`, many ranks of one frame pair) and
// field_stats.hip (the two middle ranks of every slice of a field) share.  Order statistics are found on the
// order-preserving integer key of a value, most significant digit first, in passes of RS_DIGIT bits: every wanted rank
// carries the key prefix found so far and its residual rank among the keys with that prefix; a pass counts the next digit
// of the keys under each distinct prefix (integer atomics: the counts do not depend on the order of arrival), turns the
// counts into running sums and reads each rank's digit off them.  What differs between the two users -- how many ranks
// there are, how a lane walks its data, how wide the counters are -- stays with them.
//
// As norm_kernels.h, the text compiles for the host (the host checks under tools/ supply the qualifiers).
#pragma once
#include <stdint.h>

#define RS_LANES 256                   // lanes of a workgroup that scans a histogram
#define RS_DIGIT 11                    // bits of a pass's digit (the last pass takes what is left)
#define RS_BINS (1 << RS_DIGIT)        // counters of one histogram

// ---- keys: a < b as values <=> key(a) < key(b) as unsigned integers (-0.0 sorts just below +0.0; NaN has no place) ------
__host__ __device__ inline unsigned rs_key(float v)
{
    union { float f; unsigned u; } c; c.f = v;
    return (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
}
__host__ __device__ inline float rs_unkey(unsigned k)
{
    union { float f; unsigned u; } c; c.u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return c.f;
}
__host__ __device__ inline unsigned long long rs_key(double v)
{
    union { double f; unsigned long long u; } c; c.f = v;
    return (c.u >> 63) ? ~c.u : (c.u | 0x8000000000000000ull);
}
__host__ __device__ inline double rs_unkey(unsigned long long k)
{
    union { double f; unsigned long long u; } c; c.u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return c.f;
}

// ---- the digit plan of a key of `key_bits` bits: 32 -> 11 + 11 + 10, 64 -> 5 x 11 + 9 -----------------------------------
__host__ __device__ inline int rs_passes(int key_bits) { return (key_bits + RS_DIGIT - 1) / RS_DIGIT; }
// bits below the prefix that the passes before `pass` have fixed (the whole key in pass 0)
__host__ __device__ inline int rs_prefix_shift(int key_bits, int pass) { return key_bits - RS_DIGIT * pass; }
__host__ __device__ inline int rs_digit_bits(int key_bits, int pass)
{
    const int left = rs_prefix_shift(key_bits, pass);
    return left < RS_DIGIT ? left : RS_DIGIT;
}

// ---- exclusive running sum of one histogram's RS_BINS counters, in place: lane t owns bins 8 t .. 8 t + 7 (two phases
// with a barrier between them, `part` holds RS_LANES counters in LDS)
template <typename C>
__host__ __device__ inline void rs_scan_sum(int tid, const C *h, C *part)
{
    C s = 0;
    for (int i = 0; i < RS_BINS / RS_LANES; i++) s += h[tid * (RS_BINS / RS_LANES) + i];
    part[tid] = s;
}
template <typename C>
__host__ __device__ inline void rs_scan_write(int tid, C *h, const C *part)
{
    C run = 0;
    for (int t = 0; t < tid; t++) run += part[t];
    for (int i = 0; i < RS_BINS / RS_LANES; i++) {
        C *p = h + tid * (RS_BINS / RS_LANES) + i;
        const C c = *p; *p = run; run += c;
    }
}

// the digit of residual rank r from a histogram's running sums: the last bin that starts at or below r (>= 0: cum[0] == 0)
template <typename C>
__host__ __device__ inline int rs_rank_bin(const C *cum, int bins, C r)
{
    int lo = 0, hi = bins;                                       // first bin whose start exceeds r
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cum[mid] <= r) lo = mid + 1; else hi = mid; }
    return lo - 1;
}
