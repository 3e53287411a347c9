// tf_relabel_merge: the second stage's pass over one window product (tobac_flow/linking.py:246-334
// relabel_cores_and_anvils + merge_previous_file + merge_next_file + combine_labels) in ONE read of each source and one write.
//
//   v = own[t, p]                        r = (v == 0) ? 0 : lut_own[v]
//   if r == 0 and prev_frame[t] >= 0:    u = prev[prev_frame[t], p];   r = (u == 0) ? 0 : lut_prev[u]
//   if r == 0 and next_frame[t] >= 0:    u = next[next_frame[t], p];   r = (u == 0) ? 0 : lut_next[u]
//   out[t, p] = r
//
// The reference relabels the window, relabels the shared frames of both neighbours into copies and fills the window's
// zeros from them with two np.where; composed from tf_apply_lut and torch that is index_select + three gathers + two
// selects, ~22 B per voxel for a 16-frame window sharing 4 frames on each side against ~10 B here.
//
// A streaming kernel: four voxels per lane, 16-byte nontemporal loads and stores of the volumes, the tables (a few hundred
// KB) gathered through L2.  The voxels are numbered flat over (t, p), so with hw % 4 != 0 a lane's four voxels can straddle
// two frames (or more: hw < 4) and the neighbour's frame starts unaligned: a lane takes the 16-byte neighbour load when its
// four voxels lie in one frame and the address allows it, element loads otherwise.  A neighbour is read only by lanes
// with a zero left (the branch is skipped by a wave without one).  The workgroup's first voxel is split into (frame, offset)
// once, in 64 bits and wave-uniform; a lane adds its own offset and divides in 32 bits.
//
// Ids that are consulted and lie outside their table give 0 and are counted in status[0]; frame-table entries >= the
// neighbour's frame count are treated as -1 and counted in status[1] (nothing is read through them).  One atomic per wave
// and word at most, and none when the wave counted nothing.
#include "tf_common.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct RmSide {
    const int32_t *vol;      // (n_frames, hw) or nullptr
    const int32_t *frame;    // [T]: the frame of `vol` under output frame t, or -1
    const int32_t *lut;      // [n_lut], entry 0 is 0
    int64_t n_frames;
    int n_lut;
    int aligned;             // vol is 16-byte aligned
};

__device__ __forceinline__ int32_t rm_lookup(int32_t v, const int32_t *__restrict__ lut, int n_lut, int &bad)
{
    if (v == 0) return 0;
    if ((uint32_t)v >= (uint32_t)n_lut) { bad++; return 0; }
    return lut[v];
}

// fills the zeros of r[0 .. cnt) from one neighbour; (t, p) is the frame and in-frame offset of r[0]
template <int PER>
__device__ __forceinline__ void rm_fill(const RmSide &side, int64_t t, uint32_t p, uint32_t hw, int cnt, int32_t (&r)[PER],
                                        int &bad, int &bad_frame)
{
    bool need = false;
#pragma unroll
    for (int k = 0; k < PER; k++) need |= k < cnt && r[k] == 0;
    if (!need) return;
    if constexpr (PER == 4) if (cnt == 4 && p + 3 < hw) {       // one frame under the four voxels
        const int32_t f = side.frame[t];
        if (f < 0) return;
        if (f >= side.n_frames) { bad_frame++; return; }
        const int64_t at = (int64_t)f * hw + p;
        int32_t u[4] = {0, 0, 0, 0};
        if (side.aligned && (at & 3) == 0) {
            const i32x4 q = __builtin_nontemporal_load((const i32x4 *)(side.vol + at));
            u[0] = q.x; u[1] = q.y; u[2] = q.z; u[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) if (r[k] == 0) u[k] = side.vol[at + k];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) if (r[k] == 0) r[k] = rm_lookup(u[k], side.lut, side.n_lut, bad);
        return;
    }
#pragma unroll
    for (int k = 0; k < PER; k++) {                              // a frame boundary under the lane, or the tail
        if (k < cnt && r[k] == 0) {
            const int32_t f = side.frame[t];
            if (f >= side.n_frames) bad_frame++;
            else if (f >= 0) r[k] = rm_lookup(side.vol[(int64_t)f * hw + p], side.lut, side.n_lut, bad);
        }
        if (++p == hw) { p = 0; t++; }
    }
}

__device__ __forceinline__ void rm_report(int count, unsigned long long *word)
{
    if (__any(count != 0)) {                                     // every lane of the wave is here: no early return above
        for (int off = 32; off; off >>= 1) count += __shfl_down(count, off);
        if ((threadIdx.x & 63) == 0) atomicAdd(word, (unsigned long long)count);
    }
}

// PER = 4: own and out are 16-byte aligned; PER = 1: any alignment
template <int PER>
__global__ void __launch_bounds__(256)
k_relabel_merge(const int32_t *own, const int32_t *__restrict__ lut_own, int n_own, RmSide prev, RmSide next, int64_t n,
                uint32_t hw, int32_t *out, unsigned long long *__restrict__ status)
{
    const int64_t block0 = (int64_t)blockIdx.x * (256 * PER);
    const int64_t t0 = block0 / hw;                              // wave-uniform
    const uint32_t q = (uint32_t)(block0 - t0 * hw) + threadIdx.x * PER;      // < hw + 1024 < 2^31
    const int64_t t = t0 + q / hw, i = block0 + threadIdx.x * PER;
    const uint32_t p = q % hw;
    int bad = 0, bad_frame = 0;
    if (i < n) {
        const int cnt = n - i < PER ? (int)(n - i) : PER;
        int32_t r[PER];
        const bool whole = PER == 4 && cnt == 4;                 // the 16-byte access; the last lane's tail goes by element
        if constexpr (PER == 4) {
            if (whole) {
                const i32x4 v = __builtin_nontemporal_load((const i32x4 *)(own + i));
                r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
            }
        }
        if (!whole) {
#pragma unroll
            for (int k = 0; k < PER; k++) r[k] = k < cnt ? own[i + k] : 0;
        }
#pragma unroll
        for (int k = 0; k < PER; k++) r[k] = rm_lookup(r[k], lut_own, n_own, bad);
        if (prev.vol) rm_fill<PER>(prev, t, p, hw, cnt, r, bad, bad_frame);
        if (next.vol) rm_fill<PER>(next, t, p, hw, cnt, r, bad, bad_frame);
        if constexpr (PER == 4) {
            if (whole) {
                i32x4 v; v.x = r[0]; v.y = r[1]; v.z = r[2]; v.w = r[3];
                __builtin_nontemporal_store(v, (i32x4 *)(out + i));
            }
        }
        if (!whole) {
#pragma unroll
            for (int k = 0; k < PER; k++) if (k < cnt) out[i + k] = r[k];
        }
    }
    rm_report(bad, status);
    rm_report(bad_frame, status + 1);
}

bool rm_overlaps(const int32_t *a, int64_t na, const int32_t *b, int64_t nb)
{
    return (uintptr_t)a < (uintptr_t)(b + nb) && (uintptr_t)b < (uintptr_t)(a + na);
}

}  // namespace

extern "C" int tf_relabel_merge(const int32_t *own, int64_t T, int64_t hw, const int32_t *lut_own, int n_own,
                                const int32_t *prev, int64_t T_prev, const int32_t *prev_frame, const int32_t *lut_prev, int n_prev,
                                const int32_t *next, int64_t T_next, const int32_t *next_frame, const int32_t *lut_next, int n_next,
                                int32_t *out, uint64_t *status, void *stream)
{
    TF_REQUIRE(own && lut_own && out && status && n_own > 0, "tf_relabel_merge: bad arguments");
    TF_REQUIRE(T > 0 && T < 65536 && hw > 0 && hw < ((int64_t)1 << 30), "tf_relabel_merge: bad shape");
    TF_REQUIRE(!prev || (prev_frame && lut_prev && T_prev > 0 && T_prev < 65536 && n_prev > 0), "tf_relabel_merge: bad previous product");
    TF_REQUIRE(!next || (next_frame && lut_next && T_next > 0 && T_next < 65536 && n_next > 0), "tf_relabel_merge: bad next product");
    TF_REQUIRE((uintptr_t)status % 8 == 0, "tf_relabel_merge: status must be 8-byte aligned");
    const int64_t n = T * hw;
    TF_REQUIRE(n <= ((int64_t)1 << 38), "tf_relabel_merge: more than 2^38 voxels");
    TF_REQUIRE(out == own || !rm_overlaps(out, n, own, n), "tf_relabel_merge: out must be own itself or apart from it");
    TF_REQUIRE(!prev || !rm_overlaps(out, n, prev, T_prev * hw), "tf_relabel_merge: out overlaps the previous product");
    TF_REQUIRE(!next || !rm_overlaps(out, n, next, T_next * hw), "tf_relabel_merge: out overlaps the next product");
    hipStream_t s = (hipStream_t)stream;
    TF_CHECK_HIP(hipMemsetAsync(status, 0, 2 * sizeof(uint64_t), s));
    const RmSide a = {prev, prev_frame, lut_prev, prev ? T_prev : 0, n_prev, prev && tf_vec4_ok({prev}, {})};
    const RmSide b = {next, next_frame, lut_next, next ? T_next : 0, n_next, next && tf_vec4_ok({next}, {})};
    unsigned long long *st = (unsigned long long *)status;
    if (tf_vec4_ok({own, out}, {}))
        hipLaunchKernelGGL(k_relabel_merge<4>, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, own, lut_own, n_own, a, b, n,
                           (uint32_t)hw, out, st);
    else
        hipLaunchKernelGGL(k_relabel_merge<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, own, lut_own, n_own, a, b, n,
                           (uint32_t)hw, out, st);
    TF_CHECK_LAUNCH();
    return TF_OK;
}
