// Variational refinement of a dense flow field on gfx950.
//
// Replaces cv2.VariationalRefinement.create().calc(I0, I1, flow) as the reference issues it once per direction when
// vr_steps > 0 (/root/reference/tobac_flow/flow.py:359, 513-519), with OpenCV's defaults: fixedPointIterations 5,
// sorIterations 5, alpha 20, delta 5, gamma 10, omega 1.6 (internal zeta 0.1, epsilon 0.001) --
// modules/video/src/variational_refinement.cpp, restated from the published algorithm (SURVEY.md Appendix A.2;
// PARITY UNPINNED: no OpenCV in the build image, the reference holds no vectors for this stage).
//
//   k_vr_prepare   I1 warped by the flow (bilinear, coordinates quantised to 1/32 px, replicated border), the averaged
//                  image and Iz: one float2 plane A (8 B / px) -- the sources of every derivative
//   k_vr_system    on an LDS tile of A, W and dW: the first / second central differences of the averaged image and of Iz
//                  (Sobel ksize 1, replicated border: single subtractions at clamped neighbour coordinates), the
//                  smoothness weights of the current flow W + dW (forward differences, replicated border; each weight
//                  computed once per tile and shared with the right / lower neighbour through LDS) and
//                  the 2x2 system of every pixel: data term (robust colour- and gradient-constancy weights) plus the
//                  smoothness contributions of its four edges, accumulated in OpenCV's pass order (red before black,
//                  horizontal before vertical -- the order at a pixel depends on its colour)
//   k_vr_sor       one half sweep (one colour) of red-black SOR on dW
// Every float expression is evaluated as written (-ffp-contract=off, correctly rounded divide / sqrt), so the result
// is bit-identical to the oracle's C restatement (oracle/c/varref.c).
//
// HBM layout (planar, per flow direction): A = float2 {avg, Iz}, S = float4 {A11, A22, b1, b2}, A12 float, wt float,
// W float2 (the input flow), dW float2 and its ping-pong partner: 48 B of workspace per pixel.
#include "tf_common.h"

struct VrP { float alpha2, delta2, gamma2, omega, zeta2, eps2; };
// strides between the images of a batch (tf_varref_batch; all zero-cost for one image): frames in pixels, the caller's flow
// array in float2, the workspace planes in elements
struct VrB { int64_t img, flow, plane; };

__device__ __forceinline__ int vr_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

#define VR_TW 64
#define VR_TH 16

__global__ void __launch_bounds__(256)
k_vr_prepare(const uint8_t *__restrict__ I0, const uint8_t *__restrict__ I1, const float2 *__restrict__ flow,
             int H, int W, float2 *__restrict__ A, VrB bs)
{
    {   // image blockIdx.z of a batch (tf_varref_batch): the same tile code on that image's arrays
        const int64_t b = blockIdx.z;
        I0 += b * bs.img; I1 += b * bs.img; flow += b * bs.flow; A += b * bs.plane;
    }
    const int x0 = blockIdx.x * VR_TW, y0 = blockIdx.y * VR_TH;
    // warped / averaged image and Iz of the tile's pixels; the differences are formed where they are used (k_vr_system).
    // Three stages so that a thread's loads are in flight together: flow + I0 of all its positions, then the four I1
    // taps of all of them (their addresses need the flow), then the arithmetic and the stores.
    constexpr int NL = VR_TW * VR_TH / 256;
    float2 f[NL]; float i0[NL]; bool ok[NL]; int64_t p[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) {
        const int i = threadIdx.x + 256 * j, ly = i / VR_TW, lx = i - ly * VR_TW;
        const int x = x0 + lx, y = y0 + ly;
        ok[j] = x < W && y < H;
        p[j] = ok[j] ? (int64_t)y * W + x : 0;
        f[j] = flow[p[j]]; i0[j] = (float)I0[p[j]];
    }
    float v[NL][4], wgt[NL][4];
#pragma unroll
    for (int j = 0; j < NL; j++) {
        const int i = threadIdx.x + 256 * j, ly = i / VR_TW, lx = i - ly * VR_TW;
        const int x = x0 + lx, y = y0 + ly;
        const float mx = (float)x + f[j].x, my = (float)y + f[j].y;
        const int fx = tf_cvround(mx * 32.f), fy = tf_cvround(my * 32.f);
        const int sx = tf_sat_short(fx >> 5), sy = tf_sat_short(fy >> 5);
        const int ax = fx & 31, ay = fy & 31;
        const float tx1 = (float)ax * (1.f / 32.f), tx0 = 1.f - tx1, ty1 = (float)ay * (1.f / 32.f), ty0 = 1.f - ty1;
        wgt[j][0] = ty0 * tx0; wgt[j][1] = ty0 * tx1; wgt[j][2] = ty1 * tx0; wgt[j][3] = ty1 * tx1;
        const int xa = vr_clampi(sx, W - 1), xb = vr_clampi(sx + 1, W - 1), ya = vr_clampi(sy, H - 1), yb = vr_clampi(sy + 1, H - 1);
        v[j][0] = (float)I1[(int64_t)ya * W + xa]; v[j][1] = (float)I1[(int64_t)ya * W + xb];
        v[j][2] = (float)I1[(int64_t)yb * W + xa]; v[j][3] = (float)I1[(int64_t)yb * W + xb];
    }
#pragma unroll
    for (int j = 0; j < NL; j++) {
        if (!ok[j]) continue;
        const float warped = v[j][0] * wgt[j][0] + v[j][1] * wgt[j][1] + v[j][2] * wgt[j][2] + v[j][3] * wgt[j][3];
        A[p[j]] = make_float2((i0[j] + warped) * 0.5f, warped - i0[j]);
    }
}

// ---- correctly rounded division with the reciprocal work shared between numerators -----------------------------------
// `n / d` in IEEE arithmetic costs the GPU eleven instructions: two range scalings, v_rcp, one Newton step on the
// reciprocal, q = n r, two residual corrections (the last one the final, correctly rounding FMA) and a fix-up for
// special values.  The reciprocal and its Newton step depend on d alone; the scalings and the fix-up do nothing when n
// is 0 or 2^-100 < |n| < 2^96 |d| and the quotient is a normal number.  vr_div_shared performs exactly the remaining
// five operations and the fix-up (which also gives -0 / d its sign), so its result is the hardware division's bit for bit in that range.  It is used only where the
// range is guaranteed: the derivative values k_vr_system forms are exact multiples of 2^-11 of magnitude <= 1020 (sums
// and differences of uint8 values and of bilinear samples with 1/32-quantised weights, all exact in float), so a
// product of two of them is 0 or lies in [2^-22, 2^20], and the denominators lie in [zeta^2, 2^22].
// tf_selftest_shared_divide compares the two forms on random operands of that range (tests/test_gpu_parity.py).
struct VrRcp { float d, r; };
__device__ __forceinline__ VrRcp vr_rcp_refined(float d)
{
    float r = __builtin_amdgcn_rcpf(d);
    const float e = __fmaf_rn(-d, r, 1.f);
    r = __fmaf_rn(e, r, r);
    VrRcp k; k.d = d; k.r = r;
    return k;
}
__device__ __forceinline__ float vr_div_shared(float n, VrRcp k)
{
#ifdef VR_PLAIN_DIVIDE                 /* A/B build: the hardware division */
    return n / k.d;
#endif
    float q = n * k.r;
    float e = __fmaf_rn(-k.d, q, n);
    q = __fmaf_rn(e, k.r, q);
    e = __fmaf_rn(-k.d, q, n);
    return __builtin_amdgcn_div_fixupf(__fmaf_rn(e, k.r, q), k.d, n);     // the fix-up keeps the sign of a zero numerator
}

__global__ void __launch_bounds__(256)
k_vr_selftest_divide(unsigned long long seed, int64_t count, unsigned long long *__restrict__ mismatches)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    // splitmix64 -> operands shaped like the kernel's: products of two multiples of 2^-11 over a sum of squares + zeta^2
    auto next = [](unsigned long long &z) { z += 0x9e3779b97f4a7c15ull; unsigned long long x = z; x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
                                            x = (x ^ (x >> 27)) * 0x94d049bb133111ebull; return x ^ (x >> 31); };
    unsigned long long st = seed + 0x632be59bd9b4e019ull * (unsigned long long)i;
    float v[4];
    for (int k = 0; k < 4; k++) {
        const unsigned long long r = next(st);
        const int mag = (int)(r % 2088961u) - 1044480;                   // -1020 * 1024 .. 1020 * 1024, in units of 2^-11... / 2
        const int shift = (int)((r >> 40) % 12);                          // small values as often as large ones
        v[k] = (float)(mag >> shift) * (1.f / 2048.f);
    }
    const float d = v[0] * v[0] + v[1] * v[1] + 0.1f * 0.1f, n = v[2] * v[3];
    const float fast = vr_div_shared(n, vr_rcp_refined(d)), ieee = n / d;
    if (__float_as_uint(fast) != __float_as_uint(ieee)) atomicAdd(mismatches, 1ull);
}

// smoothness weight from the current flow at a pixel (c0), its right (cr) and its lower (cd) neighbour
// FAST (TF_VR_FAST_DIVIDE, opt-in): hardware reciprocal square root / reciprocal (1 ulp) and reciprocal-multiply instead
// of the correctly rounded `/` and sqrtf -- not bit-identical to OpenCV's arithmetic any more, within 1e-4 px of it
// (tests/test_gpu_parity.py).  The default (FAST = false) evaluates every expression as written.
template <bool FAST = false>
__device__ __forceinline__ float vr_weight(float2 c0, float2 cr, float2 cd, const VrP &P)
{
    const float ux = cr.x - c0.x, vx = cr.y - c0.y, uy = cd.x - c0.x, vy = cd.y - c0.y;
    const float q = ux * ux + vx * vx + uy * uy + vy * vy + P.eps2;
    return FAST ? P.alpha2 * __builtin_amdgcn_rsqf(q) : P.alpha2 / sqrtf(q);
}
template <bool FAST> __device__ __forceinline__ float vr_quot(float n, VrRcp k) { return FAST ? n * k.r : vr_div_shared(n, k); }
template <bool FAST> __device__ __forceinline__ float vr_over_sqrt(float a, float q) { return FAST ? a * __builtin_amdgcn_rsqf(q) : a / sqrtf(q); }

__device__ __forceinline__ float2 vr_add2(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }

// ---- the 2x2 system of every pixel, from the sources -------------------------------------------------------------------
// One 256-thread workgroup owns a VRS_TW x VRS_TH tile and stages in LDS, with replicated-border (clamped) coordinates:
//   s_a   A = {avg, Iz} over the tile + 2          s_w, s_d   W and dW over the tile + 1          (origin x0 - 2 in x for all)
// then, after a barrier, every smoothness weight of the tile + 1 up / left ONCE in full-exec passes (s_wt), and after a second
// barrier the systems: wave w owns the tile rows w and w + 4, lane l the pixel pair (2l, 2l + 1) of the row -- one red and one
// black pixel, whose colours are a per-wave constant, so both accumulation orders are straight-line code.  Rows and row clamps
// are scalars, column clamps per-thread constants; a tile whose columns all lie two pixels inside the image (XIN) has none.
// The seven difference planes are k_vr_prepare's former expressions on the staged values: first differences at clamped
// neighbour coordinates, second differences of first differences taken at the NEIGHBOUR's clamped neighbours.
#define VRS_TW 128
#define VRS_TH 8
#define VRS_AW (VRS_TW + 4)
#define VRS_AH (VRS_TH + 4)
#define VRS_FH (VRS_TH + 2)
#define VRS_WH (VRS_TH + 1)
static_assert(VRS_TW == 128 && VRS_TH == 8, "one wave per tile row, two rows per wave; the extra weight passes assume 8 rows");

struct VrsX { int c, l, r, ll, lr, rl, rr; };                      // LDS columns of a pixel, its clamped neighbours and theirs

template <bool XIN>
__device__ __forceinline__ VrsX vrs_columns(int x, int x0, int W)
{
    VrsX X;
    X.c = x - x0 + 2;
    if (XIN) { X.l = X.c - 1; X.r = X.c + 1; X.ll = X.c - 2; X.lr = X.c; X.rl = X.c; X.rr = X.c + 2; return X; }
    const int l = vr_clampi(x - 1, W - 1), r = vr_clampi(x + 1, W - 1), o = 2 - x0;
    X.l = l + o; X.r = r + o;
    X.ll = vr_clampi(l - 1, W - 1) + o; X.lr = vr_clampi(l + 1, W - 1) + o;
    X.rl = vr_clampi(r - 1, W - 1) + o; X.rr = vr_clampi(r + 1, W - 1) + o;
    return X;
}

struct VrsY { int c, u, d, uu, ud, du, dd; };                      // s_a row offsets (elements), the same scheme

// one pixel: fc = its flow-array offset (row * VRS_AW + column), red = its colour
template <bool FAST>
__device__ __forceinline__ void vrs_pixel(const float2 *s_a, const float2 *s_w, const float2 *s_d, const float *s_wt,
                                          const VrsX X, const VrsY Y, int fc, bool red, bool has_l, bool has_r, bool has_u, bool has_d,
                                          const VrP &P, float4 &So, float &A12o, float &wpo)
{
    const float2 aL = s_a[Y.c + X.l], aR = s_a[Y.c + X.r], aU = s_a[Y.u + X.c], aD = s_a[Y.d + X.c];
    const float Ix = aR.x - aL.x, Iy = aD.x - aU.x, Ixz = aR.y - aL.y, Iyz = aD.y - aU.y, Iz = s_a[Y.c + X.c].y;
    const float Ixx = (s_a[Y.c + X.rr].x - s_a[Y.c + X.rl].x) - (s_a[Y.c + X.lr].x - s_a[Y.c + X.ll].x);
    const float Ixy = (s_a[Y.d + X.r].x - s_a[Y.d + X.l].x) - (s_a[Y.u + X.r].x - s_a[Y.u + X.l].x);
    const float Iyy = (s_a[Y.dd + X.c].x - s_a[Y.du + X.c].x) - (s_a[Y.ud + X.c].x - s_a[Y.uu + X.c].x);
    // a missing neighbour reads the pixel itself (the value the replicated border stands for)
    const float2 w0 = s_w[fc], wr = s_w[fc + 1], wlf = s_w[fc - 1], wd = s_w[fc + VRS_AW], wuf = s_w[fc - VRS_AW], d = s_d[fc];
    const float wp = s_wt[fc];
    const float wl = has_l ? s_wt[fc - 1] : 0.f, wu = has_u ? s_wt[fc - VRS_AW] : 0.f;
    const float du = d.x, dv = d.y;
    // ComputeDataTerm.  The fifteen quotients whose numerator is a product of two derivative values share the
    // reciprocal work of their three denominators (vr_div_shared: bit-identical to `/` in their range, see there)
    float derivNorm = Ix * Ix + Iy * Iy + P.zeta2;
    const VrRcp k1 = vr_rcp_refined(derivNorm);
    const float Ik1z = Iz + Ix * du + Iy * dv;
    float weight = vr_over_sqrt<FAST>(P.delta2, (FAST ? Ik1z * Ik1z * k1.r : Ik1z * Ik1z / derivNorm) + P.eps2);
    float A11 = weight * vr_quot<FAST>(Ix * Ix, k1) + P.zeta2;
    float A12 = weight * vr_quot<FAST>(Ix * Iy, k1);
    float A22 = weight * vr_quot<FAST>(Iy * Iy, k1) + P.zeta2;
    float b1 = -weight * vr_quot<FAST>(Iz * Ix, k1);
    float b2 = -weight * vr_quot<FAST>(Iz * Iy, k1);
    derivNorm = Ixx * Ixx + Ixy * Ixy + P.zeta2;
    const float derivNorm2 = Iyy * Iyy + Ixy * Ixy + P.zeta2;
    const VrRcp k2 = vr_rcp_refined(derivNorm), k3 = vr_rcp_refined(derivNorm2);
    const float Ik1zx = Ixz + Ixx * du + Ixy * dv;
    const float Ik1zy = Iyz + Ixy * du + Iyy * dv;
    weight = vr_over_sqrt<FAST>(P.gamma2, (FAST ? Ik1zx * Ik1zx * k2.r + Ik1zy * Ik1zy * k3.r : Ik1zx * Ik1zx / derivNorm + Ik1zy * Ik1zy / derivNorm2) + P.eps2);
    A11 += weight * (vr_quot<FAST>(Ixx * Ixx, k2) + vr_quot<FAST>(Ixy * Ixy, k3));
    A12 += weight * (vr_quot<FAST>(Ixx * Ixy, k2) + vr_quot<FAST>(Ixy * Iyy, k3));
    A22 += weight * (vr_quot<FAST>(Ixy * Ixy, k2) + vr_quot<FAST>(Iyy * Iyy, k3));
    b1 += -weight * (vr_quot<FAST>(Ixx * Ixz, k2) + vr_quot<FAST>(Ixy * Iyz, k3));
    b2 += -weight * (vr_quot<FAST>(Ixy * Ixz, k2) + vr_quot<FAST>(Iyy * Iyz, k3));
    // smoothness: each edge (p, right) / (p, down) carries the weight of its upper-left end
    // own edge terms as the horizontal / vertical passes form them at p, neighbour edge terms as they form them at the
    // left / upper neighbour
    const float own_ux = wp * (wr.x - w0.x), own_vx = wp * (wr.y - w0.y);
    const float lft_ux = wl * (w0.x - wlf.x), lft_vx = wl * (w0.y - wlf.y);
    const float own_uy = wp * (wd.x - w0.x), own_vy = wp * (wd.y - w0.y);
    const float up_uy = wu * (w0.x - wuf.x), up_vy = wu * (w0.y - wuf.y);
    if (red) {                                                       // wave-uniform
        if (has_r) { b1 += own_ux; A11 += wp; b2 += own_vx; A22 += wp; }
        if (has_l) { b1 -= lft_ux; A11 += wl; b2 -= lft_vx; A22 += wl; }
        if (has_d) { b1 += own_uy; A11 += wp; b2 += own_vy; A22 += wp; }
        if (has_u) { b1 -= up_uy; A11 += wu; b2 -= up_vy; A22 += wu; }
    } else {
        if (has_l) { b1 -= lft_ux; A11 += wl; b2 -= lft_vx; A22 += wl; }
        if (has_r) { b1 += own_ux; A11 += wp; b2 += own_vx; A22 += wp; }
        if (has_u) { b1 -= up_uy; A11 += wu; b2 -= up_vy; A22 += wu; }
        if (has_d) { b1 += own_uy; A11 += wp; b2 += own_vy; A22 += wp; }
    }
    So = make_float4(A11, A22, b1, b2); A12o = A12; wpo = wp;
}

template <bool FAST, bool XIN>
__device__ __forceinline__ void vrs_rows(const float2 *s_a, const float2 *s_w, const float2 *s_d, const float *s_wt, int wv, int lane,
                                         int x0, int y0, int H, int W, const VrP &P, float4 *__restrict__ S, float *__restrict__ A12o,
                                         float *__restrict__ wt)
{
    const int x = x0 + 2 * lane;
    const VrsX Xa = vrs_columns<XIN>(x, x0, W), Xb = vrs_columns<XIN>(x + 1, x0, W);
    const bool in_a = XIN || x < W, in_b = XIN || x + 1 < W;
    const bool has_la = XIN || x > 0, has_ra = in_b, has_rb = XIN || x + 2 < W;
#pragma unroll
    for (int k = 0; k < VRS_TH / 4; k++) {
        const int r = wv + 4 * k, y = y0 + r;                        // scalars
        if (y >= H) continue;
        const int yu = vr_clampi(y - 1, H - 1), yd = vr_clampi(y + 1, H - 1), o = 2 - y0;
        VrsY Y;
        Y.c = (r + 2) * VRS_AW; Y.u = (yu + o) * VRS_AW; Y.d = (yd + o) * VRS_AW;
        Y.uu = (vr_clampi(yu - 1, H - 1) + o) * VRS_AW; Y.ud = (vr_clampi(yu + 1, H - 1) + o) * VRS_AW;
        Y.du = (vr_clampi(yd - 1, H - 1) + o) * VRS_AW; Y.dd = (vr_clampi(yd + 1, H - 1) + o) * VRS_AW;
        const bool has_u = y > 0, has_d = y + 1 < H, red_a = (r & 1) == 0;     // x0 and y0 are even
        const int fc = (r + 1) * VRS_AW + 2 * lane + 2;
        float4 Sa, Sb; float a12a, a12b, wpa, wpb;
        vrs_pixel<FAST>(s_a, s_w, s_d, s_wt, Xa, Y, fc, red_a, has_la, has_ra, has_u, has_d, P, Sa, a12a, wpa);
        vrs_pixel<FAST>(s_a, s_w, s_d, s_wt, Xb, Y, fc + 1, !red_a, true, has_rb, has_u, has_d, P, Sb, a12b, wpb);
        const int64_t j = (int64_t)y * W + x;
        if (in_a) { S[j] = Sa; A12o[j] = a12a; wt[j] = wpa; }
        if (in_b) { S[j + 1] = Sb; A12o[j + 1] = a12b; wt[j + 1] = wpb; }
    }
}

template <bool FAST = false>
__global__ void __launch_bounds__(256)
k_vr_system(const float2 *__restrict__ A, const float2 *__restrict__ Wf, const float2 *__restrict__ dW, int H, int W, VrP P,
            float4 *__restrict__ S, float *__restrict__ A12o, float *__restrict__ wt, VrB bs)
{
    __shared__ __align__(16) float2 s_a[VRS_AH * VRS_AW], s_w[VRS_FH * VRS_AW], s_d[VRS_FH * VRS_AW];
    __shared__ __align__(16) float s_wt[VRS_WH * VRS_AW];
    {
        const int64_t b = blockIdx.z;
        A += b * bs.plane; Wf += b * bs.flow; S += b * bs.plane; A12o += b * bs.plane; wt += b * bs.plane;
        if (dW) dW += b * bs.plane;
    }
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int x0 = blockIdx.x * VRS_TW, y0 = blockIdx.y * VRS_TH;
    const float2 z2 = make_float2(0.f, 0.f);
    // Stage 1: every load of the thread, then the LDS stores.  Wave w loads the rows w, w + 4, w + 8 of each array, a lane
    // the columns lane and lane + 64; the last four columns of all rows are one more load of wave 0 (A), 2 (W) and 3 (dW).
    {
        const int gx0 = vr_clampi(x0 - 2 + lane, W - 1), gx1 = vr_clampi(x0 + 62 + lane, W - 1);
        float2 ta[3][2], tw[3][2], td[3][2];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int r = wv + 4 * k;
            const float2 *row = A + (int64_t)vr_clampi(y0 - 2 + r, H - 1) * W;
            ta[k][0] = row[gx0]; ta[k][1] = row[gx1];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int r = wv + 4 * k;
            tw[k][0] = tw[k][1] = td[k][0] = td[k][1] = z2;
            if (r < VRS_FH) {
                const int64_t ro = (int64_t)vr_clampi(y0 - 1 + r, H - 1) * W;
                tw[k][0] = Wf[ro + gx0]; tw[k][1] = Wf[ro + gx1];
                if (dW) { td[k][0] = dW[ro + gx0]; td[k][1] = dW[ro + gx1]; }
            }
        }
        // tail columns 128 .. 131: lane -> row lane / 4, column 128 + lane % 4
        const int tr = lane >> 2, tc = 128 + (lane & 3), gxt = vr_clampi(x0 - 2 + tc, W - 1);
        float2 tt = z2;
        if (wv == 0) {
            if (tr < VRS_AH) tt = A[(int64_t)vr_clampi(y0 - 2 + tr, H - 1) * W + gxt];
        } else if (wv == 2) {
            if (tr < VRS_FH) tt = Wf[(int64_t)vr_clampi(y0 - 1 + tr, H - 1) * W + gxt];
        } else if (wv == 3) {
            if (tr < VRS_FH && dW) tt = dW[(int64_t)vr_clampi(y0 - 1 + tr, H - 1) * W + gxt];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int r = wv + 4 * k;
            s_a[r * VRS_AW + lane] = ta[k][0]; s_a[r * VRS_AW + 64 + lane] = ta[k][1];
            if (r < VRS_FH) {
                s_w[r * VRS_AW + lane] = tw[k][0]; s_w[r * VRS_AW + 64 + lane] = tw[k][1];
                s_d[r * VRS_AW + lane] = td[k][0]; s_d[r * VRS_AW + 64 + lane] = td[k][1];
            }
        }
        if (wv == 0) { if (tr < VRS_AH) s_a[tr * VRS_AW + tc] = tt; }
        else if (wv == 2) { if (tr < VRS_FH) s_w[tr * VRS_AW + tc] = tt; }
        else if (wv == 3) { if (tr < VRS_FH) s_d[tr * VRS_AW + tc] = tt; }
    }
    __syncthreads();
    // Stage 2: the weight of every pixel of the tile + 1 up / left, each once (vr_weight; the staged border is replicated, so
    // a missing right / lower neighbour is the pixel itself).  Flow-array rows 0 .. 8, columns 1 .. 129: four passes of
    // a wave over its rows w and w + 4 (columns 2 .. 129), and a fifth in which wave 1 takes column 1 of all rows and
    // waves 2 and 3 the two halves of row 8.
    {
        auto weight_at = [&](int o) {
            return vr_weight<FAST>(vr_add2(s_w[o], s_d[o]), vr_add2(s_w[o + 1], s_d[o + 1]), vr_add2(s_w[o + VRS_AW], s_d[o + VRS_AW]), P);
        };
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int o = (wv + 4 * (p >> 1)) * VRS_AW + 2 + 64 * (p & 1) + lane;
            s_wt[o] = weight_at(o);
        }
        if (wv == 1) {
            if (lane < VRS_WH) { const int o = lane * VRS_AW + 1; s_wt[o] = weight_at(o); }
        } else if (wv >= 2) {
            const int o = VRS_TH * VRS_AW + 2 + 64 * (wv - 2) + lane;
            s_wt[o] = weight_at(o);
        }
    }
    __syncthreads();
    // Stage 3: the systems
    if (x0 >= 2 && x0 + VRS_TW + 2 <= W)
        vrs_rows<FAST, true>(s_a, s_w, s_d, s_wt, wv, lane, x0, y0, H, W, P, S, A12o, wt);
    else
        vrs_rows<FAST, false>(s_a, s_w, s_d, s_wt, wv, lane, x0, y0, H, W, P, S, A12o, wt);
}

// one colour of one red-black SOR sweep: thread -> the pixel of that colour in its pixel pair
__global__ void __launch_bounds__(256)
k_vr_sor(const float4 *__restrict__ S, const float *__restrict__ A12, const float *__restrict__ wt, int H, int W, int colour,
         float omega, float2 *__restrict__ dW)
{
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int x = 2 * (blockIdx.x * 64 + (threadIdx.x & 63)) + ((y + colour) & 1);
    if (x >= W || y >= H) return;
    const int64_t j = (int64_t)y * W + x;
    const float2 z = make_float2(0.f, 0.f);
    const float wp = wt[j], wl = x > 0 ? wt[j - 1] : 0.f, wu = y > 0 ? wt[j - W] : 0.f;
    const float2 dl = x > 0 ? dW[j - 1] : z, dr = x + 1 < W ? dW[j + 1] : z, du_ = y > 0 ? dW[j - W] : z, dd = y + 1 < H ? dW[j + W] : z;
    const float4 s = S[j];
    const float a12 = A12[j];
    float2 d = dW[j];
    const float sigmaU = wl * dl.x + wp * dr.x + wu * du_.x + wp * dd.x;
    const float sigmaV = wl * dl.y + wp * dr.y + wu * du_.y + wp * dd.y;
    d.x += omega * ((sigmaU + s.z - d.y * a12) / s.x - d.x);
    d.y += omega * ((sigmaV + s.w - d.x * a12) / s.y - d.y);
    dW[j] = d;
}

// ---- all sorIterations red-black sweeps of one fixed-point iteration in ONE pass over HBM -------------------------
// A half sweep only reads the four neighbours of the other colour, so 2 * sorIterations half sweeps of a tile need a
// halo of 2 * sorIterations pixels and nothing else.  One 512-thread workgroup owns a 108 x 84 tile + VRT_HALO = a
// 128 x 104 region: wave w owns the rows w, w + 8, ... (13 of them), lane l the pixel pair (2l, 2l + 1) of each.  Every
// thread keeps the system (A11, A22, b1, b2, A12) and the weight of ITS pixels in registers for the whole kernel, sorted
// by COLOUR (which pixel of a pair is red depends on the row parity = the wave parity, a per-wave constant); only dW and
// the weights of the left / upper neighbours live in LDS (12 B / px, 156 KB), in OpenCV's own red-black split: the
// pixels of one colour of a row are contiguous, so a wave's neighbour reads are unit-stride, all LDS addresses are one
// per-wave base + compile-time offsets, and row activity is a scalar branch.  The outermost ring is never updated and
// invalid values creep inwards one pixel per half sweep -- they stop short of the tile; half sweep s therefore skips the
// rows closer than s to the region's edge (their values can no longer reach the tile).
// Same expressions in the same order as k_vr_sor: bit-identical results (tests compare the two paths).
// dW_in == nullptr stands for dW = 0 (first fixed-point iteration); Wadd != nullptr (last iteration) makes the kernel
// store W + dW, the refined flow, instead of dW -- dW_out may then be the flow array itself (this kernel never reads W
// except at the pixel a thread is about to write).
// Measured and not adopted: delaying the odd workgroups of the first round by half a tile's time, so that loads and sweeps
// of different CUs overlap instead of running in lockstep: 5.63 / 5.70 / 5.74 / 5.63 ms per refinement for 0 / 5 / 10 / 20 us;
// half-height tiles (128 x 52 regions, 78 KB of LDS) with TWO 4-wave workgroups per CU, so that one loads while the other
// sweeps, at the price of more halo (region / tile 1.93 instead of 1.47): profiles/round6_vr_sor_notes.txt.
// Measured alternatives (12 x 5424^2, ms per step for all 110 launches): 128 x 64 tile, thread -> pair q = t + 512 k
// (row and pair parity vary inside a wave: per-pixel index arithmetic, activity predicates and value selects between the
// two pixels of a pair), 256 VGPRs: 93.2; the same with 1024 threads / 7 pairs / 128 VGPRs and a small spill: 95.9.
// Round 3, measured and not adopted (packed float instructions, v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32: two operations
// per lane, 1.8 x the scalar float rate in isolation, tools/microbench/pk_rate.hip):
//  * the (u, v) components of a pixel as one register pair, the two sigma sums packed (8 instead of 16 instructions per
//    update; the own weight then has to come from LDS, or the register pairs spill): 5.36 instead of 5.46 ms for ONE
//    refinement on an idle GPU, but 299 instead of 269 ms of kernel time per 48-frame step inside bench.py, back to back
//    with the other stages (with the weight in registers and one spilled register: 338 ms) -- under sustained load the
//    packed form is the slower one;
//  * two ROWS of a thread per packed instruction, the six multiply-adds of the two rows' divisions packed as well (72
//    instead of 2 x 49 instructions per pair of updates on paper): transposes between the (u, v) layout in LDS and the
//    row-pair layout in registers, wait states between dependent packed operations and 20 spilled registers: 6.30 ms.
// What an update costs is its two sequential IEEE divisions (2 x 11 instructions, the reciprocal at quarter rate): v needs
// the new u, so they cannot be paired, and a per-pixel reciprocal kept across the ten half sweeps would need 52 more
// registers than the 229 the kernel has.
#define VRT_W 108
#define VRT_HALO 10
#define VRT_RW (VRT_W + 2 * VRT_HALO)
#define VRT_PW (VRT_RW / 2)
static_assert(VRT_PW == 64, "one lane per pixel pair of a region row");
#define VRT_H 84
#define VRT_RH (VRT_H + 2 * VRT_HALO)
#define VRT_THREADS 512
#define VRT_WAVES (VRT_THREADS / 64)
#define VRT_K (VRT_RH / VRT_WAVES)
#define VRT_LDS_BYTES (2 * VRT_RH * VRT_PW * 12)
static_assert(VRT_RH % VRT_WAVES == 0, "whole rows per wave");

template <bool FAST>
__global__ void __launch_bounds__(VRT_THREADS, 2)
k_vr_sor_tile(const float4 *__restrict__ S, const float *__restrict__ A12, const float *__restrict__ wt, int H, int W,
              int n_half, float omega, const float2 *__restrict__ dW_in, const float2 *Wadd, float2 *dW_out, VrB bs)
{
    extern __shared__ __align__(16) unsigned char vr_lds[];
    {
        const int64_t b = blockIdx.z;
        S += b * bs.plane; A12 += b * bs.plane; wt += b * bs.plane;
        if (dW_in) dW_in += b * bs.plane;
        // the last fixed-point iteration writes the refined flow into the caller's array (its stride), the others dW into a plane
        if (Wadd) { Wadd += b * bs.flow; dW_out += b * bs.flow; } else dW_out += b * bs.plane;
    }
    float2 *l_dw = (float2 *)vr_lds;                                   // [2][VRT_RH][VRT_PW]
    float *l_wt = (float *)(vr_lds + 2 * VRT_RH * VRT_PW * 8);         // [2][VRT_RH][VRT_PW]
    const int x0 = blockIdx.x * VRT_W - VRT_HALO, y0 = blockIdx.y * VRT_H - VRT_HALO;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), cp = threadIdx.x & 63;
    // [ci]: image colour (0 red, 1 black).  A pixel of image colour ci has local parity lp = (r + c) & 1 = ci ^ par0 and
    // sits in column 2 cp + e with e = (lp + r) & 1; r = wv + 8 k has the parity of wv
    const int par0 = (x0 + y0) & 1;
    int e_[2], own_[2];
    bool colact[2];
#pragma unroll
    for (int ci = 0; ci < 2; ci++) {
        const int lp = ci ^ par0;
        e_[ci] = (lp + wv) & 1;
        own_[ci] = (lp * VRT_RH + wv) * VRT_PW + cp;                   // + k * VRT_WAVES * VRT_PW
        const int c = 2 * cp + e_[ci], x = x0 + c;
        colact[ci] = c > 0 && c < VRT_RW - 1 && x >= 0 && x < W;
    }
    float a11[VRT_K][2], a22[VRT_K][2], b1[VRT_K][2], b2[VRT_K][2], a12[VRT_K][2], wp[VRT_K][2];
    // Load phase, ordered so that MANY loads are in flight per wave: an LDS store right behind its own load makes the
    // compiler wait for everything issued before it (the first version ran 26 dependent round trips per thread).
    // 1. dW of one colour at a time into temporaries, then into LDS; 2. all systems and weights straight into their
    // registers; 3. the weights into LDS.
#pragma unroll
    for (int ci = 0; ci < 2; ci++) {
        float2 t[VRT_K];
        const int x = x0 + 2 * cp + e_[ci];
#pragma unroll
        for (int k = 0; k < VRT_K; k++) {
            const int y = y0 + wv + k * VRT_WAVES;
            const bool in = x >= 0 && y >= 0 && x < W && y < H;
            t[k] = make_float2(0.f, 0.f);
            if (dW_in) {                                       // uniform; nullptr = the first iteration's dW = 0
                const float2 v = dW_in[in ? (int64_t)y * W + x : 0];
                if (in) t[k] = v;
            }
        }
#pragma unroll
        for (int k = 0; k < VRT_K; k++) l_dw[own_[ci] + k * VRT_WAVES * VRT_PW] = t[k];
    }
#pragma unroll
    for (int k = 0; k < VRT_K; k++) {
        const int y = y0 + wv + k * VRT_WAVES;
#pragma unroll
        for (int ci = 0; ci < 2; ci++) {
            const int x = x0 + 2 * cp + e_[ci];
            const bool in = x >= 0 && y >= 0 && x < W && y < H;
            const int64_t p = in ? (int64_t)y * W + x : 0;
            const float4 sv = S[p];
            const float av = A12[p], wv_ = wt[p];
            a11[k][ci] = in ? sv.x : 1.f; a22[k][ci] = in ? sv.y : 1.f; b1[k][ci] = in ? sv.z : 0.f; b2[k][ci] = in ? sv.w : 0.f;
            if (FAST) { a11[k][ci] = __builtin_amdgcn_rcpf(a11[k][ci]); a22[k][ci] = __builtin_amdgcn_rcpf(a22[k][ci]); }   // divide once, multiply ten times
            a12[k][ci] = in ? av : 0.f;
            wp[k][ci] = in ? wv_ : 0.f;
        }
    }
#pragma unroll
    for (int k = 0; k < VRT_K; k++) {
#pragma unroll
        for (int ci = 0; ci < 2; ci++) l_wt[own_[ci] + k * VRT_WAVES * VRT_PW] = wp[k][ci];
    }
    __syncthreads();
    for (int s = 0; s < n_half; s += 2) {
#pragma unroll
        for (int ci = 0; ci < 2; ci++) {
            // neighbours live in the other colour's plane: left = pair cp - (1 - e), right = pair cp + e, up / down = cp
            const int opb = own_[ci ^ 1], lft = opb - (1 - e_[ci]), rgt = opb + e_[ci];
            const int reach = s + ci + 1;                              // 1-based index of this half sweep
#pragma unroll
            for (int k = 0; k < VRT_K; k++) {
                const int r = wv + k * VRT_WAVES, y = y0 + r, o = k * VRT_WAVES * VRT_PW;
                if (r < reach || r > VRT_RH - 1 - reach || y < 0 || y >= H) continue;      // wave-uniform
                if (colact[ci]) {
                    const float2 dl = l_dw[lft + o], dr = l_dw[rgt + o];
                    const float2 du_ = l_dw[opb + o - VRT_PW], dd = l_dw[opb + o + VRT_PW];
                    const float wl = l_wt[lft + o], wu = l_wt[opb + o - VRT_PW];
                    const float w = wp[k][ci];
                    float2 d = l_dw[own_[ci] + o];
                    const float sigmaU = wl * dl.x + w * dr.x + wu * du_.x + w * dd.x;
                    const float sigmaV = wl * dl.y + w * dr.y + wu * du_.y + w * dd.y;
                    if (FAST) {
                        d.x += omega * ((sigmaU + b1[k][ci] - d.y * a12[k][ci]) * a11[k][ci] - d.x);
                        d.y += omega * ((sigmaV + b2[k][ci] - d.x * a12[k][ci]) * a22[k][ci] - d.y);
                    } else {
                        d.x += omega * ((sigmaU + b1[k][ci] - d.y * a12[k][ci]) / a11[k][ci] - d.x);
                        d.y += omega * ((sigmaV + b2[k][ci] - d.x * a12[k][ci]) / a22[k][ci] - d.y);
                    }
                    l_dw[own_[ci] + o] = d;
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int k = 0; k < VRT_K; k++) {
        const int r = wv + k * VRT_WAVES, y = y0 + r;
        if (r < VRT_HALO || r >= VRT_HALO + VRT_H || y >= H) continue;
#pragma unroll
        for (int ci = 0; ci < 2; ci++) {
            const int c = 2 * cp + e_[ci], x = x0 + c;
            if (c < VRT_HALO || c >= VRT_HALO + VRT_W || x >= W) continue;
            const int64_t p = (int64_t)y * W + x;
            float2 d = l_dw[own_[ci] + k * VRT_WAVES * VRT_PW];
            if (Wadd) { const float2 w = Wadd[p]; d = make_float2(w.x + d.x, w.y + d.y); }   // last iteration: the refined flow
            dW_out[p] = d;
        }
    }
}

__global__ void __launch_bounds__(256)
k_vr_finish(const float2 *Wf, const float2 *__restrict__ dW, int64_t n, float2 *out)     // out may be Wf
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float2 w = Wf[i], d = dW[i];
    out[i] = make_float2(w.x + d.x, w.y + d.y);
}

extern "C" void tf_varref_default_params(tf_varref_params *p)
{
    p->fixed_point_iterations = 5; p->sor_iterations = 5;
    p->alpha = 20.f; p->delta = 5.f; p->gamma = 10.f; p->omega = 1.6f;
}

static size_t vr_plane(int64_t n, int64_t B) { return B > 1 ? tf_align_up((size_t)n, 64) : (size_t)n; }

extern "C" size_t tf_varref_workspace_bytes_batch(int64_t B, int64_t H, int64_t W)
{
    if (H <= 0 || W <= 0 || B <= 0) return 0;
    const size_t n = vr_plane(H * W, B) * (size_t)B;
    // S (float4), A12, wt (float), A, dW and its ping-pong partner (float2)
    return tf_align_up(n * 16, 256) + 2 * tf_align_up(n * 4, 256) + 3 * tf_align_up(n * 8, 256) + 4096;
}
extern "C" size_t tf_varref_workspace_bytes(int64_t H, int64_t W) { return tf_varref_workspace_bytes_batch(1, H, W); }

// the refinement of B images in one set of launches (grid z = image): I0 + b * img_stride, I1 + b * img_stride, flow +
// b * flow_stride (floats).  Per tile the code is the single image's, so the bits are too; what changes is the launch: at
// 1500 x 2500 a k_vr_sor_tile launch for ONE image is 282 tiles on 256 CUs -- one full round and a second one that is 10 %
// full -- and a frame pair costs 2 x 11 launches; 23 pairs at once are 6486 tiles (25.3 rounds) in 11 launches per direction.
static int vr_run(const uint8_t *I0, const uint8_t *I1, int64_t B, int64_t img_stride, int64_t H, int64_t W, const tf_varref_params *params,
                  float *flow, int64_t flow_stride, int flags, void *ws, size_t ws_bytes, void *stream)
{
    TF_REQUIRE((flags & ~(TF_VR_FAST_DIVIDE | TF_VR_FAST_SOR)) == 0, "tf_varref_ex: unknown flag");
    const bool fast = (flags & TF_VR_FAST_DIVIDE) != 0;                  // system assembly AND the sweeps
    const bool fast_sor = fast || (flags & TF_VR_FAST_SOR) != 0;        // the sweeps only
    TF_REQUIRE(I0 && I1 && flow && ws, "tf_varref: null pointer");
    TF_REQUIRE(H > 0 && W > 0 && H < 32768 && W < 32768, "tf_varref: bad shape");
    TF_REQUIRE(B >= 1 && B <= 65535, "tf_varref: bad batch size");
    TF_REQUIRE(B == 1 || (img_stride >= H * W && flow_stride >= 2 * H * W && flow_stride % 2 == 0), "tf_varref_batch: strides smaller than one image / odd flow stride");
    tf_varref_params dp;
    if (!params) { tf_varref_default_params(&dp); params = &dp; }
    TF_REQUIRE(params->fixed_point_iterations >= 0 && params->sor_iterations >= 0, "tf_varref: bad iteration counts");
    hipStream_t s = (hipStream_t)stream;
    // the fused SOR kernel covers up to VRT_HALO half sweeps; more sorIterations take one launch per half sweep (k_vr_sor)
    const bool tiled = 2 * params->sor_iterations <= VRT_HALO;
    const bool tile_path = tiled && params->sor_iterations > 0;
    if (B > 1 && !tile_path) {
        // the per-half-sweep kernels have no batch dimension: image by image
        for (int64_t b = 0; b < B; b++)
            if (const int rc = vr_run(I0 + b * img_stride, I1 + b * img_stride, 1, 0, H, W, params, flow + b * flow_stride, 0, flags, ws, ws_bytes, stream)) return rc;
        return TF_OK;
    }
    const int64_t n = H * W;
    const int64_t np = (int64_t)vr_plane(n, B);
    TfArena ar(ws, ws_bytes);
    float4 *S = ar.take<float4>(np * B);
    float2 *A = ar.take<float2>(np * B);
    float *A12 = ar.take<float>(np * B), *wt = ar.take<float>(np * B);
    float2 *dW = ar.take<float2>(np * B), *dW2 = ar.take<float2>(np * B);
    if (!ar.ok()) { tf_set_error("tf_varref: workspace too small"); return TF_ENOMEM; }
    VrP P;
    P.alpha2 = params->alpha / 4; P.delta2 = params->delta / 2; P.gamma2 = params->gamma / 2; P.omega = params->omega;
    P.zeta2 = 0.1f * 0.1f; P.eps2 = 0.001f * 0.001f;
    const VrB bs = {B > 1 ? img_stride : 0, B > 1 ? flow_stride / 2 : 0, B > 1 ? np : 0};
    const unsigned Z = (unsigned)B;
    const double nb = (double)n * (double)B;
    // W is the caller's flow array itself: it is only read until the last kernel replaces it by W + dW
    const float2 *Wf = (const float2 *)flow;
    const int iH = (int)H, iW = (int)W;
    {
        TfProfScope ps(TFK_VR_PREPARE, (1.0 + 1.0 + 8.0 + 8.0) * nb, s);
        hipLaunchKernelGGL(k_vr_prepare, dim3((iW + VR_TW - 1) / VR_TW, (iH + VR_TH - 1) / VR_TH, Z), dim3(256), 0, s,
                           I0, I1, Wf, iH, iW, A, bs);
    }
    TF_CHECK_LAUNCH();
    const dim3 g1((iW + VRS_TW - 1) / VRS_TW, (iH + VRS_TH - 1) / VRS_TH, Z), g2(((iW + 1) / 2 + 63) / 64, (iH + 3) / 4);
    if (tiled) {
        static TfDeviceOnce once;                  // function attributes are per device
        TfDeviceOnce::Guard guard(once);
        if (guard.first) {
            TF_CHECK_HIP(hipFuncSetAttribute((const void *)k_vr_sor_tile<false>, hipFuncAttributeMaxDynamicSharedMemorySize, VRT_LDS_BYTES));
            TF_CHECK_HIP(hipFuncSetAttribute((const void *)k_vr_sor_tile<true>, hipFuncAttributeMaxDynamicSharedMemorySize, VRT_LDS_BYTES));
            guard.done();
        }
    }
    // dW = 0 at the start: the tiled path passes "no dW" to the first iteration's kernels, the sweep path needs the array
    const float2 *dW_cur = nullptr;
    if (!tile_path) { TF_CHECK_HIP(hipMemsetAsync(dW, 0, (size_t)n * 8, s)); dW_cur = dW; }
    bool flow_done = false;
    for (int it = 0; it < params->fixed_point_iterations; it++) {
        {
            // algorithmic bytes: A 8, W 8, dW 8 read; S 16, A12 4, weight 4 written (no dW in the first iteration)
            TfProfScope ps(TFK_VR_SYSTEM, (8.0 + 8.0 + (dW_cur ? 8.0 : 0.0) + 16.0 + 4.0 + 4.0) * nb, s);
            if (fast)
                hipLaunchKernelGGL(k_vr_system<true>, g1, dim3(256), 0, s, (const float2 *)A, Wf, dW_cur, iH, iW, P, S, A12, wt, bs);
            else
                hipLaunchKernelGGL(k_vr_system<false>, g1, dim3(256), 0, s, (const float2 *)A, Wf, dW_cur, iH, iW, P, S, A12, wt, bs);
        }
        TF_CHECK_LAUNCH();
        if (tile_path) {
            // algorithmic bytes: system 20 + weight 4 + dW 8 read, dW 8 written, once per fixed-point iteration (no dW
            // to read in the first; W 8 more to read in the last, which writes the refined flow)
            const bool last = it == params->fixed_point_iterations - 1;
            TfProfScope ps(TFK_VR_SOR, (20.0 + 4.0 + (dW_cur ? 8.0 : 0.0) + (last ? 8.0 : 0.0) + 8.0) * nb, s);
            float2 *dst = last ? (float2 *)flow : (dW_cur == dW ? dW2 : dW);
            const float2 *wadd = last ? Wf : (const float2 *)nullptr;
            const dim3 gt((iW + VRT_W - 1) / VRT_W, (iH + VRT_H - 1) / VRT_H, Z);
            if (fast_sor)
                hipLaunchKernelGGL(k_vr_sor_tile<true>, gt, dim3(VRT_THREADS), VRT_LDS_BYTES, s, (const float4 *)S, (const float *)A12,
                                   (const float *)wt, iH, iW, 2 * params->sor_iterations, P.omega, dW_cur, wadd, dst, bs);
            else
                hipLaunchKernelGGL(k_vr_sor_tile<false>, gt, dim3(VRT_THREADS), VRT_LDS_BYTES, s, (const float4 *)S, (const float *)A12,
                                   (const float *)wt, iH, iW, 2 * params->sor_iterations, P.omega, dW_cur, wadd, dst, bs);
            dW_cur = dst;
            flow_done = last;
        } else {
            TfProfScope ps(TFK_VR_SOR, (20.0 + 4.0 + 8.0 + 8.0) * (double)n * params->sor_iterations, s);
            for (int k = 0; k < params->sor_iterations; k++) {
                hipLaunchKernelGGL(k_vr_sor, g2, dim3(256), 0, s, (const float4 *)S, (const float *)A12, (const float *)wt, iH, iW, 0, P.omega, dW);
                hipLaunchKernelGGL(k_vr_sor, g2, dim3(256), 0, s, (const float4 *)S, (const float *)A12, (const float *)wt, iH, iW, 1, P.omega, dW);
            }
        }
        TF_CHECK_LAUNCH();
    }
    if (!flow_done) {
        // no tiled last iteration: the sweep path (B == 1 here), or no iterations at all (any B, tile path with
        // fixed_point_iterations == 0).  flow = W + dW, with dW = 0 in every image's plane if nothing ran
        if (!dW_cur) { TF_CHECK_HIP(hipMemsetAsync(dW, 0, (size_t)np * (size_t)B * 8, s)); dW_cur = dW; }
        for (int64_t b = 0; b < B; b++) {
            hipLaunchKernelGGL(k_vr_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, Wf + b * bs.flow, dW_cur + b * bs.plane, n, (float2 *)flow + b * bs.flow);
            TF_CHECK_LAUNCH();
        }
    }
    return TF_OK;
}

extern "C" int tf_varref_ex(const uint8_t *I0, const uint8_t *I1, int64_t H, int64_t W, const tf_varref_params *params,
                            float *flow, int flags, void *ws, size_t ws_bytes, void *stream)
{
    return vr_run(I0, I1, 1, 0, H, W, params, flow, 0, flags, ws, ws_bytes, stream);
}

extern "C" int tf_varref(const uint8_t *I0, const uint8_t *I1, int64_t H, int64_t W, const tf_varref_params *params,
                         float *flow, void *ws, size_t ws_bytes, void *stream)
{
    return tf_varref_ex(I0, I1, H, W, params, flow, 0, ws, ws_bytes, stream);
}

extern "C" int tf_varref_batch(const uint8_t *I0, const uint8_t *I1, int64_t B, int64_t img_stride, int64_t H, int64_t W,
                               const tf_varref_params *params, float *flow, int64_t flow_stride, int flags,
                               void *ws, size_t ws_bytes, void *stream)
{
    if (ws_bytes < tf_varref_workspace_bytes_batch(B, H, W)) {
        // (a caller that sized for one image still gets its images refined -- one after the other)
        TF_REQUIRE(B >= 1 && ws_bytes >= tf_varref_workspace_bytes(H, W), "tf_varref_batch: workspace too small");
        for (int64_t b = 0; b < B; b++)
            if (const int rc = vr_run(I0 + b * img_stride, I1 + b * img_stride, 1, 0, H, W, params, flow + b * flow_stride, 0, flags, ws, ws_bytes, stream)) return rc;
        return TF_OK;
    }
    return vr_run(I0, I1, B, img_stride, H, W, params, flow, flow_stride, flags, ws, ws_bytes, stream);
}

// development aid: number of operand pairs (out of `count`, drawn from the range vr_div_shared is used in) for which the
// shared-reciprocal division differs from the hardware's correctly rounded one.  Must be 0.
extern "C" int tf_selftest_shared_divide(int64_t count, uint64_t seed, uint64_t *mismatches_host, void *stream)
{
    TF_REQUIRE(mismatches_host && count > 0, "tf_selftest_shared_divide: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *d_m = nullptr;
    TF_CHECK_HIP(hipMalloc(&d_m, 8));
    TF_CHECK_HIP(hipMemsetAsync(d_m, 0, 8, s));
    hipLaunchKernelGGL(k_vr_selftest_divide, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, (unsigned long long)seed, count, d_m);
    unsigned long long h = 0;
    hipError_t e = hipMemcpyAsync(&h, d_m, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_m);
    TF_CHECK_HIP(e);
    *mismatches_host = h;
    return TF_OK;
}
