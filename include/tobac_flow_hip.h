/* tobac_flow_hip.h -- C ABI of the MI355X (gfx950) hot path of tobac-flow.
 *
 * One shared library, libtobac_flow_hip.so, built from the .hip sources in tobac_flow_amd/csrc/.  Every entry
 * point is `extern "C"`, takes plain pointers and sizes, never retains a pointer past return
 * and never allocates device memory behind the caller's back: scratch comes from a caller
 * supplied workspace whose size is given by the matching *_workspace_bytes() query.
 *
 * All data pointers are DEVICE pointers (HBM) unless the name ends in `_host`.  `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  Calls are asynchronous with respect to
 * the host unless stated otherwise.
 *
 * Return value: 0 on success, a negative TF_E* code on failure; tf_last_error() returns a
 * thread-local message.  The Python host layer (tobac_flow_amd/) validates arguments first and
 * raises the same exception types as the reference (ValueError / AssertionError / ...).
 *
 * Each entry point names the reference interface it replaces (paths relative to
 * /root/reference/).  How a maintainer binds them from the reference is shown in INTEGRATION.md.
 */
#ifndef TOBAC_FLOW_HIP_H
#define TOBAC_FLOW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TF_OK 0
#define TF_EINVAL (-1)   /* bad argument (shape, enum, null pointer)          */
#define TF_ENOMEM (-2)   /* workspace too small                               */
#define TF_EHIP (-3)     /* a HIP runtime call or kernel launch failed        */
#define TF_ENOCONV (-4)  /* an iterative kernel hit its sweep limit           */
#define TF_EDEPTH (-5)   /* tf_watershed*: ties left at the deepest chain level the workspace allows; output written,
                            but not guaranteed to equal the reference at the reported pixels */
#define TF_ESTARVED (-6) /* tf_farneback*: a row-sum chain of the iteration kernel gave up waiting for its left neighbour
                            (a stalled device); the flow of the launches concerned holds NaN rows -- recompute */

/* interpolation of the semi-Lagrangian gathers: cv2.INTER_NEAREST / _LINEAR / _CUBIC as selected
 * by tobac_flow/convolve.py:47-54 and tobac_flow/utils/flow_utils.py:22-34 */
#define TF_INTERP_NEAREST 0
#define TF_INTERP_LINEAR 1
#define TF_INTERP_CUBIC 2
#define TF_INTERP_LANCZOS 3   /* cv2.INTER_LANCZOS4: 8 x 8 taps (convolve.py:47-54 "lanczos") */

/* element types of `data` / `out` arguments */
#define TF_F32 0
#define TF_F64 1
#define TF_I32 2
#define TF_U8 3          /* tf_edt2d_frames, tf_label_nanmin, tf_label_filter, tf_label_reduce, tf_label_order only (bool arrays have these bytes) */
#define TF_I16 4         /* tf_prepare_fields only: a packed channel */
#define TF_I8 5          /* tf_stripe_deviation, tf_prepare_fields only: a DQF plane */

/* reductions over the gathered (n_struct, H, W) stack, i.e. the `func` argument of
 * tobac_flow/convolve.py:248-348 for the callables the reference itself passes */
#define TF_FUNC_STACK 0        /* func=None: return the whole stack (n_struct, T, H, W)            */
#define TF_FUNC_SOBEL 1        /* sobel.py:66-86  _sobel_func                                      */
#define TF_FUNC_SOBEL_UPHILL 2 /* sobel.py:32-46  _sobel_func_uphill                               */
#define TF_FUNC_SOBEL_DOWNHILL 3 /* sobel.py:49-63 _sobel_func_downhill                            */
#define TF_FUNC_NANMEAN 4      /* detection.py:53-55,190-195  lambda x: np.nanmean(x, 0)           */
#define TF_FUNC_DIFF 5         /* flow.py:180-184  centred semi-Lagrangian time difference         */
#define TF_FUNC_ANY 6          /* detection.py:313-320  partial(np.any, axis=0) on int32           */
#define TF_FUNC_NANMAX 7       /* detection.py:57-59 (commented-out variant kept for completeness) */

int tf_version(void);
const char *tf_last_error(void);
/* number of visible HIP devices, or a negative TF_E* code; never initialises a context */
int tf_device_count(void);

/* ---- a3: to_8bit(linear_norm(data[i:i+2]), 0, 1) --------------------------------------------
 * replaces tobac_flow/utils/normalisation_utils.py:10-33 (to_8bit) composed with :59-72
 * (linear_norm) exactly as tobac_flow/flow.py:411-414 calls them: joint nanmin/nanmax over the
 * frame pair, scale to [0,1], clip, *255, non-finite -> 127 then patched from the other frame,
 * truncate to uint8.  ws: >= tf_to8bit_workspace_bytes() bytes. */
size_t tf_to8bit_workspace_bytes(int64_t H, int64_t W);
int tf_to8bit_pair(const float *frame0, const float *frame1, int64_t H, int64_t W,
                   uint8_t *out0, uint8_t *out1, void *ws, size_t ws_bytes, void *stream);

/* ---- a3b: to_8bit(<normalisation method>(data[i:i+2], **kwargs), 0, 1) -----------------------
 * the other joint normalisations that tobac_flow/flow.py:411-414 selects by name
 * (tobac_flow/utils/normalisation_utils.py:59-116), for float32 frames under numpy 2's promotion rules.
 *   linear        vmin / vmax optional (neither given: the same bytes as tf_to8bit_pair)
 *   log           vmax optional; vmin is ignored, as in the reference (the data minimum is reused)
 *   inverse_log   vmin optional; vmax is ignored
 *   z_score       max_std
 *   uniform       quantiles in 1 .. TF_NORM_MAX_QUANTILES; the pair must be finite (a NaN makes numpy's edges NaN): the
 *                 call does not test that -- the caller does (normalise_pair_dev / calculate_flow)
 *   local_linear  size >= 1; W <= TF_NORM_MAX_ROW (a row is filtered in LDS)
 * vmin, vmax and max_std are Python numbers as numpy 2 sees them ("weak": rounded to float32 where they meet the data,
 * double among themselves) unless TF_NORM_F32_SCALARS says that the caller held float32 scalars.  linear with bounds,
 * uniform and local_linear on NaN-free pairs give the reference's bytes; log, inverse_log, z_score and local_linear
 * with NaNs evaluate log and the moments in float64 and round, which can move a byte by 1.
 * Bad arguments: TF_EINVAL; ws_bytes < tf_norm8_workspace_bytes(H, W, method, params): TF_ENOMEM. */
typedef enum {
    TF_NORM_LINEAR = 0, TF_NORM_LOG = 1, TF_NORM_INVERSE_LOG = 2, TF_NORM_Z_SCORE = 3, TF_NORM_UNIFORM = 4,
    TF_NORM_LOCAL_LINEAR = 5
} TfNormMethod;
#define TF_NORM_HAS_VMIN 1
#define TF_NORM_HAS_VMAX 2
#define TF_NORM_F32_SCALARS 4
#define TF_NORM_MAX_QUANTILES 1024
#define TF_NORM_MAX_ROW 8192
typedef struct {
    double vmin, vmax;      /* used when the matching TF_NORM_HAS_* flag is set */
    double max_std;         /* 3   */
    int64_t quantiles;      /* 256 */
    int64_t size;           /* 100 */
    int flags;
} TfNormParams;
void tf_norm8_default_params(TfNormParams *params);
size_t tf_norm8_workspace_bytes(int64_t H, int64_t W, int method, const TfNormParams *params);
int tf_norm8_pair(const float *frame0, const float *frame1, int64_t H, int64_t W, int method, const TfNormParams *params,
                  uint8_t *out0, uint8_t *out1, void *ws, size_t ws_bytes, void *stream);

/* ---- a5: dense Farnebaeck flow for one frame pair, BOTH directions ---------------------------
 * replaces cv2.optflow.createOptFlow_Farneback().calc(prev, next, None) and
 * .calc(next, prev, None) as issued by tobac_flow/flow.py:511,516 (model factory
 * tobac_flow/utils/flow_utils.py:52-53; OpenCV defaults numLevels=5, pyrScale=0.5, winSize=13,
 * numIters=10, polyN=5, polySigma=1.1, flags=0).  The two directions share the Gaussian pyramid
 * and the polynomial expansion of both images.  flow_fwd / flow_bwd: (H, W, 2) float, (dx, dy).
 * Either output may be NULL to skip that direction. */
typedef struct {
    int num_levels;     /* 5   */
    double pyr_scale;   /* 0.5 */
    int win_size;       /* 13  */
    int num_iters;      /* 10  */
    int poly_n;         /* 5   */
    double poly_sigma;  /* 1.1 */
    int chain_form;     /* TF_FB_CHAIN_*: scheduling of the iteration kernel for THIS call; the flows are the same bits */
    int status_slot;    /* 0 = the device's shared status word; > 0 = a word of this caller's own (tf_farneback_status_acquire) */
} tf_farneback_params;
/* chain_form: the row-sum chains of the iteration kernel as one lane per chain (leaves LDS for the kernels of other streams,
 * e.g. floods of finished windows: what a caller that runs other work beside the flow wants) or in two parts one row group
 * apart (39 KB of LDS per workgroup, a CU is full: 8 % faster when the flow has the GPU to itself).  DEFAULT = one lane. */
#define TF_FB_CHAIN_DEFAULT 0
#define TF_FB_CHAIN_ONE_LANE 1
#define TF_FB_CHAIN_TWO_PART 2
void tf_farneback_default_params(tf_farneback_params *p);
size_t tf_farneback_workspace_bytes(int64_t H, int64_t W, const tf_farneback_params *p);
int tf_farneback_pair(const uint8_t *prev, const uint8_t *next, int64_t H, int64_t W,
                      const tf_farneback_params *p, float *flow_fwd, float *flow_bwd,
                      void *ws, size_t ws_bytes, void *stream);
/* Diagnostic / test entry: the 3 x 3 Gaussian of a uint8 frame and its polynomial expansion exactly as the full-resolution
 * pyramid level computes them (cv2's FarnebackPolyExp on the blurred frame), for stage-by-stage comparison with the oracle.
 * blur_out: H * W floats or NULL; R_out: 5 * H * W floats = H * W float4 {r0, r1, r2, r3} + one plane r4 (OpenCV's five
 * interleaved channels, in its order). */
int tf_farneback_expansion(const uint8_t *img, int64_t H, int64_t W, const tf_farneback_params *p,
                           float *blur_out, float *R_out, void *stream);
/* The same for B independent frame pairs in one set of launches (the loop of tobac_flow/flow.py:411-423):
 * pair b reads prev + b*img_stride / next + b*img_stride (bytes = pixels, uint8) and writes
 * flow_fwd + b*flow_stride / flow_bwd + b*flow_stride (strides in floats), so the results can land
 * directly in forward_flow[i0 + b] and backward_flow[i0 + 1 + b].  Batching keeps the coarse pyramid
 * levels -- a few hundred workgroups per pair -- busy on all 256 CUs. */
size_t tf_farneback_workspace_bytes_batch(int64_t B, int64_t H, int64_t W, const tf_farneback_params *p);
/* How many pairs to hand to tf_farneback_batch at a time.  OpenCV's box filter carries the float rounding of its running
 * column sums down a whole column (optflowgf.cpp FarnebackUpdateFlow_Blur: `vsum[x] += srow1[x] - srow0[x]`), so the
 * iteration kernel cannot split the rows of a column over workgroups: its parallelism is strips x directions x pairs,
 * and a launch costs a whole number of "rounds" of resident workgroups, at every pyramid level.  Returns the batch size
 * <= max_pairs whose workspace fits max_bytes (0 = no limit) with the best ratio of work to rounds x rows summed over
 * the levels -- the largest one within 1 % of the best (42 pairs at 5424 x 5424 on 256 CUs: full rounds at levels 0, 1, 2). */
int64_t tf_farneback_batch_hint(int64_t H, int64_t W, const tf_farneback_params *p, int64_t max_pairs, size_t max_bytes);
/* Launches are asynchronous, so what a launch found out arrives later: tf_farneback_check() -- call it once the stream the
 * batches ran on has been synchronised (or an event after them has completed) -- returns TF_ESTARVED if a row-sum chain of
 * any iteration launch of this device (made with status_slot 0) since the last report gave up waiting for its left
 * neighbour's hand-over words (bounded polls: a device stalled for seconds by a profiler's serialisation or a preempted
 * queue), TF_OK otherwise.  The flow of those launches then holds NaN rows.  Every tf_farneback_batch* call also reports (and
 * clears) on entry what earlier launches left in ITS status word, so a caller that never checks still cannot go on
 * unnoticed.  The reference has no counterpart (cv2's calc is synchronous); error convention of SURVEY section 8(b).
 *
 * Status slots (round 6): the shared word is read and cleared by whoever looks first, which is wrong as soon as two flows are
 * in flight on one device (two host threads; a deferred check beside the next stack's first batch): one flow's entry check
 * would consume the other's report.  tf_farneback_status_acquire() hands out a word of the caller's own (1 .. 255; 0 = none
 * left or no device: share the device's word); put it into tf_farneback_params.status_slot for every call of ONE flow, read
 * it with tf_farneback_status_check(slot) once that flow's launches have finished (TF_ESTARVED / TF_OK; clears), give it back
 * with tf_farneback_status_release(slot).  Calls with a slot of their own neither read nor clear the shared word. */
int tf_farneback_check(void);
int tf_farneback_status_acquire(void);
int tf_farneback_status_check(int slot);
void tf_farneback_status_release(int slot);
/* test hooks: set a status word from the host, as a starved chain would (tests of the host-side path) */
int tf_farneback_debug_set_starved(void);
int tf_farneback_debug_set_starved_slot(int slot);
/* Workgroups of the iteration kernel's full-resolution launch for B pairs, and (resident_out, may be NULL) how many the
 * device holds at once.  A launch costs whole rounds of resident workgroups: cut a batch into parts
 * (tf_farneback_batch_phase) only while a part still fills a round. */
int64_t tf_farneback_iteration_workgroups(int64_t H, int64_t W, const tf_farneback_params *p, int64_t B, int64_t *resident_out);
int tf_farneback_batch(const uint8_t *prev, const uint8_t *next, int64_t B, int64_t img_stride,
                       int64_t H, int64_t W, const tf_farneback_params *p,
                       float *flow_fwd, float *flow_bwd, int64_t flow_stride,
                       void *ws, size_t ws_bytes, void *stream);
/* tf_farneback_batch_split (round 4): the same batch with the pyramid levels >= 2 run for all B pairs at once and the two
 * finest levels in `parts` parts of ceil(B / parts) pairs -- full-size scratch for one part only
 * (tf_farneback_workspace_bytes_split), so a scratch budget that holds 21 full-size pairs still fills the coarse levels'
 * launches with 42.  Same kernels on the same data: results identical to tf_farneback_batch (parts = 1 is that call).
 * Needs pyr_scale = 0.5 (otherwise, and with fewer than three levels, it runs unsplit). */
size_t tf_farneback_workspace_bytes_split(int64_t B, int64_t parts, int64_t H, int64_t W, const tf_farneback_params *p);
int tf_farneback_batch_split(const uint8_t *prev, const uint8_t *next, int64_t B, int64_t parts, int64_t img_stride,
                             int64_t H, int64_t W, const tf_farneback_params *p,
                             float *flow_fwd, float *flow_bwd, int64_t flow_stride,
                             void *ws, size_t ws_bytes, void *stream);
/* The two halves of a split batch as calls of their own (tf_farneback_can_split says whether the geometry allows it):
 * phase 1 = pyramid levels >= 2 for B pairs, their flow left in the output frames; phase 2 = levels 1 and 0 for B pairs
 * whose output frames hold that flow (any part of the pairs of phase 1).  create_flow runs phase 1 for a whole batch, then
 * per part: phase 2, refinement, smoothing, on_frames_ready -- the coarse launches hold twice the pairs, the caller still
 * gets its frames part by part. */
int tf_farneback_can_split(int64_t H, int64_t W, const tf_farneback_params *p);
size_t tf_farneback_workspace_bytes_phase(int64_t B, int64_t H, int64_t W, const tf_farneback_params *p, int phase);
int tf_farneback_batch_phase(const uint8_t *prev, const uint8_t *next, int64_t B, int64_t img_stride,
                             int64_t H, int64_t W, const tf_farneback_params *p,
                             float *flow_fwd, float *flow_bwd, int64_t flow_stride,
                             void *ws, size_t ws_bytes, void *stream, int phase);

/* ---- a5 tail / section 8f-1: variational refinement of one flow field -------------------------------------
 * replaces cv2.VariationalRefinement.create().calc(I0, I1, flow) as tobac_flow/flow.py:359 creates it and
 * tobac_flow/flow.py:513-519 calls it once per direction when vr_steps > 0 (OpenCV defaults: fixedPointIterations 5,
 * sorIterations 5, alpha 20, delta 5, gamma 10, omega 1.6).  I0, I1: (H, W) uint8; flow: (H, W, 2) float (dx, dy),
 * refined IN PLACE.  params NULL = defaults.  Parity with OpenCV itself is unpinned. */
typedef struct {
    int fixed_point_iterations;   /* 5   */
    int sor_iterations;           /* 5   */
    float alpha;                  /* 20  smoothness term weight        */
    float delta;                  /* 5   colour constancy weight       */
    float gamma;                  /* 10  gradient constancy weight     */
    float omega;                  /* 1.6 SOR relaxation factor         */
} tf_varref_params;
void tf_varref_default_params(tf_varref_params *p);
size_t tf_varref_workspace_bytes(int64_t H, int64_t W);
int tf_varref(const uint8_t *I0, const uint8_t *I1, int64_t H, int64_t W, const tf_varref_params *params,
              float *flow, void *ws, size_t ws_bytes, void *stream);
/* tf_varref_ex = tf_varref + `flags`.
 * TF_VR_FAST_DIVIDE (opt-in): the divisions and square roots of the system assembly and of the SOR updates use the
 *   hardware reciprocal / reciprocal square root (1 ulp) and reciprocal-multiply (the SOR update divides by A11 / A22
 *   ten times per fixed-point iteration: one reciprocal, ten products).  The result is no longer bit-identical to the
 *   arithmetic of OpenCV's variational_refinement.cpp as restated in oracle/c/varref.c, but stays within the 1e-4 px the
 *   flow is specified to (given the same input flow).  The default (flags = 0) evaluates every expression as written. */
#define TF_VR_FAST_DIVIDE 1
/* TF_VR_FAST_SOR (round 4): the reciprocal-multiply form in the SOR sweeps only (one hardware reciprocal of A11 / A22 per
 * pixel and fixed-point iteration, a multiplication per update instead of a correctly rounded division); the system
 * assembly keeps its correctly rounded divisions and square roots. */
#define TF_VR_FAST_SOR 2
int tf_varref_ex(const uint8_t *I0, const uint8_t *I1, int64_t H, int64_t W, const tf_varref_params *params,
                 float *flow, int flags, void *ws, size_t ws_bytes, void *stream);
/* tf_varref_batch (round 6): the refinement of B images in ONE set of launches -- the loop of tobac_flow/flow.py:411-423 over
 * the frame pairs, one direction: image b reads I0 + b * img_stride and I1 + b * img_stride (pixels) and refines flow +
 * b * flow_stride (floats, even) in place.  The grid gains an image dimension, the code per tile is tf_varref's: the same
 * bits.  What it buys is launches that fill the chip -- at 1500 x 2500 the fused SOR kernel of ONE image is 282 tiles on
 * 256 CUs (a full round plus one that is 10 % full), of 23 images 6486 tiles in one launch -- and 11 launches per direction
 * and batch instead of 11 per image.  ws: tf_varref_workspace_bytes_batch(B, H, W) (48 B per pixel and image); with less
 * (>= one image's) the images are refined one after the other. */
size_t tf_varref_workspace_bytes_batch(int64_t B, int64_t H, int64_t W);
int tf_varref_batch(const uint8_t *I0, const uint8_t *I1, int64_t B, int64_t img_stride, int64_t H, int64_t W,
                    const tf_varref_params *params, float *flow, int64_t flow_stride, int flags,
                    void *ws, size_t ws_bytes, void *stream);

/* ---- a6: forward/backward consistency smoothing ----------------------------------------------
 * replaces tobac_flow/flow.py:530-568 smooth_flow_step (4 x cv2.remap via
 * tobac_flow/utils/flow_utils.py:80-99 + np.nanmean).  Outputs must not alias inputs. */
int tf_smooth_flow_step(const float *fwd, const float *bwd, int64_t H, int64_t W, int interp,
                        float *fwd_out, float *bwd_out, void *stream);
/* The same step with create_flow's clip (tobac_flow/flow.py:60-63, np.minimum(np.maximum(v, -max), max): NaN propagates)
 * applied to what it stores -- for the LAST smoothing pass of a stack: clipping is elementwise, so it may ride on the
 * store of the stage that produces the final vectors instead of costing another pass over both flow arrays
 * (tf_flow_finalize_ends then only mirrors the two end frames).  max_value = +inf: no clip. */
int tf_smooth_flow_step_clip(const float *fwd, const float *bwd, int64_t H, int64_t W, int interp,
                             float *fwd_out, float *bwd_out, float max_value, void *stream);

/* single-image warp: tobac_flow/utils/flow_utils.py:80-99 warp_flow (BORDER_CONSTANT NaN) */
int tf_warp_flow(const float *img, const float *flow, int64_t H, int64_t W, int interp,
                 float *out, void *stream);

/* ---- a2 tail: end-frame mirroring and clipping -------------------------------------------------
 * tobac_flow/flow.py:425-426 (forward[-1] = -backward[-1]; backward[0] = -forward[0]) and
 * tobac_flow/flow.py:60-61 (clip both to [-max_value, max_value]); in place. */
int tf_flow_finalize(float *fwd, float *bwd, int64_t T, int64_t H, int64_t W, float max_value,
                     void *stream);
/* tobac_flow/flow.py:425-426 alone, for a stack whose interior is already clipped (tf_smooth_flow_step_clip): writes
 * forward[T - 1] = -backward[T - 1] and backward[0] = -forward[0] (clipped like the rest), touches nothing else. */
int tf_flow_finalize_ends(float *fwd, float *bwd, int64_t T, int64_t H, int64_t W, float max_value,
                          void *stream);

/* ---- a8-a13: semi-Lagrangian convolve / sobel / diff ------------------------------------------
 * replaces tobac_flow/convolve.py:248-348 convolve (with :8-86 warp_flow, :89-144
 * convolve_same_step, :147-245 convolve_step fused into one gather), tobac_flow/sobel.py:89-143
 * and tobac_flow/flow.py:159-191.
 *   data      (T, H, W), data_type TF_F32 or TF_I32 (TF_I32 requires TF_INTERP_NEAREST)
 *   fwd, bwd  (T, H, W, 2) float
 *   structure 27 bytes, (3,3,3) C order, non-zero = tap present
 *   fill      value for out-of-image taps and, when func != STACK, for output pixels whose
 *             input is NaN (convolve.py:346-347)
 *   out       func == STACK: (n_struct, T, H, W); otherwise (T, H, W); element type out_type
 *             (TF_F64 reproduces Flow.sobel's dtype=None behaviour, flow.py:193-199)
 *   t0, t1    only frames t0 <= t < t1 are written (frames t0-1 and t1 are still read as
 *             neighbours) so that a time series can be sharded without a halo copy. */
int tf_convolve(const void *data, int data_type, int64_t T, int64_t H, int64_t W,
                const float *fwd, const float *bwd, const uint8_t *structure_host,
                int interp, double fill, int func, void *out, int out_type,
                int64_t t0, int64_t t1, void *stream);

/* ---- a8-a10 by name: the step-level functions of tobac_flow/convolve.py -----------------------------
 * The arithmetic of tf_convolve's STACK form in the reference's general shape: separate frames, an image that need
 * not have the flow's shape, an explicit grid, any list of offsets, a (3, m, n) structure.  All three run on the
 * caller's stream, allocate no device memory and do not synchronise.  Offsets are host arrays; a list of any length
 * is served (the kernels take them 32 at a time).  Element types: images TF_F32 or TF_I32 (TF_I32 requires
 * TF_INTERP_NEAREST), out_type TF_F32, TF_F64 or TF_I32 (the sample is cast on store).  Every shape extent < 2^15.
 *
 * tf_warp_offsets: tobac_flow/convolve.py:8-86 warp_flow.
 *   img      (h, w)
 *   flow     (H, W, 2) float; (H, W) may differ from (h, w)
 *   grid     (H, W, 2) int32 (x, y) on the device, or NULL for the pixel index (convolve.py:59-63)
 *   offsets  (K, 2) host floats (x, y)
 *   out      (K, H, W): out[k] = cv2.remap(img, map_k, interp, BORDER_CONSTANT, fill) with, per component,
 *            map_k = (float)((double)(flow + offsets[k]) + (double)grid), the sum in brackets in float32 */
int tf_warp_offsets(const void *img, int img_type, int64_t h, int64_t w, const float *flow, const int32_t *grid,
                    int64_t H, int64_t W, const float *offsets_host, int64_t K, int interp, double fill,
                    void *out, int out_type, void *stream);

/* tf_gather_offsets: tobac_flow/convolve.py:89-144 convolve_same_step.
 *   img      (h, w)
 *   grid     (H, W, 2) int32 (x, y) on the device, or NULL for the pixel index of an (H, W) raster
 *   offsets  (K, 2) host int32 (x, y)
 *   out      (K, H, W): out[k] = img[grid.y + offsets[k].y, grid.x + offsets[k].x], `fill` where that is outside img */
int tf_gather_offsets(const void *img, int img_type, int64_t h, int64_t w, const int32_t *grid, int64_t H, int64_t W,
                      const int32_t *offsets_host, int64_t K, double fill, void *out, int out_type, void *stream);

/* tf_convolve_step: tobac_flow/convolve.py:147-245 convolve_step.
 *   prev, same, next  three separate (H, W) frames of data_type (prev / next may be NULL when plane 0 / 2 of the
 *                     structure is empty, and so may bwd / fwd)
 *   fwd, bwd          (H, W, 2) float: flow from this step to the next / to the previous one
 *   grid              (H, W, 2) int32 or NULL, as above
 *   structure         3 * m * n host bytes, (3, m, n) C order, non-zero = tap present; the offset of entry (row, col) is
 *                     (x, y) = (col - m / 2, row - n / 2), the reference's centre (convolve.py:203) as it applies it
 *   out               (n_struct, H, W): taps of plane 0 warped from prev through bwd, then the same-step taps of plane 1,
 *                     then the taps of plane 2 warped from next through fwd; within a plane in C (np.where) order */
int tf_convolve_step(const void *prev, const void *same, const void *next, int data_type, int64_t H, int64_t W,
                     const float *fwd, const float *bwd, const int32_t *grid, const uint8_t *structure_host,
                     int64_t m, int64_t n, int interp, double fill, void *out, int out_type, void *stream);

/* ---- a17 piece: combined edge field --------------------------------------------------------------
 * the elementwise tail of tobac_flow/detection.py:620-642 get_combined_edge_field:
 * edges[edges > 0] += 1; edges -= field; edges[isnan(field)] = inf, in float64 like the reference;
 * out_type TF_F64 (the function's own result) or TF_F32 (the cast tobac_flow/watershed.py:64-65 applies). */
int tf_edge_field(const double *sobel, const float *field, int64_t n, void *out, int out_type, void *stream);

/* tf_sobel_edge_field: the same result in ONE kernel -- tobac_flow/detection.py:620-642 get_combined_edge_field:
 *   edges = Flow.sobel(field, direction="uphill", method=interp)     (float64 stack, sobel.py:89-143, fill NaN)
 *   edges[edges > 0] += 1;  edges = edges - field;  edges[isnan(field)] = inf;   stored as out_type
 * (TF_F32 rounds the finished value the way watershed.py:64-65 would).  Bit-identical to
 * tf_convolve(func = TF_FUNC_SOBEL_UPHILL, out_type = TF_F64) followed by tf_edge_field; the float64 Sobel volume
 * (8 B written + 8 B read per voxel) is never stored. */
int tf_sobel_edge_field(const float *field, int64_t T, int64_t H, int64_t W, const float *fwd, const float *bwd,
                        int interp, void *out, int out_type, void *stream);

/* ---- a14/a15: semi-Lagrangian marker-controlled watershed -------------------------------------
 * replaces tobac_flow/watershed.py:17-168 (wrapper) and tobac_flow/_watershed.pyx:222-344
 * (watershed_raveled, the reference's only native kernel; compactness = 0, wsl = False).
 *   field    (T, H, W) float32            image values (watershed.py:64-65 coercion is the caller's); a NaN at a
 *            floodable pixel (or at a seed next to one) is TF_EINVAL: the reference's heap order is undefined for NaN
 *   markers  (T, H, W) int32, non-zero = seed (negative allowed)
 *   mask     (T, H, W) int8 or NULL (= all ones)
 *   fwd, bwd (T, H, W, 2) float; rounded half-to-even to integer pixel offsets (watershed.py:121-141); NaN -> 0
 *   nbr_host n_nbr x 3 int8 (dt, dy, dx) neighbour list IN THE REFERENCE'S ORDER
 *            (skimage _offsets_to_raveled_neighbors, watershed.py:114-116)
 *   chain_depth  number of tie-break levels of the pop-order key (>= 1; 3 suffices for tie-free
 *            fields and for the plateau structure of detect_anvils; see DESIGN.md and the contract below)
 *   labels   (T, H, W) int32 out
 * Alignment (tf_version() >= 114): fwd and bwd 8-byte aligned (a flow vector is read as one float2), field and markers
 * 4-byte aligned; anything else is TF_EINVAL before any launch.  Arrays that are also 16-byte aligned (mask: 4-byte) take
 * the four-voxels-per-thread set-up passes; the results do not depend on it.
 * No padding is needed: out-of-volume neighbours are rejected by coordinate tests, which is what
 * the reference's zero-padded mask achieves (watershed.py:111-113).
 * Workspace: the flood keys live in compact arrays over the RELEVANT pixels (floodable pixels +
 * markers that touch one).  tf_watershed_workspace_bytes(..., max_relevant) sizes the workspace for
 * at most that many (0 = worst case T*H*W).  If the volume has more, tf_watershed returns
 * TF_ENOMEM and stats_host[6] holds the exact count to size a retry with.
 * Size limits: voxels are indexed in 64 bits (T < 65536, H, W < 32768, T*H*W <= 2^36) -- a whole long stack can be
 * flooded exactly in one call if it fits the memory; the compact ids are int32: at most 2^30 relevant pixels
 * (TF_EINVAL beyond).  tf_watershed_raveled keeps the reference's int32 strides: at most 2^31 - 1 voxels.
 * stats_host (optional, 8 x int64): [0] sweeps phase A, [1] sweeps root phase (fast path),
 * [2..4] sweeps of the chain phases when the fast path found a label conflict, [5] conflict flag,
 * [6] relevant pixel count.  This call synchronises the stream.
 *
 * EXACTNESS CONTRACT (never a silent wrong label).  After the root phase the library checks, on the device, every
 * pixel whose label was decided by the last-resort rule "smallest root index among candidates that tie on all
 * compared chain levels":
 *   - ties caused only by the cut-off at `chain_depth` levels are removed by computing further levels, up to
 *     `max_depth` (tf_watershed_ex2; tf_watershed / tf_watershed_ex have max_depth = chain_depth).  If some remain:
 *     return TF_EDEPTH (labels are still written);
 *   - ties that remain with COMPLETE chains are ties between EQUAL-VALUED MARKERS.  The reference pushes all markers
 *     with age 0 (_watershed.pyx:278-284), so their pop order is a by-product of its binary heap's array mechanics
 *     (:67-152), which no order-free formulation reproduces.  The library resolves them by push order (raster index
 *     of the marker = the reference's own marker_locations order) and returns TF_WS_AMBIGUOUS (> 0, not an error)
 *     when at least one pixel's LABEL depends on that; tf_watershed_ex2 reports which pixels.
 *   Return TF_OK therefore means: bit-identical to the reference's output for this input, whatever the tie-breaks. */
#define TF_WS_REPLAY_PENDING 2 /* tf_watershed_finish only: exported for a host replay, call tf_watershed_finish again (see there) */
#define TF_WS_AMBIGUOUS 1      /* success; stats[9] pixels carry a label that depends on the order of equal-valued markers */
#define TF_WS_MAX_DEPTH 12     /* largest chain depth (levels of the pop-order key) */
#define TF_WS_NSTATS 16
#define TF_WS_AMB_DEPENDS 1    /* `ambiguous` bits: label depends on a last-resort tie-break ...                        */
#define TF_WS_AMB_MARKER_TIE 2 /* ... the tie arises HERE, between chains that end in equal-valued markers            */
#define TF_WS_AMB_DEPTH 4      /* ... the tie arises HERE because the chains are cut off at the final depth (TF_EDEPTH) */
size_t tf_watershed_workspace_bytes(int64_t T, int64_t H, int64_t W, int n_nbr, int chain_depth,
                                    int64_t max_relevant);
int tf_watershed(const float *field, const int32_t *markers, const int8_t *mask,
                 const float *fwd, const float *bwd, int64_t T, int64_t H, int64_t W,
                 const int8_t *nbr_host, int n_nbr, int chain_depth, int32_t *labels,
                 void *ws, size_t ws_bytes, int64_t *stats_host, void *stream);
/* tf_watershed_ex = tf_watershed + `flags`.
 * TF_WS_SKIP_FAST_PATH: after phase A go straight to the chain phases instead of first trying the
 *   K2-only root phase + exactness check.  The labels are IDENTICAL either way (the fast path is only
 *   taken when no tie-break can matter); the flag is a scheduling hint for inputs known to contain
 *   label conflicts (exact plateaus, as in detect_anvils), where the speculative root phase is wasted
 *   work.  With the flag stats_host[1] = 0 and stats_host[5] = -1 (speculative phase not run). */
#define TF_WS_SKIP_FAST_PATH 1
/* TF_WS_REFERENCE_ORDER (tf_watershed_ex2, tf_watershed_begin, tf_watershed_raveled_ex): when labels hang on the order
 *   of EQUAL-VALUED MARKERS (the case otherwise reported as TF_WS_AMBIGUOUS), reproduce the order the reference's binary
 *   heap gives them.  That order is a by-product of the heap's array mechanics (_watershed.pyx:67-152, 278-284) and depends
 *   on every push and pop before it, so it cannot be derived from the tied markers alone: a first-party host routine of
 *   this library replays the heap's push / pop / sift sequence over the compact flood graph the device has built --
 *   keys only, no labels -- up to the largest marker value at which such a tie occurs, and returns each marker's pop
 *   rank; the device then repeats its root phase with the pop rank in place of the raster index as the last component
 *   of the chain comparison, and writes the labels.  The call returns TF_OK: the labels are the reference's bit for
 *   bit.  Only the heap items at or below that value have to be followed: every other item compares larger than all of
 *   them and only matters through the heap position it occupies, so the replay keeps those "small" items alone (an
 *   occupancy bitmap over the positions + a position -> item table), and the device sends only the seeds among them
 *   (heap position, key, id: 16 B each) and the SUB-GRAPH the replay can reach: the pixels it can pop plus their
 *   out-neighbours (key + neighbour row each; ~1 % of the relevant pixels on a detect_anvils window), through pinned
 *   host memory the library keeps between calls.  Cost: sequential, O(small items x log n) bit tests on one host core;
 *   nothing extra when no such tie exists.  (With more small seeds than relevant pixels -- no staging room -- or
 *   TF_WS_REFERENCE_DENSE=1 in the environment: the dense form, every seed sent and pushed.)
 *   No host pass at all in the commonest case (round 4): when every item at or below that value is a SEED OF THAT ONE
 *   VALUE (no smaller seed, no floodable pixel below it, none of those seeds among the last S heap positions), equal keys
 *   never swap and the reference's build and pops have a closed form -- seed k settles at the first node of its
 *   root-to-k chain no earlier such seed holds, and the seeds leave in the pre-order of the tree they form -- which the
 *   device evaluates itself (k_ws_tie_*: one launch per tree level); TF_WS_REFERENCE_HOST=1 keeps the host replay.
 *   stats[13] = items the replay popped, [14] = seeds the replay was given, [15] = microseconds the detour took on the
 *   host clock (export + replay + repeated root phase; 0 if not needed). */
#define TF_WS_REFERENCE_ORDER 2
/* TF_WS_DEFER_SWEEPS (tf_watershed_begin only; round 5): begin returns after the set-up and the export on a guessed tie value
 * -- the only parts that read `fwd` / `bwd`, `field` and `markers` arrays of the window -- and leaves phase A and the chain
 * levels to tf_watershed_sweeps (or to tf_watershed_finish, which runs them if nobody has).  A caller that begins several
 * windows at once starts all their host replays first and sweeps afterwards (parallel.detect_stack_windows).  Same labels. */
#define TF_WS_DEFER_SWEEPS 4
int tf_watershed_ex(const float *field, const int32_t *markers, const int8_t *mask,
                    const float *fwd, const float *bwd, int64_t T, int64_t H, int64_t W,
                    const int8_t *nbr_host, int n_nbr, int chain_depth, int flags, int32_t *labels,
                    void *ws, size_t ws_bytes, int64_t *stats_host, void *stream);
/* tf_watershed_ex2: the full form.
 *   chain_depth  depth the chain phases start at (when the speculative phase is skipped or rejected)
 *   max_depth    deepest level the call may go to on its own (chain_depth <= max_depth <= TF_WS_MAX_DEPTH); the
 *                workspace must be sized for it: tf_watershed_workspace_bytes(..., max_depth, ...)
 *   ambiguous    (T, H, W) uint8 out or NULL: TF_WS_AMB_* bits per voxel (0 everywhere when the call returns TF_OK)
 *   stats_host   TF_WS_NSTATS x int64 or NULL: [0..7] as above, [8] chain depth the labels were computed at,
 *                [9] pixels whose label depends on a last-resort tie-break, [10] origins of such ties between
 *                equal-valued markers, [11] origins left by the depth cut-off (> 0 <=> TF_EDEPTH), [12] root phases run */
int tf_watershed_ex2(const float *field, const int32_t *markers, const int8_t *mask,
                     const float *fwd, const float *bwd, int64_t T, int64_t H, int64_t W,
                     const int8_t *nbr_host, int n_nbr, int chain_depth, int max_depth, int flags,
                     int32_t *labels, uint8_t *ambiguous, void *ws, size_t ws_bytes,
                     int64_t *stats_host, void *stream);

/* One flood in three parts (round 4): the replay of TF_WS_REFERENCE_ORDER is host work, so the replays of several time
 * windows can run on worker threads while the device floods the next windows.
 *   tf_watershed_begin   set-up, phase A and the chain phases (same arguments as tf_watershed_ex2, no outputs yet).  TF_OK:
 *                        *job_out is a job that MUST be passed to tf_watershed_finish or tf_watershed_abandon; any other
 *                        code: no job.  `ws`, `markers`, `field` and the job belong together until then: the workspace must
 *                        not be used by another call (one workspace per flood in flight).
 *                        guessed_tie_key: -1, or the ordered key (tf_watershed_job_info [7] of an earlier, similar flood) of
 *                        a marker value the caller expects the largest tie between equal-valued markers at.  With
 *                        TF_WS_REFERENCE_ORDER the export of what the replay reads then happens HERE, before the relaxation
 *                        phases (it needs none of their results), the replay can run beside them, and finish runs ONE root
 *                        phase, with the pop ranks.  Any guess is safe: finish compares it with the tie value it finds and
 *                        falls back on export - replay - second root phase when the guess was too low (a guess that is too
 *                        high only makes the replay longer).
 *   tf_watershed_needs_replay   1 if tf_watershed_replay has work to do (a guess was given)
 *   tf_watershed_sweeps  phase A and the chain levels of a job begun with TF_WS_DEFER_SWEEPS (a no-op otherwise); same stream,
 *                        same thread rules as begin / finish; synchronises the stream; stats_host (NULL or TF_WS_NSTATS x int64)
 *                        receives the job's statistics so far ([0] phase A's sweeps, [5] the scheduling probe).  Optional: finish
 *                        runs them if nobody has.  On an error the job stays the caller's to abandon.
 *   tf_watershed_replay  the host replay; no HIP call, any thread, different jobs concurrently.  Optional: finish runs it
 *                        if the caller did not.  MUST have returned before the job is finished or abandoned.
 *   tf_watershed_finish  root phase (with the pop ranks if there are any) + exactness check, labels (and report) written;
 *                        frees the job; return codes and stats of tf_watershed_ex2; info_host: NULL or 12 x int64 as
 *                        tf_watershed_job_info.  Synchronises the stream.
 *                        With TF_WS_REFERENCE_ORDER and labels that hang on the order of equal-valued markers without
 *                        (sufficient) ranks it exports for the tie value it found and returns TF_WS_REPLAY_PENDING (2):
 *                        the job is NOT freed, nothing is written; the caller runs tf_watershed_replay (again: any thread)
 *                        and calls tf_watershed_finish a second time, which uploads the ranks, repeats the root phase and
 *                        completes (it runs the replay itself if the caller did not).
 *   tf_watershed_abandon frees a job without finishing it. */
int tf_watershed_begin(const float *field, const int32_t *markers, const int8_t *mask,
                       const float *fwd, const float *bwd, int64_t T, int64_t H, int64_t W,
                       const int8_t *nbr_host, int n_nbr, int chain_depth, int max_depth, int flags,
                       int64_t guessed_tie_key, void *ws, size_t ws_bytes, int64_t *stats_host, void *stream, void **job_out);
int tf_watershed_needs_replay(const void *job);
int tf_watershed_sweeps(void *job, int64_t *stats_host);
int tf_watershed_replay(void *job);
int tf_watershed_finish(void *job, int32_t *labels, uint8_t *ambiguous, int64_t *stats_host, int64_t *info_host);
void tf_watershed_abandon(void *job);
/* the stream tf_watershed_finish works on (default: the one the job was begun on; everything begin enqueued has completed
 * when begin returns, so any stream is safe): a caller that keeps its main stream busy with other work -- the flow of the
 * next frames -- finishes its floods on a second one instead of queueing the root phase behind that work */
int tf_watershed_set_stream(void *job, void *stream);
/* info (12 x int64): [0] replay form (0 none, 1 sparse, 2 dense, 3 none needed: pop ranks computed on the device in closed
 * form -- every heap item at or below the tie value was a seed of that one value), [1] seeds, [2] seeds at or below the tie value,
 * [3] pixels of the exported sub-graph, [4] relevant pixels, [5] microseconds of the export, [6] microseconds of the
 * replay (-1: not run), [7] ordered key of the largest tie value finish found (-1: no label hangs on such a tie, or not
 * finished), [8] 1 if the export ran on a guess, [9] 1 if the guess covered the tie value, [10] the tie key the export
 * used (-1: none), [11] 1 if the pop ranks came from the device's closed form */
int tf_watershed_job_info(const void *job, int64_t *info);

/* tf_watershed_raveled: the reference's only native seam, argument for argument --
 *   tobac_flow/_watershed.pyx:222-233  watershed_raveled(image, marker_locations, structure, forward_offset,
 *   backward_offset, forward_offset_locations, backward_offset_locations, mask, strides, compactness, output, wsl)
 * as tobac_flow/watershed.py:151-164 calls it (flat, padded, C-contiguous arrays; `output` mutated in place).
 *   image, forward_offset, backward_offset, mask, output, marker_locations: DEVICE arrays (n elements; marker_locations
 *   n_markers int64, strictly ascending = np.flatnonzero order); structure / *_offset_locations / strides: HOST arrays
 *   of n_structure (n_strides) entries.  compactness must be 0 and wsl 0 (the reference's call path); neighbour indices
 *   are range-checked in addition to the mask test.  Exactness contract, return codes and stats as tf_watershed_ex2
 *   (chain depth starts at min(3, max_depth)). */
size_t tf_watershed_raveled_workspace_bytes(int64_t n, int n_structure, int max_depth, int64_t max_relevant);
int tf_watershed_raveled(const float *image, int64_t n, const int64_t *marker_locations, int64_t n_markers,
                         const int64_t *structure_host, int n_structure,
                         const int32_t *forward_offset, const int32_t *backward_offset,
                         const int32_t *forward_offset_locations_host, const int32_t *backward_offset_locations_host,
                         const int8_t *mask, const int32_t *strides_host, int n_strides, double compactness,
                         int32_t *output, int wsl, int max_depth, void *ws, size_t ws_bytes,
                         int64_t *stats_host, void *stream);
/* the same with `flags` (TF_WS_REFERENCE_ORDER) */
int tf_watershed_raveled_ex(const float *image, int64_t n, const int64_t *marker_locations, int64_t n_markers,
                         const int64_t *structure_host, int n_structure,
                         const int32_t *forward_offset, const int32_t *backward_offset,
                         const int32_t *forward_offset_locations_host, const int32_t *backward_offset_locations_host,
                         const int8_t *mask, const int32_t *strides_host, int n_strides, double compactness,
                         int32_t *output, int wsl, int max_depth, int flags, void *ws, size_t ws_bytes,
                         int64_t *stats_host, void *stream);

/* ---- section 8f-2: scipy.ndimage glue of the detection recipes (bit-exact with SciPy) ---------------------
 * tf_binary_morph: scipy.ndimage.binary_erosion (op 0) / binary_dilation (op 1) of a (T, H, W) uint8 volume with a
 *   3x3x3 structuring element (27 host bytes, C order), `iterations` >= 1, `border_value` 0/1
 *   (tobac_flow/detection.py:80-93, 509, 551-553, 571-573, 608-616; binary_opening = erosion then dilation).
 *   tmp: scratch of the same size, required when iterations > 1.
 * tf_linearise: tobac_flow/utils/normalisation_utils.py:36-56 linearise_field in float32.
 * tf_apply_lut: out = lut[labels] (tobac_flow/utils/label_utils.py:265-309 remap_labels' gather). */
/* tf_correlate1d_sym: one pass of scipy.ndimage.correlate1d along `axis` (0 = t, 1 = y, 2 = x) with a SYMMETRIC kernel
 *   of 2*radius+1 host doubles, mode 'reflect' -- the pass scipy.ndimage.gaussian_filter is made of
 *   (tobac_flow/detection.py:65, 137-138, 150: ndi.gaussian_filter(field, (0, sigma, sigma)) = the y pass then the x pass,
 *   each rounding to the array's dtype).  type TF_F32 / TF_F64 (in and out alike); in != out; radius <= 64.
 *   Bit-exact with SciPy: double accumulation, centre first, then the pairs from the OUTERMOST inwards.
 * tf_grey_morph: scipy.ndimage.grey_erosion (op 0) / grey_dilation (op 1) with a flat, point-symmetric footprint inside a
 *   3x3x3 box (27 host bytes, C order), mode 'reflect' (tobac_flow/detection.py:106-108 ndi.grey_opening = erosion then
 *   dilation).  SciPy's visiting order and strict comparisons are kept, so NaNs land where SciPy puts them. */
int tf_correlate1d_sym(const void *in, int type, int64_t T, int64_t H, int64_t W, int axis,
                       const double *weights_host, int radius, void *out, void *stream);
int tf_grey_morph(const void *in, int type, int64_t T, int64_t H, int64_t W, const uint8_t *footprint_host,
                  int op, void *out, void *stream);
int tf_binary_morph(const uint8_t *in, int64_t T, int64_t H, int64_t W, const uint8_t *structure_host,
                    int op, int iterations, int border_value, uint8_t *out, uint8_t *tmp, void *stream);
int tf_linearise(const float *field, int64_t n, double lower, double upper, float *out, void *stream);
int tf_apply_lut(const int32_t *labels, int64_t n, const int32_t *lut, int n_lut, int32_t *out, void *stream);
/* tf_label_filter (version 107): tobac_flow/analysis.py:15-201 -- what find_object_lengths, mask_labels and the
 *   filter_labels_by_* family ask of one int32 (T, H, W) label volume, in ONE read of it: per label id 0 .. n_labels a
 *   record of four int32 (16 B) on the device, records[id * 4 + {0, 1, 2, 3}] = { first leading index, last leading index,
 *   hit bits, 0 }.  Bit k of the hit bits is set when some voxel of the label satisfies criteria[k] (a HOST array of
 *   n_criteria entries, 0 .. 8):
 *     dtype TF_U8            `data` is a byte mask of the volume's shape; satisfied where the byte is not 0 (op, threshold ignored)
 *     dtype TF_F32 / TF_F64  `data` is a field of the volume's shape; satisfied where `field op threshold` holds, op one of
 *                            TF_CMP_GE / GT / LE / LT.  The comparison is made in the field's own type: for TF_F32 the
 *                            threshold is rounded to float first, as NumPy compares a float32 array with a Python float.
 *                            A NaN in the field satisfies nothing.
 *   Criterion operands are read only under voxels whose label lies in [1, n_labels]; ids outside are skipped, so record 0
 *   stays empty.  The call initialises the records itself; a label that does not occur keeps { 0x7fffffff, -1, 0, 0 }, so
 *   it is absent exactly when its last index is -1.  Shape contract: 0 < T < 65536; 64-bit indexing;
 *   `records` 16-byte aligned.  Every value is exact (integer atomics only).  TF_EINVAL before any launch: null pointers,
 *   n_criteria outside 0 .. 8, a criterion without data, an unknown dtype or op, a NaN threshold. */
#define TF_CMP_GE 0
#define TF_CMP_GT 1
#define TF_CMP_LE 2
#define TF_CMP_LT 3
typedef struct { const void *data; int dtype; int op; double threshold; } tf_label_criterion;
int tf_label_filter(const int32_t *labels, int64_t T, int64_t H, int64_t W, int64_t n_labels,
                    const tf_label_criterion *criteria, int n_criteria, int32_t *records, void *stream);
/* the same gather with ids <= 0 passed through (window stitch, tobac_flow/linking.py:153-161: background -1 and 0 keep
 * their value while the positive ids are renumbered) */
int tf_apply_lut_keep_nonpositive(const int32_t *labels, int64_t n, const int32_t *lut, int n_lut, int32_t *out, void *stream);
/* tf_relabel_merge (version 111): tobac_flow/linking.py:246-334 -- relabel_cores_and_anvils of a window product, of the
 *   frames it shares with the previous and the next product, and the two combine_labels, in one read of each source and one
 *   write.  For output frame t and pixel p of the int32 (T, hw) volume `own`:
 *     v = own[t, p]                        r = (v == 0) ? 0 : lut_own[v]
 *     if r == 0 and prev_frame[t] >= 0:    u = prev[prev_frame[t], p];   r = (u == 0) ? 0 : lut_prev[u]
 *     if r == 0 and next_frame[t] >= 0:    u = next[next_frame[t], p];   r = (u == 0) ? 0 : lut_next[u]
 *     out[t, p] = r
 *   Everything is device memory.  The tables are indexed by local id (n_* entries, entry 0 is 0).  prev_frame / next_frame:
 *   int32[T], the frame of the neighbour's (T_prev, hw) / (T_next, hw) volume that shows output frame t, or -1; any order,
 *   repeats allowed.  prev or next may be NULL (its other arguments are then ignored).  out == own (in place) is allowed; out
 *   must not overlap own otherwise, nor prev or next.  Any alignment: 16-byte accesses where own and out are 16-byte aligned,
 *   element accesses otherwise.
 *   status: two uint64 words, zeroed by the call.  status[0] counts the voxels whose CONSULTED id was negative or >= its
 *   table's size (they give 0 and the next source is asked); a neighbour voxel is consulted only where the result so far is
 *   0, so ids under voxels that are never consulted are not checked.  status[1] counts the voxels that asked a frame-table
 *   entry >= T_prev / T_next (treated as -1; nothing is read through it).
 *   TF_EINVAL before any launch: null pointers, T outside 1 .. 65535, hw outside 1 .. 2^30 - 1, more than 2^38 voxels,
 *   an empty table, overlapping buffers. */
int tf_relabel_merge(const int32_t *own, int64_t T, int64_t hw, const int32_t *lut_own, int n_own,
                     const int32_t *prev, int64_t T_prev, const int32_t *prev_frame, const int32_t *lut_prev, int n_prev,
                     const int32_t *next, int64_t T_next, const int32_t *next_frame, const int32_t *lut_next, int n_next,
                     int32_t *out, uint64_t *status, void *stream);
/* tf_field_stats (version 112): tobac_flow/dataset.py:19-148 -- get_bulk_stats, get_spatial_stats, get_temporal_stats of a
 *   contiguous (T, H, W) field of dtype TF_F32 or TF_F64: per slice the number of non-NaN values and their np.nanmean,
 *   np.nanstd (ddof 0), np.nanmedian, np.nanmax, np.nanmin.  The slices, S of them:
 *     TF_FIELD_ALL    everything, S = 1 (any shape, given as T H W values; the median is np.median's: NaN if any value is NaN)
 *     TF_FIELD_FRAME  the H W values of every frame, S = T (all frames in the same launches)
 *     TF_FIELD_TIME   the T values of every pixel, S = H W
 *   count: int64[S].  stats: five planes of S doubles -- mean, std, median, max, min, in the reference's order; a slice
 *   without a non-NaN value gives count 0 and NaN five times.  Count, median, max and min are exact (the median is the mean
 *   of the two middle values computed in the field's dtype, as NumPy computes it, then widened); mean and std are float64
 *   sums combined in an order fixed by the shape (no float atomics: identical bits from run to run), std from a second
 *   sweep of (x - mean)^2.  Infinities follow IEEE arithmetic.  64-bit indices and counts.  TF_FIELD_TIME reads the
 *   volume once while T <= TF_FIELD_STATS_LDS_FRAMES_F32 / _F64 and 19 (float32) or 35 (float64) times beyond; the other
 *   two read it 5 (float32) or 8 (float64) times.  The workspace is used by TF_FIELD_ALL and TF_FIELD_FRAME only.
 *   TF_EINVAL before any launch: null pointers, another dtype, an unknown geometry, an extent < 1, more than 2^40 values,
 *   more than 65535 frames for TF_FIELD_FRAME; TF_ENOMEM: ws_bytes below tf_field_stats_workspace_bytes (0 for bad arguments). */
#define TF_FIELD_ALL 0
#define TF_FIELD_FRAME 1
#define TF_FIELD_TIME 2
#define TF_FIELD_STATS_LDS_FRAMES_F32 64
#define TF_FIELD_STATS_LDS_FRAMES_F64 32
size_t tf_field_stats_workspace_bytes(int dtype, int64_t T, int64_t H, int64_t W, int over);
int tf_field_stats(const void *field, int dtype, int64_t T, int64_t H, int64_t W, int over, int64_t *count, double *stats,
                   void *ws, size_t ws_bytes, void *stream);
/* tf_group_reduce (version 113): tobac_flow/utils/stats_utils.py:171-349, utils/filter_utils.py:33-289 and
 *   postprocess.py:313-1170 -- the per-object reductions of the third stage over N step records.  `ids` (N values, TF_I32
 *   or TF_I64: arbitrary, sparse, in any order) names every record's group; `coord` holds the G group ids, strictly
 *   ascending, in the same type.  A record's group is the rank of its id in `coord`; the members of a group are walked in
 *   the record order of the input (xarray's groupby order), so sums are float64 sums in that order and every result has the
 *   same bits from run to run.  `ops` is a HOST table of 0 .. TF_GROUP_MAX_OPS entries evaluated over the one grouping:
 *     f, w, aux   device columns of N elements; f_dtype / w_dtype / aux_dtype TF_F32, TF_F64 or TF_I64 (below).  Float
 *                 columns are evaluated in float64
 *     out         G elements of 8 bytes on the device: float64, or int64 where marked [i]
 *     TF_GROUP_COUNT                 [i] records of the group (no column)
 *     TF_GROUP_SUM / MEAN            of f skipping NaN (xarray's skipna): all NaN gives 0 / NaN
 *     TF_GROUP_MIN / MAX             of f skipping NaN, NaN when all are; f TF_I64 gives [i]
 *     TF_GROUP_PICK_ARGMIN / ARGMAX  [i] original position of np.argmin / np.argmax of f (float or TF_I64): first
 *                                    occurrence, the first NaN when there is one
 *     TF_GROUP_PICK_IDXMIN / IDXMAX  [i] the same skipping NaN; -1 when all are NaN
 *     TF_GROUP_WEIGHTED_AVERAGE      sum f w / sum w (np.average: NaN propagates); NaN for a zero weight sum
 *     TF_GROUP_COMBINED_MEAN         calc_combined_mean(f = step means, w = step areas), over records with both finite
 *     TF_GROUP_COMBINED_STD          calc_combined_std(f = step stds, aux = step means, w = step areas)
 *     TF_GROUP_AVERAGE_UNCERTAINTY   weighted_average_uncertainty(f = errors, w = weights)
 *     TF_GROUP_FIRST_MINUS_LAST / LAST_MINUS_FIRST   of f in record order; f TF_I64 gives [i]
 *     TF_GROUP_MAX_DIFF              max(np.diff(f)) in record order, 0 for one record; f TF_I64 gives [i]
 *     TF_GROUP_ANY_NAN               [i] 1 when some f is NaN
 *     TF_GROUP_GRADIENT_MIN          min, skipping NaN, of np.gradient(f, aux, edge_order=1) with aux (times, float or
 *                                    TF_I64) converted to float64; NaN for a group of one record
 *     TF_GROUP_GRADIENT_PICK_IDXMIN  [i] original position of that minimum (first occurrence), -1 where there is none
 *   status (device, two uint64): [0] = records whose id is not in `coord` (they join no group), [1] = groups without a
 *   record (their outputs are those of an empty run).  Requires N, G < 2^31 - 2.  TF_EINVAL before any launch: null
 *   pointers, an unknown op or a dtype the op does not take, more than 16 ops; TF_ENOMEM: workspace below
 *   tf_group_reduce_workspace_bytes (0 for sizes out of range). */
#define TF_I64 6         /* tf_group_reduce only: ids, times */
#define TF_GROUP_MAX_OPS 16
#define TF_GROUP_COUNT 0
#define TF_GROUP_SUM 1
#define TF_GROUP_MEAN 2
#define TF_GROUP_MIN 3
#define TF_GROUP_MAX 4
#define TF_GROUP_PICK_ARGMIN 5
#define TF_GROUP_PICK_ARGMAX 6
#define TF_GROUP_PICK_IDXMIN 7
#define TF_GROUP_PICK_IDXMAX 8
#define TF_GROUP_WEIGHTED_AVERAGE 9
#define TF_GROUP_COMBINED_MEAN 10
#define TF_GROUP_COMBINED_STD 11
#define TF_GROUP_AVERAGE_UNCERTAINTY 12
#define TF_GROUP_FIRST_MINUS_LAST 13
#define TF_GROUP_LAST_MINUS_FIRST 14
#define TF_GROUP_MAX_DIFF 15
#define TF_GROUP_ANY_NAN 16
#define TF_GROUP_GRADIENT_MIN 17
#define TF_GROUP_GRADIENT_PICK_IDXMIN 18
typedef struct { int op; int f_dtype; int w_dtype; int aux_dtype; const void *f; const void *w; const void *aux; void *out; } tf_group_op;
size_t tf_group_reduce_workspace_bytes(int64_t N, int64_t G);
int tf_group_reduce(const void *ids, int id_dtype, int64_t N, const void *coord, int64_t G, const tf_group_op *ops, int n_ops,
                    uint64_t *status, void *workspace, size_t workspace_bytes, void *stream);
/* The elementwise glue of detect_anvils' seeds (tobac_flow/detection.py:547-561, 590-617) in two passes:
 * tf_field_masks: ge1 = field >= 1, le0_or_nan = (field <= 0) | isnan(field), isnan_out = isnan(field) as 0 / 1 bytes;
 * tf_merge_seeds: seeds = (bg | isnan) ? -1 : comp. */
int tf_field_masks(const float *field, int64_t n, uint8_t *ge1, uint8_t *le0_or_nan, uint8_t *isnan_out, void *stream);
int tf_merge_seeds(const int32_t *comp, const uint8_t *bg, const uint8_t *isnan_in, int64_t n, int32_t *seeds, void *stream);
/* tf_label: scipy.ndimage.label(input, structure) for a (T, H, W) uint8 volume and a centro-symmetric 3x3x3
 *   structuring element -- used as tobac_flow/utils/label_utils.py:143-180 flat_label (time planes of the structure
 *   zeroed) and for 3-D labelling.  Component numbers follow SciPy (raster order of each component's first pixel).
 *   n_labels_host receives the component count; the call synchronises the stream. */
size_t tf_label_workspace_bytes(int64_t T, int64_t H, int64_t W);
int tf_label(const uint8_t *in, int64_t T, int64_t H, int64_t W, const uint8_t *structure_host,
             int32_t *labels, int *n_labels_host, void *ws, size_t ws_bytes, void *stream);

/* ---- a16: flow-aware labelling (tobac_flow/label.py:84-321) and section 8e/8f-3: cross-window linking ----------
 * tf_pair_counts: for two int32 volumes of n voxels, every distinct pair (a[i], b[i]) with a[i] > 0 and b[i] > 0
 *   (b[i] >= 0 when include_b_zero) and how often it occurs, sorted by (a, b) -- the counting the reference does per
 *   label with np.bincount / np.unique (tobac_flow/utils/label_utils.py:352-376, tobac_flow/linking.py:33-47).
 *   out_a / out_b / out_count: device arrays of max_pairs entries; *n_pairs_host = number of pairs.  The workspace is
 *   sized for at most max_runs runs of equal consecutive pairs (0 = worst case n); with more the call returns
 *   TF_ENOMEM and *n_pairs_host = the run count to size a retry with.  Synchronises the stream.
 * tf_label_sizes: np.bincount(labels) for ids 0 .. n_labels (device int64[n_labels + 1]).
 * tf_flow_link_overlap: tobac_flow/label.py:249-321 -- links per-step labels `flat_labels` (T, H, W) into objects:
 *   nearest-neighbour warps of the labels to t-1 / t+1 (structure * [1, 0, 1]; exactly one tap per outer plane, as the
 *   reference's tuple unpacking requires), overlap counts, the criterion `count > absolute_overlap and count >=
 *   overlap * min(n_locs, size(other))`, and the reference's first-come-first-served grouping in ascending label order
 *   (forward neighbours before backward ones).  out may alias nothing.  *n_objects_host = number of groups opened: the
 *   largest object id, unless ids without pixels follow the last id that has some (each opens a group of its own).
 * tf_flow_label: tobac_flow/label.py:84-175 with subsegment_shrink = 0: flat_label (utils/label_utils.py:143-180 =
 *   scipy.ndimage.label with the structure's t-planes zeroed) followed by the linking above.  mask: (T, H, W) uint8.
 * tf_window_overlap_pairs: tobac_flow/linking.py:49-93 / :96-140 -- `left` / `right` are the labels two consecutive
 *   time windows give to the frames they share (first and last common frame already dropped, linking.py:55-56);
 *   returns on the HOST the (left id, right id) pairs with count >= atol (count > 0 if atol == 0) and, if rtol > 0,
 *   max(count / pixels(left id), count / pixels(right id)) >= rtol; the reference uses atol = 5, rtol = 0.5.
 *   pairs_host: 2 * max_pairs int32.  Connected components of these pairs are the stitched objects (linking.py:153-161). */
/* tf_pair_rank: tobac_flow/utils/label_utils.py:183-200 (`make_step_labels`, the first step of detection.relabel_anvils
 *   :660-687) -- out[i] = 1 + the index of (a[i], b[i]) in the list of distinct pairs (pairs_a, pairs_b: device arrays as
 *   tf_pair_counts returns them, sorted by (a, b)), 0 where a[i] <= 0, b[i] <= 0 or the pair is not listed.  With a = the
 *   pieces of the non-zero mask connected within a time step (tf_label, t planes of the structure zeroed) and b = the
 *   labels this is the reference's numbering: contiguous from 1, by piece, then by original label.  Volumes that are all
 *   16-byte aligned take wide loads; any other (4-byte aligned) views -- labels[1:] with H * W % 4 != 0 -- scalar ones. */
int tf_pair_rank(const int32_t *a, const int32_t *b, int64_t n, const int32_t *pairs_a, const int32_t *pairs_b,
                 int64_t n_pairs, int32_t *out, void *stream);
size_t tf_pair_counts_workspace_bytes(int64_t n, int64_t max_runs);
int tf_pair_counts(const int32_t *a, const int32_t *b, int64_t n, int include_b_zero,
                   int32_t *out_a, int32_t *out_b, int64_t *out_count, int64_t max_pairs,
                   int64_t *n_pairs_host, void *ws, size_t ws_bytes, void *stream);
int tf_label_sizes(const int32_t *labels, int64_t n, int64_t n_labels, int64_t *sizes, void *stream);
size_t tf_flow_link_workspace_bytes(int64_t T, int64_t H, int64_t W, int64_t max_runs);
int tf_flow_link_overlap(const int32_t *flat_labels, const float *fwd, const float *bwd,
                         int64_t T, int64_t H, int64_t W, const uint8_t *structure_host,
                         double overlap, int64_t absolute_overlap, int32_t *out, int *n_objects_host,
                         void *ws, size_t ws_bytes, void *stream);
size_t tf_flow_label_workspace_bytes(int64_t T, int64_t H, int64_t W, int64_t max_runs);
int tf_flow_label(const uint8_t *mask, const float *fwd, const float *bwd, int64_t T, int64_t H, int64_t W,
                  const uint8_t *structure_host, double overlap, int64_t absolute_overlap,
                  int32_t *labels, int *n_objects_host, void *ws, size_t ws_bytes, void *stream);
int tf_window_overlap_pairs(const int32_t *left, const int32_t *right, int64_t n, int64_t atol, double rtol,
                            int32_t *pairs_host, int64_t max_pairs, int64_t *n_pairs_host,
                            void *ws, size_t ws_bytes, void *stream);

/* tf_slice_labels: tobac_flow/utils/label_utils.py:312-349 (`slice_labels`, the `*_step_label` variables of the output
 *   files, tobac_flow/dataset.py:189-229): one id per (label, time step) of an int32 (T, hw) label volume -- the pieces of
 *   a label inside one step stay together -- numbered densely from 1 in ascending (step, label) order; 0 (and anything
 *   negative) stays 0.  (As in the reference, a volume in which NO voxel is 0 loses its smallest shifted id to 0: the
 *   dense LUT is np.arange over the ids that occur.)  *n_step_labels_host = the largest id written.  The workspace holds two int32 per shifted id (sum over
 *   steps of the step's largest label, `id_capacity`); if it is too small the call returns TF_ENOMEM with
 *   *n_step_labels_host = the capacity to size a retry with.  Synchronises the stream. */
/* tf_label_stats: tobac_flow/analysis.py:293-376 (`weighted_statistics_on_labels`) and :204-245 (`get_stats_for_labels`,
 *   weights == NULL: every weight 1) -- per label id 1 .. n_labels of an int32 volume of n voxels, over the voxels whose
 *   `field` value is not NaN: out[(id - 1) * 6 + {0..5}] = { sum of all (non-NaN) weights of the label, sum of the weights
 *   at valued voxels, weighted mean, weighted standard deviation about it (sqrt(sum w (x - mean)^2 / sum w)), max and min
 *   of the values with weight > 0 } as doubles on the device (NaN where undefined).  Sums are accumulated in double. */
size_t tf_label_stats_workspace_bytes(int64_t n_labels);
int tf_label_stats(const int32_t *labels, const float *field, const float *weights, int64_t n, int64_t n_labels,
                   double *out, void *ws, size_t ws_bytes, void *stream);
/* tf_label_props: tobac_flow/dataset.py:705-1595 (`calculate_label_properties`) -- everything that function derives from
 *   ONE int32 (T, H, W) label volume, in one read of it: per label id 0 .. n_labels a record of 8 doubles (64 B) on the
 *   device, acc[id * 8 + k]:
 *     k = 0  number of voxels, stored as an int64 (np.bincount)
 *     k = 1  sum of area[y, x] over the voxels whose area is not NaN (labeled_comprehension(area, np.nansum))
 *     k = 2  sum of area[y, x], NaN propagating (the denominator of np.average(..., weights=area))
 *     k = 3 .. 6  sum of area * x[x], area * y[y], area * lat[y, x], area * lon[y, x], NaN propagating
 *     k = 7  two int32: the smallest and the largest t_rank[t] of the label's frames (0x7fffffff / -1 where it has none)
 *   area, lat, lon: (H, W) doubles; x: (W,), y: (H,) doubles; t_rank: (T,) int32 >= 0 -- the operands as they are, never
 *   broadcast to the volume; besides the labels nothing of T * H * W elements is read or allocated.  A NULL operand
 *   switches its sums off (they stay 0; NULL area switches k = 1 .. 6 off, NULL t_rank k = 7).  Ids outside
 *   [1, n_labels] are skipped, so record 0 stays empty.  Shape contract: 0 < T < 65536; 64-bit indexing.
 *   The sums are double atomics, one set per run of equal labels inside a lane's 16 voxels of a row: as with
 *   tf_label_stats the last bits of a sum depend on arrival order and can differ from run to run (N terms: N * 2^-53
 *   relative for terms of one sign); counts and the two ranks are exact. */
int tf_label_props(const int32_t *labels, int64_t T, int64_t H, int64_t W, int64_t n_labels,
                   const double *area, const double *x, const double *y, const double *lat, const double *lon,
                   const int32_t *t_rank, double *acc, void *stream);
/* tf_unique_along_t / tf_unique_per_frame: tobac_flow/utils/stats_utils.py:23-30 (`n_unique_along_axis`, which equals the
 *   number of DISTINCT NON-ZERO values along the axis) together with np.count_nonzero, as tobac_flow/analysis.py:245-290
 *   (`get_label_stats`) uses them.  Both are exact.
 *   along t: per pixel of an int32 (T, H, W) volume, unique[H * W] and nonzero[H * W] (int32).  Any int32 values.  The
 *     per-pixel set of values met so far has room for T entries; it lives in LDS for T <= 640 (*lanes_host = pixels per
 *     workgroup, 256 / 128 / 64) and otherwise in the workspace (T * H * W int32, *lanes_host = 0);
 *     tf_unique_along_t_workspace_bytes returns 0 when none is needed.
 *   per frame: per frame of an int32 (T, hw) volume, unique[T] (int32) = distinct ids in [1, n_labels] and nonzero[T]
 *     (int64) = voxels != 0.  The workspace holds one int32 per id. */
size_t tf_unique_along_t_workspace_bytes(int64_t T, int64_t H, int64_t W);
int tf_unique_along_t(const int32_t *vol, int64_t T, int64_t H, int64_t W, int32_t *unique, int32_t *nonzero,
                      int *lanes_host, void *ws, size_t ws_bytes, void *stream);
size_t tf_unique_per_frame_workspace_bytes(int64_t n_labels);
int tf_unique_per_frame(const int32_t *vol, int64_t T, int64_t hw, int64_t n_labels, int32_t *unique, int64_t *nonzero,
                        void *ws, size_t ws_bytes, void *stream);
/* tf_label_wstats: tobac_flow/utils/stats_utils.py:33-154 (`weighted_average_and_std`, `weighted_stats`,
 *   `weighted_average_uncertainty`, `weighted_uncertainties`, `weighted_stats_and_uncertainties`) applied to every label by
 *   tobac_flow/utils/label_utils.py:58-140 (`apply_func_to_labels`), as tobac_flow/postprocess.py:102-242
 *   (`weighted_label_stats`, `add_weighted_stats_to_dataset`) calls them.  labels: int32 (T, hw); field, errors (or NULL)
 *   and weights: all float32 (dtype TF_F32) or all float64 (TF_F64), nothing is cast down; weights are (T, hw), or with
 *   weights_plane != 0 ONE (hw,) plane shared by every frame (the scripts' np.repeat(area[None], T, 0), never
 *   materialised).  Per label id 1 .. n_labels, over F = its voxels with a finite field value,
 *   out[(id - 1) * 10 + k] as doubles on the device:
 *     k = 0  n = |F|                         k = 1  sum of w over F (NaN if one of them is NaN)
 *     k = 2  mean = sum w x / sum w          k = 3  std = sqrt(sum w (x - mean)^2 / sum w / c), c = 1 - sum w^2 / (sum w)^2,
 *                                                   NaN where c < 0 or 0 / 0 (one weighted voxel), inf where a / 0
 *     k = 4  min of x over F                 k = 5  max of x over F   (weight-0 voxels included)
 *     k = 6  sqrt(sum w^2 e^2) / sum w       k = 7  sqrt((std / sqrt(n))^2 + [6]^2)
 *     k = 8  e at the voxel of the minimum   k = 9  e at the voxel of the maximum
 *   k = 2 .. 9 are NaN unless n > 0 and sum w > 0; k = 6 .. 9 are NaN when errors == NULL.  Where the extreme occurs more
 *   than once the voxel with the smallest raveled index is taken (the reference's unstable argsort leaves it undefined);
 *   -0.0 and +0.0 compare equal.  Two reads of labels, field and weights (the errors once, only under labelled voxels) and
 *   a finish per label; sums are double atomics, one set per run of equal labels a lane meets, so their last bits depend
 *   on arrival order (N terms of one sign: N * 2^-53 relative); n, min, max and the two selected errors are exact.  Ids
 *   outside [1, n_labels] are background.  64-bit indexing throughout.  The workspace holds 128 B per label. */
size_t tf_label_wstats_workspace_bytes(int64_t n_labels);
int tf_label_wstats(const int32_t *labels, const void *field, const void *errors, const void *weights, int dtype,
                    int64_t T, int64_t hw, int weights_plane, int64_t n_labels, double *out, void *ws, size_t ws_bytes,
                    void *stream);
/* tf_label_proportions: tobac_flow/utils/stats_utils.py:157-168 (`get_weighted_proportions`) per label
 *   (tobac_flow/postprocess.py:245-310).  labels, flags: int32 (T, hw); weights: float32, volume or plane as above;
 *   flag_values_host: n_flags <= 64 DISTINCT int32 values in host memory.  out[(id - 1) * n_flags + k] = (sum of the
 *   label's non-NaN weights where flag == value k) / (sum of all its non-NaN weights), NaN for every k unless that total
 *   is > 0; a flag that is not listed counts towards the total only.  One read of the volume and a finish; one or two
 *   double atomics per run of equal (label, flag) pairs.  The workspace holds 1 + n_flags doubles per label. */
size_t tf_label_proportions_workspace_bytes(int64_t n_labels, int n_flags);
int tf_label_proportions(const int32_t *labels, const int32_t *flags, const float *weights, int64_t T, int64_t hw,
                         int weights_plane, int64_t n_labels, const int32_t *flag_values_host, int n_flags, double *out,
                         void *ws, size_t ws_bytes, void *stream);
/* tf_flux_cre (version 119, as tf_quality_weights and tf_label_wstats_multi): tobac_flow/postprocess.py:29-99 (`get_cre`, `add_cre_to_dataset`) in one launch.  planes_host: 13 device
 *   pointers in host memory -- toa_swdn, toa_swup, toa_swup_clr, toa_lwup, toa_lwup_clr, boa_swdn, boa_swup, boa_lwdn,
 *   boa_lwup, boa_swdn_clr, boa_swup_clr, boa_lwdn_clr, boa_lwup_clr -- of n elements each, all TF_F32 or all TF_F64;
 *   out_host: 10 device pointers, the reference's order of insertion -- toa_swup_cre, toa_lwup_cre, boa_swdn_cre,
 *   boa_swup_cre, boa_lwdn_cre, boa_lwup_cre, toa_net, toa_net_cre, boa_net, boa_net_cre.  Evaluated in the reference's
 *   tree, every operation rounded in the planes' type: cre = flux - clr; toa_net = swdn - (swup + lwup);
 *   toa_net_cre = -(swup_cre + lwup_cre); boa_net = swdn + lwdn - (swup + lwup); boa_net_cre = swdn_cre + lwdn_cre -
 *   (swup_cre + lwup_cre).  Additions, subtractions and a negation only: NumPy's values, NaN placement included.  No
 *   output may overlap an input.  Each plane is read once and each result written once. */
int tf_flux_cre(const void *const *planes_host, void *const *out_host, int dtype, int64_t n, void *stream);
/* tf_quality_weights: scripts/postprocess_seviri_nat_dcc.py:181-186.  out[t][p] = weights * (qcflag == 0) * (cth < 30) *
 *   isfinite(cot), the factors 0 or 1, multiplied in that order in the weights' type (weight_dtype TF_F32 / TF_F64, also
 *   the type of out): a NaN or infinite weight times 0 is NaN, a NaN cth compares false.  weights: (T, hw), or with
 *   weights_plane != 0 ONE (hw,) plane; qcflag: int32 (T, hw); cth, cot: (T, hw), both field_dtype TF_F32 / TF_F64. */
int tf_quality_weights(const void *weights, int weight_dtype, int weights_plane, const int32_t *qcflag, const void *cth,
                       const void *cot, int field_dtype, int64_t T, int64_t hw, void *out, void *stream);
/* tf_label_wstats_multi: tf_label_wstats for a whole SET of fields over one int32 (T, hw) label volume: two passes over
 *   the labels and one finish for all of them.  out[(f * n_labels + id - 1) * 10 + k], k = 0 .. 9 as tf_label_wstats
 *   defines them, f the field's position in its set:
 *     TF_FIELDS_PLAIN  n_planes = 1 .. 8 planes, the fields are the planes; errors_host: NULL, or n_planes pointers of which
 *                      each may be NULL (k = 6 .. 9 NaN for that field)
 *     TF_FIELDS_TOA    5 planes toa_swdn, toa_swup, toa_swup_clr, toa_lwup, toa_lwup_clr; 7 fields toa_swdn, toa_swup,
 *                      toa_swup_cre, toa_lwup, toa_lwup_cre, toa_net, toa_net_cre
 *     TF_FIELDS_BOA    8 planes boa_swdn, boa_swup, boa_lwdn, boa_lwup and their _clr planes in that order; 10 fields
 *                      boa_swdn, boa_swdn_cre, boa_swup, boa_swup_cre, boa_lwdn, boa_lwdn_cre, boa_lwup, boa_lwup_cre,
 *                      boa_net, boa_net_cre
 *   (the field orders are those of scripts/postprocess_seviri_nat_dcc.py:274-291; errors_host must be NULL for TOA and BOA).
 *   planes_host / errors_host: device pointers in host memory.  The derived fields are formed per voxel in registers by
 *   tf_flux_cre's own expressions in the field type: the derived volumes never exist.  field_dtype (planes and errors)
 *   and weight_dtype are TF_F32 or TF_F64 independently of each other; nothing is copied or cast, sums are accumulated in
 *   double.  weights: (T, hw), or with weights_plane != 0 ONE (hw,) plane.
 *   Every field has its OWN finite mask: a voxel counts for a field where THAT field's value is finite (a NaN in
 *   toa_swup_clr leaves toa_swup untouched and drops the voxel from toa_swup_cre and toa_net_cre).  Everything else is
 *   tf_label_wstats's rule field by field: min and max include weight-0 voxels, a NaN weight at a finite value makes the
 *   field's label NaN, the smallest raveled index wins among tied extremes, -0.0 equals +0.0, ids outside [1, n_labels]
 *   are background, 64-bit indexing.  Labels, weights and every input plane are read once per pass, the planes only in
 *   steps that hold a labelled voxel; errors are read by element under labelled voxels.  n, min, max and the selected
 *   errors are exact, the sums as tf_label_wstats's.  The workspace holds 128 B per field and label. */
#define TF_FIELDS_PLAIN 0
#define TF_FIELDS_TOA 1
#define TF_FIELDS_BOA 2
size_t tf_label_wstats_multi_workspace_bytes(int set, int n_planes, int64_t n_labels);
int tf_label_wstats_multi(const int32_t *labels, int set, const void *const *planes_host, const void *const *errors_host,
                          int n_planes, const void *weights, int field_dtype, int weight_dtype, int64_t T, int64_t hw,
                          int weights_plane, int64_t n_labels, double *out, void *ws, size_t ws_bytes, void *stream);
/* tf_label_reduce (version 110): what tobac_flow/utils/label_utils.py:8-55 (`labeled_comprehension`) and :58-140
 *   (`apply_func_to_labels`) need of a region when `func` is a plain NumPy reducer, for every label id of the span
 *   [id_lo, id_hi] in one read of the volume.  labels: int32 (T * hw,); ids outside the span are background, 0 and
 *   negative ids inside it are regions like any other (ndi.labeled_comprehension accepts them in `index`).  field: TF_U8
 *   (bool), TF_I32, TF_F32 or TF_F64, nothing is cast down, in one of three layouts that are never materialised:
 *     layout 0  a volume (T * hw,)      layout 1  ONE (hw,) plane shared by every frame (area[None])
 *     layout 2  ONE value per frame, (T,) (bt.t.data[:, None, None])
 *   records: (id_hi - id_lo + 1) records of eight 64-bit words (64 B, one line) on the device, record id - id_lo:
 *     0  int64 number of voxels            1  int64 number of voxels whose value is not NaN
 *     2  int64 number of voxels whose value is != 0 (NaN counts, as np.any / np.count_nonzero see it)
 *     3  sum of the non-NaN values: double for TF_F32 / TF_F64, int64 for TF_U8 / TF_I32
 *     4  key of the smallest non-NaN value, 5 of the largest: k(x) = bits of (x + 0.0) as double, all bits inverted where
 *        the sign is set, else the sign bit set; unsigned order = order of the values, +-inf take part, -0.0 and +0.0 share
 *        a key.  Without a non-NaN value slot 4 is 2^64 - 1 and slot 5 is 0
 *     6  sum of (x - mean)^2 over the non-NaN values, double, mean = slot 3 / slot 1; written only with want & 1 (a finish
 *        per label and a second read of labels and field: NumPy's two-pass form), else 0        7  spare, 0
 *   Exact and independent of arrival order: slots 0, 1, 2, 4, 5 and the int64 slot 3 (integer atomics).  The double slot 3
 *   and slot 6 are double atomics, one per run of equal labels a lane meets, so their last bits depend on arrival order:
 *   N terms differ from the exactly rounded sum by at most N * 2^-53 * sum |term|.  inf + (-inf) gives NaN as in NumPy.
 *   16 voxels per lane, background lanes load the labels only, wide loads where base and layout are 16-byte aligned,
 *   64-bit indexing throughout.  Limits: id_hi - id_lo < 2^27 (8 GiB of records), INT32_MIN < id_lo <= id_hi <= INT32_MAX;
 *   beyond them TF_EINVAL before any launch.  The workspace (needed with want & 1 only) holds one double per id.
 * tf_label_order (version 110): the order statistics np.median / np.nanmedian need, same operands and span.  records:
 *   what tf_label_reduce left for these operands; n_keys: the sum of their slot 1 (the caller has downloaded them).
 *   out[2 * (id - id_lo)], out[.. + 1] (double, device) = the two middle values of the id's non-NaN values in ascending
 *   order, elements (c - 1) / 2 and c / 2 of c; equal for an odd c, NaN for c = 0.  Exact.  Slot-1 counts -> exclusive scan
 *   -> every non-NaN voxel of the span puts a 32-bit order key (64-bit for TF_F64) into its label's segment through one
 *   atomic cursor per label -> rocPRIM segmented radix sort -> pick.  A zero comes back as +0.0.  Records that do not
 *   belong to the operands are not trusted for any address: places beyond a segment or n_keys are not written or read.
 *   n_keys <= 2^31 - 1.  The workspace scales with n_keys and the span, not with the volume (a span that contains 0
 *   makes the background a region and n_keys the volume). */
size_t tf_label_reduce_workspace_bytes(int64_t id_lo, int64_t id_hi);
int tf_label_reduce(const int32_t *labels, const void *field, int dtype, int layout, int64_t T, int64_t hw, int64_t id_lo,
                    int64_t id_hi, int want, void *records, void *ws, size_t ws_bytes, void *stream);
size_t tf_label_order_workspace_bytes(int64_t id_lo, int64_t id_hi, int64_t n_keys, int dtype);
int tf_label_order(const int32_t *labels, const void *field, int dtype, int layout, int64_t T, int64_t hw, int64_t id_lo,
                   int64_t id_hi, const void *records, int64_t n_keys, double *out, void *ws, size_t ws_bytes, void *stream);
size_t tf_slice_labels_workspace_bytes(int64_t T, int64_t id_capacity);
int tf_slice_labels(const int32_t *labels, int64_t T, int64_t hw, int32_t *out, int64_t *n_step_labels_host,
                    void *ws, size_t ws_bytes, void *stream);

/* ---- GLM validation: tobac_flow/validation.py (scripts/dcc_validation.py:145-250) ------------------------------------
 * tf_edt2d_frames: scipy.ndimage.distance_transform_edt(frame == 0) for every frame of a (T, H, W) volume (validation.py:
 *   24-36, 52-104), exact and in integers.  A voxel is a FEATURE when its value is != 0 (NaN is one, as NaN == 0 is false
 *   in NumPy).  vol: TF_U8 (bool), TF_I32, TF_F32 or TF_F64.  d2[t][y][x] = int32 squared distance to the nearest feature
 *   of frame t; nearest[t][y][x] (may be NULL) = y' * W + x' of such a feature.  A frame without a feature gets INT32_MAX
 *   and -1.  (H - 1)^2 + (W - 1)^2 < 2^31 is required.  Distances are unique; where several features are equally near
 *   the one with the smallest |x' - x| is reported, of two at the same |x' - x| the left one, within a column the upper
 *   one -- the order of the scan, the same in every run (SciPy's choice follows its Voronoi sweep and is not reproduced).
 *   A column pass (one lane per column, down and up) and a row pass (one workgroup per row, the row's column distances in
 *   LDS, a scan outward from every pixel that stops at dx^2 >= best).  Frames are processed in chunks: the workspace
 *   holds one int32 per voxel of a chunk (two where W > 16384, beyond the LDS form) and stays <= 1 GiB unless one frame
 *   needs more.
 * tf_edt_cylinder: validation.py:52-104 get_marker_distance_cylinder from the two arrays above.  dist[t][p] (double) =
 *   sqrt of the smallest d2[k][p] over k = max(t - time_margin, 0) .. min(t + time_margin, T - 1), +inf where all of them
 *   are INT32_MAX; src[t][p] (int64, may be NULL; needs nearest) = k * hw + nearest[k][p] for the EARLIEST k that holds the
 *   minimum (np.nanargmin), -1 where there is none.  The double square root is correctly rounded (= np.sqrt).
 * tf_edt_time_envelope (version 105): scipy.ndimage.distance_transform_edt with sampling = (sampling_t, 1, 1) of the whole
 *   (T, H, W) volume (validation.py:39-49 get_marker_distance_ellipse) from the same two arrays: the lower envelope along t
 *   of (sampling_t * dt)^2 + d2[k][p].  In float64, a = fl((k - t) * sampling_t), A = fl(a * a), key_k = fl(A + d2[k][p]);
 *   the winner is the k of the smallest key, of equal keys the one with the smaller |k - t|, then the earlier frame.
 *   dist[t][p] (double) = sqrt(fl(fl(A + dy * dy) + dx * dx)) with (dy, dx) from nearest[k][p]: SciPy's own expression for
 *   that feature, so the value equals SciPy's wherever the nearest feature is unique; +inf where no frame has a feature.
 *   src[t][p] (int64, may be NULL; needs nearest) = k * H * W + nearest[k][p], -1 where there is none.  nearest == NULL
 *   (then src must be NULL): dist = sqrt(key), which is not SciPy's summation order.  sampling_t must be finite and > 0,
 *   the shape one that tf_edt2d_frames accepts.  No workspace, no atomics; T * H * W may exceed 2^31.
 * tf_label_nanmin: np.nanmin of a field over every label (label_utils.py:58-140 apply_func_to_labels with func=np.nanmin,
 *   validation.py:13-21, 144-152).  labels: int32 (n,); field: TF_U8, TF_F32 or TF_F64 (n,); ids: n_ids int64 label ids on
 *   the device.  out_min[k] (double) = the minimum over the voxels of ids[k] that are not NaN, NaN where it has none;
 *   out_count[k] (int64) = the number of those voxels, -1 where the label has no voxel at all or the id lies outside
 *   [1, n_labels] (the caller's `default`).  One read of labels and field: 64-bit atomicMin on an order-preserving key,
 *   one per run of equal labels a lane meets, the runs its lanes still hold at the end combined across the wave where they
 *   agree on the label; minimum and integer count do not depend on arrival order.  -0.0 and +0.0 compare equal
 *   (+0.0 is returned).  The workspace holds 16 B per label. */
size_t tf_edt2d_frames_workspace_bytes(int64_t T, int64_t H, int64_t W);
int tf_edt2d_frames(const void *vol, int dtype, int64_t T, int64_t H, int64_t W, int32_t *d2, int32_t *nearest, void *ws,
                    size_t ws_bytes, void *stream);
int tf_edt_cylinder(const int32_t *d2, const int32_t *nearest, int64_t T, int64_t hw, int64_t time_margin, double *dist,
                    int64_t *src, void *stream);
int tf_edt_time_envelope(const int32_t *d2, const int32_t *nearest, int64_t T, int64_t H, int64_t W, double sampling_t,
                         double *dist, int64_t *src, void *stream);
size_t tf_label_nanmin_workspace_bytes(int64_t n_labels);
int tf_label_nanmin(const int32_t *labels, const void *field, int dtype, int64_t n, int64_t n_labels, const int64_t *ids,
                    int64_t n_ids, double *out_min, int64_t *out_count, void *ws, size_t ws_bytes, void *stream);

/* ---- the validation stage at the flashes only (version 118): validation.py:107-219, scripts/dcc_validation.py:145-250 ----
 * tf_flash_count / tf_flash_list: np.repeat(np.arange(n), grid.astype(int).ravel()) -- the raveled voxel of every flash, in
 *   order -- for a flash-count grid of n voxels, dtype TF_F32, TF_F64 or TF_I32.  A count is truncated toward zero (2.9 -> 2).
 *   tf_flash_count sums the counts per tile of tf_flash_tile() voxels, scans the tile sums into 64-bit offsets (left in the
 *   workspace) and hands two words to the host, synchronising the stream once: *total_host = the number of flashes,
 *   *bad_host = 0, or bit 0 set where some count is < 0 or NaN (tested before truncation, as np.repeat refuses it) and bit 1
 *   where some count is >= 2^31 (the list is then not defined and tf_flash_list must not be called).  tf_flash_list, with the same grid and workspace,
 *   writes voxel[n_flashes] (int64), n_flashes = that total: only tiles that hold a flash are read again, and the flashes of
 *   a tile are written by all lanes of its workgroup, each searching the tile's prefix sums for its voxel, however many
 *   flashes one voxel holds.  Integer sums throughout: the list is the same in every run.
 * tf_edt_cylinder_at: tf_edt_cylinder at the n voxels of a list instead of everywhere.  d2 / nearest: tf_edt2d_frames' of the
 *   TF_I32 volume `markers` (T, hw).  For flash i at voxel[i] = t * hw + p: dist[i] (double) = the correctly rounded sqrt of the
 *   smallest d2[k][p] over k = max(t - time_margin, 0) .. min(t + time_margin, T - 1), +inf where every one is INT32_MAX;
 *   closest[i] (int64, may be NULL; needs nearest and markers) = markers[k * hw + nearest[k][p]] for the EARLIEST k that holds
 *   the minimum, 0 where there is none: tf_edt_cylinder's dist gathered at voxel, and markers gathered at its src.
 *   *n_within (int64, on the device) = the number of i with dist[i] <= margin, compared in double, accumulated in integers.
 *   A voxel outside [0, T * hw) gets +inf and 0.  No workspace and no volume-sized output.
 * tf_grid_has_missing: *flag (int32, on the device) = 1 where some voxel of the grid (TF_F32, TF_F64, TF_I32) equals -1, else
 *   0; NaN is not -1.  One read of the grid.
 * tf_edge_filter: validation.py:173-219 get_edge_filter as a (T, H, W) byte mask.  0 within time_margin frames of either end
 *   and within margin pixels of the four borders (as NumPy's a[:k] = a[-k:] = False: everything for k == 0), in the frames
 *   where frame_off[t] != 0 (T bytes on the device, may be NULL: the frames around a time gap, computed by the host as
 *   validation.py:185-193 does), and, with has_missing != 0, where scipy.ndimage.binary_dilation of grid == -1 with the
 *   reference's structure reaches: output (t, y, x) is cleared exactly when some voxel (k, y - dy, x - dx) equals -1 with
 *   |k - t| <= time_margin, |dy|, |dx| <= margin and (dx + margin - 10)^2 + (dy + margin - 10)^2 < margin^2 (a disc around the
 *   reference's hard-coded index 10 in a box whose origin is margin; margin 3 gives an empty structure, margin 10 the centred
 *   open disc).  Per chunk of frames: the OR over the time window and its prefix count along every row go to the workspace
 *   (4 B per voxel of the chunk, <= 1 GiB unless one frame needs more), then every voxel still set looks up one span per
 *   row of the footprint.  has_missing == 0 (what tf_grid_has_missing found): the grid is not read and no workspace is
 *   needed.  margin <= 4000. */
int tf_flash_tile(void);
size_t tf_flash_workspace_bytes(int64_t n);
int tf_flash_count(const void *grid, int dtype, int64_t n, void *ws, size_t ws_bytes, int64_t *total_host, int *bad_host,
                   void *stream);
int tf_flash_list(const void *grid, int dtype, int64_t n, void *ws, size_t ws_bytes, int64_t *voxel, int64_t n_flashes,
                  void *stream);
int tf_edt_cylinder_at(const int32_t *d2, const int32_t *nearest, const int32_t *markers, int64_t T, int64_t hw,
                       int64_t time_margin, const int64_t *voxel, int64_t n, double margin, double *dist, int64_t *closest,
                       int64_t *n_within, void *stream);
int tf_grid_has_missing(const void *grid, int dtype, int64_t n, int32_t *flag, void *stream);
size_t tf_edge_filter_workspace_bytes(int64_t T, int64_t H, int64_t W, int has_missing);
int tf_edge_filter(const void *grid, int dtype, int64_t T, int64_t H, int64_t W, int64_t margin, int64_t time_margin,
                   const uint8_t *frame_off, int has_missing, uint8_t *out, void *ws, size_t ws_bytes, void *stream);

/* ---- subsegment_labels: tobac_flow/label.py:13-80 (version 106) -----------------------------------------------------------
 * The per-voxel passes between tf_label / tf_edt2d_frames / tf_label_sizes and the per-frame tf_watershed of the recipe
 * (tobac_flow_amd/label.py subsegment_labels).
 * tf_subseg_prepare: label.py:52-56.  labels: int32 (n,) per-step labels, 0 = background; d2: int32 (n,) squared in-plane
 *   distance to the nearest background voxel (tf_edt2d_frames of labels == 0); counts: int64[n_labels + 1] on the device
 *   (tf_label_sizes).  dist_mask[i] (double) = sqrt(d2[i]) / sqrt(counts[labels[i]] / pi): two correctly rounded square
 *   roots and one division, nothing fused and no reciprocal, so the value equals numpy's bit for bit.  shrunk[i] (uint8)
 *   = dist_mask[i] > shrink_factor.  A label outside [0, n_labels] is written as background (0 and 0).  One pass, 64-bit
 *   indexed, four voxels per lane where the arrays are 16-byte aligned.
 * tf_subseg_rank: the flood key of one frame.  values: double (n,); sorted_keys: the n_keys DISTINCT values of `values`,
 *   ascending, on the device.  rank[i] (float) = n_keys - 1 - (index of values[i] in sorted_keys) = the rank of
 *   -values[i] among the frame's distinct -values: a strictly order-preserving map of the float64 key the reference
 *   floods, exact in float32.  TF_EINVAL when n_keys > 2^24 (nothing is launched).  Binary search, 64-bit indexed; a value
 *   that is not a key gets the rank of the first key not below it. */
int tf_subseg_prepare(const int32_t *labels, const int32_t *d2, const int64_t *counts, int64_t n_labels, int64_t n,
                      double shrink_factor, double *dist_mask, uint8_t *shrunk, void *stream);
int tf_subseg_rank(const double *values, int64_t n, const double *sorted_keys, int64_t n_keys, float *rank, void *stream);

/* ---- point observations onto a grid: np.histogramdd / scipy.stats.binned_statistic_dd (version 108) ---------------------
 * The array-level binning of tobac_flow/glm.py:77-145 (np.histogram2d per frame), tobac_flow/nexrad.py:80-231 (two
 * np.histogram2d and one binned_statistic_dd per site and frame) and scripts/grid_flux.py:65-112 (two binned_statistic_2d
 * sums per variable): ONE pass over n_points points gives every output.  All pointers except the struct itself are
 * device pointers; a NULL optional pointer switches its part off.
 *   coord[d], d < n_dims (1 .. 3): n_points coordinates each, all TF_F32 or all TF_F64 (coord_dtype); float32 is widened
 *     exactly.  coord[0] is the slowest output axis.
 *   edges[d]: n_edges[d] >= 2 non-decreasing doubles (the caller checks the order), arbitrary, not uniform.
 *   bin: k = upper_bound(edges, v) - 1 = searchsorted(edges, v, side="right") - 1; the point is kept if 0 <= k <
 *     n_edges - 1 on every axis.  Always the search's answer (a guess from the mean step is only verified against the edges).
 *   rule = TF_BIN_RULE_NUMPY (np.histogramdd): v == edges[last] belongs to the last bin; any other v >= edges[last], +-inf
 *     and NaN are dropped silently.
 *   rule = TF_BIN_RULE_SCIPY (scipy.stats._binned_statistic._bin_numbers, SciPy 1.15): v >= edges[last] belongs to the last
 *     bin iff np.around(v, d) == np.around(edges[last], d), d = decimals[d] = int(-log10(min edge width)) + 6 from the
 *     host, round_scale[d] = 10^|d|; np.around is evaluated as NumPy does, in the coordinates' type, on the point and on
 *     the last edge (SciPy casts the edges to float32 for float32 samples: the caller passes such edges and their d).  A non-finite
 *     value (TF_BIN_STATUS_VALUE) or coordinate (TF_BIN_STATUS_COORD) of a point that passes its masks, falls into a time
 *     window and has an output left to add to is OR-ed into *status (uint32, may be NULL) and the point contributes
 *     nothing.  TF_BIN_STATUS_RULES_DIFFER is OR-ed in when NumPy's rule would have decided otherwise about such a point
 *     on some axis: while it is clear, the counts of this call are np.histogramdd's as well.
 *   keep (uint8, optional) gates everything; keep_value (uint8, optional) gates count_v, sum_w, sum_wv only; with
 *     TF_BIN_FINITE_VALUE in flags a non-finite value silently drops the point from those three as well (under either
 *     rule: `wh = np.isfinite(data)` of grid_flux.py:66).
 *   flip_mask: bit d set writes axis d mirrored, bin n_d - 1 - k (`np.histogram2d(y, x, (y_bins[::-1], x_bins))[0][::-1]`
 *     of glm.py:89 and nexrad.py:104 without a second pass: edges[d] is the reversed, increasing array).
 *   time (int64[n_points]) with win_start, win_end (int64[n_frames], both non-decreasing), all three or none: the point
 *     goes to every frame f with win_start[f] <= t < win_end[f], the range [upper_bound(win_end, t), upper_bound(win_start,
 *     t)).  Without them n_frames must be 1.
 *   outputs, each optional, (n_frames, n_0[, n_1[, n_2]]) with n_d = n_edges[d] - 1, ACCUMULATED into (+=): count (int32)
 *     the points that pass keep; count_v (int32) those that also pass keep_value / the finite test; sum_w, sum_wv (double)
 *     the sums of weight and of weight * value over the count_v points.  value, weight: TF_F32 or TF_F64, optional (a
 *     missing weight is 1, sum_wv needs value); the product is evaluated in NumPy's result type of the two operands
 *     (float32 * float32 rounds in float32) and then widened.
 * Counts are integer atomics: exact, identical in every run.  Sums are double atomics, one set per run of equal (frame
 * range, bin) that a lane meets among its 16 points: they differ from a sequential sum by the summation order only and
 * may differ in the last bits from run to run.  n_points < 2^31 (TF_EINVAL beyond); flat indices are 64-bit. */
#define TF_BIN_MAX_DIMS 3
#define TF_BIN_RULE_NUMPY 0
#define TF_BIN_RULE_SCIPY 1
#define TF_BIN_FINITE_VALUE 1
#define TF_BIN_STATUS_COORD 1u
#define TF_BIN_STATUS_VALUE 2u
#define TF_BIN_STATUS_RULES_DIFFER 4u
typedef struct TfBinPoints {
    int32_t n_dims, coord_dtype, value_dtype, weight_dtype, rule, flags;
    int32_t decimals[TF_BIN_MAX_DIMS];
    int32_t flip_mask;
    double round_scale[TF_BIN_MAX_DIMS];
    int64_t n_points, n_frames;
    int64_t n_edges[TF_BIN_MAX_DIMS];
    const void *coord[TF_BIN_MAX_DIMS];
    const double *edges[TF_BIN_MAX_DIMS];
    const uint8_t *keep, *keep_value;
    const void *value, *weight;
    const int64_t *time, *win_start, *win_end;
    int32_t *count, *count_v;
    double *sum_w, *sum_wv;
    uint32_t *status;
} TfBinPoints;
int tf_bin_points(const TfBinPoints *params_host, void *stream);

/* ---- bt, wvd and swd from raw channel stacks (version 109) -------------------------------------------------------------
 * The array-level work under the reference's loaders: load_mcmip (tobac_flow/dataloader.py:240-321), seviri_dataloader
 * (:588-688), seviri_nat_dataloader (:833-958), get_stripe_deviation (:234-237), fill_time_gap_nan (:341-357) and the
 * dropped frames of goes_dataloader:78-94.  The file decoders stay on the host; what they hand out goes in as it is.
 *
 * TfFieldPlane: one (T, H, W) operand with x contiguous; frame_stride and row_stride in ELEMENTS (row_stride >= W,
 *   frame_stride >= row_stride), so a [y0:y1, x0:x1] cut of full frames needs no copy.  `data` is aligned to its element.
 *   A channel is TF_F32 -- NaN and +-inf mean missing -- or TF_I16, packed: the stored bits are read as int16, or as uint16
 *   with is_unsigned (GOES CMI is _Unsigned); `fill` is the fill value in the stored type (0 .. 65535 for unsigned) and
 *   counts only with has_fill.  CF decoding: stored == fill gives NaN, anything else
 *   (float)stored * scale + offset with two float32 roundings, never a fused multiply-add.  All channels of a call have
 *   one dtype.  A DQF plane is TF_I8 or TF_U8 with an optional fill of its own; scale, offset, is_unsigned are ignored.
 *
 * tf_stripe_deviation: get_stripe_deviation of ONE DQF plane under xarray's skipna rule, a fill being NaN.  Per frame:
 *   m[x] = nanmean over y, s[x] = nanstd over y (ddof 0), dev[y] = |nanmean over x of (D[y, x] - m[x]) / (s[x] + 1e-8)|,
 *   all in float64; a row without a valid term has dev = NaN.  The count and sum D of the valid elements of a column are
 *   exact integers from integer atomics, so m = sum D / n is np.nanmean's value bit for bit; s is np.nanstd's own second
 *   pass, (D - m)^2 added down the column in row order, / n, sqrt: NumPy's value bit for bit as well.  The row sum runs in
 *   float64 in a fixed order without floating-point atomics: dev is identical from run to run and differs from NumPy's
 *   pairwise row mean by the summation order only, within (W + 4) 2^-53 mean_x |term| per row.  dev (T, H), optional: written.  row_flags (T, H) bytes, optional: 1 is
 *   stored where dev > threshold (2 in the reference), nothing elsewhere -- the caller zeroes the table once and runs its
 *   planes one after another on one stream, which ORs them without an atomic.  T <= 65535, H < 2^24, H W < 2^31.
 *   ws_bytes < tf_stripe_workspace_bytes(T, H, W): TF_ENOMEM.
 *
 * tf_prepare_fields: up to TF_FIELD_MAX_RECIPES outputs, contiguous float32 (T_out, H, W).  Output r is channel[a], or
 *   channel[a] - channel[b] with one float32 rounding (b = -1: none), then with has_floor np.maximum(x, floor) (NaN stays
 *   NaN).  Output frame k is made from input frame src[k] (int32[T_out] on the device); src[k] < 0 or >= T is an all-NaN
 *   frame: dropping, sorting and gap filling cost no pass of their own.  A voxel is bad, and EVERY output is NaN there, when
 *   any output is non-finite there (infinities count), any of the n_dqf planes is non-zero or equals its fill there, or
 *   row_flags[src[k] * H + y] (optional, the table of tf_stripe_deviation) is set.  n_masked (int32[T_out], optional):
 *   written, the number of NaN voxels of each output frame, exact (one integer atomic per workgroup).
 *   flags = TF_FIELD_COPY: no mask at all -- every output keeps the values of its recipe, infinities included, and only
 *   the frame table acts (fill_time_gap_nan of a finished field); n_dqf = 0, row_flags and n_masked NULL.
 * Bad arguments are TF_EINVAL before any launch. */
#define TF_FIELD_MAX_CHANNELS 8
#define TF_FIELD_MAX_DQF 8
#define TF_FIELD_MAX_RECIPES 4
#define TF_FIELD_COPY 1
typedef struct TfFieldPlane {
    const void *data;
    int64_t frame_stride, row_stride;
    int32_t dtype, has_fill, is_unsigned, fill;
    float scale, offset;
} TfFieldPlane;
typedef struct TfFieldRecipe {
    int32_t a, b, has_floor;
    float floor;
    float *out;
} TfFieldRecipe;
typedef struct TfFieldPrep {
    int64_t T, H, W, T_out;
    int32_t n_channels, n_dqf, n_recipes, flags;
    TfFieldPlane channel[TF_FIELD_MAX_CHANNELS];
    TfFieldPlane dqf[TF_FIELD_MAX_DQF];
    TfFieldRecipe recipe[TF_FIELD_MAX_RECIPES];
    const int32_t *src;
    const uint8_t *row_flags;
    int32_t *n_masked;
} TfFieldPrep;
size_t tf_stripe_workspace_bytes(int64_t T, int64_t H, int64_t W);
int tf_stripe_deviation(const TfFieldPlane *dqf, int64_t T, int64_t H, int64_t W, double threshold,
                        double *dev /* (T, H), optional */, uint8_t *row_flags /* (T, H), OR-ed into, optional */,
                        void *ws, size_t ws_bytes, void *stream);
int tf_prepare_fields(const TfFieldPrep *params_host, void *stream);

/* ---- measurement aid (bench.py's roofline figure) ---------------------------------------------
 * tf_profile_enable(1): every kernel launch of the library is bracketed by HIP events on its own
 * stream and tagged with its ALGORITHMIC byte count.  tf_profile_collect() synchronises
 * the recorded events and returns, per kernel id < tf_profile_kernel_count(), the number of
 * launches, their summed duration in ms and their summed algorithmic bytes, then clears them. */
int tf_profile_enable(int on);
int tf_profile_kernel_count(void);
const char *tf_profile_kernel_name(int id);
int tf_profile_collect(int64_t *calls, double *ms, double *bytes);

/* ---- host staging: the containers of the reference's API <-> HBM ------------------------------------------------------
 * The reference's entry points take and return numpy / xarray containers (tobac_flow/decorators.py:21-61,
 * scripts/dcc_detect_goes.py:164-303); a drop-in caller therefore pays PCIe for every field and every label volume, and
 * pageable memory moves at a third of the link's rate.  These entry points are what the Python layer moves host containers
 * with ("pinned-host staging to HBM"); pointers named *_host are HOST pointers.
 *
 * tf_host_alloc / tf_host_free: PINNED host blocks from a pool kept by size class (a freed block is handed out again; the
 *   pool keeps at most TF_PINNED_CACHE_GB = 16 GB of free blocks, tf_host_pool_trim(keep_bytes) returns more of them to the
 *   system).  A new block is mmap'ed with MADV_HUGEPAGE, touched by
 *   the host threads and registered (hipHostRegister): 22 ms for 1.88 GB where hipHostMalloc takes 250 ms
 *   (tools/microbench/pin_cost.hip); hipHostMalloc is the fallback.  A result is
 *   downloaded straight into such a block, which the caller wraps as the array it returns: no second host copy.
 *   tf_host_is_pinned: 1 if [ptr, ptr + bytes) lies inside a block that is handed out.  tf_host_pool_spare: how many free
 *   blocks of a size class the pool holds.  (Allocating blocks AHEAD on a background thread, while the device computes, was
 *   measured in round 6 and dropped: hipHostMalloc holds up the launching thread's runtime calls -- the first pass of the
 *   script sequence got slower, 3.02 s against 2.70 s.)
 * tf_upload(dst, src_host, bytes, hash_out_host, stream): host -> device on `stream`.  A pageable source is copied by host
 *   threads (<= 16, TF_STAGING_THREADS) chunk by chunk (8 MiB, TF_STAGING_CHUNK_MB) into a ring of pinned slots, each chunk's
 *   DMA enqueued as soon as it is staged; returns when the SOURCE has been read completely (the caller may free or change it),
 *   the last DMAs and everything enqueued after the call stay asynchronous.  A source inside a pool block goes out as one DMA
 *   and the call waits for it on `stream`: the same contract -- on return the block has been read, the caller may change it
 *   or give it back to the pool (which orders nothing by stream: a freed block may be handed out or unmapped at once), and
 *   everything enqueued after the call stays asynchronous.  hash_out_host != NULL: the 128-bit content checksum of the
 *   source (two uint64), computed by the copying threads on the way.
 * tf_download(dst_host, src, bytes, stream): device -> host, complete on return (DMA at the link's rate into a pool block).
 * tf_hash_host / tf_hash_dev: the same 128-bit checksum of a host buffer (host threads) / of device memory (one kernel; the
 *   two words are returned on the host, the call synchronises `stream`): sums over 16-byte blocks of
 *   fold(mul128(w0 ^ a_i, w1 ^ b_i)), position-keyed, the byte length folded in -- any split over threads or lanes gives the
 *   same words, so the checksum of a device result equals the checksum of its downloaded copy.  The Python layer keys its
 *   cache of device twins with it (tobac_flow_amd/_staging.py): a host array presented again is recognised by CONTENT -- the
 *   same object, or another temporary with the same values (`wvd - swd` of scripts/dcc_detect_goes.py:227,241) -- never
 *   trusted by its address.  Not cryptographic. */
int tf_host_alloc(size_t bytes, void **ptr_out_host);
int tf_host_free(void *ptr_host);
int tf_host_is_pinned(const void *ptr_host, size_t bytes);
int tf_host_pool_stats(int64_t *live_bytes, int64_t *cached_bytes);
int tf_host_pool_spare(size_t bytes);      /* free blocks of the size class of `bytes` in the pool */
int tf_host_pool_trim(size_t keep_bytes);
int tf_upload(void *dst, const void *src_host, size_t bytes, uint64_t *hash_out_host, void *stream);
int tf_download(void *dst_host, const void *src, size_t bytes, void *stream);
int tf_hash_host(const void *src_host, size_t bytes, uint64_t *hash_out_host);
int tf_hash_dev(const void *src, size_t bytes, uint64_t *hash_out_host, void *stream);

/* ---- geodesy (version 115) ------------------------------------------------------------------------------------------------
 * What the reference does with pyproj on the host (abi.py:8-104, geo.py:14-246, utils/geo_utils.py:9-84, nexrad.py:60-77).
 * Everything is float64 inside; angles of the Earth in degrees, scan angles in radians, lengths in the unit of `a`.  No
 * atomics: every output is identical from run to run.  Formulas, contract and divergences: DESIGN.md, "Geodesy".
 *
 * TfGeos: PROJ's `geos` projection on the ellipsoid (a, rf = inverse flattening, 0 = a sphere) seen from h above the
 *   equator at lon_0; sweep_y = 0 the GOES convention (sweep "x"), 1 Meteosat's.  lat_0 != 0 is TF_EINVAL, as PROJ refuses
 *   it.  flags & TF_GEOS_INF: an off-disk ray gives +inf (Proj.__call__) where it otherwise gives NaN (get_abi_lat_lon).
 * tf_geos_inverse: x (W), y (H) scan angles -> lat, lon (H, W), float64 or float32 (out_dtype TF_F64 / TF_F32: the float64
 *   result rounded once).  A lane takes four consecutive pixels of the raveled grid and stores 16 bytes at a time where lat
 *   and lon are 16-byte aligned.  tf_geos_inverse_points: n pairs.
 * tf_geos_forward: n points (lat, lon) -> scan angles (x, y); beyond the limb (PROJ's visibility test) +inf.  With alt
 *   (metres, may be NULL) the parallax step of map_nexrad_to_goes runs in the same launch: project, shift lat and lon by
 *   degrees(alt tan(...) / 6.371e6), project again.
 * tf_geod_inverse: Geod.inv of n pairs -- az12 (at point 1 towards 2), az21 (at point 2 back towards 1, pyproj's
 *   convention) in degrees, dist in the unit of a; each output may be NULL.  Vincenty's iteration, at most 24 steps.  NaN
 *   in: NaN out.  Coincident points: dist 0, (az12, az21) = (180, 0) for lat1 >= 0 and (0, -180) below, as GeographicLib
 *   gives.  A pair that does not converge (near the antipode) is NaN in all three outputs and counted: *status (device
 *   uint32, written, not accumulated) is their number.  Workspace: tf_geod_inverse_workspace_bytes(n), TF_ENOMEM below.
 * tf_grid_spacing: lat, lon (H, W) -> dx, dy (km), area (km2), each may be NULL: the reference's rule (the first pixel of a
 *   row or column keeps its own raw spacing, an interior one the mean of its two, the last one the previous; a one-pixel
 *   axis 0).  Every raw spacing is computed once, into the workspace.  NaN propagates as in the reference; *status counts
 *   the raw spacings that did not converge.
 * tf_view_angles: one pixel per lane, operations in the reference's order.  scalars (host): TF_VIEW_SZA delta, eqt, hours
 *   -> out0 = zenith (rad); TF_VIEW_SZA_AZI declination, eqt, hour of day -> out0, out1 = zenith, azimuth (deg);
 *   TF_VIEW_SATELLITE sat_lat, sat_lon, sat_alt (km) -> out0, out1 = zenith, azimuth (deg); TF_VIEW_ABI_ZENITH lat_0, lon_0
 *   with x (W) and y (n / W) the grid's scan angles -> out0 (deg).  out1 is NULL for the one-angle modes. */
#define TF_GEOS_INF 1
#define TF_VIEW_SZA 0
#define TF_VIEW_SZA_AZI 1
#define TF_VIEW_SATELLITE 2
#define TF_VIEW_ABI_ZENITH 3
typedef struct TfGeos {
    double h, lon_0, lat_0, a, rf;
    int32_t sweep_y, flags;
} TfGeos;
int tf_geos_inverse(const TfGeos *geos, const double *x, int64_t W, const double *y, int64_t H, void *lat, void *lon, int out_dtype,
                    void *stream);
int tf_geos_inverse_points(const TfGeos *geos, const double *x, const double *y, int64_t n, double *lat, double *lon, void *stream);
int tf_geos_forward(const TfGeos *geos, const double *lat, const double *lon, const double *alt, int64_t n, double *x, double *y,
                    void *stream);
size_t tf_geod_inverse_workspace_bytes(int64_t n);
int tf_geod_inverse(double a, double rf, const double *lon1, const double *lat1, const double *lon2, const double *lat2, int64_t n,
                    double *az12, double *az21, double *dist, uint32_t *status, void *ws, size_t ws_bytes, void *stream);
size_t tf_grid_spacing_workspace_bytes(int64_t H, int64_t W);
int tf_grid_spacing(double a, double rf, const double *lat, const double *lon, int64_t H, int64_t W, double *dx, double *dy,
                    double *area, uint32_t *status, void *ws, size_t ws_bytes, void *stream);
int tf_view_angles(int mode, const double *scalars, int n_scalars, const double *lat, const double *lon, int64_t n, const double *x,
                   const double *y, int64_t W, double *out0, double *out1, void *stream);

/* ---- ECEF and the GLM parallax correction (version 116) ------------------------------------------------------------------
 * What the reference's glm.py:25-57 does through the lmatools coordinate systems of _lmatools.py (pyproj Transformers
 * between latlong, geocent and geos).  float64 inside, degrees and metres; one element per lane, one launch, no workspace,
 * no atomics.  n = 0 is a successful no-op; a null pointer with n > 0 is TF_EINVAL.
 *
 * tf_ecef: mode TF_ECEF_FROM_GEODETIC (in = lon, lat, alt -> out = X, Y, Z) or TF_ECEF_TO_GEODETIC (in = X, Y, Z -> out =
 *   lon, lat, alt) on the ellipsoid (a, rf); the geodetic triple is in pyproj's order.  To geodetic: Bowring's iteration
 *   with two updates, no data-dependent loop (below 1e-16 rad up to 160 km above the ellipsoid); on the polar axis lon = 0
 *   and lat = +-90; the origin, a NaN or an infinite coordinate give NaN in all three.
 * tf_geos_to_ecef: scan angles (x, y) of the system `geos` -> the nearer point at which the ray meets the system's
 *   ellipsoid, turned into the Earth's frame by lon_0, in metres.  The satellite stands a + h from the centre with the
 *   system's own a, as PROJ places it.  A ray that misses gives +inf in all three (NaN for a NaN angle).
 * tf_glm_parallax: for n flashes at (lat, lon) degrees (in_dtype TF_F32 or TF_F64; float32 is widened exactly): the
 *   offsets (dlon, dlat) of get_glm_parallax_offsets -- the flash projected with `grid`, the ray with the same scan angles
 *   of the system `ltg` (the lightning ellipsoid) met with that system's ellipsoid, the point read as longitude and
 *   latitude on the ellipsoid (lla_a, lla_rf), minus the flash's own -- and the scan angles (x, y) on `grid` of the flash
 *   moved back by them (get_corrected_glm_x_y).  The pair dlon, dlat and the pair x, y may each be NULL, not both.  `ltg`
 *   shares lon_0 and sweep_y with `grid` (TF_EINVAL otherwise).  A flash beyond the limb of `grid`, or whose ray misses
 *   the lightning ellipsoid: NaN offsets, x = y = +inf (tf_bin_points drops such a point).  NaN in: NaN in all four. */
#define TF_ECEF_FROM_GEODETIC 0
#define TF_ECEF_TO_GEODETIC 1
int tf_ecef(int mode, double a, double rf, const double *in0, const double *in1, const double *in2, int64_t n, double *out0,
            double *out1, double *out2, void *stream);
int tf_geos_to_ecef(const TfGeos *geos, const double *x, const double *y, int64_t n, double *X, double *Y, double *Z, void *stream);
int tf_glm_parallax(const TfGeos *grid, const TfGeos *ltg, double lla_a, double lla_rf, const void *lat, const void *lon, int in_dtype,
                    int64_t n, double *dlon, double *dlat, double *x, double *y, void *stream);

/* tf_copy16: dst = src, 16 bytes per lane per access -- the measured practical HBM ceiling of bench.py's roofline.
 * (Round 5's tf_stream_create_cu_mask / tf_stream_create_priority / tf_stream_destroy / tf_debug_cu_histogram served two
 * scheduling experiments that were not adopted; they live in tools/experiments/stream_experiments.hip now, outside the
 * library: DESIGN.md section 7.) */
int tf_copy16(const void *src, void *dst, size_t bytes, void *stream);
int tf_copy16_variant(const void *src, void *dst, size_t bytes, void *stream, int variant);   /* development forms of the same copy */

/* SURVEY.md 8(b) "ownership": the library never retains a caller's pointer past return and owns no device memory (all
 * scratch is the caller's workspace); its only pooled resource is the HIP events of the timing facility above.
 * tf_shutdown() switches timing off and destroys them.  Idempotent; the library remains usable afterwards. */
int tf_shutdown(void);

/* development aid (tests): compares, on `count` pseudo-random operand pairs drawn from the range it is used in, the
 * shared-reciprocal division of the refinement's system kernel with the hardware's correctly rounded division;
 * *mismatches_host must come back 0.  Allocates and frees 8 bytes of device memory. */
int tf_selftest_shared_divide(int64_t count, uint64_t seed, uint64_t *mismatches_host, void *stream);

#ifdef __cplusplus
}
#endif
#endif
