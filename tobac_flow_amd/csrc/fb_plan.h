// The level plan of the Farnebaeck host driver (farneback.hip): the one statement of the pyramid's geometry, of the scratch a
// phase of levels needs per pair, and of how a batch is cut into phases.  Workspace sizes, the carving of a workspace, the level
// loop and the batch hint are all read off it, so they cannot drift apart.  Plain C++: nothing here touches the HIP runtime,
// and tools/fb_plan_check.cpp compiles it with g++ and checks it against itself.
#pragma once
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include "../../include/tobac_flow_hip.h"

#define FB_MAX_KSIZE 255
#define FBI_M 6
#define FBI_WIN (2 * FBI_M + 1)     // the window size the fused iteration kernel is built for; others take the unfused pair
#ifndef FBI_T
#define FBI_T 128                   // threads = evaluated columns per workgroup
#endif
#define FBI_OW (FBI_T - 2 * FBI_M)  // output columns of a strip
#define FBI_HDR 16384               // bytes of ticket counters in front of a batch's hand-over words: 16 ints per launch of a level (8 used: one per XCD)
#define FBI_HW 20                   // hand-over words per row and strip: (g, V[next strip's x - 7]) x 5 channels x two halves, stored as four planes of H x 5
#define FB_SPLIT_LEVEL 2            // levels >= FB_SPLIT_LEVEL of a split batch run for all its pairs at once, the finer ones in parts

// ---- level geometry ---------------------------------------------------------------------------------------------------
// level k is the frame at scale pyr_scale^k (the product formed factor by factor, as OpenCV forms it), rounded to pixels
struct FbLevel { int k, h, w; double scale; };
static inline FbLevel fb_level(int64_t H, int64_t W, const tf_farneback_params *p, int k) {
    double scale = 1; for (int i = 0; i < k; i++) scale *= p->pyr_scale;
    return FbLevel{k, (int)lrint(H * scale), (int)lrint(W * scale), scale};
}
// the coarsest level: the last of at most num_levels whose unrounded size is still 32 px both ways
static inline int fb_levels(int64_t H, int64_t W, const tf_farneback_params *p) {
    int k = 0;
    for (; k < p->num_levels; k++) { const double s = fb_level(H, W, p, k + 1).scale; if (W * s < 32 || H * s < 32) break; }
    return k;
}
static inline int64_t fb_strips(int64_t w) { return (w + FBI_OW - 1) / FBI_OW; }       // workgroups of k_fb_iter across a row
// floats of blur scratch the iteration kernel borrows per pair at a level: FBI_HDR bytes of ticket counters + the strips'
// hand-over words (8 bytes each, both directions)
static inline size_t fb_hand_floats(const FbLevel &l) { return FBI_HDR / 4 + 2 * (size_t)(2 * (fb_strips(l.w) - 1) * l.h * FBI_HW); }
static inline bool fb_can_split(int64_t H, int64_t W, const tf_farneback_params *p) {
    // (only at scale 0.5 is every level >= FB_SPLIT_LEVEL a sampled blur: no full-size plane in the coarse phase)
    return p && H > 0 && W > 0 && fb_levels(H, W, p) >= FB_SPLIT_LEVEL && p->pyr_scale == 0.5;
}

// ---- phases and their scratch -----------------------------------------------------------------------------------------
// A call runs the whole pyramid in one phase (FB_WHOLE), or it is a SPLIT BATCH (round 4).  A launch of the iteration kernel
// costs whole rounds of resident workgroups; at the coarse levels a round holds the strips of ~40 pairs, at full resolution
// those of ~10 -- but the scratch of a pair is sized by its full-resolution planes.  So the levels >= 2 run for ALL pairs of the
// batch at once, with scratch strides of the level-2 plane (1 / 16 of a full one), and leave their flow in the caller's output
// frames (FB_COARSE); the two finest levels then run part by part on full-size scratch for B / parts pairs (FB_FINE).  Same
// kernels on the same data: the results are those of the unsplit batch.  Every scratch array holds the pairs of a phase back
// to back; stride[] = floats per pair.
enum { FB_WHOLE, FB_COARSE, FB_FINE };
enum { FB_TMP, FB_BLUR, FB_I, FB_R0, FB_R1, FB_M, FB_F0, FB_F1, FB_ARRAYS };
struct FbPhase {
    int k_hi, k_lo;                 // the levels it runs, coarse to fine
    int slot, pw, ph;               // ping-pong slot and size of the flow it starts from; pw == 0: none, level k_hi starts from zeros in `slot`
    bool fused;
    size_t stride[FB_ARRAYS];       // tmp (sampled blur rows / hand-over words), blur, I, R[2], M (unfused only), flow scratch [2]
};
// The slot the coarsest level starts in, so that the result of level 0 lands in slot 0 (the caller's buffer): every level flips
// the slot num_iters times (+1 for the upsample on all but the coarsest level); the unfused fallback iterates in place.
// (Two levels of num_iters + 1 flips follow FB_SPLIT_LEVEL: its flow is in slot 0 as well, whatever the parity of num_iters.)
static inline int fb_start_slot(int levels, int num_iters, bool fused) { return ((levels + 1) * ((fused ? num_iters : 0) + 1) - 1) % 2; }
static inline size_t fb_align64(size_t v) { return (v + 63) / 64 * 64; }
static inline FbPhase fb_phase(int64_t H, int64_t W, const tf_farneback_params *p, int which) {
    const int levels = fb_levels(H, W, p);
    FbPhase ph = {};
    ph.k_hi = which == FB_FINE ? FB_SPLIT_LEVEL - 1 : levels; ph.k_lo = which == FB_COARSE ? FB_SPLIT_LEVEL : 0;
    ph.fused = p->win_size == FBI_WIN;
    ph.slot = fb_start_slot(levels, p->num_iters, ph.fused);
    if (which == FB_FINE) { const FbLevel l = fb_level(H, W, p, FB_SPLIT_LEVEL); ph.slot = 0; ph.pw = l.w; ph.ph = l.h; }
    // Planes are those of the phase's finest level; tmp serves every level from the pyramid's top down to it (a fine phase
    // has a whole batch's strides).  Level 0 asks for a whole image + 2 H + 64 floats (what a two-pass blur needs -- the
    // size workspaces and batch hints have been computed from), a coarser level for the sampled blur's H rows of w float2:
    // 2 H w floats, more than n from a pyramid scale above 0.5 on (1.2 n at level 1 of scale 0.6: sized by n + 2H + 64, one
    // pair's rows ran into the next pair's scratch); every level for its hand-over words.
    size_t tmp = 0, plane = 0;
    for (int k = ph.k_lo; k <= levels; k++) {
        const FbLevel l = fb_level(H, W, p, k);
        const size_t blur = k == 0 ? (size_t)H * W + 2 * (size_t)H + 64 : 2 * (size_t)H * l.w + 64, hand = fb_hand_floats(l);
        plane = std::max(plane, (size_t)l.h * l.w);
        tmp = std::max(tmp, std::max(blur, hand));
    }
    const size_t n = fb_align64(plane);
    ph.stride[FB_TMP] = fb_align64(tmp); ph.stride[FB_BLUR] = ph.stride[FB_I] = n; ph.stride[FB_R0] = ph.stride[FB_R1] = 5 * n;
    ph.stride[FB_M] = ph.fused ? 0 : 5 * n;      // the fused iteration never stores the 5-plane matrix
    ph.stride[FB_F0] = ph.stride[FB_F1] = fb_align64(2 * plane);
    return ph;
}
static inline size_t fb_pair_bytes(const FbPhase &ph) {
    size_t f = 0; for (int a = 0; a < FB_ARRAYS; a++) f += ph.stride[a];
    return f * sizeof(float);
}
// bytes of workspace for B pairs: the arrays + room for the 256-byte alignment of each
static inline size_t fb_phase_bytes(const FbPhase &ph, int64_t B) { return (size_t)B * fb_pair_bytes(ph) + 8192; }
// byte offsets of the arrays of B pairs in a workspace; returns the end of the last one
static inline size_t fb_carve_offsets(const FbPhase &ph, int64_t B, size_t off[FB_ARRAYS]) {
    size_t used = 0;
    for (int a = 0; a < FB_ARRAYS; a++) { off[a] = (used + 255) / 256 * 256; used = off[a] + ph.stride[a] * (size_t)B * sizeof(float); }
    return used;
}

// ---- workspace sizes of the entry points ------------------------------------------------------------------------------
// one phase for B pairs (0: bad arguments, or half a split batch of a geometry that does not split)
static inline size_t fb_bytes(int which, int64_t B, int64_t H, int64_t W, const tf_farneback_params *p) {
    return B > 0 && H > 0 && W > 0 && p && (which == FB_WHOLE || fb_can_split(H, W, p)) ? fb_phase_bytes(fb_phase(H, W, p, which), B) : 0;
}
// parts a batch of B is really cut into (1: one whole phase)
static inline int64_t fb_parts(int64_t B, int64_t parts, int64_t H, int64_t W, const tf_farneback_params *p) {
    return (parts <= 1 || B < 2 || !fb_can_split(H, W, p)) ? 1 : (parts > B ? B : parts);
}
// a split batch: the coarse phase for all pairs, then the workspace again for one part's fine phase
static inline size_t fb_bytes_split(int64_t B, int64_t parts, int64_t H, int64_t W, const tf_farneback_params *p) {
    parts = fb_parts(B, parts, H, W, p);
    const size_t coarse = fb_bytes(FB_COARSE, B, H, W, p), fine = fb_bytes(FB_FINE, (B + parts - 1) / parts, H, W, p);
    return parts == 1 ? fb_bytes(FB_WHOLE, B, H, W, p) : (coarse > fine ? coarse : fine);
}

// ---- batch hint --------------------------------------------------------------------------------------------------------
// A launch of the iteration kernel costs whole ROUNDS of resident workgroups (`slots` of them), each as long as the level is
// high, at EVERY pyramid level: B pairs cost sum_l ceil(B strips_l / slots) rows_l and do sum_l (B strips_l / slots) rows_l of
// work.  The batch with the best ratio wins, the larger one among those within 1 % of it (at 5424^2 on 256 CUs: 42
// pairs, 94.6 %: full rounds at levels 0, 1 AND 2; 54 pairs: 92.1 %, 43 pairs: 85 % -- level 1 spills into a third round).
static inline int64_t fb_batch_hint(int64_t H, int64_t W, const tf_farneback_params *p, int64_t max_pairs, size_t max_bytes, int64_t slots) {
    if (H <= 0 || W <= 0 || !p || max_pairs < 1) return 0;
    const size_t per_pair_bytes = fb_pair_bytes(fb_phase(H, W, p, FB_WHOLE));
    int64_t cap = max_pairs;
    if (max_bytes > 0 && (int64_t)(max_bytes / per_pair_bytes) < cap) cap = (int64_t)(max_bytes / per_pair_bytes);
    if (cap < 1) cap = 1;
    if (cap > 1024) cap = 1024;
    const int levels = fb_levels(H, W, p);
    auto efficiency = [&](int64_t B) {
        double cost = 0, work = 0;
        for (int k = 0; k <= levels; k++) {
            const FbLevel l = fb_level(H, W, p, k);
            const int64_t chains = 2 * B * fb_strips(l.w), rounds = (chains + slots - 1) / slots;
            cost += (double)rounds * (double)l.h; work += (double)chains / (double)slots * (double)l.h;
        }
        return work / cost;
    };
    double best_eff = 0;
    for (int64_t B = 1; B <= cap; B++) { const double e = efficiency(B); if (e > best_eff) best_eff = e; }
    for (int64_t B = cap; B > 1; B--) if (efficiency(B) >= best_eff - 0.01) return B;
    return 1;
}
