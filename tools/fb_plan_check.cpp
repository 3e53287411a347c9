// The level plan of the Farnebaeck host driver (tobac_flow_amd/csrc/fb_plan.h) checked against itself: what the size
// functions report, what carving hands out and what the levels of a phase put into each array, over a grid of geometries,
// parameters, batch sizes and parts.  A stand-alone program, also for AddressSanitizer + UBSan:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/fb_plan_check.cpp -o fb_plan_check
//   ./fb_plan_check
#include <stdio.h>
#include <algorithm>
#include "../tobac_flow_amd/csrc/fb_plan.h"

static long n_checks = 0, n_failed = 0;
static char ctx[256];
#define CHECK(cond) do { n_checks++; if (!(cond)) { if (n_failed++ < 20) printf("FAILED %s  [%s] (line %d)\n", #cond, ctx, __LINE__); } } while (0)

// one phase for B pairs: the carved arrays lie inside the reported bytes, one after the other, and every level's contents
// fit a pair's stride (so pair b never reaches pair b + 1)
static void check_phase(int64_t H, int64_t W, const tf_farneback_params *p, int which, int64_t B)
{
    const FbPhase ph = fb_phase(H, W, p, which);
    size_t off[FB_ARRAYS];
    const size_t end = fb_carve_offsets(ph, B, off), bytes = fb_bytes(which, B, H, W, p);
    CHECK(end <= bytes);
    CHECK(bytes == fb_phase_bytes(ph, B));
    size_t prev_end = 0;
    for (int a = 0; a < FB_ARRAYS; a++) {
        CHECK(off[a] % 256 == 0 && off[a] >= prev_end);
        prev_end = off[a] + (size_t)B * ph.stride[a] * sizeof(float);
    }
    CHECK(prev_end == end);
    CHECK(ph.fused == (p->win_size == FBI_WIN) && (ph.stride[FB_M] == 0) == ph.fused);
    CHECK(ph.k_lo >= 0 && ph.k_hi >= ph.k_lo && ph.k_hi <= fb_levels(H, W, p));
    for (int k = ph.k_hi; k >= ph.k_lo; k--) {
        const FbLevel l = fb_level(H, W, p, k);
        const size_t plane = (size_t)l.h * l.w;
        CHECK(l.k == k && l.h >= 1 && l.w >= 1 && (k > 0 || (l.h == H && l.w == W)));
        CHECK(plane <= ph.stride[FB_BLUR] && plane <= ph.stride[FB_I] && (k > 0 || (size_t)H * W <= ph.stride[FB_BLUR]));
        CHECK(5 * plane <= ph.stride[FB_R0] && 5 * plane <= ph.stride[FB_R1] && (ph.fused || 5 * plane <= ph.stride[FB_M]));
        CHECK(2 * plane <= ph.stride[FB_F0] && 2 * plane <= ph.stride[FB_F1]);
        // the sampled blur's H rows of w float2, at every level that is not the full-size frame itself (that one is blurred
        // in one pass, into `blur`)
        CHECK(ph.stride[FB_TMP] % 2 == 0 && ((l.h == H && l.w == W) || 2 * (size_t)H * l.w <= ph.stride[FB_TMP]));
        const size_t nx = (size_t)((l.w + FBI_OW - 1) / FBI_OW);
        for (size_t nd = 1; nd <= 2; nd++) CHECK(FBI_HDR + nd * (nx - 1) * l.h * FBI_HW * 8 <= ph.stride[FB_TMP] * sizeof(float));
    }
    // the ping-pong slot: every level but the pyramid's top flips it for the upsample, the fused iteration once per launch
    for (int iters = 1; iters <= 10; iters++) {
        tf_farneback_params q = *p; q.num_iters = iters;
        const FbPhase pq = fb_phase(H, W, &q, which);
        int cur = pq.slot; bool have_flow = pq.pw != 0;
        for (int k = pq.k_hi; k >= pq.k_lo; k--) { if (have_flow) cur ^= 1; if (pq.fused) cur ^= iters & 1; have_flow = true; }
        CHECK(cur == 0);
    }
}

int main()
{
    static const int shapes[][2] = {{1, 1}, {31, 31}, {32, 32}, {33, 70}, {64, 64}, {65, 127}, {131, 140}, {203, 331}, {333, 517},
                                    {1500, 2500}, {3712, 3712}, {5424, 5424}};
    static const double scales[] = {0.5, 0.6, 0.8};
    static const int wins[] = {13, 9}, levels[] = {0, 1, 5};
    static const int64_t batches[] = {1, 2, 3, 5, 23, 42};
    for (const auto &hw : shapes) for (double sc : scales) for (int win : wins) for (int nl : levels) {
        const int64_t H = hw[0], W = hw[1];
        tf_farneback_params p = {};
        p.num_levels = nl; p.pyr_scale = sc; p.win_size = win; p.num_iters = 10; p.poly_n = 5; p.poly_sigma = 1.1;
        const bool splits = fb_can_split(H, W, &p);
        CHECK(splits == (fb_levels(H, W, &p) >= FB_SPLIT_LEVEL && sc == 0.5));
        for (int64_t B : batches) {
            snprintf(ctx, sizeof ctx, "%dx%d scale %.1f win %d levels %d B %d", (int)H, (int)W, sc, win, nl, (int)B);
            check_phase(H, W, &p, FB_WHOLE, B);
            const size_t batch = fb_bytes(FB_WHOLE, B, H, W, &p);
            CHECK(batch > 0 && fb_bytes_split(B, 1, H, W, &p) == batch);
            if (splits) {
                check_phase(H, W, &p, FB_COARSE, B);
                check_phase(H, W, &p, FB_FINE, B);
                const FbPhase coarse = fb_phase(H, W, &p, FB_COARSE), fine = fb_phase(H, W, &p, FB_FINE);
                const FbLevel l = fb_level(H, W, &p, FB_SPLIT_LEVEL);
                CHECK(coarse.k_hi == fb_levels(H, W, &p) && coarse.k_lo == FB_SPLIT_LEVEL && coarse.pw == 0);
                CHECK(fine.k_hi == FB_SPLIT_LEVEL - 1 && fine.k_lo == 0 && fine.slot == 0 && fine.pw == l.w && fine.ph == l.h);
                CHECK(fb_bytes(FB_FINE, B, H, W, &p) == batch);
            } else
                CHECK(fb_bytes(FB_COARSE, B, H, W, &p) == 0 && fb_bytes(FB_FINE, B, H, W, &p) == 0);
            for (int64_t parts : {(int64_t)1, (int64_t)2, (int64_t)3, B}) {
                const int64_t np = fb_parts(B, parts, H, W, &p);
                CHECK(np == ((splits && B >= 2 && parts >= 2) ? std::min(parts, B) : 1));
                const size_t want = np == 1 ? batch : std::max(fb_bytes(FB_COARSE, B, H, W, &p), fb_bytes(FB_FINE, (B + np - 1) / np, H, W, &p));
                CHECK(fb_bytes_split(B, parts, H, W, &p) == want);
            }
        }
    }
    // bad arguments size to nothing
    tf_farneback_params d = {}; d.num_levels = 5; d.pyr_scale = 0.5; d.win_size = 13; d.num_iters = 10;
    snprintf(ctx, sizeof ctx, "bad arguments");
    CHECK(fb_bytes(FB_WHOLE, 0, 64, 64, &d) == 0 && fb_bytes(FB_WHOLE, 1, 0, 64, &d) == 0 && fb_bytes(FB_WHOLE, 1, 64, 64, nullptr) == 0);
    CHECK(fb_bytes_split(0, 2, 256, 256, &d) == 0 && fb_bytes_split(4, 2, 256, 256, nullptr) == 0 && fb_batch_hint(64, 64, &d, 0, 0, 1024) == 0);
    printf("%ld checks, %ld failed\n", n_checks, n_failed);
    if (n_failed == 0) printf("plan consistent\n");
    return n_failed != 0;
}
