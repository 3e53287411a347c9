"""The arithmetic of the flow scheduler (flow.py): batch sizes, what is queued again when a batch does not fit, images per
refinement launch.  No torch, no device call: what the rules need from the library or the device is handed in."""

# the fused SOR kernel's tile (VRT_W / VRT_H in csrc/varref.hip)
VR_TILE_W, VR_TILE_H = 108, 84


def even_batches(n_pairs, chunk):
    """`n_pairs` in ceil(n_pairs / chunk) batches of nearly equal size (edges rounded half to even), e.g. 10 by 3 -> 2, 3, 3, 2"""
    n_b = max(1, -(-n_pairs // chunk))
    edges = [round(k * n_pairs / n_b) for k in range(n_b + 1)]
    return [b - a for a, b in zip(edges[:-1], edges[1:]) if b > a]


def flow_budget(requested, held, free):
    # never more than the scratch kept from the last call plus 60 % of what is free now (the stages after the flow need room too)
    return int(max(min(requested, held + 0.6 * free), 1))


def budget_caps(pixels, lib_per_pair, budget, parts):
    """(the most pairs a batch may have within `budget` bytes, the library's share of the budget).  A pair costs the library's
    scratch (full size for B / parts pairs only, tf_farneback_batch_split) plus 18 bytes per pixel of 8-bit frames and raw flow."""
    # the library's hint counts ITS scratch only: it gets the library's share of the budget, so that both sides price a pair the
    # same way (a hint ~25 % over the budget went through the halving path: release, empty_cache, half batches from then on)
    per_pair = lib_per_pair // parts + pixels * (2 + 16)
    return max(1, budget // per_pair), max(1, int(budget * ((lib_per_pair // parts) / per_pair)))


def budget_batches(n_pairs, pixels, lib_per_pair, budget, parts, hint):
    """Batch sizes within `budget` bytes: those of `hint(max_pairs, max_bytes)` (tf_farneback_batch_hint), the rest in one."""
    # The fused iteration kernel walks whole columns (OpenCV's running column sums cannot be split over rows,
    # csrc/farneback.hip), so its parallelism is strips x directions x PAIRS and a launch costs a whole number of rounds of
    # resident workgroups -- at every pyramid level.  Within the budget the library picks the batch whose rounds are fullest
    # summed over the levels (42 pairs at 5424^2 -- full rounds at levels 0, 1 and 2 -- rather than the 54 that fit); what is
    # left at the end goes into one batch, which never costs more rounds than splitting it
    cap, lib_budget = budget_caps(pixels, lib_per_pair, budget, parts)
    sizes, left = [], n_pairs
    while left > 0:
        if left <= cap:
            B = left
        else:       # the hint sizes the FULL-resolution launches: B / parts pairs of them
            B = min(cap, left, max(1, int(hint(-(-left // parts), lib_budget))) * parts)
        sizes.append(B)
        left -= B
    return sizes


def requeue_halved(done, stop, pending, half):
    """The queue after a batch [.., stop) failed with `done` leading pairs final: the rest of it and every batch of `pending`
    [(first pair, pairs)] cut to at most `half` pairs, in order.  Nothing before `done` runs again (it may have been handed out)."""
    out = []
    for j0, Bj in [(done, stop - done)] + list(pending):
        while Bj > half:
            out.append((j0, half))
            j0, Bj = j0 + half, Bj - half
        if Bj > 0:
            out.append((j0, Bj))
    return out


def varref_tiles(H, W):
    return -(-W // VR_TILE_W) * -(-H // VR_TILE_H)


def varref_group(B, tiles, cus, rounds, bytes_per_image):
    """Images per launch of the batched refinement: groups that fill ~`rounds` rounds of the fused SOR kernel's tiles on the
    device's CUs, within 6.5 GB of scratch.  With 256 CUs and rounds = 32: 19 of the 23 pairs of 1500 x 2500 (432 tiles) per
    set of launches; one image per launch at 5424^2 (3315 tiles, 12.9 rounds by itself); three at 3712^2 (1575 tiles)."""
    group = int(max(1, min(B, -(-rounds * cus // tiles))))
    # ... but only where ONE image does not fill the chip for several rounds by itself (fewer tiles than 4 x the CUs).  At 5424^2
    # three images per launch were measured 3 % slower in bench.py's timed region (vr_sor 925 -> 952 ms per step: longer
    # launches interleave worse with the floods' kernels)
    if tiles >= 4 * cus and rounds > 0:
        # ... unless its last round is poorly filled: the smallest group of up to four images that wastes < 3 % of its rounds
        # (3712^2: 1575 tiles = 6.15 rounds, 14 % of 7 rounds idle by itself, 5 % of 13 in pairs, 3 % of 19 in threes)
        def waste(g):
            r = g * tiles / cus
            return -(-g * tiles // cus) / r - 1.0
        few = range(1, min(B, 4) + 1)
        group = next((g for g in few if waste(g) < 0.03), min(few, key=waste))
    return int(max(1, min(group, 6.5e9 // max(1, bytes_per_image))))
