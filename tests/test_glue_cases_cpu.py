"""CPU checks of tests/glue_cases.py: the host model of tf_label's edge selection against scipy.ndimage.label, the rule
each named mask is there for (asserted and printed), and the kernel form / tile count each morphology geometry claims.

Measured: 14 s for this file on one CPU core, 12 s of it the 16 384 model runs over all structures (0.7 ms each, beside
one ndi.label call); the named subset on the named masks (2 300 runs) takes 2 s."""
import numpy as np
import scipy.ndimage as ndi

import glue_cases as gl


def _small_masks():
    rng = np.random.default_rng(5)
    a = rng.random((2, 5, 70)) < 0.55                      # seg = 64: one segment boundary per row
    b = rng.random((3, 4, 9)) < 0.6                        # seg = 4: two boundaries per row on a volume of 108 voxels
    return ((a, 64), (b, 4))


def test_symmetric_structures_are_the_8192_and_the_named_subset_holds_what_it_must():
    all_s = gl.symmetric_structures()
    assert all_s.shape == (8192, 3, 3, 3) and all_s[:, 1, 1, 1].all()
    assert np.array_equal(all_s, all_s[:, ::-1, ::-1, ::-1])
    assert len({s.tobytes() for s in all_s}) == 8192
    assert int(all_s[:, 1, 1, 2].sum()) == 4096            # half of them hold the (0, 0, +1) tap
    named = gl.named_structures()
    for c in (1, 2, 3):
        st = ndi.generate_binary_structure(3, c)
        assert np.array_equal(named[f"conn{c}"], st)
        st = st.copy()
        st[0] = st[2] = False
        assert np.array_equal(named[f"flat{c}"], st)
    assert named["centre_only"].sum() == 1 and gl.forward_taps(named["centre_only"]) == []
    assert gl.forward_taps(named["x_only"]) == [(0, 0, 1)] and gl.forward_taps(named["y_only"]) == [(0, 1, 0)]
    assert gl.forward_taps(named["t_only"]) == [(1, 0, 0)]
    assert named["cube_minus_x"].sum() == 25 and not gl.has_x_tap(named["cube_minus_x"])
    for name in ("x_diag_yx", "x_diag_tx", "x_diag_tyx", "x_one_diag"):      # a diagonal tap whose sibling is absent
        taps = gl.forward_taps(named[name])
        assert (0, 0, 1) in taps and any(dx != 0 and (dt, dy) != (0, 0) and (dt, dy, 0) not in taps for dt, dy, dx in taps)
    rnd = [s for k, s in named.items() if k.startswith("random")]
    assert len(rnd) >= 48 and len({s.tobytes() for s in rnd}) == len(rnd)
    assert sum(gl.has_x_tap(s) for s in rnd) == 24
    for s in named.values():
        assert s[1, 1, 1] and np.array_equal(s, s[::-1, ::-1, ::-1])


def test_model_equals_scipy_label_for_all_8192_structures():
    total = dict.fromkeys(gl.COUNTERS, 0)
    for mask, seg in _small_masks():
        for k, st in enumerate(gl.symmetric_structures()):
            want, n = ndi.label(mask, structure=st)
            got, ng, counts = gl.ccl_model(mask, st, seg)
            assert ng == n and np.array_equal(got, want), f"structure {k}, seg {seg}"
            assert (counts["plain"] == 0) == (gl.has_x_tap(st) or k == 0)
            for c in gl.COUNTERS:
                total[c] += counts[c]
    print("rule counts over 2 x 8192 structures:", total)
    assert all(v > 1000 for v in total.values()), total


def test_model_equals_scipy_label_for_the_named_subset_on_every_named_mask():
    total = dict.fromkeys(gl.COUNTERS, 0)
    named = gl.named_structures()
    for case in gl.label_masks():
        for sname, st in named.items():
            want, n = ndi.label(case["mask"], structure=st)
            got, ng, counts = gl.ccl_model(case["mask"], st)
            assert ng == n and np.array_equal(got, want), f"{case['name']} under {sname}"
            for c in gl.COUNTERS:
                total[c] += counts[c]
    assert all(v > 0 for v in total.values()), total


def test_every_named_mask_fires_the_rules_it_is_named_for():
    named = gl.named_structures()
    seen = set()
    for case in gl.label_masks():
        for sname, must in case["claims"]:
            counts = gl.ccl_model(case["mask"], named[sname])[2]
            print(f"{case['name']:24s} {sname:14s} " + " ".join(f"{k}={v}" for k, v in counts.items()))
            assert all(counts[c] > 0 for c in must), (case["name"], sname, must, counts)
            assert (counts["plain"] > 0) <= (not gl.has_x_tap(named[sname]))
            seen.update(must)
    assert seen == set(gl.COUNTERS), set(gl.COUNTERS) - seen          # across the case set every counter is claimed by a case


def test_masks_that_claim_to_test_the_sibling_bit_tell_the_wrong_rule_apart():
    """`no_sibling` > 0 only says that the situation occurs.  pixel_over_run and full must also LABEL differently when rule
    (iv) skips without looking at the sibling bit (ccl_model(ignore_sibling=True))."""
    named = gl.named_structures()
    cases = {c["name"]: c["mask"] for c in gl.label_masks()}
    st = named["x_diag_yx"]
    for name in ("pixel_over_run", "full"):
        want, n = ndi.label(cases[name], structure=st)
        got, ng, counts = gl.ccl_model(cases[name], st, ignore_sibling=True)
        assert counts["no_sibling"] > 0
        assert ng != n and not np.array_equal(got, want), name
    assert ndi.label(cases["pixel_over_run"], structure=st)[1] == 5
    wrong = sum(gl.ccl_model(c["mask"], st, ignore_sibling=True)[1] != ndi.label(c["mask"], structure=st)[1]
                for c in gl.label_masks() if c["name"].startswith("random"))
    print("random masks the wrong rule (iv) mislabels under x_diag_yx:", wrong)
    assert wrong >= 6


def test_named_masks_hold_the_shapes_and_patterns_the_label_tests_need():
    cases = {c["name"]: c["mask"] for c in gl.label_masks()}
    shapes = [m.shape for m in cases.values()]
    assert {s[2] for s in shapes} >= {1, 2, 63, 64, 65, 127, 128, 129, 200}
    assert {s[1] for s in shapes} >= {1, 3, 4, 5} and {s[0] for s in shapes} >= {1, 2, 3}
    rnd = [m.shape for k, m in cases.items() if k.startswith("random")]
    assert sorted(rnd) == sorted(gl.RANDOM_MASK_SHAPES) and sorted(s[2] for s in rnd) == sorted(2 * [1, 2, 63, 64, 65, 127, 128, 129, 200])
    assert {(s[0], s[1]) for s in rnd} == {(T, H) for T in (1, 2, 3) for H in (1, 3, 4, 5)}
    sizes = {m.size for m in cases.values()}
    assert {n % 256 for n in sizes} >= {0, 1, 255} and any(n % 4 for n in sizes)
    assert cases["full"].all() and not cases["empty"].any()
    # runs that start at lane 0 / end at lane 63, with and without a continuation over the boundary
    m = cases["lane0_lane63"][0]
    starts = m & ~np.pad(m, ((0, 0), (1, 0)))[:, :-1]
    ends = m & ~np.pad(m, ((0, 0), (0, 1)))[:, 1:]
    assert starts[:, 0].any() and starts[:, 64].any() and starts[:, 63].any()
    assert ends[:, 63].any() and ends[:, 127].any() and ends[:, 64].any()
    assert (m[:, 63] & m[:, 64]).any() and (m[:, 63] & ~m[:, 64]).any() and (~m[:, 63] & m[:, 64]).any()
    m = cases["cross64"]
    for k in (64, 128, 192):
        assert (m[..., k - 1] & m[..., k]).any()
    # the checkerboards: n / 2 components under connectivity 1, over more than four 256-voxel blocks; the last block
    # partial with roots in one, without any voxel set in the other
    cb = cases["checker_partial_block"]
    assert ndi.label(cb)[1] == cb.size // 2 and cb.size % 256 != 0 and cb.size > 4 * 256 and cb.ravel()[-(cb.size % 256):].any()
    tail = cases["checker_rootless_tail"]
    assert not tail.ravel()[-(tail.size % 256) - 256:].any() and ndi.label(tail)[1] == tail.sum() > 256
    # comb and spiral: one component under connectivity 1 whose smallest index is far from most of its voxels
    for name in ("comb_spine_right", "spiral"):
        assert ndi.label(cases[name])[1] == 1
    assert ndi.label(cases["comb_spine_bottom"][:1])[1] == 1
    sp = cases["spiral"]
    assert ndi.label(sp, structure=np.ones((3, 3, 3)))[1] == 1 and sp.sum() < 0.6 * sp.size
    # thin staircases: connected by the diagonal taps only
    st = cases["staircases_yx"][:1, :30]                                 # (the rows before the two diagonals cross)
    assert ndi.label(st)[1] == st.sum() == 60 and ndi.label(st, structure=ndi.generate_binary_structure(3, 2))[1] == 2


def test_morphology_geometries_give_the_forms_and_tile_counts_they_claim():
    by_form = {}
    for T, H, W in gl.MORPH_GEOMETRIES:
        form, n_tiles = gl.morph_form(T, H, W)
        # the formulas of tf_binary_morph, recomputed
        quads, words = W % 16 == 0, W % 4 == 0
        assert form == ("uint4" if quads else "word" if words else "byte")
        if quads:
            assert n_tiles == ((W // 16 + 63) // 64) * ((H + 7) // 8)
        by_form.setdefault(form, []).append((T, H, W, n_tiles))
        print(f"T={T} H={H} W={W}: {form}" + (f", n_tiles={n_tiles} (% 8 = {n_tiles % 8})" if quads else ""))
    u4 = by_form["uint4"]
    assert {(T, n % 8) for T, H, W, n in u4} >= {(T, r) for T in (1, 2, 5) for r in (0, 1, 7)}
    assert {W for T, H, W, n in u4} >= {16, 1024, 1040, 2064}
    assert {W for T, H, W, n in by_form["word"]} >= {4, 260} and {W for T, H, W, n in by_form["byte"]} >= {1, 45}
    assert {H for T, H, W in gl.MORPH_GEOMETRIES} >= {1, 3, 4, 7, 8, 9}
    assert any(H < 4 for T, H, W, n in u4) and {H % 8 for T, H, W, n in u4} >= {0, 1, 7}
    assert max(((n + 7) // 8) * 8 * T for T, H, W, n in u4) > 8          # more than one slot group somewhere
    # the alignment fallbacks: a 16-divisible width 4 bytes / 1 byte off a 16-byte boundary
    assert gl.morph_form(2, 9, 1040, 4)[0] == "word" and gl.morph_form(2, 9, 1040, 1)[0] == "byte"
    assert gl.morph_form(2, 9, 260, 1)[0] == "byte" and gl.morph_form(2, 9, 260, 16)[0] == "word"


def test_morphology_structures_and_grey_footprints_hold_what_they_claim():
    ms = gl.morph_structures()
    assert len(ms) >= 13 + 32 and len({s.tobytes() for s in ms.values()}) == len(ms)
    cross = ndi.generate_binary_structure(3, 1) * np.array([0, 1, 0])[:, None, None].astype(bool)
    assert np.array_equal(ms["cross2d"], cross) and ms["cube"].all() and np.array_equal(ms["conn1"], ndi.generate_binary_structure(3, 1))
    assert all(s.any() for s in ms.values())
    assert sum(s.sum() == 1 and not s[1, 1, 1] for s in ms.values()) >= 5               # single off-centre taps
    dxmask = lambda s: {int(r[0]) + 2 * int(r[1]) + 4 * int(r[2]) for r in s.reshape(9, 3)}      # noqa: E731
    assert dxmask(ms["row5"]) == {0, 5} and dxmask(ms["rows5"]) == {5}
    assert not ms["no_centre"][1, 1, 1] and ms["no_centre"].sum() == 26
    rnd = [s for k, s in ms.items() if k.startswith("random")]
    assert len(rnd) >= 32 and sum(not np.array_equal(s, s[::-1, ::-1, ::-1]) for s in rnd) >= 16
    assert set().union(*(dxmask(s) for s in rnd)) == set(range(8))
    fps = gl.grey_footprints()
    assert len([k for k in fps if k.startswith("random")]) >= 32 and len({s.tobytes() for s in fps.values()}) == len(fps)
    for s in fps.values():
        assert s.any() and not s.all() and np.array_equal(s, s[::-1, ::-1, ::-1])
    assert sum(np.flatnonzero(s)[0] != 13 for s in fps.values()) >= 32                   # first cell in C order off-centre
    assert sum(not s[1, 1, 1] for s in fps.values()) >= 6


def test_element_vectors_put_every_special_value_in_quads_and_in_tails():
    assert gl.ELEMENT_COUNTS == (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4097)
    for lo, hi in gl.THRESHOLD_PAIRS:
        sv = gl.special_values(lo, hi)
        assert np.isnan(sv).sum() == 1 and np.isposinf(sv).any() and np.isneginf(sv).any()
        assert (np.signbit(sv) & (sv == 0)).any() and (~np.signbit(sv) & (sv == 0)).any()
        for c in (lo, hi, 0.0, 1.0):
            c = np.float32(c)
            assert {c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))} <= set(sv.tolist())
        key = lambda v: v.view(np.uint32)                                                 # noqa: E731
        in_tail, in_body = set(), set()
        for n in gl.ELEMENT_COUNTS:
            for seed in range(sv.size):
                v = gl.element_vector(n, lo, hi, seed)
                assert v.dtype == np.float32 and v.shape == (n,)
                in_body.update(key(v[:n - n % 4]).tolist())
                in_tail.update(key(v[n - n % 4:]).tolist())
        assert set(key(sv).tolist()) <= in_body and set(key(sv).tolist()) <= in_tail
