"""The label glue without a GPU: the oracle's restatements (oracle/np_label.py, oracle/np_dataset.py), the host forms of
tobac_flow_amd/utils/label_utils.py and the host statement of the window rule (parallel._overlap_pairs_host) against what
the REFERENCE's own functions wrote into tests/golden/label_glue_ref.npz, on the cases of tests/label_glue_cases.py.  Every
comparison is an equality of integers."""
import numpy as np
import pytest

import label_glue_cases as gc


@pytest.fixture(scope="module")
def ref():
    return gc.fixture()


@pytest.fixture(scope="module")
def flow_cases():
    return gc.flow_label_cases()


@pytest.fixture(scope="module")
def link_cases(ref):
    return gc.link_cases({gc.shape_name(s): ref[f"utils/{gc.shape_name(s)}/make_step_labels"] for s in gc.SHAPES})


def f32(v):
    return v.astype(np.float32)


def test_generators_are_deterministic_and_equal_the_stored_inputs(ref, flow_cases):
    again = gc.flow_label_cases()
    assert len(flow_cases) == 15 + 6 and set(gc.SEEDED) <= set(flow_cases)
    for name, (mask, forward, backward, _) in flow_cases.items():
        assert mask.dtype == bool and forward.dtype == backward.dtype == np.int8
        for a, b in zip((mask, forward, backward), again[name][:3]):
            assert np.array_equal(a, b), name
        assert np.array_equal(gc.unpack(ref[f"mask/{name}"]), mask), name
        stored = gc.unpack_flows(ref[f"flows/{name}"])
        assert np.array_equal(stored[0], forward) and np.array_equal(stored[1], backward), name
    for shape in gc.SHAPES:
        seed0, seed2 = gc.seeded_flows(shape, 0), gc.seeded_flows(shape, 2)
        assert np.array_equal(seed0[1], -seed0[0]) and abs(seed0[0]).max() == 2
        assert seed2[0][..., 0].min() == -40 and seed2[1][..., 1].max() == 40       # whole labels sample outside the frame
        assert np.array_equal(ref[f"utils/{gc.shape_name(shape)}/labels"], gc.tile_labels(shape))
    for name, (left, right, _) in gc.window_cases().items():
        assert np.array_equal(ref[f"window/{name}/left"], left) and np.array_equal(ref[f"window/{name}/right"], right), name
    assert np.array_equal(ref["link_input/gap_ids"], gc.make_gap_ids()[0])
    assert np.array_equal(gc.unpack_flows(ref["flows/gap_ids"])[0], gc.make_gap_ids()[1])
    assert "integer-valued" in str(ref["note"]) and str(ref["numpy_version"]) and str(ref["scipy_version"])


def test_shapes_reach_the_boundaries_they_are_there_for():
    n = {s: int(np.prod(s)) for s in gc.SHAPES}
    assert list(gc.SHAPES) == [(1, 5, 65), (2, 7, 130), (3, 33, 67), (5, 48, 64), (4, 31, 37)]
    assert 65 > 64 and 5 % 4 and n[(1, 5, 65)] % 4
    assert 130 > 2 * 64 and n[(2, 7, 130)] % 256
    assert n[(3, 33, 67)] > 4096 and (33 * 67 * 4) % 16                          # labels[1:] of an int32 volume: 4-byte aligned only
    assert 64 % 16 == 0 and (48 * 64 * 4) % 16 == 0 and n[(5, 48, 64)] % 256 == 0
    assert 31 % 4 and 37 % 4 and n[(4, 31, 37)] % 4 == 0 and (31 * 37 * 4) % 16
    for shape in ((1, 5, 65), (2, 7, 130)):                                       # a run goes on across a 64-pixel row segment
        assert any(gc.seeded_mask(shape, seed)[:, :, 63:65].all(-1).any() for seed in gc.SEEDS), shape
    assert gc.seeded_mask((2, 7, 130), 0)[:, :, 127:129].all(-1).any() or gc.seeded_mask((2, 7, 130), 1)[:, :, 127:129].all(-1).any()


def test_the_fixture_keeps_its_teeth(ref, flow_cases):
    """the decisive edges, against the stored values: a regenerated fixture cannot lose them"""
    edge = gc.expected_flow_label("product_edge", flow_cases["product_edge"][3])
    assert 0.28 * 25 > 7 and 7 / 25 >= 0.28                                        # the product misses what the quotient meets
    assert edge[(0.27, 0)].max() == 1 and edge[(0.28, 0)].max() == 2 and edge[(0.29, 0)].max() == 2
    absolute = gc.expected_flow_label("absolute_edge", flow_cases["absolute_edge"][3])
    assert absolute[(0, 6)].max() == 1 and absolute[(0, 7)].max() == 2             # the strict >: 7 px link at 6, not at 7
    window = gc.expected_window("quotient_edge", gc.QUOTIENT_GRID)
    for g in ((5, 0.27), (5, 0.28), (7, 0.28), (0, 0.28), (0, 0.0)):
        assert window[g][0].tolist() == [[3, 2]], g
    for g in ((5, 0.29), (8, 0.28)):
        assert len(window[g][0]) == 0, g
    directed, symmetric = gc.check_visit_order()
    visit, flat = gc.expected_flow_label("visit_order", flow_cases["visit_order"][3])[(0, 0)], gc.expected_flat("visit_order")
    assert int(flat.max()) == 6 >= 5
    got = {label: int(visit[flat == label][0]) for label in directed}
    assert got == directed and got != symmetric
    assert len(gc.expected_window("over_zero", gc.WINDOW_GRID)[(5, 0.5)][0]) == 1
    outside = gc.expected_window("mostly_outside", gc.WINDOW_GRID)
    assert len(outside[(5, 0.5)][0]) == 0 and len(outside[(0, 0.3)][0]) == 1       # 12 / 80 over ALL of the right label; 12 / 40 == 0.3
    gap = gc.expected_link("gap_ids", gc.make_gap_ids()[0], gc.GAP_GRID)
    assert (gap[(0, 0)][0].max(), gap[(0, 0)][1]) == (4, 6) and (gap[(0, 12)][0].max(), gap[(0, 12)][1]) == (7, 7)
    nontrivial = eligible = 0
    for name in gc.SEEDED:
        if flow_cases[name][0].shape[0] >= 2:
            n_steps = int(gc.expected_flat(name).max())
            for labels in gc.expected_flow_label(name, gc.FLOW_GRID).values():
                eligible += 1
                nontrivial += 1 < labels.max() < n_steps
    assert 2 * nontrivial >= eligible > 0


def test_flat_label_of_the_oracle_and_the_host_form(ref, flow_cases):
    from oracle import np_label
    from tobac_flow_amd.utils import label_utils as host
    for name in gc.FLAT_CASES:
        mask = flow_cases[name][0]
        for structure, kwargs in (("default", {}), ("full", {"structure": gc.FULL.astype(int)})):
            want = gc.expected_flat(name, structure)
            for fn in (np_label.flat_label, host.flat_label):
                got = fn(mask, **kwargs)
                assert got.dtype == np.int32 and np.array_equal(got, want), (name, structure, fn.__module__)
    for shape in gc.SHAPES:                                        # the diagonal taps merge something at every shape
        assert any(gc.expected_flat(gc.seeded_name(shape, seed), "full").max() < gc.expected_flat(gc.seeded_name(shape, seed)).max()
                   for seed in gc.SEEDS), shape


def test_flow_label_and_flow_link_overlap_of_the_oracle(ref, flow_cases, link_cases):
    from oracle import np_label
    for name, (mask, forward, backward, grid) in flow_cases.items():
        for (overlap, absolute), want in gc.expected_flow_label(name, grid).items():
            got = np_label.flow_label(f32(forward), f32(backward), mask, overlap=overlap, absolute_overlap=absolute)
            assert got.dtype == np.int32 and np.array_equal(got, want), (name, overlap, absolute)
    for name, (flat, forward, backward, grid) in link_cases.items():
        for (overlap, absolute), (want, _) in gc.expected_link(name, flat, grid).items():
            got = np_label.flow_link_overlap(f32(forward), f32(backward), flat, overlap=overlap, absolute_overlap=absolute)
            assert np.array_equal(got, want), (name, overlap, absolute)


def test_find_overlapping_labels_of_the_oracle_and_the_host_form(ref, flow_cases):
    from oracle import np_label
    from tobac_flow_amd.utils import label_utils as host
    for name in gc.OVERLAPPING_CASES:
        mask, forward, backward, _ = flow_cases[name]
        flat = gc.expected_flat(name)
        back, fwd = gc.warped_labels(flat, forward, backward)
        bins, args = np.cumsum(np.bincount(flat.ravel())), np.argsort(flat.ravel())
        for (overlap, absolute), want in gc.expected_overlapping(name, gc.overlapping_grid(name)).items():
            for fn in (np_label.find_overlapping_labels, host.find_overlapping_labels):
                rows = [(d, label, int(m)) for d, warped in enumerate((fwd, back)) for label in range(1, bins.size)
                        for m in fn(warped, args[bins[label - 1]:bins[label]], bins, overlap, absolute)]
                assert np.array_equal(np.array(rows, np.int64).reshape(-1, 3), want), (name, overlap, absolute, fn.__module__)
    edge = gc.expected_overlapping("product_edge", gc.overlapping_grid("product_edge"))
    assert len(edge[(0.27, 0)]) == 2 and len(edge[(0.28, 0)]) == 0 and len(edge[(0, 6)]) == 2 and len(edge[(0, 7)]) == 0


def test_label_utils_host_forms_and_the_dataset_oracle(ref):
    from oracle import np_dataset
    from tobac_flow_amd.utils import label_utils as host
    for shape in gc.SHAPES:
        key = f"utils/{gc.shape_name(shape)}/"
        labels = gc.tile_labels(shape)
        step = host.make_step_labels(labels)
        assert np.array_equal(step, ref[key + "make_step_labels"]), shape
        assert step.max() > labels.max()                                             # pieces hold several labels and the reverse
        for fn in (host.slice_labels, np_dataset.slice_labels):
            assert np.array_equal(fn(labels.copy()), ref[key + "slice_labels"]), (shape, fn.__module__)
        assert np.array_equal(host.relabel_objects(gc.gappy(labels)), ref[key + "relabel_objects"]), shape
        in_place = gc.gappy(labels)
        assert host.relabel_objects(in_place, inplace=True) is in_place and np.array_equal(in_place, ref[key + "relabel_objects"])
        for form, (locations, new_labels) in gc.remap_arguments(labels).items():
            got = host.remap_labels(labels, locations, new_labels)
            assert got.dtype == labels.dtype and np.array_equal(got, ref[key + "remap_" + form]), (shape, form)
        locations, new_labels = gc.remap_arguments(labels)["int"]
        assert np.array_equal(np_dataset.remap_labels(labels, locations, new_labels), ref[key + "remap_int"]), shape
        got, want = host.get_step_labels_for_label(labels, step), gc.ragged(ref, key + "steps_for_label")
        assert len(got) == len(want) == labels.max()
        for g, w in zip(got, want):
            assert (g is None and w is None) or np.array_equal(g, w), shape


def test_window_rule_of_the_oracle_and_the_host_statement(ref):
    from oracle import np_label
    from tobac_flow_amd.parallel import _overlap_pairs_host
    for name, (left, right, grid) in gc.window_cases().items():
        n_left, n_right = int(left.max()), int(right.max())
        for (atol, rtol), (pairs, components) in gc.expected_window(name, grid).items():
            x, y = np_label.link_overlap_pairs(left, right, atol, rtol)
            assert np.array_equal(np.stack([x, y], 1).reshape(-1, 2), pairs), (name, atol, rtol)
            got = _overlap_pairs_host(left, right, atol, rtol)
            assert got.dtype == np.int64 and np.array_equal(got, pairs), (name, atol, rtol)
            nodes = gc.node_ids(pairs[:, 0], pairs[:, 1], n_left)
            assert np.array_equal(np_label.find_new_labels(*nodes, n_left + n_right + 1), components), (name, atol, rtol)
