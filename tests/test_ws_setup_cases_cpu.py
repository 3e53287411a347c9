"""The restatement of the watershed set-up (tests/ws_setup_cases.py) against the oracle's flood, on the CPU, and the
conditions that keep its cases from degrading without notice."""
import os
import re

import numpy as np
import pytest

import ws_setup_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nbrs():
    return wc.neighbour_lists()


def test_case_list_and_neighbour_lists_are_what_the_gpu_tests_parametrise_over(nbrs):
    assert list(wc.cases()) == wc.CASE_NAMES and tuple(nbrs) == wc.NEIGHBOUR_LISTS
    assert {c["shape"] for c in wc.cases().values()} == set(wc.TINY + wc.SHAPES)
    faces = {tuple(o) for o in nbrs["conn1"].tolist()}
    assert {tuple(o) for o in nbrs["faces_reversed"].tolist()} == faces and nbrs["faces_reversed"].tolist() != nbrs["conn1"].tolist()
    assert not ({tuple(o) for o in nbrs["diagonals6"].tolist()} & faces) - {(-1, 0, 0), (1, 0, 0)}
    assert sorted(np.abs(nbrs["diagonals6"]).sum(1).tolist()) == [1, 1, 2, 2, 2, 2]
    for c in wc.cases().values():
        assert c["field"].dtype == np.float32 and c["markers"].dtype == np.int32 and c["fwd"].dtype == c["bwd"].dtype == np.float32
        assert c["mask"] is None or c["mask"].dtype == np.int8
        assert c["fwd"].shape == c["bwd"].shape == c["shape"] + (2,)
        assert np.unique(c["field"]).size == c["field"].size                     # continuous values: no ties
        nan = np.isnan(c["fwd"]).any() or np.isnan(c["bwd"]).any()
        assert not nan or (c["family"] == "blobs" and "zero_flow" not in c["name"]), c["name"]
        assert nan or not (c["family"] == "blobs" and "zero_flow" not in c["name"] and c["field"].size >= 512), c["name"]
        values = np.concatenate([c["fwd"].ravel(), c["bwd"].ravel()])
        assert set(values[~np.isnan(values)].tolist()) <= set(wc.FLOW_VALUES.tolist())
    zero = wc.cases()["blobs_3x17x20_zero_flow"]
    assert not zero["fwd"].any() and not zero["bwd"].any()


def test_round_flow_is_half_to_even_and_nan_is_zero():
    got = wc.round_flow(np.array([-20, -7.5, -2.5, -1.5, -0.5, 0, 0.5, 1.5, 2.5, 3.5, 20, np.nan], np.float32))
    assert got.tolist() == [-20, -8, -2, -2, 0, 0, 0, 2, 2, 4, 20, 0]


@pytest.mark.parametrize("nbr_name", ["conn3", "diagonals6", "faces_reversed"])
def test_vectorised_restatement_equals_the_definition_voxel_by_voxel(nbrs, nbr_name):
    for name, c in wc.cases().items():
        if c["field"].size <= 3 * 17 * 20:
            assert np.array_equal(wc.relevant(c, nbrs[nbr_name]), wc.relevant_by_loops(c, nbrs[nbr_name])), name


@pytest.mark.parametrize("nbr_name", wc.NEIGHBOUR_LISTS)
@pytest.mark.parametrize("name", wc.CASE_NAMES)
def test_irrelevant_markers_can_be_masked_out_without_changing_any_other_label(nbrs, name, nbr_name):
    """The oracle's labels with every irrelevant marker taken out (markers = 0, mask = 0 there) equal the original labels at
    every other voxel, and each irrelevant marker keeps its own id in the original: a marker the restatement calls
    irrelevant takes no part in the flood."""
    from oracle import ws_oracle
    c = wc.cases()[name]
    rel = wc.relevant(c, nbrs[nbr_name])
    irrelevant = (c["markers"] != 0) & ~rel
    want = wc.oracle_labels(name, nbr_name)
    assert np.array_equal(want[irrelevant], c["markers"][irrelevant])
    markers, mask = c["markers"].copy(), np.ones(c["shape"], np.int8) if c["mask"] is None else c["mask"].copy()
    markers[irrelevant] = 0
    mask[irrelevant] = 0
    got = ws_oracle.watershed(wc.nan_to_zero(c["fwd"]), wc.nan_to_zero(c["bwd"]), c["field"], markers, mask, offsets=nbrs[nbr_name])
    assert np.array_equal(got[~irrelevant], want[~irrelevant])
    assert not got[irrelevant].any()


@pytest.mark.parametrize("nbr_name", wc.NEIGHBOUR_LISTS)
def test_every_case_holds_what_it_was_built_for(nbrs, nbr_name):
    offsets = nbrs[nbr_name]
    for name, c in wc.cases().items():
        rel, marker = wc.relevant(c, offsets), c["markers"] != 0
        if c["family"] == "blobs":
            assert (marker & ~rel).any() and (marker & rel).any(), name
            assert (c["mask"] == 0).any() and (~marker & (c["mask"] != 0)).any(), name
        if c["family"] == "temporal":
            only = wc.temporal_only(c, offsets)
            assert only.any() and (marker & ~rel).any(), name
            assert np.array_equal(only, marker & rel), name                       # no marker has a floodable in-plane neighbour
            assert marker[::2].all() and not marker[1::2].any()
            # the displaced targets land on floodable voxels, on masked ones and outside the volume
            cls = wc.classes(c["markers"], c["mask"])
            assert (cls[1::2] == 0).any() and (cls[1::2] == 1).any()
    big = wc.cases()["blobs_3x33x48"]
    assert (big["markers"] < 0).any() and len(np.unique(big["markers"])) >= 8


def test_the_six_by_four_path_meets_all_four_bytes_of_a_quad_undecided():
    """W % 4 == 0 temporal cases: every aligned quad of a marker frame is four markers without a floodable in-plane neighbour
    (`need` = all four bytes in k_ws_relevant6x4), and the four answers differ within some quads"""
    offsets = wc.neighbour_lists()["conn1"]
    for name in ("temporal_2x16x16", "temporal_3x17x20", "temporal_3x33x48"):
        c = wc.cases()[name]
        assert c["shape"][2] % 4 == 0
        quads = wc.relevant(c, offsets)[::2].reshape(-1, 4)
        assert 0 < (quads.any(1) & ~quads.all(1)).sum()
        for j in range(4):                                                        # each byte position decides on its own somewhere
            others = np.delete(quads, j, 1)
            assert (quads[:, j] & ~others.any(1)).any() or (~quads[:, j] & others.all(1)).any(), (name, j)


def test_relevant_counts_of_the_retry_volumes():
    """the figures tests/test_gpu_ws_setup.py expects of the Python retry: (4, 64, 64), zero flows, connectivity 1, markers
    everywhere except [:, ::2, ::2]"""
    shape = (4, 64, 64)
    markers = np.ones(shape, np.int32)
    markers[:, ::2, ::2] = 0
    z = np.zeros(shape + (2,), np.float32)
    case = dict(markers=markers, mask=None, fwd=z, bwd=z)
    rel = wc.relevant(case, wc.neighbour_lists()["conn1"])
    floodable = int((markers == 0).sum())
    assert floodable == 4096 and int(rel.sum()) == 12288
    assert min(markers.size, int(floodable * 1.5) + 4096) == 10240 < 12288         # the first guess of watershed_begin


def test_alignment_contract_is_declared():
    from tobac_flow_amd import _lib
    assert _lib.lib().tf_version() >= 114
    header = open(os.path.join(ROOT, "include", "tobac_flow_hip.h")).read()
    header = re.sub(r"[\s*]+", " ", header)
    assert "fwd and bwd 8-byte aligned" in header and "field and markers 4-byte aligned" in header
