"""What one flood job publishes on every path of the host driver in csrc/watershed.hip -- the return code of each entry
point, stats_host[0..15] and the job info [0..11] after begin, sweeps and each finish, and the labels -- against
tests/golden/ws_job_paths.json, recorded twice at the commit named in its metadata (tests/golden/make_ws_job_paths.py).
The other flood tests assert a few statistics per path; a value that lands in the wrong slot passes them.  Slots that hang
on the arrival order of atomics (sweep counts, entries processed) or on the clock are listed in the metadata and skipped;
every other slot, every code and every label is compared for equality."""
import importlib.util
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_ws_job_paths", os.path.join(HERE, "golden", "make_ws_job_paths.py"))
paths = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(paths)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "ws_job_paths.json")) as f:
        return json.load(f)


def test_the_golden_file_covers_every_path(golden):
    assert sorted(golden["paths"]) == sorted(paths.PATHS)
    assert golden["meta"]["excluded_st"] == paths.EXCLUDED_ST and golden["meta"]["excluded_info"] == paths.EXCLUDED_INFO


@pytest.mark.parametrize("name", list(paths.PATHS))
def test_every_entry_point_publishes_what_it_published_at_the_recording(golden, name):
    meta = golden["meta"]
    got = paths.pinned(paths.run_path(name), meta["excluded_st"], meta["excluded_info"])
    want = paths.pinned(golden["paths"][name], meta["excluded_st"], meta["excluded_info"])
    assert got["rc"] == want["rc"]
    assert [(e["call"], e["rc"], e["needs_replay"]) for e in got["entries"]] == [(e["call"], e["rc"], e["needs_replay"]) for e in want["entries"]]
    for g, w in zip(got["entries"], want["entries"]):
        assert g["st"] == w["st"], (name, g["call"], "stats_host without " + str(meta["excluded_st"]))
        assert g["info"] == w["info"], (name, g["call"], "job info without " + str(meta["excluded_info"]))
    assert got["labels_sha1"] == want["labels_sha1"], name
