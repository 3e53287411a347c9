"""Records tests/golden/ws_job_paths.json: what one flood job publishes -- return code, stats_host[0..15] and the job info
[0..11] after EVERY entry point (begin, sweeps, each finish), and a checksum of the labels -- on each path the host driver
of csrc/watershed.hip can take.  The inputs are the ones the existing tests reach these paths with
(test_gpu_reference_order.py, test_gpu_pipeline.py, test_gpu_edge_cases.py); here they go through the C ABI directly, so
that no memo of the Python side decides the path.  tests/test_gpu_ws_job_paths.py replays the same paths and compares.

Needs a GPU.  The file is recorded against the PARENT commit's library (TF_LIB_PATH), twice, in two processes:

    TF_LIB_PATH=<parent build> python tests/golden/make_ws_job_paths.py --record a.json
    TF_LIB_PATH=<parent build> python tests/golden/make_ws_job_paths.py --record b.json
    python tests/golden/make_ws_job_paths.py --pin a.json b.json --parent <commit> --out tests/golden/ws_job_paths.json

--pin keeps the first recording, lists the slots that may differ from run to run (sweep counts and the processed count hang
on the arrival order of atomics, the times on the clock) in the metadata, and refuses if any OTHER slot differs between the
two recordings."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

SKIP_FAST_PATH, REFERENCE_ORDER, DEFER_SWEEPS = 1, 2, 4
REPLAY_PENDING = 2
EXCLUDED_ST = [0, 1, 2, 3, 4, 7, 15]          # sweeps per phase, entries processed, microseconds of the detour
EXCLUDED_INFO = [5, 6]                        # microseconds of the export and of the replay
ENV_AIDS = ("TF_WS_REFERENCE_DENSE", "TF_WS_REFERENCE_HOST", "TF_WS_REFERENCE_NO_CODES")

# name -> (input, flags, guess, environment, how the entry points are driven, what makes the path the named one)
#   guess: None, an ordered key, or "covering": the tie key a flood of the same input without a guess reports
#   drive: "parts" begin + finish; "sweeps" begin (deferred) + tf_watershed_sweeps + finish; "one_call" tf_watershed_ex2;
#          "raveled" tf_watershed_raveled_ex
#   expect: {(vector, slot): value} of the LAST entry, and "finishes": how often finish is entered
PATHS = {
    "host_sparse": ("one_value_class", REFERENCE_ORDER | DEFER_SWEEPS, None, {"TF_WS_REFERENCE_HOST": "1"}, "sweeps",
                    {("info", 0): 1, ("info", 11): 0, "finishes": 2}),
    "host_dense_coded": ("E_const_plateau_c1", REFERENCE_ORDER | DEFER_SWEEPS, None, {"TF_WS_REFERENCE_DENSE": "1"}, "sweeps",
                         {("info", 0): 2, "finishes": 2}),
    "host_dense_list": ("E_const_plateau_c1", REFERENCE_ORDER | DEFER_SWEEPS, None,
                        {"TF_WS_REFERENCE_DENSE": "1", "TF_WS_REFERENCE_NO_CODES": "1"}, "sweeps", {("info", 0): 2, "finishes": 2}),
    "plain": ("E_const_plateau_c1", REFERENCE_ORDER | DEFER_SWEEPS, None, {"TF_WS_REFERENCE_DENSE": "2"}, "sweeps",
              {("info", 0): 2, "finishes": 2}),
    "device_no_guess": ("one_value_class", REFERENCE_ORDER | DEFER_SWEEPS, None, {}, "sweeps",
                        {("info", 0): 3, ("info", 8): 0, ("info", 11): 1, "finishes": 1}),
    "device_covering_guess": ("one_value_class", REFERENCE_ORDER | DEFER_SWEEPS, "covering", {}, "sweeps",
                              {("info", 0): 3, ("info", 8): 1, ("info", 9): 1, ("info", 11): 1, "finishes": 1}),
    "guess_too_low": ("E_const_plateau_c1", REFERENCE_ORDER | SKIP_FAST_PATH, 0, {}, "parts",
                      {("info", 8): 0, ("info", 9): 0, ("st", 12): 2, "finishes": 2}),
    "deferred_sweeps": ("E_const_plateau_c1", REFERENCE_ORDER | DEFER_SWEEPS, None, {}, "parts", {"finishes": 2}),
    "tie_free_fast_path": ("A_cont_c1", REFERENCE_ORDER, None, {}, "parts",
                           {("st", 13): 0, ("st", 14): 0, ("info", 0): 0, ("info", 7): -1, "finishes": 1}),
    "skip_fast_path": ("E_const_plateau_c1", REFERENCE_ORDER | SKIP_FAST_PATH, None, {}, "parts", {("st", 5): -1, ("st", 12): 2, "finishes": 2}),
    "one_call": ("E_const_plateau_c1", REFERENCE_ORDER, None, {}, "one_call", {}),
    "raveled": ("E_const_plateau_c1", REFERENCE_ORDER, None, {}, "raveled", {}),
    "no_relevant_pixels": ("single_seed", REFERENCE_ORDER, None, {}, "parts", {("st", 6): 0, ("st", 12): 0, ("info", 4): 0, "finishes": 1}),
}

_inputs = {}


def _input(name):
    """(fwd, bwd, field, markers, mask, connectivity) as numpy arrays, built once"""
    if name not in _inputs:
        if name == "one_value_class":
            from test_gpu_reference_order import _one_value_class_case
            _inputs[name] = _one_value_class_case(0)
        elif name == "single_seed":                              # test_watershed_degenerate_volumes: a seed with nothing to flood
            z = np.zeros((1, 1, 1, 2), np.float32)
            _inputs[name] = (z, z, np.zeros((1, 1, 1), np.float32), np.array([[[3]]], np.int32), None, 1)
        else:
            z = np.load(os.path.join(HERE, "watershed_ref.npz"))
            c = {k.split("/")[1]: z[k] for k in z.files if k.startswith(name + "/")}
            _inputs[name] = (c["fwd"], c["bwd"], c["field"], c["markers"], c.get("mask"), int(c["conn"]))
    return _inputs[name]


def _flood_parts(inp, flags, guess, call_sweeps):
    """tf_watershed_begin [/ _sweeps] / _replay / _finish until the job is done: the entries, the last code, the labels"""
    import ctypes
    import torch
    from tobac_flow_amd import _lib
    from tobac_flow_amd.watershed import DEFAULT_CHAIN_DEPTH, neighbour_offsets
    L = _lib.lib()
    fwd, bwd, field, markers, mask, conn = inp
    d = [_lib.to_dev(fwd, torch.float32), _lib.to_dev(bwd, torch.float32), _lib.to_dev(field, torch.float32), _lib.to_dev(markers, torch.int32),
         None if mask is None else _lib.to_dev(np.asarray(mask).astype(np.int8), torch.int8)]
    T, H, W = field.shape
    nbr = np.ascontiguousarray(neighbour_offsets(conn), np.int8)
    start, cap = DEFAULT_CHAIN_DEPTH, DEFAULT_CHAIN_DEPTH + 2
    ws = torch.empty(L.tf_watershed_workspace_bytes(T, H, W, len(nbr), cap, 0), dtype=torch.uint8, device="cuda")
    labels = torch.zeros((T, H, W), dtype=torch.int32, device="cuda")
    st, info = np.zeros(16, np.int64), np.zeros(12, np.int64)
    entries = []

    def note(call, rc, job):
        if job is not None:
            assert L.tf_watershed_job_info(job, info.ctypes.data_as(_lib._P)) == 0
        entries.append({"call": call, "rc": int(rc), "needs_replay": int(L.tf_watershed_needs_replay(job)) if job is not None else 0,
                        "st": st.tolist(), "info": info.tolist()})

    job = ctypes.c_void_p()
    rc = L.tf_watershed_begin(_lib.ptr(d[2]), _lib.ptr(d[3]), _lib.ptr(d[4]), _lib.ptr(d[0]), _lib.ptr(d[1]), T, H, W,
                              nbr.ctypes.data_as(_lib._P), len(nbr), start, cap, flags, -1 if guess is None else int(guess),
                              _lib.ptr(ws), ws.numel(), st.ctypes.data_as(_lib._P), _lib.stream_ptr(), ctypes.byref(job))
    assert rc == 0, (rc, L.tf_last_error())
    note("begin", rc, job)
    if call_sweeps:
        rc = L.tf_watershed_sweeps(job, st.ctypes.data_as(_lib._P))
        assert rc == 0, (rc, L.tf_last_error())
        note("sweeps", rc, job)
    for _ in range(3):
        if L.tf_watershed_needs_replay(job):
            assert L.tf_watershed_replay(job) == 0
        rc = L.tf_watershed_finish(job, _lib.ptr(labels), None, st.ctypes.data_as(_lib._P), info.ctypes.data_as(_lib._P))
        note("finish", rc, job if rc == REPLAY_PENDING else None)
        if rc != REPLAY_PENDING:
            break
    assert rc != REPLAY_PENDING, "finish asked for a replay three times"
    return entries, int(rc), labels.cpu().numpy()


def _flood_one_call(inp, flags):
    import torch
    from tobac_flow_amd import _lib
    from tobac_flow_amd.watershed import DEFAULT_CHAIN_DEPTH, neighbour_offsets
    L = _lib.lib()
    fwd, bwd, field, markers, mask, conn = inp
    d = [_lib.to_dev(fwd, torch.float32), _lib.to_dev(bwd, torch.float32), _lib.to_dev(field, torch.float32), _lib.to_dev(markers, torch.int32),
         None if mask is None else _lib.to_dev(np.asarray(mask).astype(np.int8), torch.int8)]
    T, H, W = field.shape
    nbr = np.ascontiguousarray(neighbour_offsets(conn), np.int8)
    start, cap = DEFAULT_CHAIN_DEPTH, DEFAULT_CHAIN_DEPTH + 2
    ws = torch.empty(L.tf_watershed_workspace_bytes(T, H, W, len(nbr), cap, 0), dtype=torch.uint8, device="cuda")
    labels = torch.zeros((T, H, W), dtype=torch.int32, device="cuda")
    st = np.zeros(16, np.int64)
    rc = L.tf_watershed_ex2(_lib.ptr(d[2]), _lib.ptr(d[3]), _lib.ptr(d[4]), _lib.ptr(d[0]), _lib.ptr(d[1]), T, H, W,
                            nbr.ctypes.data_as(_lib._P), len(nbr), start, cap, flags, _lib.ptr(labels), None, _lib.ptr(ws), ws.numel(),
                            st.ctypes.data_as(_lib._P), _lib.stream_ptr())
    return [{"call": "ex2", "rc": int(rc), "needs_replay": 0, "st": st.tolist(), "info": None}], int(rc), labels.cpu().numpy()


def _flood_raveled(inp, flags):
    """test_the_raveled_twin_in_reference_order, with the whole statistics vector"""
    import torch
    from oracle import ws_oracle
    from tobac_flow_amd import _lib
    from tobac_flow_amd.watershed import MAX_CHAIN_DEPTH
    L = _lib.lib()
    fwd, bwd, field, markers, mask, conn = inp
    p = ws_oracle.prepare(fwd, bwd, field, markers, mask, conn)
    image = np.ascontiguousarray(p["field"].ravel(), np.float32)
    n = image.size
    structure = np.ascontiguousarray(p["nbr"], np.int64)
    floc, bloc = np.ascontiguousarray(p["fwd_loc"], np.int32), np.ascontiguousarray(p["bwd_loc"], np.int32)
    strides = np.ascontiguousarray(p["strides"], np.int32)
    d_img, d_loc = _lib.to_dev(image), _lib.to_dev(np.ascontiguousarray(p["markers"], np.int64))
    d_fo, d_bo = _lib.to_dev(np.ascontiguousarray(p["fwd_off"].ravel(), np.int32)), _lib.to_dev(np.ascontiguousarray(p["bwd_off"].ravel(), np.int32))
    d_mask, d_out = _lib.to_dev(np.ascontiguousarray(p["mask"].ravel(), np.int8)), _lib.to_dev(np.ascontiguousarray(p["out"].ravel(), np.int32))
    ws = torch.empty(L.tf_watershed_raveled_workspace_bytes(n, structure.size, MAX_CHAIN_DEPTH, 0), dtype=torch.uint8, device="cuda")
    st = np.zeros(16, np.int64)
    rc = L.tf_watershed_raveled_ex(_lib.ptr(d_img), n, _lib.ptr(d_loc), p["markers"].size, structure.ctypes.data_as(_lib._P), structure.size,
                                   _lib.ptr(d_fo), _lib.ptr(d_bo), floc.ctypes.data_as(_lib._P), bloc.ctypes.data_as(_lib._P), _lib.ptr(d_mask),
                                   strides.ctypes.data_as(_lib._P), strides.size, 0.0, _lib.ptr(d_out), 0, MAX_CHAIN_DEPTH, flags,
                                   _lib.ptr(ws), ws.numel(), st.ctypes.data_as(_lib._P), _lib.stream_ptr())
    return [{"call": "raveled_ex", "rc": int(rc), "needs_replay": 0, "st": st.tolist(), "info": None}], int(rc), d_out.cpu().numpy()


def run_path(name):
    """one path of PATHS on the library that is loaded -> {"rc", "labels_sha1", "entries"}; checks that it IS that path"""
    inp_name, flags, guess, env, drive, expect = PATHS[name]
    inp = _input(inp_name)
    saved = {k: os.environ.pop(k, None) for k in ENV_AIDS}
    try:
        if guess == "covering":                                   # the tie key a flood without a guess finds (the memo of the Python side)
            guess = _flood_parts(inp, flags, None, True)[0][-1]["info"][7]
            assert guess >= 0, "the input has no tie between equal-valued markers"
        os.environ.update(env)
        if drive == "one_call":
            entries, rc, labels = _flood_one_call(inp, flags)
        elif drive == "raveled":
            entries, rc, labels = _flood_raveled(inp, flags)
        else:
            entries, rc, labels = _flood_parts(inp, flags, guess, drive == "sweeps")
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert rc == 0, (name, rc)                                  # reference order applied (or nothing to apply): TF_OK on every path
    last = entries[-1]
    for key, want in expect.items():
        if key == "finishes":
            got = sum(e["call"] == "finish" for e in entries)
        else:
            got = last[key[0]][key[1]]
        assert got == want, (name, key, got, want, last)
    return {"rc": rc, "labels_sha1": hashlib.sha1(np.ascontiguousarray(labels, np.int32).tobytes()).hexdigest(), "entries": entries}


def pinned(result, excluded_st=EXCLUDED_ST, excluded_info=EXCLUDED_INFO):
    """a result of run_path without the slots that may differ from run to run"""
    out = {"rc": result["rc"], "labels_sha1": result["labels_sha1"], "entries": []}
    for e in result["entries"]:
        out["entries"].append({"call": e["call"], "rc": e["rc"], "needs_replay": e["needs_replay"],
                               "st": [v for i, v in enumerate(e["st"]) if i not in excluded_st],
                               "info": None if e["info"] is None else [v for i, v in enumerate(e["info"]) if i not in excluded_info]})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--record", metavar="OUT", help="run every path once on the loaded library and write the raw recording")
    ap.add_argument("--pin", nargs=2, metavar=("A", "B"), help="two raw recordings -> the golden file")
    ap.add_argument("--parent", help="commit the recordings were made at")
    ap.add_argument("--out", help="the golden file (--pin)")
    a = ap.parse_args()
    if a.record:
        rec = {name: run_path(name) for name in PATHS}
        os.makedirs(os.path.dirname(os.path.abspath(a.record)), exist_ok=True)
        with open(a.record, "w") as f:
            json.dump(rec, f, indent=1)
        for name, r in rec.items():
            print(name, r["rc"], r["labels_sha1"][:12], [(e["call"], e["rc"]) for e in r["entries"]], "st", r["entries"][-1]["st"], "info", r["entries"][-1]["info"])
    elif a.pin:
        ra, rb = (json.load(open(p)) for p in a.pin)
        bad = [name for name in PATHS if pinned(ra[name]) != pinned(rb[name])]
        for name in bad:
            print("DIFFERS outside the excluded slots:", name, "\n ", pinned(ra[name]), "\n ", pinned(rb[name]))
        if bad:
            sys.exit(1)
        gold = {"meta": {"recorded_at_commit": a.parent, "recordings_compared": 2, "excluded_st": EXCLUDED_ST, "excluded_info": EXCLUDED_INFO,
                         "why_excluded": "st[0..4] sweeps per phase and st[7] entries processed hang on the arrival order of atomics; "
                                         "st[15], info[5], info[6] are times on the host clock"},
                "paths": {name: ra[name] for name in PATHS}}
        with open(a.out, "w") as f:
            json.dump(gold, f, indent=1)
            f.write("\n")
        print("pinned", len(PATHS), "paths ->", a.out)
    else:
        ap.error("--record or --pin")


if __name__ == "__main__":
    main()
