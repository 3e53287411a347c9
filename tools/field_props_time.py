"""Time the fifth stage (cloud and flux properties per object, tobac_flow_amd.postprocess) on a synthetic SEVIRI-sized
T x N^2 product, device-resident: three step-label volumes of discs (2.4 % of the voxels labelled, one id per disc and
frame), float32 fields and a float64 (N, N) area plane as weights -- the production dtype mix.  HIP events, operands
allocated beforehand, the median of 5 after one warm-up.

  figure a  the flux stage, add_flux_properties (the scripts' twenty variables x 3 step volumes), against the SAME stage
            composed from add_cre_to_dataset and the loop of add_weighted_stats_to_dataset in the same process -- the only
            way to run it without this stage, and so the baseline; the results of the two are compared.  Then the cloud
            stage likewise (cloud_quality_weights, eleven variables of which seven have uncertainties, five flags).
  figure b  tf_flux_cre alone against the 23 planes it moves, and one tf_label_wstats_multi call (init, two passes, finish)
            of the BOA set, the TOA set and 8 / 3 / 1 plain planes against the bytes its two passes read -- all operands,
            and the labels alone, which is what a step without a labelled voxel costs; the BOA set and tf_label_wstats
            of one field also on a volume without any labelled voxel -- next to tf_copy16 in the same run.

Usage: python tools/field_props_time.py [all|kernels] [N] [T] [output file] (development aid; the figures are kept in
profiles/field_properties.txt)"""
import statistics
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

from tobac_flow_amd import _lib, postprocess as pp
from tobac_flow_amd.dataset import LabelDataset

MODE = sys.argv[1] if len(sys.argv) > 1 else "all"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 3712
T = int(sys.argv[3]) if len(sys.argv) > 3 else 16
OUT = open(sys.argv[4], "w") if len(sys.argv) > 4 else None
WARM, RUNS = 1, 5
CELL, RADIUS = 155, 13.5                                          # pi 13.5^2 / 155^2 = 2.4 %
FLAGS = {"lsflag": (0, 1), "lusflag": (0, 1, 2), "illum": (1, 2, 3), "cldtype": (0, 1, 2, 3, 4), "phase": (0, 1, 2)}
UNCERTAIN = ("cot", "cer", "ctp", "cth", "ctt", "stemp", "cwp")


def say(*words):
    line = " ".join(str(w) for w in words)
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n")
        OUT.flush()


def events(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median(f):
    for _ in range(WARM):
        f()
    ts = [events(f) for _ in range(RUNS)]
    return statistics.median(ts), min(ts), max(ts)


def product():
    """the dcc dataset with three step-label volumes of discs (shifted against each other) and their coordinates"""
    dev = _lib.device()
    dcc = LabelDataset()
    cells = (N + CELL - 1) // CELL
    frames = torch.arange(T, device=dev, dtype=torch.int32)[:, None, None]
    for k, dim in enumerate(pp.STEP_DIMS):
        p = torch.arange(N, device=dev, dtype=torch.int32) + 40 * k
        cell, off = p // CELL, (p % CELL - CELL // 2).float()
        disc = off[:, None] ** 2 + off[None, :] ** 2 < RADIUS ** 2
        ids = 1 + (cell[:, None] % cells) * cells + (cell[None, :] % cells)
        volume = torch.where(disc[None], frames * (cells * cells) + ids[None], torch.zeros((), dtype=torch.int32, device=dev))
        dcc.add(f"{dim}_label", volume.to(torch.int32).contiguous(), ("t", "y", "x"))
        dcc.coords[dim] = np.arange(1, T * cells * cells + 1, dtype=np.int32)
    return dcc


def planes(names, seed):
    g = torch.Generator(device=_lib.device()).manual_seed(seed)
    return {n: torch.randn((T, N, N), generator=g, device=_lib.device(), dtype=torch.float32) * 120 + 80 for n in names}


def area_plane():
    y, x = np.linspace(0.12, -0.12, N), np.linspace(-0.12, 0.12, N)
    yy, xx = np.meshgrid(y, x, indexing="ij")
    return torch.from_numpy(9.0 / np.cos(2.0 * yy + xx) ** 2).to(_lib.device())      # float64, as the geodesy returns it


def stat_names(ds):
    return [n for n in ds if not n.endswith("_label")]


def compare(got, want, what):
    names = stat_names(want)
    assert stat_names(got) == names, what
    worst = 0.0
    for n in names:
        a, b = np.asarray(got[n], np.float64), np.asarray(want[n], np.float64)
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, n)
        if n.endswith(("_min", "_max", "_min_error", "_max_error")):
            assert np.array_equal(a, b, equal_nan=True), (what, n)
        else:
            ok = ~np.isnan(b) & (b != 0)
            worst = max(worst, float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]), initial=0.0)))
    say(f"figure a: {what}: {len(names)} results, the same names in the same order; NaN patterns, min, max and the errors at them "
        f"equal; largest relative difference of a summed result {worst:.2e} (results are stored as float32: 6e-8 is one rounding)")


def figure_a(dcc, area):
    labelled = float(np.mean([float((dcc[f"{d}_label"] != 0).float().mean()) for d in pp.STEP_DIMS]))
    say(f"{T} x {N}^2 product on the device, {labelled * 100:.2f} % of the voxels labelled, {dcc.coords[pp.STEP_DIMS[0]].size} ids per "
        f"step volume; float32 fields, float64 ({N}, {N}) area plane")
    raw = pp._SET_PLANES["TOA"] + pp._SET_PLANES["BOA"] + ("lts", "fth", "cbh")
    flx = planes(raw, 1)
    results = {}

    def fused():
        results["fused"] = pp.add_flux_properties(LabelDataset(dcc, coords=dict(dcc.coords)), flx, area)

    def composed():
        ds = LabelDataset(dcc, coords=dict(dcc.coords))
        full = pp.add_cre_to_dataset(dict(flx))
        for var in pp.FLUX_VARIABLES:
            for dim in pp.STEP_DIMS:
                pp.add_weighted_stats_to_dataset(ds, full, area, var, dim)
        results["composed"] = ds

    f, c = median(fused), median(composed)
    say(f"figure a: flux stage, 20 variables x 3 step volumes: add_flux_properties median {f[0]:.1f} ms (min {f[1]:.1f}, max {f[2]:.1f}); "
        f"composed from add_cre_to_dataset + 60 add_weighted_stats_to_dataset calls median {c[0]:.1f} ms (min {c[1]:.1f}, max {c[2]:.1f}); "
        f"ratio {c[0] / f[0]:.2f}")
    compare(results["fused"], results["composed"], "flux stage")
    del flx, results
    torch.cuda.empty_cache()

    cld = planes(pp.CLOUD_VARIABLES + tuple(f"{v}_uncertainty" for v in UNCERTAIN), 2)
    cld["cth"] = cld["cth"] * 0.1 + 4                             # km: most of it below 30
    g = torch.Generator(device=_lib.device()).manual_seed(3)
    for name, values in FLAGS.items():
        cld[name] = torch.randint(0, max(values) + 1, (T, N, N), generator=g, device=_lib.device(), dtype=torch.int8)
    qcflag = (torch.rand((T, N, N), generator=g, device=_lib.device()) < 0.1).to(torch.int32)
    w = median(lambda: pp.cloud_quality_weights(area, qcflag, cld["cth"], cld["cot"]))
    say(f"figure a: cloud_quality_weights (float64 plane in, float64 volume out): median {w[0]:.2f} ms (min {w[1]:.2f}, max {w[2]:.2f}) = "
        f"{(4 + 4 + 4 + 8) * T * N * N / 1e9 / w[0] * 1e3:.0f} GB/s of the 20 B per voxel it moves")
    weights = pp.cloud_quality_weights(area, qcflag, cld["cth"], cld["cot"])
    results = {}

    def fused_cloud():
        results["fused"] = pp.add_cloud_properties(LabelDataset(dcc, coords=dict(dcc.coords)), cld, weights, flags=FLAGS)

    def composed_cloud():
        ds = LabelDataset(dcc, coords=dict(dcc.coords))
        for var in pp.CLOUD_VARIABLES:
            for dim in pp.STEP_DIMS:
                pp.add_weighted_stats_to_dataset(ds, cld, weights, var, dim)
        for name, values in FLAGS.items():
            for dim in pp.STEP_DIMS:
                pp.add_weighted_proportions_to_dataset(ds, cld[name], weights, dim, flag_values=values, name=name)
        results["composed"] = ds

    def proportions_only():
        ds = LabelDataset(dcc, coords=dict(dcc.coords))
        for name, values in FLAGS.items():
            for dim in pp.STEP_DIMS:
                pp.add_weighted_proportions_to_dataset(ds, cld[name], weights, dim, flag_values=values, name=name)

    f, c, p = median(fused_cloud), median(composed_cloud), median(proportions_only)
    say(f"figure a: cloud stage, 11 variables (7 with uncertainties) + 5 flags x 3 step volumes, float64 weight volume: "
        f"add_cloud_properties median {f[0]:.1f} ms (min {f[1]:.1f}, max {f[2]:.1f}); composed from 33 add_weighted_stats_to_dataset + 15 "
        f"add_weighted_proportions_to_dataset calls median {c[0]:.1f} ms (min {c[1]:.1f}, max {c[2]:.1f}); ratio {c[0] / f[0]:.2f}; the 15 "
        f"proportion calls, which both forms make alike, {p[0]:.1f} ms of each")
    compare(results["fused"], results["composed"], "cloud stage")


def figure_b(dcc, area):
    L, dev = _lib.lib(), _lib.device()
    n_vox = T * N * N
    src = planes(pp._SET_PLANES["TOA"] + pp._SET_PLANES["BOA"], 4)
    ins = [src[n] for n in pp._SET_PLANES["TOA"] + pp._SET_PLANES["BOA"]]
    outs = [torch.empty_like(ins[0]) for _ in range(10)]
    pi, po = pp._pointers(ins), pp._pointers(outs)
    m = median(lambda: _lib.check(L.tf_flux_cre(pi, po, _lib.TF_F32, n_vox, _lib.stream_ptr()), "tf_flux_cre"))
    gb = 23 * 4 * n_vox / 1e9
    say(f"figure b: tf_flux_cre, 13 float32 planes in and 10 out: median {m[0]:.3f} ms (min {m[1]:.3f}, max {m[2]:.3f}) = "
        f"{gb / m[0] * 1e3:.0f} GB/s of the {gb:.2f} GB it moves")
    del outs
    lab = dcc[f"{pp.STEP_DIMS[0]}_label"]
    n_labels = int(dcc.coords[pp.STEP_DIMS[0]].size)
    empty = torch.zeros_like(lab)                                 # no labelled voxel: what streaming the labels alone costs

    def multi(what, set_id, names, labels, n_fields):
        tensors = [src[n] for n in names]
        ptrs = pp._pointers(tensors)
        out = torch.empty((n_fields, n_labels, 10), dtype=torch.float64, device=dev)
        ws = torch.empty(L.tf_label_wstats_multi_workspace_bytes(set_id, len(names), n_labels), dtype=torch.uint8, device=dev)
        m = median(lambda: _lib.check(L.tf_label_wstats_multi(_lib.ptr(labels), set_id, ptrs, None, len(names), _lib.ptr(area), _lib.TF_F32,
                                                              _lib.TF_F64, T, N * N, 1, n_labels, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                                              _lib.stream_ptr()), "tf_label_wstats_multi"))
        every, least = 2 * (4 + len(names) * 4 + 8) * n_vox / 1e9, 2 * 4 * n_vox / 1e9
        say(f"figure b: tf_label_wstats_multi, {what} ({len(names)} float32 planes -> {n_fields} fields, float64 plane weights, {n_labels} ids): "
            f"whole call (init, two passes, finish) median {m[0]:.3f} ms (min {m[1]:.3f}, max {m[2]:.3f}), {m[0] / 2:.3f} ms per pass, "
            f"{m[0] / n_fields:.3f} ms per field = {every / m[0] * 1e3:.0f} GB/s of the {every:.2f} GB of all operands twice, "
            f"{least / m[0] * 1e3:.0f} GB/s of the {least:.2f} GB of the labels twice (planes are loaded only in steps that hold a labelled voxel)")

    toa, boa = pp._SET_PLANES["TOA"], pp._SET_PLANES["BOA"]
    multi("BOA set", _lib.TF_FIELDS_BOA, boa, lab, 10)
    multi("BOA set on a volume WITHOUT labelled voxels", _lib.TF_FIELDS_BOA, boa, empty, 10)
    multi("TOA set", _lib.TF_FIELDS_TOA, toa, lab, 7)
    multi("PLAIN, 8 planes", _lib.TF_FIELDS_PLAIN, boa, lab, 8)
    multi("PLAIN, 3 planes", _lib.TF_FIELDS_PLAIN, boa[:3], lab, 3)
    multi("PLAIN, 1 plane", _lib.TF_FIELDS_PLAIN, boa[:1], lab, 1)
    one = src["boa_swdn"]
    out1 = torch.empty((n_labels, 10), dtype=torch.float64, device=dev)
    ws1 = torch.empty(L.tf_label_wstats_workspace_bytes(n_labels), dtype=torch.uint8, device=dev)
    one64 = one.double()
    m1 = median(lambda: _lib.check(L.tf_label_wstats(_lib.ptr(lab), _lib.ptr(one64), None, _lib.ptr(area), _lib.TF_F64, T, N * N, 1, n_labels,
                                                     _lib.ptr(out1), _lib.ptr(ws1), ws1.numel(), _lib.stream_ptr()), "tf_label_wstats"))
    m0 = median(lambda: _lib.check(L.tf_label_wstats(_lib.ptr(empty), _lib.ptr(one64), None, _lib.ptr(area), _lib.TF_F64, T, N * N, 1, n_labels,
                                                     _lib.ptr(out1), _lib.ptr(ws1), ws1.numel(), _lib.stream_ptr()), "tf_label_wstats"))
    say(f"figure b: tf_label_wstats of ONE field on a volume WITHOUT labelled voxels: median {m0[0]:.3f} ms (min {m0[1]:.3f}, max {m0[2]:.3f})")
    up = median(lambda: one.double())
    say(f"figure b: tf_label_wstats of ONE field (float64, as the mixed dtypes make it): median {m1[0]:.3f} ms (min {m1[1]:.3f}, max {m1[2]:.3f}); "
        f"the float32 -> float64 copy of a field before it: median {up[0]:.3f} ms")
    del one64
    a = torch.empty(2 * n_vox, dtype=torch.float32, device=dev).zero_()
    b = torch.empty_like(a)
    m = median(lambda: _lib.check(L.tf_copy16(_lib.ptr(a), _lib.ptr(b), a.numel() * 4, _lib.stream_ptr()), "tf_copy16"))
    say(f"figure b: tf_copy16 of {a.numel() * 4 / 1e9:.2f} GB: median {m[0]:.3f} ms = {2 * a.numel() * 4 / 1e9 / m[0] * 1e3:.0f} GB/s read + written")


if __name__ == "__main__":
    dcc, area = product(), area_plane()
    if MODE == "all":
        figure_a(dcc, area)
        _lib.release_workspaces()
        torch.cuda.empty_cache()
    figure_b(dcc, area)
