"""Time the second stage (tobac_flow_amd/linking.py) on one GPU.

(a) tf_relabel_merge on a T x N^2 window that shares SHARED frames with the previous and with the next window, `share` of
    its voxels labelled (3-D components of the cold tops of tools/synth.blob_stack, the threshold set to reach the share),
    against the same result composed from the entry points the tree had before it: index_select of the neighbours' shared
    frames, three tf_apply_lut, two torch.where on the shared frames.  Raw entry points, tables on the device; the rate of
    tf_copy16 over buffers of the window's size in the same run is the ceiling.
(b) process_file on the middle one of three windows of T x H x W cut from one sequence, device-resident and on NumPy
    containers (host remap and merges, uploads inside dataset.py's functions).

Each sample is REPS back-to-back calls between two device synchronises, divided by REPS; median of RUNS samples after WARM
warm-ups, the two forms of (a) alternating.
Usage: python tools/linking_time.py [N] [T] [H] [W] [a|b|ab] [output file] (development aid; figures in profiles/linking.txt)"""
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import numpy as np
import torch

from tobac_flow_amd import _lib, linking, ndimage_dev as nd
from tobac_flow_amd.dataset import LabelDataset

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5424
T = int(sys.argv[2]) if len(sys.argv) > 2 else 16
H = int(sys.argv[3]) if len(sys.argv) > 3 else 1500
W = int(sys.argv[4]) if len(sys.argv) > 4 else 2500
WHICH = sys.argv[5] if len(sys.argv) > 5 else "ab"
OUT = open(sys.argv[6], "w") if len(sys.argv) > 6 else None
SHARED, SHARE = 4, 0.024
WARM, RUNS, REPS = 2, 7, 100


def say(line=""):
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n")
        OUT.flush()


def sample(f, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def medians(forms, reps=REPS, runs=RUNS, warm=WARM):
    """{name: (median, min, max) ms} of the forms, alternating"""
    ts = {name: [] for name in forms}
    for k in range(warm + runs):
        for name, f in forms.items():
            ms = sample(f, reps)
            if k >= warm:
                ts[name].append(ms)
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ts.items()}


def cold_labels(bt, share):
    """3-D components of the coldest `share` of the voxels (the threshold from a strided sample)"""
    thr = torch.quantile(bt.flatten()[::997][:4_000_000].float(), share)
    labels, n = nd.label(bt < thr)
    return labels, int(n)


def part_a():
    from synth import blob_stack
    L = _lib.lib()
    own, n_own = cold_labels(torch.nan_to_num(blob_stack(T, N, N), nan=290.0), SHARE)
    share = float((own != 0).float().mean())
    gen = torch.Generator(device="cuda").manual_seed(11)

    def neighbour(frames):
        """the window's own frames under other ids, a tenth of the objects missing"""
        table = torch.randperm(n_own, generator=gen, device="cuda").to(torch.int32) + 1
        table[torch.rand(n_own, generator=gen, device="cuda") < 0.1] = 0
        table = torch.cat([torch.zeros(1, dtype=torch.int32, device="cuda"), table])
        return table[own[frames].long()].contiguous()
    prev, nxt = neighbour(slice(0, SHARED)), neighbour(slice(T - SHARED, T))
    own = own.clone()
    own[:SHARED][torch.rand((SHARED, N, N), generator=gen, device="cuda") < 0.3] = 0      # something for the merge to fill
    own[T - SHARED:][torch.rand((SHARED, N, N), generator=gen, device="cuda") < 0.3] = 0
    luts = [torch.cat([torch.zeros(1, dtype=torch.int32, device="cuda"),
                       torch.randint(1, 3 * n_own, (n_own,), generator=gen, device="cuda", dtype=torch.int32)]) for _ in range(3)]
    prev_frame = np.full(T, -1, np.int32)
    prev_frame[:SHARED - 1] = np.arange(SHARED - 1)                  # the previous product gives all shared frames but the last
    next_frame = np.full(T, -1, np.int32)
    next_frame[T - SHARED + 1:] = np.arange(1, SHARED)               # the next one all but the first
    pf, nf = torch.from_numpy(prev_frame).cuda(), torch.from_numpy(next_frame).cuda()
    out = torch.empty_like(own)
    status = torch.zeros(2, dtype=torch.int64, device="cuda")
    hw, n_lut = N * N, n_own + 1
    say(f"(a) {T} x {N}^2 window, {SHARED} frames shared on each side ({SHARED - 1} merged from each neighbour), "
        f"{share * 100:.2f} % of the voxels labelled, {n_own} ids (tables of {4 * n_lut / 1e3:.0f} KB)")

    def fused():
        _lib.check(L.tf_relabel_merge(_lib.ptr(own), T, hw, _lib.ptr(luts[0]), n_lut, _lib.ptr(prev), SHARED, _lib.ptr(pf),
                                      _lib.ptr(luts[1]), n_lut, _lib.ptr(nxt), SHARED, _lib.ptr(nf), _lib.ptr(luts[2]), n_lut,
                                      _lib.ptr(out), _lib.ptr(status), _lib.stream_ptr()), "tf_relabel_merge")

    def apply_lut(labels, lut):
        res = torch.empty_like(labels)
        _lib.check(L.tf_apply_lut(_lib.ptr(labels), labels.numel(), _lib.ptr(lut), n_lut, _lib.ptr(res), _lib.stream_ptr()), "tf_apply_lut")
        return res
    ip = torch.arange(0, SHARED - 1, device="cuda")
    inx = torch.arange(1, SHARED, device="cuda")
    composed_out = {}

    def composed():
        r = apply_lut(own, luts[0])
        p = apply_lut(prev.index_select(0, ip), luts[1])
        q = apply_lut(nxt.index_select(0, inx), luts[2])
        head, tail = r[:SHARED - 1], r[T - SHARED + 1:]
        torch.where(head == 0, p, head, out=head)
        torch.where(tail == 0, q, tail, out=tail)
        composed_out["r"] = r

    fused()
    composed()
    torch.cuda.synchronize()
    assert torch.equal(out, composed_out["r"]) and status.cpu().tolist() == [0, 0]
    filled = int(((apply_lut(own, luts[0]) == 0) & (out != 0)).sum())
    say(f"  the two forms agree on all {own.numel()} voxels; the merge fills {filled} of them")
    src = own.view(-1)
    dst = torch.empty_like(src)

    def copy():
        _lib.check(L.tf_copy16(_lib.ptr(src), _lib.ptr(dst), 4 * src.numel(), _lib.stream_ptr()), "tf_copy16")
    res = medians({"fused": fused, "composed": composed, "copy": copy})
    vox = own.numel()
    merged_frames = 2 * (SHARED - 1)
    fused_bytes = vox * 8 + merged_frames * hw * 4                   # read own, write out, read the merged neighbour frames
    # composed: gather own (8 B / voxel); per merged frame: index_select (8) + gather (8) + `== 0` (5) + where in place (13)
    composed_bytes = vox * 8 + merged_frames * hw * 34
    for name, by in (("fused", fused_bytes), ("composed", composed_bytes), ("copy", 8 * vox)):
        med, lo, hi = res[name]
        label = {"fused": "tf_relabel_merge", "composed": "index_select + 3 tf_apply_lut + 2 torch.where", "copy": "tf_copy16, the window's size"}[name]
        say(f"  {label}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); {by / vox:.1f} B per voxel algorithmic, "
            f"{by / med / 1e9:.2f} TB/s of that")
    say(f"  composed / fused = x{res['composed'][0] / res['fused'][0]:.2f}; fused reaches "
        f"{(fused_bytes / res['fused'][0]) / (8 * vox / res['copy'][0]) * 100:.0f} % of the copy's rate "
        f"({RUNS} samples of {REPS} calls after {WARM} warm-ups, the forms alternating)")


def part_b():
    from synth import blob_stack
    step = T - SHARED
    t0 = np.datetime64("2020-06-01T00:00", "ns")
    names, store, thr = [], {}, None
    for w in range(3):
        bt = torch.nan_to_num(blob_stack(T, H, W, t0=w * step), nan=290.0)
        if thr is None:                                      # one set of thresholds for the three windows: shared frames agree
            thr = torch.quantile(bt.flatten()[::97][:4_000_000].float(), torch.tensor([SHARE / 4, SHARE, 2 * SHARE], device="cuda"))
        ds = LabelDataset(coords=dict(t=t0 + (w * step + np.arange(T)) * np.timedelta64(5, "m")))
        for name, k in (("core_label", 0), ("thick_anvil_label", 1), ("thin_anvil_label", 2)):
            ds.add(name, nd.label(bt < thr[k])[0], ("t", "y", "x"))
        # the anvil coordinate is shared: thin ids are numbered behind the thick ones
        top = int(ds["thick_anvil_label"].max())
        ds["thin_anvil_label"] = torch.where(ds["thin_anvil_label"] > 0, ds["thin_anvil_label"] + top, 0).to(torch.int32)
        ds.add("bt", bt, ("t", "y", "x"))
        ds.coords["core"] = np.arange(1, int(ds["core_label"].max()) + 1, dtype=np.int32)
        ds.coords["anvil"] = np.arange(1, int(ds["thin_anvil_label"].max()) + 1, dtype=np.int32)
        stamp = lambda k: (t0 + k * np.timedelta64(5, "m")).astype("datetime64[s]").item().strftime("%Y%m%d_%H%M%S")
        first, end = w * step + (SHARED // 2 if w else 0), (w + 1) * step + SHARED // 2
        names.append(f"synthetic_S{stamp(first)}_E{stamp(end)}_X0000_Y0000.nc")
        store[names[-1]] = ds
    say(f"(b) three windows of {T} x {H} x {W}, {SHARED} frames shared; cores / anvils per window: "
        f"{[int(store[n].coords['core'].size) for n in names]} / {[int(store[n].coords['anvil'].size) for n in names]}")
    res = {}
    links = {}

    def link():
        links["ds"] = linking.process_linking_output([linking.find_overlap_between_files(a, b, store) for a, b in zip(names[:-1], names[1:])])
    res["link"] = medians({"link": link}, reps=1, runs=3, warm=1)["link"]
    say(f"  find_overlap_between_files x 2 + process_linking_output, device-resident: median {res['link'][0]:.1f} ms")
    host_store = {n: LabelDataset({k: v.cpu().numpy() for k, v in ds.items()}, coords=ds.coords) for n, ds in store.items()}
    for n, ds in store.items():
        host_store[n].dims.update(ds.dims)
    got = {}
    dev = medians({"dev": lambda: got.update(d=linking.process_file(names[1], links["ds"], store))}, reps=1, runs=3, warm=1)["dev"]
    merge = medians({"m": lambda: linking.relabel_and_merge_file(names[1], links["ds"], store)}, reps=1, runs=3, warm=1)["m"]
    host = medians({"host": lambda: got.update(h=linking.process_file(names[1], links["ds"], host_store))}, reps=1, runs=1, warm=0)["host"]
    same = all(np.array_equal(got["d"][k].cpu().numpy() if hasattr(got["d"][k], "cpu") else got["d"][k], got["h"][k]) for k in got["h"] if k != "bt")
    say(f"  process_file of the middle window, device-resident: median {dev[0]:.1f} ms (min {dev[1]:.1f}, max {dev[2]:.1f}; 3 runs), "
        f"of which relabel_and_merge_file {merge[0]:.1f} ms")
    say(f"  process_file on NumPy containers: {host[0]:.0f} ms (1 run); the two agree variable by variable: {same}; "
        f"NumPy / device = x{host[0] / dev[0]:.1f}")


if __name__ == "__main__":
    if "a" in WHICH:
        part_a()
        torch.cuda.empty_cache()
    if "b" in WHICH:
        part_b()
