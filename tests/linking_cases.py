"""Cases of the second stage (tobac_flow_amd/linking.py, tf_relabel_merge), shared by tests/golden/make_linking_golden.py,
tests/test_linking_cases_cpu.py and tests/test_gpu_linking.py, and a NumPy restatement of every function of the
reference's "new linking functions" (tobac_flow/linking.py:30-396), written line by line after them.

A product here is a plain dict {"coords": {name: array}, variable name: array} (the form oracle/np_dataset.py works on);
`to_label_dataset` turns one into the package's container.  A store is a dict name -> product.

The expected values live in tests/golden/linking_ref.npz.  The fixture's `source/<function>` entries say which of the two
wrote them: the REFERENCE's own functions (find_overlaps, find_overlap_between_cores / _anvils, find_new_labels,
remap_labels(new_labels=...), get_dates_from_filename; on duck-typed datasets) or this restatement (the functions that
need a real xarray object: process_linking_output, the label maps, the merges, process_file).  The generator asserts that
the two agree wherever both ran.

Worlds.  One consistent global labelling of 14 frames -- cores, thick anvils, thin anvils -- is cut into three windows
[0:7], [4:11], [8:14]; each window renumbers the ids it holds by a permutation of its own, with gaps.  Every object that
is present in a frame two windows share is present in the frame the linking compares (the middle one of the three), so the
linked ids must reproduce the global partition.  In each window some objects are zeroed in a shared frame that the
neighbour fills (the previous product gives the first two shared frames, the next one the last two), so the merge has
something to do and the merged windows must equal the global labelling up to the names of the ids.
  tiny   (14, 3, 5):    objects are whole rows (5 px, the smallest the rule links); hw = 15 is odd
  wide   (14, 33, 300): boxes drifting 3 px per frame; a row is longer than one 256-lane workgroup
Time cases cut two products from the tiny world so that they share exactly 3, 2, 1 and 0 frames, and 4 frames of which
one product lacks a middle one (a non-contiguous intersection).  Rule cases are label_glue_cases' (atol, rtol) edges
(quotient_edge, over_zero, mostly_outside) through padded_window."""
import os
from datetime import timedelta
from functools import partial

import numpy as np
import scipy.sparse
import scipy.sparse.csgraph
from scipy.ndimage import labeled_comprehension

import label_glue_cases as gc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linking_ref.npz")
VOLUMES = (("core_label", "core"), ("thick_anvil_label", "anvil"), ("thin_anvil_label", "anvil"))
T0 = np.datetime64("2018-06-19T12:00:00", "ns")
STEP = np.timedelta64(5, "m")
N_FRAMES = 14
WINDOWS = ((0, 7), (4, 11), (8, 14))
OWNED = ((0, 5), (5, 9), (9, 14))            # the frames each window's file name claims: [start, end)
WORLDS = {"tiny": (3, 5), "wide": (33, 300)}
NEW_FUNCTIONS = ("find_overlaps", "find_overlap_between_cores", "find_overlap_between_anvils", "find_overlap_between_files",
                 "find_new_labels", "process_linking_output", "get_core_label_map_for_file", "get_anvil_label_map_for_file",
                 "relabel_cores_and_anvils", "combine_labels", "merge_previous_file", "merge_next_file",
                 "relabel_and_merge_file", "process_file", "increment_step_coords")


def times(frames):
    return T0 + np.asarray(frames) * STEP


def file_name(first, end, tag="win"):
    """a name whose dates claim the frames [first, end)"""
    stamp = lambda k: (T0 + k * STEP).astype("datetime64[s]").item().strftime("%Y%m%d_%H%M%S")
    return f"/data/{tag}/detected_dccs_G16_S{stamp(first)}_E{stamp(end)}_X0000_Y0000.nc"


# ---- the worlds -------------------------------------------------------------------------------------------------------------
# (first frame, last frame): every lifetime that touches a shared frame (4-6, 8-10) covers the compared one (5, 9)
_TINY_ROWS = {0: ((0, 6), (8, 13)), 1: ((0, 13),), 2: ((0, 3), (5, 9), (11, 13))}
_WIDE_LIVES = ((0, 3), (0, 5), (2, 9), (5, 13), (0, 13), (7, 11), (9, 13), (11, 13), (5, 5), (3, 6))


def global_world(world):
    """{volume name: int32 (14, H, W)} and bt (float32, a few NaNs)"""
    H, W = WORLDS[world]
    core, thick, thin = (np.zeros((N_FRAMES, H, W), np.int32) for _ in range(3))
    if world == "tiny":
        ident = 0
        for row, lives in _TINY_ROWS.items():
            for first, last in lives:
                ident += 1
                thin[first:last + 1, row] = ident
                if (row, first) != (2, 0):                    # the first anvil of row 2 is thin only (frames 0-3)
                    thick[first:last + 1, row] = ident
                if row < 1:
                    core[first:last + 1, row] = ident
    else:
        for k, (first, last) in enumerate(_WIDE_LIVES):
            y0 = 1 + 3 * k                                    # bands of three rows: thin 3 x 44, thick 2 x 40, core 1 x 7
            for f in range(first, last + 1):
                x0 = 10 + 17 * k + 3 * f
                thin[f, y0:y0 + 3, x0:x0 + 44] = k + 1
                if k != 0:                                    # anvil 1 is thin only (frames 0-3: inside the first window)
                    thick[f, y0:y0 + 2, x0 + 2:x0 + 42] = k + 1
                if k % 3 != 2:
                    core[f, y0, x0 + 5:x0 + 12] = 2 * k + 1   # core ids differ from their anvils'
        assert 10 + 17 * 9 + 3 * 13 + 44 <= W and 1 + 3 * 9 + 3 <= H
    bt = np.full((N_FRAMES, H, W), 250.0, np.float32)
    bt[2, 0, 0] = bt[6, H - 1, W - 1] = bt[12, H // 2, W // 2] = np.nan
    return {"core_label": core, "thick_anvil_label": thick, "thin_anvil_label": thin, "bt": bt}


def _renumber(ids, salt):
    """{global id: local id}: a permutation of this window's own, with gaps"""
    ids = np.asarray(sorted(ids))
    order = np.argsort((ids * 7 + salt * 5) % 11 + ids / 100.0)
    return {int(g): 2 * (rank + 1) + (rank % 2) for rank, g in zip(np.argsort(order), ids)}


# (window, volume, frame): one object of that volume is zeroed there; the frame is filled by the neighbour's merge
_ZEROED = ((0, "core_label", 6), (0, "thick_anvil_label", 6), (1, "core_label", 4), (1, "thin_anvil_label", 4),
           (1, "thick_anvil_label", 10), (2, "thin_anvil_label", 8), (2, "core_label", 8))


def window_products(world):
    """(names, store, global world): the three windows as products, each under its own ids"""
    glob = global_world(world)
    names, store = [], {}
    for w, ((a, b), (first, end)) in enumerate(zip(WINDOWS, OWNED)):
        product = {"coords": {"t": times(range(a, b))}, "bt": glob["bt"][a:b].copy()}
        for kind in ("core", "anvil"):
            volumes = [n for n, k in VOLUMES if k == kind]
            present = set(np.unique(np.concatenate([glob[n][a:b].ravel() for n in volumes])).tolist()) - {0}
            table = np.zeros(max(present) + 1, np.int32)
            for g, local in _renumber(present, w + (kind == "anvil")).items():
                table[g] = local
            for n in volumes:
                product[n] = table[glob[n][a:b]]
            product["coords"][kind] = np.unique(table[table > 0]).astype(np.int32)
        for zw, n, frame in _ZEROED:
            if zw == w:
                ids = np.unique(product[n][frame - a])
                ids = ids[ids > 0]
                assert ids.size, (world, zw, n, frame)
                product[n][frame - a][product[n][frame - a] == ids[-1]] = 0
        name = file_name(first, end, world)
        names.append(name)
        store[name] = product
    return names, store, glob


def cut(product, frames):
    """the product's frames at these positions"""
    out = {"coords": dict(product["coords"])}
    out["coords"]["t"] = product["coords"]["t"][frames]
    for k, v in product.items():
        if k != "coords":
            out[k] = v[frames].copy()
    return out


TIME_CASES = {"common3": (list(range(0, 7)), list(range(4, 11))), "common2": (list(range(0, 6)), list(range(4, 11))),
              "common1": (list(range(0, 5)), list(range(4, 11))), "common0": (list(range(0, 4)), list(range(4, 11))),
              "gap": ([0, 1, 2, 3, 4, 5, 7, 8], list(range(4, 12)))}


def time_case(name):
    """(names, store): two products cut from the tiny world's frames, the second under other ids"""
    glob = global_world("tiny")
    frames_1, frames_2 = TIME_CASES[name]
    store, names = {}, []
    for w, frames in enumerate((frames_1, frames_2)):
        product = {"coords": {"t": times(frames)}}
        for kind in ("core", "anvil"):
            volumes = [n for n, k in VOLUMES if k == kind]
            present = set(np.unique(np.concatenate([glob[n][frames].ravel() for n in volumes])).tolist()) - {0}
            table = np.zeros(max(present) + 1, np.int32)
            for g, local in _renumber(present, 3 * w + (kind == "anvil")).items():
                table[g] = local
            for n in volumes:
                product[n] = table[glob[n][frames]]
            product["coords"][kind] = np.unique(table[table > 0]).astype(np.int32)
        if w == 0:                                            # something for the merge to fill from the second product
            last = product["thin_anvil_label"][-1]
            last[last == last.max()] = 0
        names.append(file_name(frames[0], frames[-1] + 1, f"{name}_{w}"))
        store[names[-1]] = product
    return names, store


RULE_CASES = ("quotient_edge", "over_zero", "mostly_outside")


def rule_case(name):
    """(names, store): label_glue_cases' window case through padded_window, as cores and as (thick and thin) anvils"""
    left, right, _ = gc.window_cases()[name]
    names, store = [], {}
    for w, frames in enumerate(gc.padded_window(left, right)):
        ids = np.unique(frames[frames > 0]).astype(np.int32)
        product = {"coords": {"t": times(range(frames.shape[0])), "core": ids, "anvil": ids}}
        for n, _ in VOLUMES:
            product[n] = frames.copy()
        names.append(file_name(0, frames.shape[0], f"{name}_{w}"))
        store[names[-1]] = product
    return names, store


def chains():
    """{case name: (names, store)}: every chain of products the fixture covers"""
    out = {world: window_products(world)[:2] for world in WORLDS}
    out.update({f"time/{n}": time_case(n) for n in TIME_CASES})
    out.update({f"rule/{n}": rule_case(n) for n in RULE_CASES})
    return out


def to_label_dataset(product, device=None):
    """the package's container of a product; device: the label volumes and bt become tensors there"""
    from tobac_flow_amd.dataset import LabelDataset
    ds = LabelDataset(coords={k: np.array(v) for k, v in product["coords"].items()})
    for k, v in product.items():
        if k == "coords":
            continue
        data = np.array(v)
        if device is not None:
            import torch
            data = torch.from_numpy(data).to(device)
        ds.add(k, data, ("t", "y", "x"))
    return ds


def to_store(store, device=None):
    return {name: to_label_dataset(p, device) for name, p in store.items()}


# ---- the restatement (tobac_flow/linking.py:33-396, tobac_flow/utils/datetime_utils.py:9-106) -------------------------------
def np_find_overlaps(x, atol, rtol, max_label, label_counts):
    overlap_counts = np.bincount(x, minlength=max_label + 1)
    wh_overlap = overlap_counts >= atol if atol > 0 else overlap_counts > 0
    if rtol > 0:
        wh_overlap = np.logical_and(wh_overlap, np.maximum(overlap_counts / x.size, overlap_counts / label_counts) >= rtol)
    wh_overlap[0] = False
    return np.where(wh_overlap)[0]


def _sel(values, t, wanted):
    at = np.searchsorted(t, wanted)
    assert np.array_equal(t[at], wanted)
    return values[at]


def _np_find_overlap_between(current_ds, next_ds, coord, volume):
    min_id = current_ds["coords"][coord].max().item()
    max_id = next_ds["coords"][coord].max().item()
    t_overlap = np.intersect1d(current_ds["coords"]["t"], next_ds["coords"]["t"])
    if t_overlap.size > 2:
        t_overlap = t_overlap[1:-1]
        current_overlap = _sel(current_ds[volume], current_ds["coords"]["t"], t_overlap)
        next_overlap = _sel(next_ds[volume], next_ds["coords"]["t"], t_overlap)
        label_counts = np.maximum(np.bincount(next_overlap.flatten(), minlength=max_id + 1), 1)
        comp_func = partial(np_find_overlaps, atol=5, rtol=0.5, max_label=max_id, label_counts=label_counts)
        overlap_labels = labeled_comprehension(next_overlap.flatten(), current_overlap.flatten(), current_ds["coords"][coord],
                                               comp_func, list, [[]])
        x = np.repeat(current_ds["coords"][coord], [len(n) for n in overlap_labels])
        y = np.concatenate(overlap_labels, dtype=next_overlap.dtype, casting="unsafe")
    else:
        x = np.array([], dtype=current_ds["coords"][coord].dtype)
        y = np.array([], dtype=next_ds["coords"][coord].dtype)
    return min_id, max_id, x, y


def np_find_overlap_between_cores(current_ds, next_ds):
    return _np_find_overlap_between(current_ds, next_ds, "core", "core_label")


def np_find_overlap_between_anvils(current_ds, next_ds):
    return _np_find_overlap_between(current_ds, next_ds, "anvil", "thick_anvil_label")


def np_find_overlap_between_files(filename_1, filename_2, store):
    ds_1, ds_2 = store[filename_1], store[filename_2]
    anvil_result = np_find_overlap_between_anvils(ds_1, ds_2)
    core_result = np_find_overlap_between_cores(ds_1, ds_2)
    return dict(filename_1=filename_1, filename_2=filename_2, anvil=anvil_result, core=core_result)


def np_find_new_labels(x, y, size):
    overlap_graph = scipy.sparse.coo_array((np.ones(x.size), (x, y)), shape=(size, size))
    return scipy.sparse.csgraph.connected_components(overlap_graph, directed=False)[1]


def np_process_linking_output(overlap_results):
    filename = [str(o["filename_1"]) for o in overlap_results] + [str(overlap_results[-1]["filename_2"])]
    save_ds = {"coords": {"filename": np.array(filename)}}
    save_ds["previous_filename"] = np.array([""] + filename[:-1])
    save_ds["next_filename"] = np.array([str(o["filename_2"]) for o in overlap_results] + [""])
    core_start = np.cumsum([0] + [o["core"][0] for o in overlap_results]).astype(np.int32)
    save_ds["core_start"] = core_start
    max_core = np.sum([overlap_results[0]["core"][0]] + [o["core"][1] for o in overlap_results])
    x_core = np.concatenate([o["core"][2] + start for o, start in zip(overlap_results, core_start)])
    y_core = np.concatenate([o["core"][3] + start for o, start in zip(overlap_results, core_start[1:])])
    save_ds["core_labels"] = np_find_new_labels(x_core, y_core, max_core + 1).astype(np.int32)
    anvil_start = np.cumsum([0] + [o["anvil"][0] for o in overlap_results]).astype(np.int32)
    save_ds["anvil_start"] = anvil_start
    max_anvil = np.sum([overlap_results[0]["anvil"][0]] + [o["anvil"][1] for o in overlap_results])
    x_anvil = np.concatenate([o["anvil"][2] + start for o, start in zip(overlap_results, anvil_start)])
    y_anvil = np.concatenate([o["anvil"][3] + start for o, start in zip(overlap_results, anvil_start[1:])])
    save_ds["anvil_labels"] = np_find_new_labels(x_anvil, y_anvil, max_anvil + 1).astype(np.int32)
    return save_ds


def _at_file(links_ds, name, file):
    at = np.nonzero(links_ds["coords"]["filename"] == str(file))[0]
    assert at.size == 1, file
    return links_ds[name][at[0]].item()


def np_get_core_label_map_for_file(file, links_ds):
    start = _at_file(links_ds, "core_start", file) + 1
    next_file = _at_file(links_ds, "next_filename", file)
    stop = _at_file(links_ds, "core_start", next_file) + 1 if next_file else None
    return links_ds["core_labels"][start:stop].copy()


def np_get_anvil_label_map_for_file(file, links_ds):
    start = _at_file(links_ds, "anvil_start", file) + 1
    next_file = _at_file(links_ds, "next_filename", file)
    stop = _at_file(links_ds, "anvil_start", next_file) + 1 if next_file else None
    return links_ds["anvil_labels"][start:stop].copy()


def np_remap_labels(labels, new_labels):
    """tobac_flow/utils/label_utils.py:293-309 with locations = None"""
    max_label = np.nanmax(labels)
    max_label = np.maximum(max_label, new_labels.size)
    remapper = np.zeros(max_label + 1, labels.dtype)
    remapper[1:] = new_labels
    return remapper[labels]


def np_relabel_cores_and_anvils(ds, file, links_ds):
    core_label_map = np_get_core_label_map_for_file(file, links_ds)
    ds["core_label"] = np_remap_labels(ds["core_label"], core_label_map)
    anvil_label_map = np_get_anvil_label_map_for_file(file, links_ds)
    ds["thick_anvil_label"] = np_remap_labels(ds["thick_anvil_label"], anvil_label_map)
    ds["thin_anvil_label"] = np_remap_labels(ds["thin_anvil_label"], anvil_label_map)
    return ds


def np_combine_labels(ds, merge_ds):
    """the documented intent: the zeros of ds are filled (linking.py:261-277; File_Linker.combine_labels writes through .loc)"""
    at = np.searchsorted(ds["coords"]["t"], merge_ds["coords"]["t"])
    assert np.array_equal(ds["coords"]["t"][at], merge_ds["coords"]["t"])
    for name, _ in VOLUMES:
        ds[name][at] = np.where(ds[name][at] == 0, merge_ds[name], ds[name][at])
    return ds


def _load_required_vars(store, file):
    src = store[file]
    ds = {"coords": {k: v.copy() for k, v in src["coords"].items() if k not in ("core", "anvil")}}
    for name in ("bt", "core_label", "thick_anvil_label", "thin_anvil_label"):
        if name in src:
            ds[name] = src[name].copy()
    return ds


def _sel_t(ds, wanted):
    t = ds["coords"]["t"]
    out = {"coords": dict(ds["coords"], t=np.asarray(wanted))}
    for k, v in ds.items():
        if k != "coords":
            out[k] = _sel(v, t, wanted)
    return out


def np_merge_previous_file(ds, file, links_ds, store):
    prev_file = _at_file(links_ds, "previous_filename", file)
    if prev_file:
        prev_ds = _load_required_vars(store, prev_file)
        t_overlap = np.intersect1d(ds["coords"]["t"], prev_ds["coords"]["t"])
        if t_overlap.size > 1:
            prev_ds = _sel_t(prev_ds, t_overlap[:-1])
            prev_ds = np_relabel_cores_and_anvils(prev_ds, prev_file, links_ds)
            ds = np_combine_labels(ds, prev_ds)
    return ds


def np_merge_next_file(ds, file, links_ds, store):
    next_file = _at_file(links_ds, "next_filename", file)
    if next_file:
        next_ds = _load_required_vars(store, next_file)
        t_overlap = np.intersect1d(ds["coords"]["t"], next_ds["coords"]["t"])
        if t_overlap.size > 1:
            next_ds = _sel_t(next_ds, t_overlap[1:])
            next_ds = np_relabel_cores_and_anvils(next_ds, next_file, links_ds)
            ds = np_combine_labels(ds, next_ds)
    return ds


def np_relabel_and_merge_file(file, links_ds, store, merge=True):
    ds = _load_required_vars(store, file)
    ds = np_relabel_cores_and_anvils(ds, file, links_ds)
    if merge:
        ds = np_merge_previous_file(ds, file, links_ds, store)
        ds = np_merge_next_file(ds, file, links_ds, store)
    return ds


def np_get_dates_from_filename(filename):
    from dateutil.parser import parse as parse_date
    start_date = parse_date(filename.split("/")[-1].split("_S")[-1][:15], fuzzy=True)
    end_date = parse_date(filename.split("/")[-1].split("_E")[-1][:15], fuzzy=True)
    return start_date, end_date


def np_trim_file_start_and_end(ds, filename):
    start, end = np_get_dates_from_filename(filename)
    t = ds["coords"]["t"]
    keep = (t >= np.datetime64(start)) & (t <= np.datetime64(end - timedelta(seconds=1)))
    out = {"coords": dict(ds["coords"], t=t[keep])}
    for k, v in ds.items():
        if k != "coords":
            out[k] = v[keep] if v.ndim == 3 else v
    return out


_BY_COORD = {"core": ("core_edge_label_flag", "core_start_label_flag", "core_end_label_flag", "core_nan_flag", "core_anvil_index"),
             "anvil": tuple(f"{k}_{f}" for k in ("thick_anvil", "thin_anvil") for f in ("edge_label_flag", "start_label_flag",
                                                                                       "end_label_flag", "nan_flag"))
             + ("anvil_core_count",)}


def _np_add_label_coords(ds):
    """dataset.py:230-297 on oracle.np_dataset's dict: the new coordinates, and what the old ones index cut down to them"""
    from oracle import np_dataset
    old = {k: ds["coords"][k] for k in ("core", "anvil") if k in ds["coords"]}
    np_dataset.add_label_coords(ds)
    for coord, before in old.items():
        at = np.searchsorted(before, ds["coords"][coord])
        assert np.array_equal(before[at], ds["coords"][coord])
        for name in _BY_COORD[coord]:
            if name in ds:
                ds[name] = ds[name][at]
    return ds


def np_process_file(file, links_ds, store, merge=True):
    from oracle import np_dataset
    ds = np_relabel_and_merge_file(file, links_ds, store, merge=merge)
    ds = _np_add_label_coords(ds)
    start, end = np_get_dates_from_filename(file)
    np_dataset.flag_edge_labels(ds, np.datetime64(start), np.datetime64(end))
    if "bt" in ds:
        np_dataset.flag_nan_adjacent_labels(ds, ds["bt"])
    ds = np_trim_file_start_and_end(ds, file)
    ds = _np_add_label_coords(ds)             # ds.sel(core=isin(core, core_label), anvil=isin(anvil, thick | thin))
    np_dataset.link_cores_and_anvils(ds)
    np_dataset.add_step_labels(ds)
    ds = _np_add_label_coords(ds)
    np_dataset.link_step_labels(ds)
    return ds


def np_increment_step_coords(new_ds, past_ds):
    for name in ("core_step", "thick_anvil_step", "thin_anvil_step"):
        steps = new_ds["coords"][name]
        steps[steps != 0] += past_ds["coords"][name].max().item()
    return new_ds


def np_link_chain(names, store):
    """find_overlap_between_files along the chain and process_linking_output: (overlap results, links)"""
    results = [np_find_overlap_between_files(a, b, store) for a, b in zip(names[:-1], names[1:])]
    return results, np_process_linking_output(results)


def merged_partition_check(world):
    """the three-window property: the relabelled and merged windows equal the global labelling up to the names of the ids"""
    names, store, glob = window_products(world)
    _, links = np_link_chain(names, store)
    for name, _ in VOLUMES:
        merged = np.concatenate([np_relabel_and_merge_file(n, links, store)[name].ravel() for n in names])
        truth = np.concatenate([glob[name][a:b].ravel() for a, b in WINDOWS])
        assert np.array_equal(gc.canonical_partition(merged), gc.canonical_partition(truth)), (world, name)
        plain = np.concatenate([np_relabel_and_merge_file(n, links, store, merge=False)[name].ravel() for n in names])
        assert not np.array_equal(plain, merged), (world, name, "the merge filled nothing")


# ---- the relabel-merge kernel's statement and its cases -----------------------------------------------------------------------
def np_relabel_merge(own, lut_own, prev=None, next=None):
    """tf_relabel_merge of include/tobac_flow_hip.h: prev / next = None or (volume, table, frame table).  Returns
    (out, number of consulted ids outside their table)."""
    T = own.shape[0]
    flat = own.reshape(T, -1).astype(np.int64)
    bad = 0

    def look(v, lut):
        inside = (v >= 0) & (v < lut.size)
        return np.where((v != 0) & inside, lut[np.where(inside, v, 0)], 0), int(((v != 0) & ~inside).sum())

    r, n_bad = look(flat, np.asarray(lut_own))
    bad += n_bad
    for side in (prev, next):
        if side is None:
            continue
        vol, lut, frames = side
        vol = vol.reshape(vol.shape[0], -1).astype(np.int64)
        for t in range(T):
            if frames[t] < 0:
                continue
            ask = r[t] == 0
            got, n_bad = look(np.where(ask, vol[frames[t]], 0), np.asarray(lut))
            r[t] = np.where(ask, got, r[t])
            bad += n_bad
    return r.reshape(own.shape).astype(np.int32), bad


def fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def flatten_product(prefix, ds):
    """{fixture key: array} of a product or of a links table (strings as they are, datetimes as int64 nanoseconds)"""
    out = {}
    for k, v in list(ds["coords"].items()) + [(k, v) for k, v in ds.items() if k != "coords"]:
        v = np.asarray(v)
        if v.dtype.kind == "M":
            v = v.astype("datetime64[ns]").astype(np.int64)
        if v.dtype.kind == "f":
            continue                                          # bt: an input, not a result
        out[f"{prefix}/{k}"] = v
    return out


def product_arrays(ds):
    """the same keys for a package LabelDataset (device tensors downloaded)"""
    plain = {"coords": ds.coords}
    for k, v in ds.items():
        plain[k] = v.cpu().numpy() if hasattr(v, "cpu") else v
    return flatten_product("", plain)
