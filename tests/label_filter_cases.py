"""Cases and yardsticks of the label filters (tf_label_filter, ndimage_dev.label_filter and the device branch of
tobac_flow_amd.analysis):

  * the volumes, chosen for where the kernel can go wrong rather than for size, each with its fields and criteria;
  * CALLS: the calls of the ten analysis functions that the fixture records for every volume;
  * restate(): tf_label_filter in NumPy -- records int32[n_labels + 1][4] = {tmin, tmax, hit bits, 0};
  * from_records(): what an analysis function returns (or raises) given such records;
  * reference(): the reference's own results (tests/golden/label_filter_ref.npz, written by
    tests/golden/make_label_filter_golden.py, which ran tobac_flow/analysis.py itself).

The tests read the inputs STORED in the fixture, so that a different NumPy cannot change an input.

A criterion is ("mask", name) -- a bool volume, satisfied where True -- or (field name, op, threshold).  The reference takes
masks only: the generator hands it `field op threshold` as NumPy evaluates it, which for a float32 field compares in float32
(NumPy 1.26 and 2.x alike)."""
import operator
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label_filter_ref.npz")
OPS = {">=": operator.ge, ">": operator.gt, "<=": operator.le, "<": operator.lt}
INT_MAX = 0x7fffffff
MIN_LENGTHS = (1, 2, 3)
F32_07 = np.float32(0.7)            # 0.699999988...: >= 0.7 in float32, < 0.7 in float64


# ---- volumes ------------------------------------------------------------------------------------------------------------
def make_odd():
    """(3, 33, 67): the row tail is no multiple of 16 and W % 4 != 0 (scalar path).  Region 1 spans four 16-voxel chunks
    over two frames; region 2 ends at a row's last voxel and continues at the next row's first; regions 3 and 4 are the
    first and the last voxel of the volume."""
    shape = (3, 33, 67)
    labels = np.zeros(shape, np.int32)
    labels[0:2, 5, 3:51] = 1
    labels[1:3, 10, 60:67] = 2
    labels[1:3, 11, 0:5] = 2
    labels[0, 0, 0] = 3
    labels[2, 32, 66] = 4
    background_only = np.zeros(shape, bool)                       # true only under background: no hit
    background_only[0, 6, :] = True
    background_only[2, 5, 3:51] = True
    one_voxel = np.zeros(shape, bool)                             # true at exactly one voxel of the multi-chunk region
    one_voxel[1, 5, 37] = True
    f = np.full(shape, 0.1, np.float32)
    f[labels == 0] = 5.0                                          # the background would satisfy >= 0.7
    f[0, 5, 20] = np.nan                                          # a NaN inside region 1
    f[2, 11, 2] = F32_07                                          # the one voxel of region 2 that reaches the threshold
    g = np.zeros(shape, np.float64)
    g[labels == 1] = -2.0
    g[labels == 3] = -2.0
    g[1, 5, 4] = np.nan
    criteria = [("mask", "background_only"), ("mask", "one_voxel"), ("f", ">=", 0.7), ("g", "<", -1.0), ("f", "<", 0.5)]
    extra = [("f", ">", 0.7), ("g", "<=", -2.0), ("g", ">", 0.0)]
    return dict(labels=labels, fields=dict(background_only=background_only, one_voxel=one_voxel, f=f, g=g),
                criteria=criteria, extra=extra)


def make_aligned():
    """(2, 40, 64): 16-byte aligned rows (int4 path); random boxes, ids compacted so that none is missing"""
    rng = np.random.default_rng(515)
    shape = (2, 40, 64)
    labels = np.zeros(shape, np.int32)
    for i in range(1, 15):
        t0, y0, x0 = rng.integers(0, 2), rng.integers(0, 36), rng.integers(0, 50)
        t1 = rng.integers(t0 + 1, 3)
        labels[t0:t1, y0:y0 + rng.integers(1, 5), x0:x0 + rng.integers(1, 40)] = i
    labels = np.unique(labels, return_inverse=True)[1].reshape(shape).astype(np.int32)
    sparse = rng.random(shape) < 0.02
    f = rng.normal(size=shape).astype(np.float32)
    g = rng.normal(size=shape)
    criteria = [("mask", "sparse"), ("f", ">", 1.5), ("g", "<=", -1.0)]
    extra = [("f", "<", -2.5), ("g", ">=", 2.0), ("f", ">=", 0.0), ("g", "<", 0.0), ("f", "<=", -1.0)]
    return dict(labels=labels, fields=dict(sparse=sparse, f=f, g=g), criteria=criteria, extra=extra)


def make_one():
    labels = np.ones((1, 1, 1), np.int32)
    return dict(labels=labels, fields=dict(none=np.zeros((1, 1, 1), bool), f=np.full((1, 1, 1), F32_07, np.float32)),
                criteria=[("f", ">=", 0.7), ("mask", "none")], extra=[("f", ">", 0.7)])


def make_zero():
    shape = (2, 5, 7)
    return dict(labels=np.zeros(shape, np.int32), fields=dict(all=np.ones(shape, bool), f=np.ones(shape, np.float32)),
                criteria=[("mask", "all"), ("f", ">", 0.0)], extra=[])


def make_gap():
    """(2, 6, 20): ids 1 and 3 occur, id 2 does not -- the reference's find_objects yields None for it"""
    shape = (2, 6, 20)
    labels = np.zeros(shape, np.int32)
    labels[0:2, 1, 2:19] = 1
    labels[1, 4, 5:8] = 3
    touch = np.zeros(shape, bool)
    touch[1, 4, 6] = True
    touch[0, 1, 2] = True
    f = np.zeros(shape, np.float32)
    f[1, 4, 7] = 2.0
    return dict(labels=labels, fields=dict(touch=touch, f=f), criteria=[("mask", "touch"), ("f", ">", 1.0)], extra=[])


GENERATORS = {"odd": make_odd, "aligned": make_aligned, "one": make_one, "zero": make_zero, "gap": make_gap}
VOLUMES = tuple(GENERATORS)


def as_mask(case, criterion):
    """the criterion as the bool volume NumPy makes of it"""
    if criterion[0] == "mask":
        return case["fields"][criterion[1]]
    name, op, threshold = criterion
    with np.errstate(invalid="ignore"):
        return OPS[op](case["fields"][name], threshold)


def calls(case):
    """[(key, function name, indices into case["criteria"] or None, min_length or None)]: the recorded calls"""
    K = len(case["criteria"])
    out = [("lengths", "find_object_lengths", None, None)]
    out += [(f"mask_labels/{k}", "mask_labels", (k,), None) for k in range(K)]
    out += [(f"by_mask/{k}", "filter_labels_by_mask", (k,), None) for k in range(K)]
    subsets = [tuple(range(K)), (K - 1,), (0, K - 1), (1 % K, K - 1)] + ([(2, 4), (3, 4)] if K >= 5 else [])
    subsets = list(dict.fromkeys(subsets))
    out += [(f"by_multimask/{'_'.join(map(str, s))}", "filter_labels_by_multimask", s, None) for s in subsets]
    for ml in MIN_LENGTHS:
        out.append((f"by_length/{ml}", "filter_labels_by_length", None, ml))
        out.append((f"by_length_legacy/{ml}", "filter_labels_by_length_legacy", None, ml))
        out.append((f"by_length_and_mask/{K - 1}/{ml}", "filter_labels_by_length_and_mask", (K - 1,), ml))
        out.append((f"by_length_and_mask_legacy/{K - 1}/{ml}", "filter_labels_by_length_and_mask_legacy", (K - 1,), ml))
        for s in subsets[1:3]:
            tag = "_".join(map(str, s))
            out.append((f"by_length_and_multimask/{tag}/{ml}", "filter_labels_by_length_and_multimask", s, ml))
            out.append((f"by_length_and_multimask_legacy/{tag}/{ml}", "filter_labels_by_length_and_multimask_legacy", s, ml))
    return out


LIST_OF_MASKS = ("filter_labels_by_multimask", "filter_labels_by_length_and_multimask", "filter_labels_by_length_and_multimask_legacy")


def call(module, name, labels, masks, min_length):
    """module.name(labels, ...) with the argument list of that function; masks: a list (possibly of device tensors)"""
    fn = getattr(module, name)
    args = [labels]
    if masks is not None:
        args.append(list(masks) if name in LIST_OF_MASKS else masks[0])
    if min_length is not None:
        args.append(min_length)
    return fn(*args)


# ---- the fixture ----------------------------------------------------------------------------------------------------------
_GOLDEN = None
_CASES = {}


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with np.load(GOLDEN) as z:
            _GOLDEN = {k: z[k] for k in z.files}
    return _GOLDEN


def case(volume):
    """the volume as the reference saw it: labels, fields (bool volumes unpacked), criteria, extra.  Do not modify."""
    if volume not in _CASES:
        z, made = golden(), GENERATORS[volume]()
        labels = z[f"{volume}/labels"].astype(np.int32)
        fields = {}
        for name, a in made["fields"].items():
            if a.dtype == bool:
                fields[name] = np.unpackbits(z[f"{volume}/field/{name}"])[:labels.size].reshape(labels.shape).astype(bool)
            else:
                fields[name] = z[f"{volume}/field/{name}"]
            fields[name].setflags(write=False)
        labels.setflags(write=False)
        _CASES[volume] = dict(labels=labels, fields=fields, criteria=made["criteria"], extra=made["extra"])
    return _CASES[volume]


def reference(volume, key):
    """the reference's result of a recorded call: an array, or the name of the exception it raised"""
    z = golden()
    if f"{volume}/{key}/raises" in z:
        return str(z[f"{volume}/{key}/raises"])
    return z[f"{volume}/{key}"]


# ---- the restatement ------------------------------------------------------------------------------------------------------
def satisfied(case, criterion):
    """the criterion evaluated as tf_label_filter does: a mask where non-zero; a field in its own dtype, the threshold of
    a float32 field rounded to float32 first; a NaN satisfies nothing"""
    if criterion[0] == "mask":
        return case["fields"][criterion[1]] != 0
    name, op, threshold = criterion
    field = case["fields"][name]
    assert field.dtype in (np.float32, np.float64)
    with np.errstate(invalid="ignore"):
        return OPS[op](field, field.dtype.type(threshold))


def restate(labels, n_labels, truths):
    """records of tf_label_filter: `truths` = one bool volume per criterion.  Labels <= 0 or > n_labels are ignored."""
    rec = np.zeros((n_labels + 1, 4), np.int32)
    rec[:, 0], rec[:, 1] = INT_MAX, -1
    for l in range(1, n_labels + 1):
        where = labels == l
        frames = np.nonzero(where.any(axis=(1, 2)))[0]
        if frames.size:
            rec[l, 0], rec[l, 1] = frames[0], frames[-1]
            rec[l, 2] = sum(int(bool(m[where].any())) << k for k, m in enumerate(truths))
    return rec


_RECORDS = {}


def records(volume):
    """restate() of a volume with its criteria, computed once; do not modify"""
    if volume not in _RECORDS:
        c = case(volume)
        n = max(int(c["labels"].max()), 0)
        _RECORDS[volume] = restate(c["labels"], n, [satisfied(c, q) for q in c["criteria"]])
        _RECORDS[volume].setflags(write=False)
    return _RECORDS[volume]


def from_records(labels, rec, name, which, min_length):
    """the result of analysis.<name> given the records: an array, or the name of the exception the reference raises.
    `which`: indices of the criteria the call uses."""
    r = rec[1:].astype(np.int64)
    n = len(r)
    present = r[:, 1] >= 0
    lengths = np.where(present, r[:, 1] - r[:, 0] + 1, 0)
    hits = [((r[:, 2] >> k) & 1).astype(bool) for k in (which or ())]
    measures_lengths = name in ("find_object_lengths",) or "length" in name
    uses_comprehension = name != "mask_labels" and which is not None and "legacy" not in name
    if n == 0:
        if name == "find_object_lengths":
            return np.zeros(0)
        if name == "mask_labels":
            return np.zeros(0, bool)
        return "ValueError" if uses_comprehension else labels.copy()
    if measures_lengths and not present.all():
        return "TypeError"
    if name == "find_object_lengths":
        return lengths
    if name == "mask_labels":
        return hits[0]
    if name == "filter_labels_by_mask" and not present.all():
        return "ValueError"
    keep = np.ones(n, bool)
    if min_length is not None:
        keep &= lengths >= min_length
    for h in hits:
        keep &= h
    lut = np.zeros(n + 1, labels.dtype)
    lut[1:] = np.cumsum(keep) * keep
    return lut[labels]
