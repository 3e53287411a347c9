"""The flow scheduler's host logic (tobac_flow_amd/_flow_plan.py, flow._drive_batches) without a GPU: batch sizes, the
requeue rule, the refinement's images per launch and the out-of-memory protocol of the batch driver with stand-ins.  The
library's hint and size functions touch no device; the hint assumes 256 CUs where none answers, the MI355X's count.  The
expected figures are those of the expressions that stood inline in flow.py before the plan functions existed."""
import ctypes

import pytest

from tobac_flow_amd import _flow_plan as fp


@pytest.mark.parametrize("n_pairs,chunk,want", [(10, 3, [2, 3, 3, 2]), (10, 4, [3, 4, 3]), (7, 2, [2, 2, 1, 2]), (5, 2, [2, 1, 2]), (7, 64, [7]),
                                                (0, 16, []), (143, 16, [16, 16, 16, 16, 15, 16, 16, 16, 16])])
def test_even_batches_known_answers(n_pairs, chunk, want):
    assert fp.even_batches(n_pairs, chunk) == want


def test_even_batches_equal_the_inline_expression_on_a_sweep():
    for n in range(0, 41):
        for chunk in range(1, 10):
            n_b = max(1, -(-n // chunk))
            edges = [round(k * n / n_b) for k in range(n_b + 1)]
            want = [b - a for a, b in zip(edges[:-1], edges[1:]) if b > a]
            got = fp.even_batches(n, chunk)
            assert got == want and sum(got) == n and all(0 < b <= chunk + 1 for b in got), (n, chunk)


def _library_terms(H, W):
    from tobac_flow_amd import _lib
    L = _lib.lib()
    p = _lib.FarnebackParams(5, 0.5, 13, 10, 5, 1.1, 0, 0)
    lib_per_pair = max(1, int(L.tf_farneback_workspace_bytes_batch(1, H, W, ctypes.byref(p))))
    return lib_per_pair, lambda pairs, nbytes: L.tf_farneback_batch_hint(H, W, ctypes.byref(p), pairs, nbytes)


# (H, W, pairs, budget, parts) -> cap, the library's share of the budget (None: not pinned), batches
BUDGET_CASES = [
    ((5424, 5424, 143, 115e9, 1), 45, 90930726938, [42, 42, 42, 17]),
    ((5424, 5424, 143, 60e9, 2), 39, 39231121988, [38, 38, 38, 29]),
    ((5424, 5424, 143, 86.4e9, 2), 56, None, [42, 42, 42, 17]),          # bench.py's config F
    ((5424, 5424, 143, 8e9, 1), None, None, [3] * 47 + [2]),
    ((5424, 5424, 15, 115e9, 1), None, None, [15]),
    ((1500, 2500, 23, 115e9, 1), 356, None, [23]),
    ((3712, 3712, 47, 40e9, 2), 55, None, [47]),
]


@pytest.mark.parametrize("case,cap,lib_budget,want", BUDGET_CASES, ids=["%dx%d-%d-%gGB-%d" % (c[0][0], c[0][1], c[0][2], c[0][3] / 1e9, c[0][4]) for c in BUDGET_CASES])
def test_budget_batches_with_the_librarys_hint(case, cap, lib_budget, want):
    H, W, n_pairs, budget, parts = case
    lib_per_pair, hint = _library_terms(H, W)
    if H == 5424:
        assert lib_per_pair == 2000596736
    got_cap, got_lib_budget = fp.budget_caps(H * W, lib_per_pair, int(budget), parts)
    assert cap is None or got_cap == cap
    assert lib_budget is None or got_lib_budget == lib_budget
    assert fp.budget_batches(n_pairs, H * W, lib_per_pair, int(budget), parts, hint) == want


def test_budget_batches_clamp_with_a_stand_in_hint():
    """min(cap, left, hint x parts) from each side: the hint binds, the cap binds, what is left goes out whole once it fits"""
    asked = []

    def hint(answer):
        def f(pairs, nbytes):
            asked.append((pairs, nbytes))
            return answer
        return f
    # one part: 100 bytes per pair, ten pairs fit, 82 % of the budget is the library's
    assert fp.budget_caps(1, 82, 1000, 1) == (10, 820)
    assert fp.budget_batches(25, 1, 82, 1000, 1, hint(4)) == [4, 4, 4, 4, 9] and asked == [(25, 820), (21, 820), (17, 820), (13, 820)]
    assert fp.budget_batches(25, 1, 82, 1000, 1, hint(100)) == [10, 10, 5]
    assert fp.budget_batches(10, 1, 82, 1000, 1, None) == [10]                  # fits: the hint is not asked
    # two parts: the hint sizes the full-resolution launches (pairs / parts of them) and its answer counts per part
    del asked[:]
    assert fp.budget_caps(1, 82, 1000, 2) == (16, 694)
    assert fp.budget_batches(40, 1, 82, 1000, 2, hint(3)) == [6, 6, 6, 6, 16] and asked == [(20, 694), (17, 694), (14, 694), (11, 694)]
    assert fp.budget_batches(40, 1, 82, 1000, 2, hint(50)) == [16, 16, 8]
    assert fp.budget_batches(19, 1, 82, 1000, 2, hint(0)) == [2, 2, 15]           # a hint of nothing still moves on
    assert fp.budget_batches(5, 1, 82, 50, 1, hint(7)) == [1, 1, 1, 1, 1]      # a budget below one pair: one pair at a time


def test_flow_budget():
    assert fp.flow_budget(115e9, 0, 250e9) == 115000000000
    assert fp.flow_budget(115e9, 0, 100e9) == 60000000000                       # never more than 60 % of the free memory ...
    assert fp.flow_budget(115e9, 40e9, 100e9) == 100000000000                   # ... beside the scratch held from the last call
    assert fp.flow_budget(115e9, 0, 0) == 1 and fp.flow_budget(0, 5e9, 5e9) == 1


@pytest.mark.parametrize("done,stop,pending,half,want", [
    (0, 9, [], 4, [(0, 4), (4, 4), (8, 1)]),
    (0, 4, [(4, 4), (8, 1)], 2, [(0, 2), (2, 2), (4, 2), (6, 2), (8, 1)]),
    (5, 10, [], 5, [(5, 5)]),
    (5, 10, [(10, 7)], 5, [(5, 5), (10, 5), (15, 2)]),
    (3, 3, [(3, 4)], 1, [(3, 1), (4, 1), (5, 1), (6, 1)]),                     # nothing of a finished batch is queued again
])
def test_requeue_halved(done, stop, pending, half, want):
    before = list(pending)
    assert fp.requeue_halved(done, stop, pending, half) == want and pending == before


@pytest.mark.parametrize("B,H,W,tiles,want", [(23, 1500, 2500, 432, [19, 1, 1, 2]), (42, 5424, 5424, 3315, [1, 1, 1, 1]),
                                              (21, 3712, 3712, 1575, [3, 1, 3, 3]), (9, 180, 236, 9, [9, 1, 9, 9]), (5, 96, 128, 4, [5, 1, 5, 5])])
def test_refinement_images_per_launch(B, H, W, tiles, want):
    from tobac_flow_amd import _lib
    assert fp.varref_tiles(H, W) == tiles
    per_image = _lib.lib().tf_varref_workspace_bytes(H, W)
    assert [fp.varref_group(B, tiles, 256, rounds, per_image) for rounds in (32, 0, 1, 2)] == want
    assert fp.varref_group(B, tiles, 256, 32, 6.5e9) == 1 and fp.varref_group(B, tiles, 256, 32, 7e9) == 1      # the scratch bound


def _stand_in_driver(script, on_done=None):
    """flow._drive_batches over generators that follow `script`: {(i0, B): [what each next() does]}, an int is yielded, an
    exception raised"""
    from tobac_flow_amd.flow import _drive_batches
    log = {"made": [], "seen": [], "released": [], "closed": []}

    def make_work(i0, B):
        log["made"].append((i0, B))
        try:
            for step in script[(i0, B)]:
                if isinstance(step, BaseException):
                    raise step
                yield step
        finally:
            log["closed"].append((i0, B))

    def seen(n):
        log["seen"].append(n)
        if on_done is not None:
            on_done(n)
    return log, lambda batches: _drive_batches(batches, make_work, seen, lambda half: log["released"].append(half))


def test_driver_requeues_only_what_is_not_final_when_a_batch_does_not_fit():
    import torch
    log, drive = _stand_in_driver({(0, 10): [5, torch.OutOfMemoryError("part 2 does not fit")], (5, 5): [10]})
    drive([(0, 10)])
    assert log["made"] == [(0, 10), (5, 5)] and log["seen"] == [5, 10] and log["released"] == [5]
    # the batches behind the failed one are cut too, and nothing is run twice
    log, drive = _stand_in_driver({(0, 4): [torch.OutOfMemoryError("does not fit")], (0, 2): [2], (2, 2): [4], (4, 2): [6], (6, 1): [7]})
    drive([(0, 4), (4, 3)])
    assert log["made"] == [(0, 4), (0, 2), (2, 2), (4, 2), (6, 1)] and log["seen"] == [2, 4, 6, 7] and log["released"] == [2]
    assert log["closed"] == log["made"]


def test_driver_leaves_an_out_of_memory_error_of_the_callback_to_the_caller():
    import torch

    def greedy(n):
        raise torch.OutOfMemoryError("the caller's own allocation failed")
    log, drive = _stand_in_driver({(0, 4): [2, 4], (4, 4): [8]}, on_done=greedy)
    with pytest.raises(torch.OutOfMemoryError, match="caller's own"):
        drive([(0, 4), (4, 4)])
    assert log["made"] == [(0, 4)] and log["seen"] == [2] and log["released"] == []


def test_driver_gives_up_on_a_batch_of_one_pair():
    import torch
    log, drive = _stand_in_driver({(0, 1): [torch.OutOfMemoryError("one pair does not fit")]})
    with pytest.raises(torch.OutOfMemoryError, match="one pair"):
        drive([(0, 1), (1, 1)])
    assert log["made"] == [(0, 1)] and log["seen"] == [] and log["released"] == []
