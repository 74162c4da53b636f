"""Join modes of the HIP two-phase tile merge join vs the CPU reference,
bit-exact, on inputs sized to reach each kernel path (tile = 2048 left
rows, LDS window = 2048 right keys); plus outer/anti joins through the
executor on the device.

Run on a GPU box: python -m pytest tests/test_join_types_gpu.py -m gpu -q
"""

import functools

import numpy as np
import pytest
import torch

import hyperspace_amd.ops as ops
from hyperspace_amd.execution.executor import Executor
from hyperspace_amd.ops import cpu_ref, native
from hyperspace_amd.plan.expr import col
from hyperspace_amd.plan.nodes import IndexScan

from join_types_common import (MODES, batch_rows, indexed_session,
                               join_rows_oracle, segmented_keys)

pytestmark = pytest.mark.gpu

TILE = 2048
U64_MAX_AS_I64 = -1  # bit pattern of 2**64 - 1


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native.available(), "HIP extension must load on a GPU box"


def _split(values, seg_of_residue):
    """Deal values into segments by value (as co-bucketing does: equal
    keys share a segment on both sides)."""
    n_seg = len(seg_of_residue)
    return [values[seg_of_residue[values % n_seg] == s].tolist()
            for s in range(n_seg)]


def _boundary_tiles():
    # 5000 left rows = two full tiles + a partial one over 64 segments,
    # so every tile spans segment boundaries; about half the left keys
    # have a match, duplicates on both sides
    rng = np.random.default_rng(1)
    left = rng.integers(0, 2000, 5000)
    right = rng.integers(0, 1000, 3000) * 2
    seg_of_residue = rng.permutation(64)
    return _split(left, seg_of_residue), _split(right, seg_of_residue)


def _single_segment_lds():
    rng = np.random.default_rng(2)
    return ([rng.integers(0, 1500, 4096).tolist()],
            [(rng.integers(0, 750, 1000) * 2).tolist()])


def _beyond_lds_window():
    # one tile whose right window is 3000 copies of one key (> the LDS
    # window) matched by five left rows among unmatched ones
    left = list(range(1, 200, 2)) + [500] * 5 + list(range(601, 800, 2))
    right = [0, 2, 4] + [500] * 3000 + [900, 902]
    return [left], [right]


def _extreme_tiles():
    # tile 0: no left row matches; tile 1: every left row matches
    left = list(range(1, 2 * TILE, 2)) + \
        [10_000 + 2 * (i // 2) for i in range(TILE)]
    right = list(range(0, 2 * TILE, 2)) + list(range(10_000, 12_100, 2))
    return [left], [right]


def _segment_extremes():
    # first and last segment empty on the right
    rng = np.random.default_rng(3)
    lparts = [rng.integers(0, 50, 300).tolist() for _ in range(5)]
    rparts = [[]] + [rng.integers(0, 50, 100).tolist()
                     for _ in range(3)] + [[]]
    return lparts, rparts


def _key_extremes():
    ext = [0, 0, 1, 2**62, -2**63, -5, U64_MAX_AS_I64, U64_MAX_AS_I64]
    return [ext + [7, 9]], [[0, 3, 2**62, 2**62, -2**63 + 1,
                             U64_MAX_AS_I64, U64_MAX_AS_I64, 9]]


CASES = {
    "boundary_tiles": _boundary_tiles,
    "single_segment_lds": _single_segment_lds,
    "beyond_lds_window": _beyond_lds_window,
    "extreme_tiles": _extreme_tiles,
    "segment_extremes": _segment_extremes,
    "key_extremes": _key_extremes,
    "one_left_row_hit": lambda: ([[4]], [[3, 4, 4, 5]]),
    "one_left_row_miss": lambda: ([[4]], [[3, 5]]),
    "empty_right": lambda: ([[1, 2, 2], list(range(3000))], [[], []]),
    "empty_left": lambda: ([[], []], [[1, 2], [3]]),
}


@functools.lru_cache(maxsize=None)
def _inputs(case):
    lparts, rparts = CASES[case]()
    lk, lseg = segmented_keys(lparts)
    rk, rseg = segmented_keys(rparts)
    return lk, rk, lseg, rseg, lk.cuda(), rk.cuda()


@functools.lru_cache(maxsize=None)
def _reference(case, mode):
    lk, rk, lseg, rseg, _, _ = _inputs(case)
    return cpu_ref.merge_join(lk, rk, lseg, rseg, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_merge_join_modes_match_cpu(case, mode):
    _, _, lseg, rseg, lk_d, rk_d = _inputs(case)
    want_l, want_r = _reference(case, mode)
    got_l, got_r = ops.merge_join(lk_d, rk_d, lseg, rseg, mode)
    assert got_l.is_cuda and got_r.is_cuda
    assert got_l.dtype == torch.int64 and got_r.dtype == torch.int64
    assert torch.equal(got_l.cpu(), want_l)
    assert torch.equal(got_r.cpu(), want_r)


def test_case_shapes_reach_their_paths():
    """The inputs above have the shapes their names promise."""
    lk, rk, lseg, _, _, _ = _inputs("boundary_tiles")
    assert lk.numel() == 5000 and lseg.numel() == 65
    spanning = sum(
        int(torch.searchsorted(lseg, torch.tensor(b), right=True))
        != int(torch.searchsorted(
            lseg, torch.tensor(min(b + TILE, 5000) - 1), right=True))
        for b in range(0, 5000, TILE))
    assert spanning == 3
    matched = _reference("boundary_tiles", "left_semi")[0].numel()
    assert 0.3 < matched / 5000 < 0.7
    lk, rk, lseg, _, _, _ = _inputs("single_segment_lds")
    assert lk.numel() == 2 * TILE and lseg.numel() == 2 and \
        rk.numel() <= TILE
    lk, rk, _, _, _, _ = _inputs("beyond_lds_window")
    assert lk.numel() <= TILE and int((rk == 500).sum()) > TILE
    semi = _reference("extreme_tiles", "left_semi")[0]
    assert semi.numel() == TILE and int(semi.min()) == TILE


def test_inner_mode_is_the_old_call():
    for case in ("boundary_tiles", "beyond_lds_window", "key_extremes"):
        _, _, lseg, rseg, lk_d, rk_d = _inputs(case)
        old_l, old_r = native.ext().merge_join(lk_d, rk_d, lseg, rseg)
        for new_l, new_r in (
                native.ext().merge_join(lk_d, rk_d, lseg, rseg, 0),
                native.ext().merge_join(lk_d, rk_d, lseg, rseg, mode=0),
                ops.merge_join(lk_d, rk_d, lseg, rseg),
                ops.merge_join(lk_d, rk_d, lseg, rseg, mode="inner")):
            assert torch.equal(old_l, new_l) and torch.equal(old_r, new_r)
        want_l, want_r = _reference(case, "inner")
        assert torch.equal(old_l.cpu(), want_l)
        assert torch.equal(old_r.cpu(), want_r)
    with pytest.raises(RuntimeError):
        native.ext().merge_join(lk_d, rk_d, lseg, rseg, 4)


def test_executor_join_types_on_device(tmp_path, monkeypatch):
    monkeypatch.setenv("HYPERSPACE_SYSTEM_PATH", str(tmp_path / "indexes"))
    session, left, right, lrows, rrows = indexed_session(
        tmp_path, "cuda", 8, n_left=3000, n_right=2000)
    session.enable_hyperspace()
    for how, canonical in (("left", "left_outer"), ("full", "full_outer"),
                           ("anti", "left_anti")):
        plan = left.join(right, on="k", how=how).optimized_plan()
        assert sum(isinstance(leaf, IndexScan)
                   for leaf in plan.collect_leaves()) == 2, plan.pretty()
        ex = Executor(session)
        out = ex.execute(plan)
        assert ex.stats.merge_joins == 1 and ex.stats.shuffles == 0
        assert out.device.type == "cuda"
        assert batch_rows(out)[1] == join_rows_oracle(lrows, rrows,
                                                      canonical), how
    # zero-row right side: null columns are built, nothing is gathered
    out = left.join(right.filter(col("b") < 0), on="k", how="left").collect()
    assert out.device.type == "cuda"
    assert batch_rows(out)[1] == join_rows_oracle(lrows, [], "left_outer",
                                                  rwidth=3)
