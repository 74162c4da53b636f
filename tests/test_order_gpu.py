"""The HIP top-k kernels (ops.topk_rows, the descending order key) against
the CPU reference on inputs aimed at the tile size, and ordered queries
through the executor on the device.

Run on a GPU box: python -m pytest tests/test_order_gpu.py -m gpu -q
"""

import functools

import pytest
import torch

import hyperspace_amd.ops as ops
from hyperspace_amd.ops import cpu_ref, native

from topk_common import (SIZES, TILE, grid_case, k_values, op_cases,
                         order_key_columns, tie_cases)
from topk_common import (MULTI_ORDERS, ORDER_COLUMNS, OrderEnv,
                         scenario_bucketed, scenario_bucketed_hybrid,
                         scenario_bucketed_nullable_key,
                         scenario_limit_alone, scenario_multi_column,
                         scenario_order_by_alone, scenario_over_aggregate,
                         scenario_over_join, scenario_select_between,
                         scenario_single_column, scenario_unique_column)

DEVICE = "cuda"

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native.available(), "HIP extension must load on a GPU box"
    assert ops.topk_tile_size() == TILE


def _dev(t):
    return None if t is None else t.cuda()


def _check(keys_d, valid_d, keys, valid, k, keep_ties):
    want = cpu_ref.topk_rows(keys, k, valid, keep_ties)
    got = ops.topk_rows(keys_d, k, valid_d, keep_ties)
    assert got.is_cuda and got.dtype == torch.int64
    assert torch.equal(got.cpu(), want), (k, keep_ties)
    return got


# ---------------------------------------------------------------------------
# topk_rows
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _op_cases():
    return op_cases(TILE)


@pytest.mark.parametrize("n", SIZES(TILE))
def test_topk_rows_bit_exact(n):
    """Every key pattern and validity shape of this size, every k, both
    tie rules: the row indices equal the reference's."""
    for name, (keys, valid) in _op_cases().items():
        if not name.endswith(f"-n={n}"):
            continue
        n_valid = n if valid is None else int(valid.sum())
        kd, vd = keys.cuda(), _dev(valid)
        for k in k_values(n_valid):
            for keep in (False, True):
                _check(kd, vd, keys, valid, k, keep)


@pytest.mark.parametrize("name", list(tie_cases(TILE)))
def test_topk_rows_tie_quota_across_tile_edge(name):
    keys, valid, ks = tie_cases(TILE)[name]
    kd, vd = keys.cuda(), _dev(valid)
    for k in ks:
        for keep in (False, True):
            _check(kd, vd, keys, valid, k, keep)


@functools.lru_cache(maxsize=None)
def _grid():
    keys, valid, edge = grid_case(TILE)
    return keys, valid, edge, keys.cuda(), valid.cuda()


def _grid_counts():
    keys, valid, edge, _, _ = _grid()
    n_less = int((valid & (keys == 7)).sum())
    n_tie = int((valid & (keys == 1000)).sum())
    return n_less, n_tie, int(valid.sum())


def test_topk_rows_grid_spanning_small_k():
    """2048 * TILE + TILE + 5 rows: blocks walk two tiles; the tie group
    lies across two blocks' ranges and the quota ends inside it."""
    keys, valid, edge, kd, vd = _grid()
    n_less, n_tie, _ = _grid_counts()
    assert n_less < 64 < n_less + n_tie
    for k in (0, 1, 2, 64, n_less + n_tie // 2 + 3):
        for keep in (False, True):
            got = _check(kd, vd, keys, valid, k, keep)
    # the last call kept every tie: rows on both sides of the block edge
    assert bool(((got >= edge - 50) & (got < edge)).any())
    assert bool(((got >= edge) & (got < edge + 50)).any())


def test_topk_rows_grid_spanning_large_k():
    keys, valid, _, kd, vd = _grid()
    _, _, n_valid = _grid_counts()
    for k in (TILE + 1, n_valid - 1, n_valid, n_valid + 1):
        for keep in (False, True):
            _check(kd, vd, keys, valid, k, keep)


def test_topk_rows_unaligned_view():
    # contiguous slices that start 8 bytes / 1 byte into their allocations
    keys, valid = _op_cases()[f"low_byte-fifth_null-n={3 * TILE + 17}"]
    kd, vd = keys.cuda()[1:], valid.cuda()[1:]
    assert kd.data_ptr() % 16 == 8
    for k in (1, 64, TILE + 1):
        for keep in (False, True):
            _check(kd, vd, keys[1:], valid[1:], k, keep)
            _check(kd, None, keys[1:], None, k, keep)


def test_topk_rows_deterministic():
    keys, valid = _op_cases()[f"two_values-fifth_null-n={3 * TILE + 17}"]
    kd, vd = keys.cuda(), valid.cuda()
    for keep in (False, True):
        a = ops.topk_rows(kd, TILE + 1, vd, keep)
        b = ops.topk_rows(kd, TILE + 1, vd, keep)
        assert torch.equal(a, b)


def test_topk_rows_empty_input():
    e = torch.empty(0, dtype=torch.int64, device="cuda")
    assert ops.topk_rows(e, 3).numel() == 0
    assert ops.topk_rows(e, 3).dtype == torch.int64


# ---------------------------------------------------------------------------
# order keys
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(order_key_columns()))
def test_order_key_descending_is_complement(name):
    col = order_key_columns()[name]
    want = cpu_ref.sql_key(col)
    d = col.cuda()
    assert torch.equal(ops.order_key(d, False).cpu(), want)
    assert torch.equal(ops.order_key(d, True).cpu(), ~want)
    # the ascending key is what existing callers get
    assert torch.equal(ops.sql_key(d).cpu(), want)


# ---------------------------------------------------------------------------
# ordered queries
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def system_path(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("HYPERSPACE_SYSTEM_PATH",
              str(tmp_path_factory.mktemp("indexes")))
    yield
    mp.undo()


@pytest.fixture(scope="module")
def env(tmp_path_factory, system_path, _require_native):
    """Shared by the tests that only read: no index, rules off."""
    return OrderEnv(tmp_path_factory.mktemp("order"), DEVICE)


@pytest.fixture(scope="module")
def indexed_env(tmp_path_factory, system_path, _require_native):
    """Indexes on i (no nulls) and n32 (nulls), 8 buckets."""
    e = OrderEnv(tmp_path_factory.mktemp("order_ix"), DEVICE)
    e.index("ix_i", "i")
    e.index("ix_n32", "n32")
    return e


@pytest.mark.parametrize("col", ORDER_COLUMNS)
def test_order_limit_one_column(env, col, monkeypatch):
    scenario_single_column(env, col, monkeypatch)


@pytest.mark.parametrize("name", list(MULTI_ORDERS))
def test_order_limit_mixed_columns(env, name):
    scenario_multi_column(env, name)


def test_order_limit_unique_column_whole_rows(env):
    scenario_unique_column(env)


def test_order_by_alone_is_stable(env):
    scenario_order_by_alone(env)


def test_limit_alone(env):
    scenario_limit_alone(env)


def test_order_select_limit(env):
    scenario_select_between(env)


def test_order_over_aggregate(env):
    scenario_over_aggregate(env)


def test_order_over_join(env, tmp_path):
    scenario_over_join(env, tmp_path)


def test_topk_bucketed(indexed_env):
    scenario_bucketed(indexed_env)


def test_topk_bucketed_nullable_key_takes_select(indexed_env):
    scenario_bucketed_nullable_key(indexed_env)


def test_topk_bucketed_hybrid_scan(tmp_path, tmp_system_path):
    e = OrderEnv(tmp_path, DEVICE)
    e.index("ix_i", "i")
    scenario_bucketed_hybrid(e)


def test_distributed_session_refuses_order_and_limit(env, monkeypatch):
    from hyperspace_amd.exceptions import HyperspaceException
    from hyperspace_amd.parallel import dist_context as dc
    monkeypatch.setattr(dc, "is_distributed", lambda: True)
    monkeypatch.setattr(dc, "get_world_size", lambda: 2)
    monkeypatch.setattr(dc, "get_rank", lambda: 0)
    for q in (env.df.order_by("i"), env.df.limit(3),
              env.df.order_by("i").limit(3)):
        with pytest.raises(HyperspaceException,
                           match="per-rank order is not a global one"):
            q.collect()
