"""ORDER BY / LIMIT on the CPU: the top-k reference against brute force,
the order keys, and ordered queries through the executor.

The same cases run on the device in test_order_gpu.py."""

import functools

import pytest
import torch

import hyperspace_amd.ops as ops
from hyperspace_amd import functions as F
from hyperspace_amd.ops import cpu_ref

from topk_common import (SIZES, TILE, BruteTopK, k_values, op_cases,
                         order_key_columns, tie_cases)
from topk_common import (MULTI_ORDERS, ORDER_COLUMNS, OrderEnv,
                         scenario_bucketed, scenario_bucketed_hybrid,
                         scenario_bucketed_nullable_key,
                         scenario_limit_alone, scenario_multi_column,
                         scenario_order_by_alone, scenario_over_aggregate,
                         scenario_over_join, scenario_select_between,
                         scenario_single_column, scenario_unique_column)

DEVICE = "cpu"


# ---------------------------------------------------------------------------
# topk_rows: the reference against brute force
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _op_cases():
    return op_cases(TILE)


def _check(keys, valid, brute, k, keep_ties):
    got = ops.topk_rows(keys, k, valid, keep_ties)
    assert got.dtype == torch.int64
    assert got.tolist() == brute(k, keep_ties), (k, keep_ties)


@pytest.mark.parametrize("n", SIZES(TILE))
def test_topk_rows_reference_matches_brute_force(n):
    for name, (keys, valid) in _op_cases().items():
        if not name.endswith(f"-n={n}"):
            continue
        brute = BruteTopK(keys, valid)
        for k in k_values(brute.n_valid):
            for keep in (False, True):
                _check(keys, valid, brute, k, keep)


@pytest.mark.parametrize("name", list(tie_cases(TILE)))
def test_topk_rows_reference_tie_quota(name):
    keys, valid, ks = tie_cases(TILE)[name]
    brute = BruteTopK(keys, valid)
    for k in ks:
        for keep in (False, True):
            _check(keys, valid, brute, k, keep)
        # exactly min(k, n_valid) rows without ties
        assert ops.topk_rows(keys, k, valid).numel() == min(k, brute.n_valid)


def test_topk_rows_reference_ignores_null_keys():
    keys = torch.tensor([5, 0, 7, 1, 6], dtype=torch.int64)
    valid = torch.tensor([True, False, True, False, True])
    # the two null rows hold the smallest stored keys
    assert ops.topk_rows(keys, 2, valid).tolist() == [0, 4]
    assert ops.topk_rows(keys, 2).tolist() == [1, 3]
    assert cpu_ref.topk_rows(keys, 9, valid).tolist() == [0, 2, 4]
    assert cpu_ref.topk_rows(keys, 0, valid).tolist() == []


# ---------------------------------------------------------------------------
# order keys
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(order_key_columns()))
def test_order_key_descending_is_complement(name):
    col = order_key_columns()[name]
    want = cpu_ref.sql_key(col)
    assert torch.equal(ops.order_key(col, False), want)
    assert torch.equal(ops.order_key(col, True), ~want)


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
def env(tmp_path_factory, system_path):
    """Shared by the tests that only read: no index, rules off."""
    return OrderEnv(tmp_path_factory.mktemp("order"), DEVICE)


@pytest.fixture(scope="module")
def indexed_env(tmp_path_factory, system_path):
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


# ---------------------------------------------------------------------------
# the interface: what is refused when the frame is built
# ---------------------------------------------------------------------------

def test_interface_errors(env):
    from hyperspace_amd.exceptions import HyperspaceException
    df = env.df
    for bad in (lambda: df.order_by("nope"),
                lambda: df.order_by("i", "I"),
                lambda: df.order_by("i", F.desc("i")),
                lambda: df.order_by(),
                lambda: df.order_by("i", "f", ascending=[True]),
                lambda: df.order_by(3),
                lambda: df.limit(-1),
                lambda: df.limit(2.0),
                lambda: df.limit(True),
                lambda: df.limit("3")):
        with pytest.raises(HyperspaceException):
            bad()


def test_interface_spellings_and_rendering(env):
    from hyperspace_amd.plan.expr import SortOrder, col
    from hyperspace_amd.plan.nodes import Limit, Sort
    df = env.df
    # names resolve case-insensitively to the plan's spelling
    q = df.orderBy("I", col("F").desc(), F.asc_nulls_last("S"),
                   col("n32").desc_nulls_first()).limit(10)
    assert q.plan.pretty().splitlines()[:2] == [
        "Limit(10)",
        "  Sort([i ASC NULLS FIRST, f DESC NULLS LAST, s ASC NULLS LAST, "
        "n32 DESC NULLS FIRST])"]
    assert isinstance(q.plan, Limit) and isinstance(q.plan.child, Sort)
    assert q.plan.output_columns() == df.plan.output_columns()
    assert q.plan.child.output_columns() == df.plan.output_columns()
    # with_children rebuilds the same node
    again = q.plan.with_children([q.plan.child.with_children(
        [df.plan])])
    assert again.pretty() == q.plan.pretty()
    # ascending as a list, and the defaults of every builder
    s = df.sort("i", "f", ascending=[False, True]).plan
    assert repr(s.orders[0]) == "i DESC NULLS LAST"
    assert repr(s.orders[1]) == "f ASC NULLS FIRST"
    for built, text in ((col("i").asc(), "i ASC NULLS FIRST"),
                        (col("i").desc(), "i DESC NULLS LAST"),
                        (col("i").asc_nulls_last(), "i ASC NULLS LAST"),
                        (col("i").desc_nulls_first(), "i DESC NULLS FIRST"),
                        (F.asc("i"), "i ASC NULLS FIRST"),
                        (F.desc("i"), "i DESC NULLS LAST"),
                        (F.asc_nulls_last("i"), "i ASC NULLS LAST"),
                        (F.desc_nulls_first("i"), "i DESC NULLS FIRST")):
        assert isinstance(built, SortOrder) and repr(built) == text
    # limit(0): an empty batch with the schema
    out = df.order_by("i").limit(0).collect()
    assert out.num_rows == 0 and out.names == df.plan.output_columns()
    out = df.limit(0).collect()
    assert out.num_rows == 0 and out.names == df.plan.output_columns()
