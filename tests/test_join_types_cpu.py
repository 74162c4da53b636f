"""Outer, semi and anti joins: the CPU reference merge join against a
nested-loop oracle, and every join type end to end through the public
API (indexed co-bucketed path and un-indexed shuffled path) against a
brute-force row-set oracle."""

import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import hyperspace_amd as hs
from hyperspace_amd.exceptions import HyperspaceException
from hyperspace_amd.execution.columnar import StringColumn
from hyperspace_amd.execution.executor import Executor
from hyperspace_amd.ops import cpu_ref
from hyperspace_amd.plan.expr import col
from hyperspace_amd.plan.nodes import IndexScan, Join

from join_types_common import (HOW_GROUPS, MODES, batch_rows,
                               brute_merge_join, indexed_session,
                               join_rows_oracle, segmented_keys)

I64_MIN, I64_MAX = -2**63, 2**63 - 1


# ---------------------------------------------------------------------------
# 1. cpu_ref.merge_join vs nested loops
# ---------------------------------------------------------------------------

def _norm(vals):
    return cpu_ref.normalize_key(
        torch.tensor(vals, dtype=torch.int64)).tolist()


ORACLE_CASES = {
    # duplicates on both sides over several segments; segment 1 has an
    # empty right side under a non-empty left one, segment 2 an empty
    # left side
    "segments": ([[1, 1, 2, 5, 5, 9], [3, 4, 4], [], [7, 7, 8, 20]],
                 [[1, 2, 2, 5, 5, 5, 6], [], [1, 2], [7, 8, 8, 21]]),
    "empty_right": ([[1, 2, 2], [3]], [[], []]),
    "one_left_row_hit": ([[4]], [[3, 4, 4, 5]]),
    "one_left_row_miss": ([[4]], [[3, 5]]),
    # int64 extremes map to u64 0 and 2**64-1; with 0 in between the
    # normalized keys straddle the int64 sign bit
    "key_extremes": ([_norm([I64_MIN, I64_MIN, -1, 0, I64_MAX])],
                     [_norm([I64_MIN, 0, 0, 5, I64_MAX, I64_MAX])]),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sorted(ORACLE_CASES))
def test_cpu_ref_matches_nested_loop(case, mode):
    lparts, rparts = ORACLE_CASES[case]
    lk, lseg = segmented_keys(lparts)
    rk, rseg = segmented_keys(rparts)
    got_l, got_r = cpu_ref.merge_join(lk, rk, lseg, rseg, mode)
    want_l, want_r = brute_merge_join(lk, rk, lseg, rseg, mode)
    assert torch.equal(got_l, want_l), (got_l, want_l)
    assert torch.equal(got_r, want_r), (got_r, want_r)


def test_cpu_ref_default_mode_is_inner():
    lk, lseg = segmented_keys(ORACLE_CASES["segments"][0])
    rk, rseg = segmented_keys(ORACLE_CASES["segments"][1])
    a = cpu_ref.merge_join(lk, rk, lseg, rseg)
    b = cpu_ref.merge_join(lk, rk, lseg, rseg, "inner")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):
        cpu_ref.merge_join(lk, rk, lseg, rseg, "cross")


# ---------------------------------------------------------------------------
# 2. every join type through DataFrame.join
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def env(tmp_path_factory):
    root = tmp_path_factory.mktemp("join_types")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("HYPERSPACE_SYSTEM_PATH", str(root / "indexes"))
        yield indexed_session(root, "cpu", 4, n_left=400, n_right=300)


def _columns(how):
    if how in ("left_semi", "left_anti"):
        return ["k", "a", "s"]
    return ["k", "a", "s", "k_r", "b", "t"]


@pytest.mark.parametrize("canonical", sorted(HOW_GROUPS))
def test_join_types_end_to_end(env, canonical):
    session, left, right, lrows, rrows = env
    want = join_rows_oracle(lrows, rrows, canonical)
    assert sum(want.values()) > 0
    for how in HOW_GROUPS[canonical]:
        q = left.join(right, on="k", how=how)
        assert q.plan.join_type == canonical

        session.enable_hyperspace()
        try:
            plan = q.optimized_plan()
            assert sum(isinstance(leaf, IndexScan)
                       for leaf in plan.collect_leaves()) == 2, plan.pretty()
            ex = Executor(session)
            out = ex.execute(plan)
        finally:
            session.disable_hyperspace()
        assert ex.stats.merge_joins == 1 and ex.stats.shuffles == 0, \
            ex.stats.operators
        names, got = batch_rows(out)
        assert names == _columns(canonical)
        assert got == want, how

        names, got = batch_rows(q.collect())
        assert names == _columns(canonical)
        assert got == want, how


def test_operator_names(env):
    session, left, right, _, _ = env
    session.enable_hyperspace()
    try:
        ex = Executor(session)
        ex.execute(left.join(right, on="k").optimized_plan())
        assert "SortMergeJoin(co-bucketed)" in ex.stats.operators
        ex = Executor(session)
        ex.execute(left.join(right, on="k", how="left").optimized_plan())
        assert "SortMergeJoin(co-bucketed, left_outer)" in ex.stats.operators
    finally:
        session.disable_hyperspace()
    ex = Executor(session)
    ex.execute(left.join(right, on="k", how="anti").plan)
    assert "SortMergeJoin(shuffled, left_anti)" in ex.stats.operators
    assert ex.stats.shuffles == 2 and ex.stats.merge_joins == 0


def test_explain_and_why_not_accept_non_inner_joins(env):
    session, left, right, _, _ = env
    h = hs.Hyperspace(session)
    for how in ("left", "semi", "full"):
        q = left.join(right, on="k", how=how)
        text = h.explain(q)
        assert "jt_l" in text and "jt_r" in text
        assert h.why_not(q) is not None


# ---------------------------------------------------------------------------
# 3. multi-key join
# ---------------------------------------------------------------------------

def test_multikey_join_types(tmp_path, monkeypatch):
    monkeypatch.setenv("HYPERSPACE_SYSTEM_PATH", str(tmp_path / "idx"))
    ld, rd = tmp_path / "l", tmp_path / "r"
    ld.mkdir()
    rd.mkdir()
    # (k1=3, k2=99): k1 matches right rows, k2 never does
    lrows = [(k1, k2, 100 * k1 + k2) for k1 in range(6) for k2 in range(4)]
    lrows += [(3, 99, -1), (3, 99, -2), (50, 0, -3)]
    rrows = [(k1, k2, 7 * k1 + k2) for k1 in range(2, 9)
             for k2 in (1, 2, 2, 5)]
    for d, rows, v in ((ld, lrows, "v"), (rd, rrows, "w")):
        pq.write_table(pa.table({
            "k1": pa.array([r[0] for r in rows], type=pa.int64()),
            "k2": pa.array([r[1] for r in rows], type=pa.int64()),
            v: pa.array([r[2] for r in rows], type=pa.int64())}),
            str(d / "part-0.parquet"))
    session = hs.HyperspaceSession(device="cpu")
    session.conf.set(hs.IndexConstants.INDEX_NUM_BUCKETS, 4)
    h = hs.Hyperspace(session)
    left, right = session.read_parquet(str(ld)), session.read_parquet(str(rd))
    h.create_index(left, hs.CoveringIndexConfig("mk_l", ["k1", "k2"], ["v"]))
    h.create_index(right, hs.CoveringIndexConfig("mk_r", ["k1", "k2"],
                                                 ["w"]))
    for how in sorted(HOW_GROUPS):
        want = join_rows_oracle(lrows, rrows, how, nkeys=2)
        q = left.join(right, on=["k1", "k2"], how=how)
        session.enable_hyperspace()
        ex = Executor(session)
        out = ex.execute(q.optimized_plan())
        session.disable_hyperspace()
        assert ex.stats.merge_joins == 1 and ex.stats.shuffles == 0
        assert batch_rows(out)[1] == want, how
        assert batch_rows(q.collect())[1] == want, how
    # the k1-only match is unmatched, not half-matched
    lone = (3, 99, -1)
    assert join_rows_oracle(lrows, rrows, "left_outer", nkeys=2)[
        lone + (None, None, None)] == 1
    assert join_rows_oracle(lrows, rrows, "left_anti", nkeys=2)[lone] == 1
    assert join_rows_oracle(lrows, rrows, "left_semi", nkeys=2)[lone] == 0


# ---------------------------------------------------------------------------
# 4. empty right side
# ---------------------------------------------------------------------------

def _check_empty_right(left, right, lrows):
    out = left.join(right, on="k", how="left").collect()
    names, got = batch_rows(out)
    assert names == ["k", "a", "s", "k_r", "b", "t"]
    assert got == join_rows_oracle(lrows, [], "left_outer", rwidth=3)
    assert out.num_rows == len(lrows)
    assert out.column("k_r").dtype == torch.int64
    assert out.column("b").dtype == torch.int64
    assert isinstance(out.column("t"), StringColumn)
    for name in ("k_r", "b", "t"):
        assert not bool(out.mask(name).any())
    names, got = batch_rows(left.join(right, on="k", how="anti").collect())
    assert names == ["k", "a", "s"]
    assert got == join_rows_oracle(lrows, [], "left_anti", rwidth=3)
    assert sum(got.values()) == len(lrows)
    assert left.join(right, on="k", how="semi").collect().num_rows == 0
    assert left.join(right, on="k", how="inner").collect().num_rows == 0
    names, got = batch_rows(left.join(right, on="k", how="full").collect())
    assert got == join_rows_oracle(lrows, [], "full_outer", rwidth=3)


@pytest.mark.parametrize("enabled", [False, True])
def test_right_side_empty_after_filter(env, enabled):
    session, left, right, lrows, _ = env
    if enabled:
        session.enable_hyperspace()
    try:
        _check_empty_right(left, right.filter(col("b") < 0), lrows)
    finally:
        session.disable_hyperspace()


def test_right_relation_empty(env, tmp_path):
    session, left, _, lrows, _ = env
    rd = tmp_path / "empty_right"
    rd.mkdir()
    pq.write_table(pa.table({
        "k": pa.array([], type=pa.int64()),
        "b": pa.array([], type=pa.int64()),
        "t": pa.array([], type=pa.string())}), str(rd / "part-0.parquet"))
    _check_empty_right(left, session.read_parquet(str(rd)), lrows)


# ---------------------------------------------------------------------------
# 5. string join key, independently built dictionaries
# ---------------------------------------------------------------------------

def test_string_key_outer_and_anti(tmp_path, monkeypatch):
    monkeypatch.setenv("HYPERSPACE_SYSTEM_PATH", str(tmp_path / "idx"))
    ld, rd = tmp_path / "l", tmp_path / "r"
    ld.mkdir()
    rd.mkdir()
    lrows = [(f"sku-{(i * 7) % 40:03d}", i) for i in range(200)]
    lrows[5] = (None, 5)
    rrows = [(f"sku-{i:03d}", 1000 + i) for i in range(20, 70)]
    pq.write_table(pa.table({
        "sku": pa.array([r[0] for r in lrows], type=pa.string()),
        "v": pa.array([r[1] for r in lrows], type=pa.int64())}),
        str(ld / "part-0.parquet"))
    pq.write_table(pa.table({
        "sku": pa.array([r[0] for r in rrows], type=pa.string()),
        "w": pa.array([r[1] for r in rrows], type=pa.int64())}),
        str(rd / "part-0.parquet"))
    session = hs.HyperspaceSession(device="cpu")
    session.conf.set(hs.IndexConstants.INDEX_NUM_BUCKETS, 4)
    h = hs.Hyperspace(session)
    left, right = session.read_parquet(str(ld)), session.read_parquet(str(rd))
    h.create_index(left, hs.CoveringIndexConfig("sk_l", ["sku"], ["v"]))
    h.create_index(right, hs.CoveringIndexConfig("sk_r", ["sku"], ["w"]))
    session.enable_hyperspace()
    for how in ("left_outer", "left_anti", "full_outer"):
        ex = Executor(session)
        out = ex.execute(left.join(right, on="sku", how=how)
                         .optimized_plan())
        assert ex.stats.merge_joins == 1 and ex.stats.shuffles == 0
        assert batch_rows(out)[1] == join_rows_oracle(lrows, rrows, how), how


# ---------------------------------------------------------------------------
# 6. plan strings
# ---------------------------------------------------------------------------

def test_plan_strings(env):
    session, left, right, _, _ = env
    inner = left.join(right, on="k").plan
    cond = repr(inner.condition)
    assert inner._node_str() == f"Join({cond})"
    assert left.join(right, on="k", how="inner").plan._node_str() == \
        f"Join({cond})"
    for canonical, spellings in HOW_GROUPS.items():
        if canonical == "inner":
            continue
        for how in spellings + [spellings[0].upper()]:
            plan = left.join(right, on="k", how=how).plan
            assert plan.join_type == canonical
            assert plan._node_str() == f"Join({canonical}, {cond})"
            assert plan.with_children(plan.children).join_type == canonical
    for how in ("cross", "left_semi_join", "", "natural"):
        with pytest.raises(HyperspaceException):
            left.join(right, on="k", how=how)
    with pytest.raises(HyperspaceException):
        Join(left.plan, right.plan, inner.condition, "cross")
    lcols = left.plan.output_columns()
    for how in ("semi", "anti"):
        assert left.join(right, on="k", how=how).plan.output_columns() == \
            lcols
    assert left.join(right, on="k", how="left").plan.output_columns() == \
        lcols + right.plan.output_columns()
