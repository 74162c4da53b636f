"""Group-by on the CPU path: the cpu_ref ops against brute force (they
are the oracle of the HIP kernels), and the DataFrame API — construction,
names, errors and Spark null/overflow semantics through the executor."""

import functools
import math

import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import hyperspace_amd as hs
from hyperspace_amd import functions as F
from hyperspace_amd.ops import cpu_ref
import hyperspace_amd.ops as ops
from hyperspace_amd.plan.expr import AggExpr, col
from hyperspace_amd.plan.nodes import Aggregate

from aggregate_common import (TILE, brute_group_offsets,
                              brute_segmented_reduce, group_oracle,
                              offset_cases, reduce_cases, sort_key,
                              special_reduce_cases)
from join_types_common import batch_rows

DTYPES = (torch.int64, torch.int32, torch.float64, torch.float32)


# ---------------------------------------------------------------------------
# ops
# ---------------------------------------------------------------------------

def test_sort_key_matches_normalize_key():
    floats = [0.0, -0.0, 1.5, -1.5, float("inf"), float("-inf"),
              float("nan"), -float("nan"), 5e-324]
    got = cpu_ref.normalize_key(torch.tensor(floats, dtype=torch.float64))
    assert [int(v) & (2**64 - 1) for v in got] == \
        [sort_key(x) for x in floats]
    ints = [0, -1, 1, 2**63 - 1, -2**63]
    got = cpu_ref.normalize_key(torch.tensor(ints, dtype=torch.int64))
    assert [int(v) & (2**64 - 1) for v in got] == [sort_key(x) for x in ints]


@functools.lru_cache(maxsize=None)
def _offset_cases():
    return offset_cases(TILE)


@pytest.mark.parametrize("name", list(offset_cases(TILE)))
def test_group_offsets_ref_vs_brute(name):
    keys, masks = _offset_cases()[name]
    got = ops.group_offsets(keys, masks)
    assert got.dtype == torch.int64
    want = brute_group_offsets(
        [k.tolist() for k in keys],
        None if masks is None else
        [None if m is None else m.tolist() for m in masks])
    assert got.tolist() == want


def test_group_offsets_rejects_bad_column_count():
    with pytest.raises(ValueError):
        ops.group_offsets([])
    with pytest.raises(ValueError):
        ops.group_offsets([torch.zeros(1, dtype=torch.int64)] * 9)


def _same_value(a, b):
    """Equal as sort keys: tells -0.0 from +0.0 and equates NaNs of one
    sign."""
    return sort_key(a) == sort_key(b)


def _check_vs_brute(values, valid, offsets, exact_sum=True):
    is_float = values.dtype.is_floating_point
    got = ops.segmented_reduce(values, valid, offsets)
    assert got["count"].dtype == torch.int64
    assert got["sum"].dtype == (torch.float64 if is_float else torch.int64)
    assert got["min"].dtype == values.dtype
    assert got["max"].dtype == values.dtype
    want = brute_segmented_reduce(
        values.tolist(), None if valid is None else valid.tolist(),
        offsets.tolist(), is_float)
    cast = float if is_float else int
    for g, (cnt, s, mn, mx) in enumerate(want):
        assert int(got["count"][g]) == cnt
        if cnt == 0:
            continue
        assert _same_value(cast(got["min"][g]), mn), (g, "min")
        assert _same_value(cast(got["max"][g]), mx), (g, "max")
        gs = cast(got["sum"][g])
        if is_float and math.isnan(s):
            assert math.isnan(gs)
        elif exact_sum:
            assert gs == s, (g, gs, s)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_segmented_reduce_ref_vs_brute(dtype):
    for name, (values, valid, offsets) in reduce_cases(dtype).items():
        _check_vs_brute(values, valid, offsets)


@pytest.mark.parametrize("name", list(special_reduce_cases()))
def test_segmented_reduce_ref_special(name):
    values, valid, offsets = special_reduce_cases()[name]
    _check_vs_brute(values, valid, offsets,
                    exact_sum=not values.dtype.is_floating_point)


def test_segmented_reduce_ref_wraps_and_widens():
    v, _, off = special_reduce_cases()["int64_wrap"]
    got = ops.segmented_reduce(v, None, off, ("sum",))
    assert list(got) == ["sum"]
    assert got["sum"].tolist() == [3 * 2**62 - 2**64, 0, -2**63]
    v, _, off = special_reduce_cases()["int32_past_2_31"]
    got = ops.segmented_reduce(v, None, off)
    assert got["sum"].tolist() == [5 * (2**31 - 1),
                                   (2 * TILE - 5) * (2**31 - 1)]
    # narrow integers and bool are widened to int32
    got = ops.segmented_reduce(torch.tensor([100, 100, -3], dtype=torch.int8),
                               None, torch.tensor([0, 2, 3]))
    assert got["sum"].tolist() == [200, -3]
    assert got["max"].dtype == torch.int32
    with pytest.raises(ValueError):
        ops.segmented_reduce(v, None, off, ("median",))


# ---------------------------------------------------------------------------
# API
# ---------------------------------------------------------------------------

ROWS = [
    # k,   a,     f,    s,    d (decimal(10,2) unscaled)
    (1, 10, 1.5, "b", 125),
    (1, None, None, "a", 250),
    (2, None, None, None, None),
    (2, None, None, None, None),
    (None, 7, 2.0, "z", 100),
    (None, 8, None, "y", None),
    (3, 2**62, -0.5, "q", 1),
    (3, 2**62, 0.25, "q", 2),
    (3, 2**62, 4.0, "r", 3),
]


@pytest.fixture
def frame(tmp_path, tmp_system_path):
    import decimal
    d = tmp_path / "t"
    d.mkdir()
    pq.write_table(pa.table({
        "k": pa.array([r[0] for r in ROWS], type=pa.int64()),
        "a": pa.array([r[1] for r in ROWS], type=pa.int64()),
        "f": pa.array([r[2] for r in ROWS], type=pa.float32()),
        "s": pa.array([r[3] for r in ROWS], type=pa.string()),
        "d": pa.array([None if r[4] is None
                       else decimal.Decimal(r[4]).scaleb(-2)
                       for r in ROWS], type=pa.decimal128(10, 2)),
        "i": pa.array([2**31 - 1] * len(ROWS), type=pa.int32()),
    }), str(d / "part-0.parquet"))
    session = hs.HyperspaceSession(device="cpu")
    return session, session.read_parquet(str(d))


def _wrap(v):
    return None if v is None else (v + 2**63) % 2**64 - 2**63


def test_group_by_agg_matches_oracle(frame):
    _, df = frame
    out = df.group_by("k").agg(
        F.count(), F.count("a"), F.sum("a"), F.min("a"), F.max("a"),
        F.avg("f"), F.sum("f"), F.min("s"), F.max("s"), F.sum("d"),
        F.avg("d")).collect()
    names, rows = batch_rows(out)
    assert names == ["k", "count(1)", "count(a)", "sum(a)", "min(a)",
                     "max(a)", "avg(f)", "sum(f)", "min(s)", "max(s)",
                     "sum(d)", "avg(d)"]
    want = group_oracle(ROWS, 1, [
        ("count", None), ("count", 1), ("sum", 1), ("min", 1), ("max", 1),
        ("avg", 2), ("sum", 2), ("min", 3), ("max", 3), ("sum", 4),
        ("avg", 4)])
    # int64 sums wrap around
    want = type(want)({r[:3] + (_wrap(r[3]),) + r[4:]: c
                       for r, c in want.items()})
    assert rows == want
    # spot checks of the semantics the oracle encodes
    by_key = {r[0]: r for r in rows}
    assert by_key[2][1:] == (2, 0) + (None,) * 9      # all-null group
    assert by_key[None][1] == 2                          # null keys: 1 group
    assert by_key[3][3] == 3 * 2**62 - 2**64             # wrap-around
    assert by_key[1][10] == 375 and by_key[1][11] == 187.5  # unscaled avg
    assert out.tensor("sum(f)").dtype == torch.float64
    assert out.tensor("avg(f)").dtype == torch.float64
    assert out.tensor("min(a)").dtype == torch.int64
    assert isinstance(out.column("min(s)"),
                      hs.execution.columnar.StringColumn)


def test_int32_sum_past_2_31(frame):
    _, df = frame
    out = df.agg(F.sum("i"), F.max("i"))
    b = out.collect()
    assert b.tensor("sum(i)").dtype == torch.int64
    assert b.tensor("sum(i)").tolist() == [len(ROWS) * (2**31 - 1)]
    assert b.tensor("max(i)").dtype == torch.int32


def test_both_spellings_aliases_and_dict_form(frame):
    _, df = frame
    a = df.group_by("k").agg(F.sum("a").alias("total"), F.count())
    b = df.groupBy(col("K")).agg({"a": "sum", "*": "count"})
    assert a.plan.output_columns() == ["k", "total", "count(1)"]
    assert b.plan.output_columns() == ["k", "sum(a)", "count(1)"]
    assert isinstance(a.plan, Aggregate)
    assert a.plan._node_str() == \
        "Aggregate(keys=[k], [sum(a) AS total, count(1)])"
    ra, rb = batch_rows(a.collect())[1], batch_rows(b.collect())[1]
    assert ra == rb
    c = df.group_by("k").count()
    assert c.plan.output_columns() == ["k", "count(1)"]
    assert {r[:2] for r in batch_rows(c.collect())[1]} == \
        {(1, 2), (2, 2), (None, 2), (3, 3)}
    # column names resolve case-insensitively to the plan's spelling
    assert df.group_by("K").agg(F.min("A")).plan.output_columns() == \
        ["k", "min(a)"]


def test_construction_errors(frame):
    _, df = frame
    with pytest.raises(hs.HyperspaceException):
        df.group_by("nope")
    with pytest.raises(hs.HyperspaceException):
        df.group_by("k").agg(F.sum("nope"))
    with pytest.raises(hs.HyperspaceException):
        df.group_by("k").agg(F.sum("a"), F.sum("A"))       # duplicate name
    with pytest.raises(hs.HyperspaceException):
        df.group_by("k").agg(F.sum("a").alias("k"))        # clashes with key
    with pytest.raises(hs.HyperspaceException):
        df.group_by("k").agg({"a": "median"})
    with pytest.raises(hs.HyperspaceException):
        AggExpr("stddev", "a")
    with pytest.raises(hs.HyperspaceException):
        AggExpr("sum")                                     # needs a column
    with pytest.raises(hs.HyperspaceException):
        df.group_by("k").agg()
    with pytest.raises(hs.HyperspaceException):
        df.agg("sum(a)")


def test_distinct(frame):
    _, df = frame
    d = df.select("k", "s").distinct()
    assert isinstance(d.plan, Aggregate) and d.plan.aggs == []
    assert d.plan.group_cols == ["k", "s"]
    _, rows = batch_rows(d.collect())
    assert rows == type(rows)({(r[0], r[3]): 1 for r in ROWS})
    assert d._last_stats.operators[-1] == "SortAggregate(shuffled)"
    assert d._last_stats.shuffles == 1


def test_global_agg_non_empty_and_empty(frame):
    _, df = frame
    q = df.agg(F.count(), F.count("a"), F.sum("a"), F.min("s"), F.avg("f"))
    _, rows = batch_rows(q.collect())
    want = group_oracle(ROWS, 0, [
        ("count", None), ("count", 1), ("sum", 1), ("min", 3), ("avg", 2)])
    assert rows == type(want)(
        {r[:2] + (_wrap(r[2]),) + r[3:]: c for r, c in want.items()})
    assert list(rows) == [(9, 6, _wrap(3 * 2**62 + 25), "a", 7.25 / 5)]
    assert q._last_stats.shuffles == 0
    assert q._last_stats.sort_aggregates == 1
    empty = df.filter("k > 100").agg(
        F.count(), F.count("a"), F.sum("a"), F.min("s"), F.max("f"),
        F.avg("f"))
    out = empty.collect()
    assert out.num_rows == 1
    assert batch_rows(out)[1] == type(rows)(
        {(0, 0, None, None, None, None): 1})
    # a grouped aggregate of no rows has no groups
    assert df.filter("k > 100").group_by("k").count().collect().num_rows == 0


def test_float_grouping_keys_are_refused(frame):
    _, df = frame
    q = df.group_by("f").count()        # builds fine
    with pytest.raises(hs.HyperspaceException, match="NaN"):
        q.collect()
    with pytest.raises(hs.HyperspaceException, match="float"):
        df.select("f").distinct().collect()


def test_string_sum_is_refused(frame):
    _, df = frame
    with pytest.raises(hs.HyperspaceException):
        df.agg(F.sum("s")).collect()


def test_multi_column_group_by_with_null_keys(frame):
    _, df = frame
    out = df.group_by("k", "s").agg(F.count(), F.sum("a")).collect()
    _, rows = batch_rows(out)
    want = group_oracle([(r[0], r[3], r[1]) for r in ROWS], 2,
                        [("count", None), ("sum", 2)])
    want = type(want)({r[:3] + (_wrap(r[3]),): c for r, c in want.items()})
    assert rows == want
