"""The HIP group-by kernels (group_offsets, segmented_reduce) against the
CPU reference on inputs aimed at the tile size, and grouped queries
through the executor on the device.

Run on a GPU box: python -m pytest tests/test_aggregate_gpu.py -m gpu -q
"""

import functools
import os
from collections import Counter

import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import hyperspace_amd as hs
import hyperspace_amd.ops as ops
from hyperspace_amd import functions as F
from hyperspace_amd.ops import cpu_ref, native
from hyperspace_amd.plan.nodes import BucketUnionNode, IndexScan

from aggregate_common import (TILE, agg_session, big_reduce_case,
                              fsum_bound, group_oracle, offset_cases,
                              plan_nodes, reduce_cases, special_reduce_cases,
                              standard_aggs)
from join_types_common import batch_rows, join_rows_oracle

pytestmark = pytest.mark.gpu

DTYPES = (torch.int64, torch.int32, torch.float64, torch.float32)
OUTPUTS = ("sum", "min", "max", "count")


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native.available(), "HIP extension must load on a GPU box"
    assert ops.group_tile_size() == TILE


def _bits(t):
    """Bit patterns, so NaN and the sign of zero compare exactly."""
    t = t.cpu()
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    return t


def _dev(t):
    return None if t is None else t.cuda()


# ---------------------------------------------------------------------------
# group_offsets
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _offset_cases():
    return offset_cases(TILE)


@pytest.mark.parametrize("name", list(offset_cases(TILE)))
def test_group_offsets_bit_exact(name):
    keys, masks = _offset_cases()[name]
    want = cpu_ref.group_offsets(keys, masks)
    got = ops.group_offsets(
        [k.cuda() for k in keys],
        None if masks is None else [_dev(m) for m in masks])
    assert got.is_cuda and got.dtype == torch.int64
    assert torch.equal(got.cpu(), want)


def test_group_offsets_unaligned_view():
    # a contiguous slice that starts 8 bytes into its allocation
    keys, _ = _offset_cases()[f"n={3 * TILE + 17}"]
    k = keys[0].cuda()[1:]
    m = (torch.arange(k.numel()) % 5 != 0).cuda()[1:]
    k = k[:m.numel()]
    want = cpu_ref.group_offsets([k.cpu()], [m.cpu()])
    assert torch.equal(ops.group_offsets([k], [m]).cpu(), want)


# ---------------------------------------------------------------------------
# segmented_reduce
# ---------------------------------------------------------------------------

def _check_exact(values, valid, offsets):
    want = cpu_ref.segmented_reduce(values, valid, offsets)
    got = ops.segmented_reduce(values.cuda(), _dev(valid), offsets.cuda())
    for o in OUTPUTS:
        assert got[o].dtype == want[o].dtype, o
        assert torch.equal(_bits(got[o]), _bits(want[o])), o
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_segmented_reduce_bit_exact(dtype):
    """Integers, min/max and sums of integer-valued floats below 2**53
    (exact in any order) are bit-exact against the reference."""
    for name, (values, valid, offsets) in reduce_cases(dtype).items():
        _check_exact(values, valid, offsets)


@pytest.mark.parametrize("name", ["int64_wrap", "int32_past_2_31"])
def test_segmented_reduce_overflow(name):
    values, valid, offsets = special_reduce_cases()[name]
    got = _check_exact(values, valid, offsets)
    if name == "int64_wrap":
        assert got["sum"].tolist() == [3 * 2**62 - 2**64, 0, -2**63]
    else:
        assert got["sum"].tolist()[0] == 5 * (2**31 - 1)


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32),
                         ids=("float64", "float32"))
def test_segmented_reduce_float_order(dtype):
    """min/max over NaN, +-0.0 and +-inf follow normalize_key order."""
    name = f"float_order_{str(dtype).split('.')[1]}"
    values, valid, offsets = special_reduce_cases()[name]
    want = cpu_ref.segmented_reduce(values, valid, offsets)
    got = ops.segmented_reduce(values.cuda(), None, offsets.cuda())
    for o in ("min", "max", "count"):
        assert torch.equal(_bits(got[o]), _bits(want[o])), o
    # the order itself, from the keys: the min of a group has the smallest
    keys = cpu_ref.normalize_key(values) ^ (-2**63)
    off = offsets.tolist()
    for g in range(len(off) - 1):
        seg = keys[off[g]:off[g + 1]]
        mn = cpu_ref.normalize_key(got["min"][g:g + 1].cpu()) ^ (-2**63)
        mx = cpu_ref.normalize_key(got["max"][g:g + 1].cpu()) ^ (-2**63)
        assert int(mn) == int(seg.min()) and int(mx) == int(seg.max())
    # sums over NaN / inf - inf are NaN on both sides
    assert torch.equal(got["sum"].cpu().isnan(), want["sum"].isnan())


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32),
                         ids=("float64", "float32"))
def test_segmented_reduce_general_float_sums(dtype):
    """General floats: within (n-1) * 2**-53 * sum|x| of math.fsum per
    group, the worst case of any summation order; and two runs agree
    bit for bit."""
    for name in ("one_group_5T+3", "random_64_buckets_valid",
                 "straddling_group", "singletons_3T+1"):
        values, valid, offsets = reduce_cases(dtype, exact=False)[name]
        a = ops.segmented_reduce(values.cuda(), _dev(valid), offsets.cuda())
        b = ops.segmented_reduce(values.cuda(), _dev(valid), offsets.cuda())
        for o in OUTPUTS:
            assert torch.equal(_bits(a[o]), _bits(b[o])), (name, o)
        sums = a["sum"].tolist()
        for g, (bound, exact) in enumerate(
                fsum_bound(values, valid, offsets)):
            assert abs(sums[g] - exact) <= bound, (name, g, sums[g], exact)


def test_segmented_reduce_want_subset_and_unaligned():
    values, valid, offsets = reduce_cases(torch.int64)[
        "random_64_buckets_valid"]
    v, m = values.cuda()[1:], valid.cuda()[1:]
    off = (offsets - 1).clamp_min(0)    # the first row is cut off
    if int(off[1]) == 0:
        off = off[1:]                   # ... and with it a group of one
    want = cpu_ref.segmented_reduce(values[1:], valid[1:], off)
    got = ops.segmented_reduce(v, m, off.cuda(), ("max", "count"))
    assert list(got) == ["max", "count"]
    assert torch.equal(got["max"].cpu(), want["max"])
    assert torch.equal(got["count"].cpu(), want["count"])


@pytest.mark.parametrize("dtype", (torch.int64, torch.float64),
                         ids=("int64", "float64"))
def test_segmented_reduce_more_tiles_than_blocks(dtype):
    """Past 2048 tiles a block walks several tiles and carries the open
    group across them, and groups span many blocks."""
    values, valid, offsets = big_reduce_case(dtype)
    want = cpu_ref.segmented_reduce(values, valid, offsets)
    dv, do = values.cuda(), offsets.cuda()
    got = ops.segmented_reduce(dv, None, do)
    for o in OUTPUTS:
        assert torch.equal(_bits(got[o]), _bits(want[o])), o
    keys = torch.repeat_interleave(
        torch.arange(offsets.numel() - 1), offsets[1:] - offsets[:-1])
    goff = ops.group_offsets([ops.normalize_key(keys.cuda())])
    assert torch.equal(goff.cpu(), offsets)


# ---------------------------------------------------------------------------
# through the executor
# ---------------------------------------------------------------------------

@pytest.fixture
def env(tmp_path, tmp_system_path):
    return agg_session(tmp_path, "cuda", lineage=True)


def _grouped(left):
    aggs, specs = standard_aggs()
    return left.group_by("k").agg(*aggs), specs


def test_bucketed_group_by_on_device(env):
    session, h, left, right, lrows, rrows, ldir = env
    session.enable_hyperspace()
    q, specs = _grouped(left)
    plan = q.optimized_plan()
    scans = plan_nodes(plan, IndexScan)
    assert scans and scans[0].use_bucket_spec, plan.pretty()
    out = q.collect()
    assert out.device.type == "cuda"
    assert batch_rows(out)[1] == group_oracle(lrows, 1, specs)
    st = q._last_stats
    assert "SortAggregate(bucketed)" in st.operators
    assert st.shuffles == 0 and st.sort_aggregates == 1
    session.disable_hyperspace()
    base = q.collect()
    assert batch_rows(base)[1] == group_oracle(lrows, 1, specs)
    assert "SortAggregate(shuffled)" in q._last_stats.operators
    assert q._last_stats.shuffles == 1


def test_hybrid_scan_appended_and_deleted_on_device(env):
    session, h, left, right, lrows, rrows, ldir = env
    session.conf.set(hs.IndexConstants.INDEX_HYBRID_SCAN_ENABLED, True)
    session.conf.set(
        hs.IndexConstants.INDEX_HYBRID_SCAN_APPENDED_RATIO_THRESHOLD, 0.9)
    session.conf.set(
        hs.IndexConstants.INDEX_HYBRID_SCAN_DELETED_RATIO_THRESHOLD, 0.9)
    new = [(None, 900, "l9"), (5, 901, "l0"), (5, 902, "zz"), (77, 903, "a")]
    pq.write_table(pa.table({
        "k": pa.array([r[0] for r in new], type=pa.int64()),
        "a": pa.array([r[1] for r in new], type=pa.int64()),
        "s": pa.array([r[2] for r in new], type=pa.string())}),
        os.path.join(ldir, "part-9.parquet"))
    session.enable_hyperspace()
    df = session.read_parquet(ldir)
    q, specs = _grouped(df)
    plan = q.optimized_plan()
    assert plan_nodes(plan, BucketUnionNode), plan.pretty()
    assert batch_rows(q.collect())[1] == group_oracle(lrows + new, 1, specs)
    assert "SortAggregate(bucketed)" in q._last_stats.operators

    # delete the first source file: its rows leave the answer
    os.unlink(os.path.join(ldir, "part-0.parquet"))
    df = session.read_parquet(ldir)
    q, specs = _grouped(df)
    plan = q.optimized_plan()
    scans = plan_nodes(plan, IndexScan)
    assert scans and scans[0].excluded_source_file_ids, plan.pretty()
    kept = lrows[len(lrows) // 2:] + new
    assert batch_rows(q.collect())[1] == group_oracle(kept, 1, specs)
    assert "SortAggregate(bucketed)" in q._last_stats.operators


def test_aggregate_over_join_on_device(env):
    session, h, left, right, lrows, rrows, ldir = env
    session.enable_hyperspace()
    q = left.join(right, "k").group_by("k").agg(
        F.count(), F.sum("b"), F.max("t"))
    out = q.collect()
    joined = join_rows_oracle(lrows, rrows, "inner")
    rows = [r for r, c in joined.items() for _ in range(c)]
    # joined tuple: (k, a, s, k, b, t)
    want = group_oracle(rows, 1, [("count", None), ("sum", 4), ("max", 5)])
    assert batch_rows(out)[1] == want
    st = q._last_stats
    assert "SortMergeJoin(co-bucketed)" in st.operators
    assert "SortAggregate(shuffled)" in st.operators
    assert st.shuffles == 1


def test_global_agg_and_distinct_on_device(env):
    session, h, left, right, lrows, rrows, ldir = env
    session.enable_hyperspace()
    aggs, specs = standard_aggs()
    q = left.agg(*aggs)
    assert batch_rows(q.collect())[1] == group_oracle(lrows, 0, specs)
    assert q._last_stats.shuffles == 0
    e = left.filter("a < 0").agg(*aggs)
    assert batch_rows(e.collect())[1] == Counter(
        {(0, None, None, None, None): 1})
    d = left.select("k", "s").distinct()
    want = group_oracle([(r[0], r[2]) for r in lrows], 2, [])
    assert batch_rows(d.collect())[1] == want
    assert "SortAggregate(shuffled)" in d._last_stats.operators
