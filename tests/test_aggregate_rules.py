"""AggregateIndexRule: when it fires, what the rewritten plan and the
physical stats look like, the whyNot reasons when it does not, hybrid
scan, refreshed multi-file buckets with null keys, aggregates over an
indexed join, and the ranker."""

import os

import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import hyperspace_amd as hs
from hyperspace_amd import functions as F
from hyperspace_amd.plan.nodes import (Aggregate, BucketUnionNode, Filter,
                                       IndexScan, Join, Project, Scan)
from hyperspace_amd.rules.apply_hyperspace import ApplyHyperspace
from hyperspace_amd.rules.filter_reason import FilterReasons, ReasonCollector

from aggregate_common import (agg_session, group_oracle, plan_nodes,
                              standard_aggs)
from join_types_common import batch_rows, join_rows_oracle


@pytest.fixture
def env(tmp_path, tmp_system_path):
    return agg_session(tmp_path, "cpu", lineage=True)


def _reason_codes(session, df, index_name):
    reasons = ReasonCollector(enabled=True)
    plan = ApplyHyperspace(session, reasons).apply(df.plan)
    return plan, {r.code for r in reasons.all_for_index(index_name)}


def _assert_bucketed(q, want):
    plan = q.optimized_plan()
    assert isinstance(plan, Aggregate)
    scans = plan_nodes(plan, IndexScan)
    assert len(scans) == 1 and scans[0].use_bucket_spec, plan.pretty()
    assert not plan_nodes(plan, Scan), plan.pretty()
    assert batch_rows(q.collect())[1] == want
    st = q._last_stats
    assert "SortAggregate(bucketed)" in st.operators
    assert st.shuffles == 0
    assert st.sort_aggregates == 1
    return plan


def test_rule_fires_on_scan(env):
    session, h, left, right, lrows, rrows, ldir = env
    session.enable_hyperspace()
    aggs, specs = standard_aggs()
    plan = _assert_bucketed(left.group_by("k").agg(*aggs),
                            group_oracle(lrows, 1, specs))
    assert plan.pretty().splitlines()[1].strip() == \
        "IndexScan(jt_l, bucketed)"
    # the index scan reads only what the aggregate needs
    assert [c.lower() for c in plan.child.columns] == ["k", "a", "s"]


def test_rule_fires_on_filter_not_on_indexed_column(env):
    session, h, left, right, lrows, rrows, ldir = env
    session.enable_hyperspace()
    q = left.filter("a >= 100").group_by("K").agg(F.count(), F.max("s"))
    plan = _assert_bucketed(q, group_oracle(
        [r for r in lrows if r[1] >= 100], 1,
        [("count", None), ("max", 2)]))
    assert isinstance(plan.child, Filter)
    assert isinstance(plan.child.child, IndexScan)


def test_rule_fires_on_project_filter_scan(env):
    session, h, left, right, lrows, rrows, ldir = env
    session.enable_hyperspace()
    q = left.filter("a < 300").select("k", "a").group_by("k").agg(
        F.sum("a").alias("total"), F.avg("a"))
    plan = _assert_bucketed(q, group_oracle(
        [r for r in lrows if r[1] < 300], 1, [("sum", 1), ("avg", 1)]))
    assert isinstance(plan.child, Project)
    assert isinstance(plan.child.child, Filter)
    assert plan.output_columns() == ["k", "total", "avg(a)"]


def test_disabled_hyperspace_gives_identical_answers(env):
    session, h, left, right, lrows, rrows, ldir = env
    aggs, specs = standard_aggs()
    q = left.filter("a >= 50").group_by("k").agg(*aggs)
    session.enable_hyperspace()
    with_ix = batch_rows(q.collect())
    assert "SortAggregate(bucketed)" in q._last_stats.operators
    session.disable_hyperspace()
    without = batch_rows(q.collect())
    assert q._last_stats.operators[-1] == "SortAggregate(shuffled)"
    assert q._last_stats.shuffles == 1
    assert with_ix == without


def test_no_fire_grouping_column_not_indexed(env):
    session, h, left, right, lrows, rrows, ldir = env
    session.enable_hyperspace()
    q = left.group_by("s").agg(F.count(), F.sum("a"))
    plan, codes = _reason_codes(session, q, "jt_l")
    assert not plan_nodes(plan, IndexScan), plan.pretty()
    assert FilterReasons.GROUP_COLS_NOT_INDEXED_COL in codes
    assert batch_rows(q.collect())[1] == group_oracle(
        [(r[2], r[1]) for r in lrows], 1, [("count", None), ("sum", 1)])
    assert q._last_stats.operators[-1] == "SortAggregate(shuffled)"
    # two grouping columns, one of them the indexed one: same reason
    q2 = left.group_by("k", "s").count()
    plan2, codes2 = _reason_codes(session, q2, "jt_l")
    assert not plan_nodes(plan2, IndexScan)
    assert FilterReasons.GROUP_COLS_NOT_INDEXED_COL in codes2


def test_no_fire_two_column_index(env):
    session, h, left, right, lrows, rrows, ldir = env
    h.delete_index("jt_l")
    h.create_index(left, hs.CoveringIndexConfig("two", ["k", "a"], ["s"]))
    session.enable_hyperspace()
    q = left.group_by("k").agg(F.count(), F.min("s"))
    plan, codes = _reason_codes(session, q, "two")
    assert not plan_nodes(plan, IndexScan), plan.pretty()
    assert FilterReasons.GROUP_COLS_NOT_INDEXED_COL in codes
    # nor for a group-by on both of its columns (multi-column keys take
    # the sort path)
    q2 = left.group_by("k", "a").count()
    plan2, codes2 = _reason_codes(session, q2, "two")
    assert not plan_nodes(plan2, IndexScan)
    assert FilterReasons.GROUP_COLS_NOT_INDEXED_COL in codes2
    assert batch_rows(q.collect())[1] == group_oracle(
        lrows, 1, [("count", None), ("min", 2)])


def test_no_fire_missing_covered_column(env):
    session, h, left, right, lrows, rrows, ldir = env
    h.delete_index("jt_l")
    h.create_index(left, hs.CoveringIndexConfig("narrow", ["k"], ["a"]))
    session.enable_hyperspace()
    q = left.group_by("k").agg(F.sum("a"), F.min("s"))
    plan, codes = _reason_codes(session, q, "narrow")
    assert not plan_nodes(plan, IndexScan), plan.pretty()
    assert FilterReasons.MISSING_REQUIRED_COL in codes
    # a filter column outside the index blocks it too
    q2 = left.filter("s = 'l1'").group_by("k").agg(F.sum("a"))
    plan2, codes2 = _reason_codes(session, q2, "narrow")
    assert not plan_nodes(plan2, IndexScan)
    assert FilterReasons.MISSING_REQUIRED_COL in codes2
    # what it covers still runs bucketed
    q3 = left.group_by("k").agg(F.sum("a"))
    assert plan_nodes(q3.optimized_plan(), IndexScan)


def test_no_fire_conf_switch_off(env):
    session, h, left, right, lrows, rrows, ldir = env
    session.enable_hyperspace()
    key = hs.IndexConstants.INDEX_AGGREGATE_RULE_ENABLED
    assert key == "spark.hyperspace.index.aggregateRule.enabled"
    assert session.conf.aggregate_rule_enabled is True
    session.conf.set(key, False)
    aggs, specs = standard_aggs()
    q = left.group_by("k").agg(*aggs)
    plan, codes = _reason_codes(session, q, "jt_l")
    assert not plan_nodes(plan, IndexScan), plan.pretty()
    assert not codes            # switched off: the rule looks at nothing
    assert batch_rows(q.collect())[1] == group_oracle(lrows, 1, specs)
    assert q._last_stats.shuffles == 1
    session.conf.set(key, True)
    assert plan_nodes(q.optimized_plan(), IndexScan)


def test_aggregate_beats_filter_only_rewrite(env):
    session, h, left, right, lrows, rrows, ldir = env
    session.enable_hyperspace()
    # a filter on the indexed column: FilterIndexRule (50) would rewrite
    # the child alone, the aggregate rule (70) must win
    q = left.filter("k >= 20").group_by("k").agg(F.count())
    plan = q.optimized_plan()
    scans = plan_nodes(plan, IndexScan)
    assert scans and scans[0].use_bucket_spec, plan.pretty()
    assert batch_rows(q.collect())[1] == group_oracle(
        [r for r in lrows if r[0] is not None and r[0] >= 20], 1,
        [("count", None)])
    assert "SortAggregate(bucketed)" in q._last_stats.operators


def test_explain_shows_node_and_physical_operator(env):
    session, h, left, right, lrows, rrows, ldir = env
    session.enable_hyperspace()
    q = left.group_by("k").agg(F.sum("a").alias("total"), F.count())
    text = h.explain(q, verbose=True)
    assert "Aggregate(keys=[k], [sum(a) AS total, count(1)])" in text
    assert "SortAggregate(bucketed)" in text
    assert "SortAggregate(shuffled)" in text     # the plan without indexes
    assert "jt_l" in text


def _write_left(ldir, name, rows):
    pq.write_table(pa.table({
        "k": pa.array([r[0] for r in rows], type=pa.int64()),
        "a": pa.array([r[1] for r in rows], type=pa.int64()),
        "s": pa.array([r[2] for r in rows], type=pa.string())}),
        os.path.join(ldir, name))


NEW_ROWS = [(None, 900, "l9"), (5, 901, "l0"), (5, 902, "zz"),
            (77, 903, "a"), (None, 904, "b")]


def _hybrid(session):
    c = hs.IndexConstants
    session.conf.set(c.INDEX_HYBRID_SCAN_ENABLED, True)
    session.conf.set(c.INDEX_HYBRID_SCAN_APPENDED_RATIO_THRESHOLD, 0.9)
    session.conf.set(c.INDEX_HYBRID_SCAN_DELETED_RATIO_THRESHOLD, 0.9)


def test_hybrid_scan_appended_files(env):
    session, h, left, right, lrows, rrows, ldir = env
    _hybrid(session)
    _write_left(ldir, "part-9.parquet", NEW_ROWS)
    session.enable_hyperspace()
    df = session.read_parquet(ldir)
    aggs, specs = standard_aggs()
    q = df.group_by("k").agg(*aggs)
    plan = q.optimized_plan()
    unions = plan_nodes(plan, BucketUnionNode)
    assert unions and unions[0].bucket_columns == ["k"], plan.pretty()
    assert batch_rows(q.collect())[1] == group_oracle(
        lrows + NEW_ROWS, 1, specs)
    st = q._last_stats
    assert "SortAggregate(bucketed)" in st.operators
    assert st.shuffles == 1      # the appended rows' repartition, no more


def test_hybrid_scan_deleted_files(env):
    session, h, left, right, lrows, rrows, ldir = env
    _hybrid(session)
    os.unlink(os.path.join(ldir, "part-0.parquet"))
    session.enable_hyperspace()
    df = session.read_parquet(ldir)
    aggs, specs = standard_aggs()
    q = df.group_by("k").agg(*aggs)
    plan = q.optimized_plan()
    scans = plan_nodes(plan, IndexScan)
    assert scans and scans[0].excluded_source_file_ids, plan.pretty()
    assert batch_rows(q.collect())[1] == group_oracle(
        lrows[len(lrows) // 2:], 1, specs)
    assert "SortAggregate(bucketed)" in q._last_stats.operators
    assert q._last_stats.shuffles == 0


def test_refreshed_index_two_files_per_bucket_null_keys(env):
    session, h, left, right, lrows, rrows, ldir = env
    # appended rows whose nulls store other placeholders than the first
    # build's: the re-sort of a two-file bucket scatters them
    extra = [(None, 1000 + i, f"n{i % 3}") for i in range(7)] + \
            [(k, 2000 + k, "x") for k in range(0, 60, 3)]
    _write_left(ldir, "part-7.parquet", extra)
    h.refresh_index("jt_l", mode="incremental")
    session.enable_hyperspace()
    df = session.read_parquet(ldir)
    aggs, specs = standard_aggs()
    q = df.group_by("k").agg(*aggs)
    plan = q.optimized_plan()
    scans = plan_nodes(plan, IndexScan)
    assert scans and scans[0].use_bucket_spec, plan.pretty()
    files = [f for f in scans[0].entry.content.os_files()
             if f.endswith(".parquet")]
    assert len(files) > 4        # more than one file in some bucket
    rows = batch_rows(q.collect())[1]
    want = group_oracle(lrows + extra, 1, specs)
    assert rows == want
    null_group = [r for r in rows if r[0] is None]
    assert len(null_group) == 1
    assert null_group[0][1] == sum(1 for r in lrows + extra if r[0] is None)
    assert "SortAggregate(bucketed)" in q._last_stats.operators
    assert q._last_stats.shuffles == 0


def test_aggregate_over_indexed_join(env):
    session, h, left, right, lrows, rrows, ldir = env
    session.enable_hyperspace()
    q = left.join(right, "k").group_by("k").agg(
        F.count(), F.sum("b"), F.max("t"))
    plan = q.optimized_plan()
    joins = plan_nodes(plan, Join)
    assert len(joins) == 1
    assert all(isinstance(c, IndexScan) and c.use_bucket_spec
               for c in joins[0].children), plan.pretty()
    out = q.collect()
    joined = join_rows_oracle(lrows, rrows, "inner")
    rows = [r for r, c in joined.items() for _ in range(c)]
    assert batch_rows(out)[1] == group_oracle(
        rows, 1, [("count", None), ("sum", 4), ("max", 5)])
    st = q._last_stats
    assert "SortMergeJoin(co-bucketed)" in st.operators
    assert "SortAggregate(shuffled)" in st.operators
    assert st.merge_joins == 1 and st.shuffles == 1


def test_ranker_picks_among_two_eligible(env):
    session, h, left, right, lrows, rrows, ldir = env
    # same indexed column, fewer included columns: smaller, so preferred
    h.create_index(left, hs.CoveringIndexConfig("jt_small", ["k"], ["a"]))
    session.enable_hyperspace()
    q = left.group_by("k").agg(F.sum("a"))
    scans = plan_nodes(q.optimized_plan(), IndexScan)
    assert [s.entry.name for s in scans] == ["jt_small"]
    assert batch_rows(q.collect())[1] == group_oracle(
        lrows, 1, [("sum", 1)])
    # a query only the wide one covers
    q2 = left.group_by("k").agg(F.min("s"))
    scans2 = plan_nodes(q2.optimized_plan(), IndexScan)
    assert [s.entry.name for s in scans2] == ["jt_l"]
