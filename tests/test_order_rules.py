"""TopKIndexRule: when it fires, what the rewritten plan looks like, the
whyNot reasons when it does not, the conf switch and explain."""

import pytest

import hyperspace_amd as hs
from hyperspace_amd.plan.nodes import (Filter, IndexScan, Limit, Project,
                                       Scan, Sort)
from hyperspace_amd.rules.apply_hyperspace import ApplyHyperspace
from hyperspace_amd.rules.candidate_collector import CandidateIndexCollector
from hyperspace_amd.rules.filter_reason import FilterReasons, ReasonCollector
from hyperspace_amd.rules.hyperspace_rules import (FilterIndexRule,
                                                   TopKIndexRule)

from aggregate_common import plan_nodes
from topk_common import COLUMNS, OrderEnv, check_topk, ops_of


@pytest.fixture
def env(tmp_path, tmp_system_path):
    e = OrderEnv(tmp_path, "cpu")
    e.index("ix_i", "i")
    e.session.enable_hyperspace()
    return e


def _reasons(env, q, index_name):
    reasons = ReasonCollector(enabled=True)
    plan = ApplyHyperspace(env.session, reasons).apply(q.plan)
    return plan, {r.code for r in reasons.all_for_index(index_name)}, reasons


def test_rule_fires_and_keeps_sort_and_limit(env):
    q = env.df.order_by("i").limit(10)
    plan, codes, reasons = _reasons(env, q, "ix_i")
    assert plan.pretty().splitlines() == [
        "Limit(10)", "  Sort([i ASC NULLS FIRST])",
        "    IndexScan(ix_i, bucketed)"]
    assert reasons.applied == {"ix_i": ["TopKIndexRule"]}
    assert not plan_nodes(plan, Scan)
    # the original plan is untouched
    assert plan_nodes(q.plan, Scan) and not plan_nodes(q.plan, IndexScan)
    check_topk(q, env.names, env.rows, [("i", True, True)], 10)
    assert "TopK(bucketed)" in ops_of(q)


def test_rule_fires_through_projections(env):
    # a projection under the sort: the index scan reads what it names
    q = env.df.select("rid", "I", "s").order_by("i").limit(5)
    plan = q.optimized_plan()
    assert isinstance(plan, Limit) and isinstance(plan.child, Sort)
    assert isinstance(plan.child.child, Project)
    scan = plan.child.child.child
    assert isinstance(scan, IndexScan) and scan.use_bucket_spec
    assert [c.lower() for c in scan.columns] == ["rid", "i", "s"]
    # a projection over the sort: what it keeps, and the order column
    q = env.df.order_by("i", ascending=False).select("rid", "d").limit(5)
    plan = q.optimized_plan()
    assert isinstance(plan.child, Project)
    assert isinstance(plan.child.child, Sort)
    scan = plan.child.child.child
    assert isinstance(scan, IndexScan)
    assert [c.lower() for c in scan.columns] == ["rid", "d", "i"]
    check_topk(q, env.names, env.rows, [("i", False, False)], 5)


def test_rule_score_is_the_filter_rules_weight(env):
    from hyperspace_amd.log.constants import States
    q = env.df.order_by("i").limit(3)
    reasons = ReasonCollector(enabled=True)
    entries = env.session.index_manager().get_indexes([States.ACTIVE])
    cands = CandidateIndexCollector(env.session, reasons).collect(
        q.plan, entries)
    new_plan, score = TopKIndexRule(env.session, reasons).apply(
        q.plan, cands)
    assert plan_nodes(new_plan, IndexScan)
    assert TopKIndexRule.SCORE == FilterIndexRule.SCORE == 50.0
    # the index covers the whole source: coverage 1
    assert score == pytest.approx(50.0)


def test_no_fire_two_column_order(env):
    q = env.df.order_by("i", "f").limit(10)
    plan, codes, _ = _reasons(env, q, "ix_i")
    assert not plan_nodes(plan, IndexScan), plan.pretty()
    check_topk(q, env.names, env.rows,
               [("i", True, True), ("f", True, True)], 10)
    assert "TopK(select)" in ops_of(q)


def test_no_fire_order_column_not_indexed(env):
    q = env.df.order_by("u").limit(10)
    plan, codes, _ = _reasons(env, q, "ix_i")
    assert not plan_nodes(plan, IndexScan), plan.pretty()
    assert FilterReasons.SORT_COL_NOT_INDEXED_COL in codes
    assert FilterReasons.SORT_COL_NOT_INDEXED_COL == \
        "SORT_COL_NOT_INDEXED_COL"


def test_no_fire_multi_column_index(env):
    env.h.delete_index("ix_i")
    env.h.create_index(env.df, hs.CoveringIndexConfig(
        "two", ["i", "u"], [c for c in COLUMNS if c not in ("i", "u")]))
    q = env.df.order_by("i").limit(10)
    plan, codes, _ = _reasons(env, q, "two")
    assert not plan_nodes(plan, IndexScan), plan.pretty()
    assert FilterReasons.SORT_COL_NOT_INDEXED_COL in codes


def test_no_fire_uncovered_column(env):
    env.h.delete_index("ix_i")
    env.h.create_index(env.df, hs.CoveringIndexConfig(
        "narrow", ["i"], ["rid"]))
    q = env.df.order_by("i").limit(10)        # needs every column
    plan, codes, _ = _reasons(env, q, "narrow")
    assert not plan_nodes(plan, IndexScan), plan.pretty()
    assert FilterReasons.MISSING_REQUIRED_COL in codes
    # what it covers is served
    q2 = env.df.select("rid", "i").order_by("i").limit(10)
    assert plan_nodes(q2.optimized_plan(), IndexScan)


def test_no_fire_filter_below(env):
    # filtered queries belong to the filter rules
    q = env.df.filter("u >= 0").order_by("i").limit(10)
    plan = q.optimized_plan()
    assert not plan_nodes(plan, IndexScan), plan.pretty()
    assert isinstance(plan.child.child, Filter)


def test_no_fire_sort_or_limit_alone(env):
    assert not plan_nodes(env.df.order_by("i").optimized_plan(), IndexScan)
    assert not plan_nodes(env.df.limit(4).optimized_plan(), IndexScan)


def test_conf_switch(env):
    key = hs.IndexConstants.INDEX_TOPK_RULE_ENABLED
    assert key == "spark.hyperspace.index.topKRule.enabled"
    assert env.session.conf.topk_rule_enabled is True
    q = env.df.order_by("i").limit(10)
    env.session.conf.set(key, False)
    plan, codes, _ = _reasons(env, q, "ix_i")
    assert not plan_nodes(plan, IndexScan) and not codes
    check_topk(q, env.names, env.rows, [("i", True, True)], 10)
    assert "TopK(select)" in ops_of(q)
    env.session.conf.set(key, True)
    assert plan_nodes(q.optimized_plan(), IndexScan)


def test_why_not_reports_the_reasons(env):
    env.h.create_index(env.df, hs.CoveringIndexConfig(
        "narrow", ["i"], ["rid"]))
    text = env.h.why_not(env.df.order_by("u").limit(10))
    assert "SORT_COL_NOT_INDEXED_COL" in text
    env.h.delete_index("ix_i")
    text = env.h.why_not(env.df.order_by("i").limit(10))
    assert "MISSING_REQUIRED_COL" in text


def test_explain_shows_index_scan_and_physical_operator(env):
    q = env.df.order_by("i", ascending=False).limit(10)
    text = env.h.explain(q, verbose=True)
    assert "Limit(10)" in text
    assert "Sort([i DESC NULLS LAST])" in text
    assert "IndexScan(ix_i, bucketed)" in text
    assert "TopK(bucketed)" in text
    assert "TopK(select)" in text            # the plan without indexes
    assert "ix_i" in text
