"""bucket_layout(plan) and the three consumer predicates built on it, over
plan shapes.  No data is read: the index entries are stand-ins carrying
only what the layout looks at.

The expected values are written out by hand from the rules the join, the
aggregate and the top-k have always applied:

    consumer   walks down through   needs a covering index   key match
    join       Project              no                       full list
    aggregate  Project, Filter      yes                      one column
    top-k      Project              yes                      one column
"""

from types import SimpleNamespace

import pytest

from hyperspace_amd.execution.layout import (BucketLayout, bucket_layout,
                                             group_source_bucketed,
                                             join_side_bucketed,
                                             order_source_bucketed)
from hyperspace_amd.plan.expr import col
from hyperspace_amd.plan.nodes import (BucketUnionNode, Filter, IndexScan,
                                       Project, Scan)


def _scan(indexed, kind="CoveringIndex", bucketed=True):
    entry = SimpleNamespace(name="ix", derivedDataset=SimpleNamespace(
        kind=kind, indexed_columns=list(indexed)))
    return IndexScan(entry, list(indexed) + ["v"], bucketed)


def _plain():
    schema = SimpleNamespace(field_names=lambda: ["K", "v"])
    return Scan(SimpleNamespace(schema=schema))


def _project(child):
    return Project(["K", "v"], child)


def _filter(child):
    return Filter(col("v") > 1, child)


def _union(columns):
    return BucketUnionNode([_scan(columns), _plain()], 4, list(columns))


L = BucketLayout
# name -> (plan, keys asked for, layout, join, aggregate, top-k);
# aggregate and top-k take one key: None where more are asked for
CASES = {
    "index_scan": (
        _scan(["K"]), ["k"],
        L(("k",), True, True, True), True, True, True),
    "index_scan_without_bucket_spec": (
        _scan(["K"], bucketed=False), ["k"],
        None, False, False, False),
    "zorder_scan": (
        _scan(["K"], kind="ZOrderCoveringIndex"), ["k"],
        L(("k",), False, True, True), True, False, False),
    "zorder_scan_without_bucket_spec": (
        _scan(["K"], kind="ZOrderCoveringIndex", bucketed=False), ["k"],
        None, False, False, False),
    "under_project": (
        _project(_scan(["K"])), ["K"],
        L(("k",), True, True, True), True, True, True),
    "under_two_projects": (
        _project(_project(_scan(["K"]))), ["K"],
        L(("k",), True, True, True), True, True, True),
    "under_filter": (
        _filter(_scan(["K"])), ["K"],
        L(("k",), True, True, False), False, True, False),
    "under_project_filter": (
        _project(_filter(_scan(["K"]))), ["K"],
        L(("k",), True, True, False), False, True, False),
    "under_filter_project": (
        _filter(_project(_scan(["K"]))), ["K"],
        L(("k",), True, True, False), False, True, False),
    "zorder_under_filter": (
        _filter(_scan(["K"], kind="ZOrderCoveringIndex")), ["K"],
        L(("k",), False, True, False), False, False, False),
    "bucket_union": (
        _union(["K"]), ["k"],
        L(("k",), True, True, True), True, True, True),
    "bucket_union_under_project": (
        _project(_union(["K"])), ["k"],
        L(("k",), True, True, True), True, True, True),
    "bucket_union_under_filter": (
        _filter(_union(["K"])), ["k"],
        L(("k",), True, True, False), False, True, False),
    "plain_scan": (
        _plain(), ["k"], None, False, False, False),
    "plain_scan_under_project_filter": (
        _project(_filter(_plain())), ["k"], None, False, False, False),
    "key_differs_in_case": (
        _scan(["Key"]), ["kEY"],
        L(("key",), True, True, True), True, True, True),
    "key_differs": (
        _scan(["K"]), ["v"],
        L(("k",), True, True, True), False, False, False),
    "two_keys_match": (
        _scan(["K", "J"]), ["k", "j"],
        L(("k", "j"), True, True, True), True, None, None),
    "two_keys_in_other_order": (
        _scan(["K", "J"]), ["j", "k"],
        L(("k", "j"), True, True, True), False, None, None),
    "keys_are_a_prefix": (
        _scan(["K", "J"]), ["k"],
        L(("k", "j"), True, True, True), False, False, False),
    "keys_are_a_superset": (
        _scan(["K"]), ["k", "j"],
        L(("k",), True, True, True), False, None, None),
    "union_keys_are_a_prefix": (
        _union(["K", "J"]), ["k"],
        L(("k", "j"), True, True, True), False, False, False),
    "union_two_keys_match": (
        _union(["K", "J"]), ["K", "J"],
        L(("k", "j"), True, True, True), True, None, None),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_layout_and_consumers(name):
    plan, keys, layout, join, aggregate, topk = CASES[name]
    assert bucket_layout(plan) == layout
    assert bool(join_side_bucketed(plan, keys)) is join
    if len(keys) == 1:
        assert bool(group_source_bucketed(plan, keys[0])) is aggregate
        assert bool(order_source_bucketed(plan, keys[0])) is topk
    else:
        assert aggregate is None and topk is None
