"""How a subplan's rows are laid out in buckets — from the plan alone.

``bucket_layout(plan)`` is the single answer to "is this input bucketed":
the join, the aggregate and the top-k each ask it through one small
predicate below, and the names of the physical operators an Aggregate or
a Limit runs as are derived from those predicates (the executor and
explain() both use them, so they cannot disagree).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

from ..plan.nodes import (Aggregate, BucketUnionNode, Filter, IndexScan,
                          Limit, LogicalPlan, Project, Sort)


@dataclass(frozen=True)
class BucketLayout:
    """Layout of a subplan over a bucketed IndexScan or a BucketUnion.

    columns        lower-cased bucket (and per-bucket sort) columns
    covering       the leaf is a CoveringIndex scan or a BucketUnion (a
                   z-order scan's "buckets" are chunk ids, not hash buckets)
    rows_adjacent  rows with equal keys are adjacent within a bucket;
                   Project and Filter both keep row order
    has_segments   executing the subplan returns the bucket segment
                   offsets; a Project passes them on, a Filter drops them
    """
    columns: Tuple[str, ...]
    covering: bool
    rows_adjacent: bool
    has_segments: bool

    def keyed_on(self, keys: List[str]) -> bool:
        return self.columns == tuple(k.lower() for k in keys)


def bucket_layout(plan: LogicalPlan) -> Optional[BucketLayout]:
    """Layout of ``plan`` walked down through Project and Filter nodes, or
    None when the leaf is neither an IndexScan with ``use_bucket_spec`` nor
    a BucketUnion."""
    node = plan
    has_segments = True
    while isinstance(node, (Project, Filter)):
        if isinstance(node, Filter):
            has_segments = False
        node = node.child
    if isinstance(node, IndexScan) and node.use_bucket_spec:
        index = node.entry.derivedDataset
        columns, covering = index.indexed_columns, \
            index.kind == "CoveringIndex"
    elif isinstance(node, BucketUnionNode):
        columns, covering = node.bucket_columns, True
    else:
        return None
    return BucketLayout(tuple(c.lower() for c in columns), covering,
                        True, has_segments)


def join_side_bucketed(plan: LogicalPlan, key_names: List[str]) -> bool:
    """A join side whose segments partition it on exactly the join keys
    (the merge join then needs no sort and no exchange on this side)."""
    lay = bucket_layout(plan)
    return lay is not None and lay.has_segments and lay.keyed_on(key_names)


def group_source_bucketed(plan: LogicalPlan, key: str) -> bool:
    """An aggregate input in which every group of the single grouping
    column lies inside one bucket with its rows adjacent."""
    lay = bucket_layout(plan)
    return lay is not None and lay.covering and lay.rows_adjacent and \
        lay.keyed_on([key])


def order_source_bucketed(plan: LogicalPlan, key: str) -> bool:
    """A top-k input whose buckets are each sorted on the single order
    column, with the segment offsets the bucket heads come from."""
    lay = bucket_layout(plan)
    return lay is not None and lay.covering and lay.has_segments and \
        lay.keyed_on([key])


def aggregate_operator_name(plan: Aggregate) -> str:
    """Physical operator an Aggregate node runs as."""
    if not plan.group_cols:
        return "SortAggregate(global)"
    if len(plan.group_cols) == 1 and \
            group_source_bucketed(plan.child, plan.group_cols[0]):
        return "SortAggregate(bucketed)"
    return "SortAggregate(shuffled)"


def _limit_sort_shape(plan: Limit):
    """(Sort, Project or None) when the Limit sits on a Sort, directly or
    through one Project; (None, None) otherwise."""
    node = plan.child
    if isinstance(node, Sort):
        return node, None
    if isinstance(node, Project) and isinstance(node.child, Sort):
        return node.child, node
    return None, None


def topk_operator_name(plan: Limit) -> str:
    """Physical operator a Limit node runs as: ``Limit`` on its own, over
    a Sort ``TopK(bucketed)`` when there is one order column and the
    Sort's child is bucketed on it, else ``TopK(select)``.  (A bucketed
    source whose key column holds nulls falls to the select at run
    time.)"""
    sort, _ = _limit_sort_shape(plan)
    if sort is None:
        return "Limit"
    if len(sort.orders) == 1 and \
            order_source_bucketed(sort.child, sort.orders[0].column):
        return "TopK(bucketed)"
    return "TopK(select)"
