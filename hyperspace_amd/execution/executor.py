"""Physical plan executor.

Executes LogicalPlan trees over ColumnBatches.  On a GPU box all hot paths
run the hand-written HIP kernels via hyperspace_amd.ops (which raises if
the extension is missing — no silent eager fallback); on CPU the torch
reference ops run instead (test/plumbing mode, BASELINE config 1).

This module holds the dispatch (``Executor._exec``) and the operators
that are a few lines each; the rest of the package holds one concern per
module.  Operator -> data-plane mapping -> module:
  Scan            K1  parquet decode (host pyarrow path or device decode)
  Filter          K7 / filter scan: native select_range + gather
                      (predicate.py; the pruned reads are chosen here)
  Join            K4  per-bucket merge join (zero exchange when
                      co-bucketed) (join.py)
  IndexScan       bucket-pruned index read (FilterIndexRule target)
                      (index_read.py)
  BucketUnionNode K5  partition-aligned concat (+ per-bucket re-sort)
  Aggregate       K13 group_offsets + fused segmented_reduce over adjacent
                      runs (no sort, no exchange, when the child is
                      bucketed on the grouping column) (aggregate.py)
  Sort / Limit    K14 stable radix sort by order keys; Limit over Sort runs
                      as a top-k: radix select of the candidates, or the
                      heads of the buckets of an index on the order column
                      (ordering.py)

Whether an input counts as bucketed for the join, the aggregate or the
top-k is one property of its plan: ``layout.bucket_layout``.
"""

from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import ordering
from .aggregate import exec_aggregate
from .columnar import ColumnBatch, _empty_batch
from .index_read import _zorder_prune, exec_index_scan
from .join import exec_join
from .layout import _limit_sort_shape, topk_operator_name
from .predicate import _predicate_indices, _single_equality
from .. import ops
from ..config import IndexConstants
from ..exceptions import HyperspaceException
from ..ops.string_hash import bucket_hash_keys
from ..parallel import dist_context as dc
from ..plan.expr import Expr
from ..plan.nodes import (Aggregate, BucketUnionNode, Filter, IndexScan,
                          Join, Limit, LogicalPlan, Project, Scan, Sort,
                          UnionNode)


class PhysicalStats:
    """Per-execution counters (telemetry + tests assert on these —
    e.g. shuffle/exchange elimination in the indexed join path)."""

    def __init__(self):
        self.scanned_files = 0
        self.scanned_bytes = 0
        self.shuffles = 0          # on-the-fly repartitions (Exchange analog)
        self.merge_joins = 0
        self.hash_joins = 0
        self.sort_aggregates = 0
        self.sorts = 0             # full ORDER BY sorts (a top-k is none)
        self.bucket_pruned_files = 0
        self.operators: List[str] = []

    def record(self, name: str):
        self.operators.append(name)


class Executor:
    def __init__(self, session):
        self.session = session
        self.stats = PhysicalStats()

    @property
    def device(self):
        return self.session.device

    # ------------------------------------------------------------------
    def execute(self, plan: LogicalPlan) -> ColumnBatch:
        batch, _ = self._exec(plan)
        return batch

    def _exec(self, plan: LogicalPlan
              ) -> Tuple[ColumnBatch, Optional[torch.Tensor]]:
        """Returns (batch, bucket segment offsets or None).

        The second element is set when the batch is bucket-partitioned
        (IndexScan with use_bucket_spec, BucketUnion) — segment offsets
        have length num_buckets+1.
        """
        if isinstance(plan, Scan):
            return self._exec_scan(plan), None
        if isinstance(plan, IndexScan):
            return exec_index_scan(self, plan)
        if isinstance(plan, Filter):
            return self._exec_filter(plan)
        if isinstance(plan, Project):
            batch, seg = self._exec(plan.child)
            self.stats.record("Project")
            return batch.select(plan.columns), seg
        if isinstance(plan, Join):
            return exec_join(self, plan), None
        if isinstance(plan, BucketUnionNode):
            return self._exec_bucket_union(plan)
        if isinstance(plan, Aggregate):
            return exec_aggregate(self, plan), None
        if isinstance(plan, Sort):
            return self._exec_sort(plan), None
        if isinstance(plan, Limit):
            return self._exec_limit(plan), None
        if isinstance(plan, UnionNode):
            self.stats.record("Union")
            parts = [self._exec(c)[0] for c in plan.children]
            cols = plan.output_columns()
            return ColumnBatch.concat(
                [p.select(cols) for p in parts if p.num_rows > 0]
                or [parts[0].select(cols)]), None
        raise HyperspaceException(f"Cannot execute {type(plan).__name__}")

    # ------------------------------------------------------------------
    def _exec_scan(self, plan: Scan, file_subset: Optional[List[str]] = None,
                   lineage_tracker=None, shard: bool = False) -> ColumnBatch:
        self.stats.record("ParquetScan")
        files = plan.relation.all_files()
        if file_subset is None and plan.file_subset is not None:
            file_subset = plan.file_subset
        if file_subset is not None:
            subset = set(file_subset)
            files = [f for f in files if f.name in subset]
        if shard:
            # distributed build: round-robin file shard per rank
            if dc.is_distributed():
                files = files[dc.get_rank()::dc.get_world_size()]
        paths = [f.name for f in files]
        self.stats.scanned_files += len(paths)
        self.stats.scanned_bytes += sum(f.size for f in files)
        if paths:
            batch, row_counts = plan.relation.read_files(
                paths, None, self.device)
        else:
            batch, row_counts = _empty_batch(plan.relation.schema), []
        if lineage_tracker is not None:
            # device-side lineage materialization (see ScanStream)
            fids = torch.tensor(
                [lineage_tracker.add_file(f.name, f.size, f.modifiedTime)
                 for f in files], dtype=torch.int64, device=batch.device)
            counts = torch.tensor(row_counts, dtype=torch.int64,
                                  device=batch.device)
            batch = batch.with_column(
                IndexConstants.DATA_FILE_NAME_ID_COLUMN,
                torch.repeat_interleave(fids, counts))
        if self.device.type == "cuda":
            batch = batch.to(self.device)
        return batch

    # ------------------------------------------------------------------
    def _exec_filter(self, plan: Filter
                     ) -> Tuple[ColumnBatch, Optional[torch.Tensor]]:
        child = plan.child
        # z-order path: prune index files via their Parquet column stats
        if isinstance(child, IndexScan) and \
                child.entry.derivedDataset.kind == "ZOrderCoveringIndex" \
                and child.version_files is None:
            pruned = _zorder_prune(self, plan.condition, child)
            if pruned is not None:
                batch, _ = exec_index_scan(self, pruned)
                self.stats.record("Filter")
                return self._apply_predicate(batch, plan.condition), None
        # bucket pruning: Filter(eq on first indexed col, IndexScan)
        if isinstance(child, IndexScan) and child.use_bucket_spec:
            eq = _single_equality(plan.condition)
            index = child.entry.derivedDataset
            if eq is not None and index.indexed_columns and \
                    eq[0].lower() == index.indexed_columns[0].lower():
                batch, _ = exec_index_scan(self, child, eq_prune=eq)
                self.stats.record("Filter")
                return self._apply_predicate(batch, plan.condition), None
        # hive partition pruning: partition-only conjuncts drop files on
        # metadata alone (Spark's PartitioningAwareFileIndex pruning);
        # composes with a data-skipping file_subset by intersection
        if isinstance(child, Scan):
            prune = getattr(child.relation, "prune_partitions", None)
            kept = prune(plan.condition) if prune is not None else None
            if kept is not None:
                if child.file_subset is not None:
                    subset = set(child.file_subset)
                    kept = [p for p in kept if p in subset]
                batch = self._exec_scan(child, file_subset=kept)
                self.stats.record("Filter(partition-pruned)")
                return self._apply_predicate(batch, plan.condition), None
        batch, _ = self._exec(child)
        self.stats.record("Filter")
        return self._apply_predicate(batch, plan.condition), None

    def _apply_predicate(self, batch: ColumnBatch, cond: Expr) -> ColumnBatch:
        if batch.num_rows == 0:
            return batch
        return batch.gather(_predicate_indices(batch, cond))

    # ------------------------------------------------------------------
    def _refuse_distributed_order(self, what: str):
        if dc.is_distributed() and dc.get_world_size() > 1:
            raise HyperspaceException(
                f"{what} is not supported in a distributed session: every "
                "rank holds a partition of the rows, and a per-rank order "
                "is not a global one")

    def _exec_sort(self, plan: Sort) -> ColumnBatch:
        """Full ORDER BY: gather by the stable multi-column permutation."""
        self._refuse_distributed_order("ORDER BY")
        batch, _ = self._exec(plan.child)
        self.stats.record("Sort")
        self.stats.sorts += 1
        if batch.num_rows > 1:
            batch = batch.gather(ordering.order_perm(batch, plan.orders))
        return batch

    def _exec_limit(self, plan: Limit) -> ColumnBatch:
        """LIMIT n: the child's first n rows; over a Sort (directly or
        through one Project) a top-k that never sorts the whole input.

        TopK(bucketed): one order column, and the child is bucketed and
        sorted on it (no nulls in it): the first (last) n rows of every
        bucket are the candidates.  TopK(select): everything else, by
        radix select on the leading order column.  Both sort only their
        candidates."""
        self._refuse_distributed_order("LIMIT")
        sort, project = _limit_sort_shape(plan)
        n = plan.n
        if sort is None:
            batch, _ = self._exec(plan.child)
            self.stats.record("Limit")
            return batch.slice(0, min(n, batch.num_rows))
        batch, seg = self._exec(sort.child)
        op = topk_operator_name(plan)
        # TopK(bucketed) is planned only where the layout has segments, so
        # seg is set; what the plan cannot tell is whether the key holds
        # nulls: multi-file buckets re-sort on the stored placeholder of
        # null rows, so nulls are not reliably first there
        if op == "TopK(bucketed)" and batch.has_nulls(sort.orders[0].column):
            op = "TopK(select)"
        self.stats.record(op)
        if n == 0 or batch.num_rows == 0:
            out = batch.slice(0, 0)
        elif op == "TopK(bucketed)":
            out = ordering.topk_bucketed(batch, seg, sort.orders[0], n)
        else:
            out = ordering.topk_select(batch, sort.orders, n)
        if project is not None:
            self.stats.record("Project")
            out = out.select(project.columns)
        return out

    # ------------------------------------------------------------------
    def _exec_bucket_union(self, plan: BucketUnionNode
                           ) -> Tuple[ColumnBatch, Optional[torch.Tensor]]:
        """Partition-aligned union: concatenate same-bucket segments from
        each child, re-sorting each merged bucket by the bucket columns
        (K5; appended data was shuffled in by K2/K6 beforehand)."""
        self.stats.record("BucketUnion")
        n = plan.num_buckets
        child_parts: List[Tuple[ColumnBatch, torch.Tensor]] = []
        for c in plan.children:
            batch, seg = self._exec(c)
            if seg is None:
                # on-the-fly repartition of appended data (K2/K6)
                self.stats.shuffles += 1
                batch, seg = self._repartition(batch, plan.bucket_columns, n)
            child_parts.append((batch, seg))

        # vectorized union: concatenate children, rebuild per-row bucket
        # ids from the segment offsets, then ONE device-wide
        # sort-by-(bucket, key) pass restores the merged bucketed+sorted
        # layout (no per-bucket Python loop)
        from ..index.covering.index import sort_by_bucket_and_keys
        cols = child_parts[0][0].names
        batches = []
        bucket_ids = []
        for batch, seg in child_parts:
            if batch.num_rows == 0:
                continue
            batches.append(batch.select(cols))
            seg_d = seg.to(batch.device)
            counts = (seg_d[1:] - seg_d[:-1])
            bucket_ids.append(torch.repeat_interleave(
                torch.arange(n, dtype=torch.int64, device=batch.device),
                counts))
        if not batches:
            return child_parts[0][0].slice(0, 0), torch.zeros(
                n + 1, dtype=torch.int64)
        merged = ColumnBatch.concat(batches)
        all_buckets = torch.cat(bucket_ids).to(torch.int32)
        return sort_by_bucket_and_keys(merged, all_buckets,
                                       [plan.bucket_columns[0]], n)

    def _repartition(self, batch: ColumnBatch, bucket_cols: List[str],
                     num_buckets: int
                     ) -> Tuple[ColumnBatch, torch.Tensor]:
        """Hash-repartition + per-bucket sort (K2+K3 on the fly)."""
        # local: the index package imports this one for ColumnBatch
        from ..index.covering.index import sort_by_bucket_and_keys
        keys = bucket_hash_keys(batch, bucket_cols)
        key_masks = [batch.mask(c) for c in bucket_cols]
        bucket_ids = ops.murmur3_bucket(
            keys, num_buckets,
            key_masks if any(m is not None for m in key_masks) else None)
        return sort_by_bucket_and_keys(batch, bucket_ids, bucket_cols,
                                       num_buckets)
