"""Physical plan executor.

Executes LogicalPlan trees over ColumnBatches.  On a GPU box all hot paths
run the hand-written HIP kernels via hyperspace_amd.ops (which raises if
the extension is missing — no silent eager fallback); on CPU the torch
reference ops run instead (test/plumbing mode, BASELINE config 1).

Operator -> data-plane mapping:
  Scan            K1  parquet decode (host pyarrow path or device decode)
  Filter          K7 / filter scan: native select_range + gather
  Join            K4  per-bucket merge join (zero exchange when co-bucketed)
  IndexScan       bucket-pruned index read (FilterIndexRule target)
  BucketUnionNode K5  partition-aligned concat (+ per-bucket re-sort)
  Aggregate       K13 group_offsets + fused segmented_reduce over adjacent
                      runs (no sort, no exchange, when the child is
                      bucketed on the grouping column)
  Sort / Limit    K14 stable radix sort by order keys; Limit over Sort runs
                      as a top-k: radix select of the candidates, or the
                      heads of the buckets of an index on the order column
"""

from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import torch

from .columnar import ColumnBatch, StringColumn
from . import sql_compare
from .. import ops
from ..config import IndexConstants
from ..exceptions import HyperspaceException
from ..plan.expr import (And, BinComp, Col, Expr, In, IsNotNull, IsNull,
                         Lit, Not, Or, extract_equi_join_keys)
from ..plan.nodes import (Aggregate, BucketUnionNode, Filter, IndexScan,
                          Join, Limit, LogicalPlan, Project, Scan, Sort,
                          UnionNode)
from ..sources.parquet_io import (read_files_batch,
                                  read_files_batch_device,
                                  bucket_id_of_file)


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
            return self._exec_index_scan(plan, eq_prune=None)
        if isinstance(plan, Filter):
            return self._exec_filter(plan)
        if isinstance(plan, Project):
            batch, seg = self._exec(plan.child)
            self.stats.record("Project")
            return batch.select(plan.columns), seg
        if isinstance(plan, Join):
            return self._exec_join(plan), None
        if isinstance(plan, BucketUnionNode):
            return self._exec_bucket_union(plan)
        if isinstance(plan, Aggregate):
            return self._exec_aggregate(plan), None
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
            from ..parallel import dist_context as dc
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
    def _exec_index_scan(self, plan: IndexScan,
                         eq_prune: Optional[Tuple[str, object]] = None
                         ) -> Tuple[ColumnBatch, Optional[torch.Tensor]]:
        """Read covering-index data.  When ``use_bucket_spec`` the result is
        ordered by bucket with segment offsets returned; ``eq_prune`` =
        (column, value) prunes to the single matching bucket file set."""
        self.stats.record("IndexScan")
        entry = plan.entry
        index = entry.derivedDataset
        # z-order indexes have chunk ids, not hash buckets: size the
        # segment array to the max id seen
        num_buckets = getattr(index, "num_buckets", 0)
        all_files = (plan.version_files if plan.version_files is not None
                     else [f for f in entry.content.os_files()
                           if f.endswith(".parquet")])

        # group files by bucket id from the filename contract
        by_bucket: Dict[int, List[str]] = {}
        for p in all_files:
            b = bucket_id_of_file(p)
            if b is None:
                raise HyperspaceException(f"Index file without bucket id: {p}")
            by_bucket.setdefault(b, []).append(p)

        if by_bucket:
            num_buckets = max(num_buckets, max(by_bucket) + 1)
        wanted_buckets = sorted(by_bucket)
        # distributed query: each rank serves its owned buckets
        # (b % world == rank); results are per-rank partitions of the
        # answer, co-located with the join's other side by construction
        from ..parallel import dist_context as dc
        if dc.is_distributed() and dc.get_world_size() > 1 and \
                plan.use_bucket_spec:
            rank, world = dc.get_rank(), dc.get_world_size()
            wanted_buckets = [b for b in wanted_buckets
                              if b % world == rank]
        read_cols = list(plan.columns)
        if plan.excluded_source_file_ids:
            lineage_col = IndexConstants.DATA_FILE_NAME_ID_COLUMN
            if lineage_col not in read_cols:
                read_cols = read_cols + [lineage_col]

        # -- device-resident load, cached (288 GB HBM keeps indexes hot) --
        cache = self.session.index_data_cache()

        # equality bucket pruning, cold-path aware: if the full index is
        # already cached we slice it; otherwise we only LOAD the single
        # matching bucket (first-query latency = one bucket, not the
        # whole index)
        prune_bucket = None
        if eq_prune is not None:
            col_name, value = eq_prune
            prune_bucket = self._bucket_of_value(index, col_name, value,
                                                 num_buckets)
            full_files = [p for b in wanted_buckets
                          for p in sorted(by_bucket[b])]
            full_key = (cache.key(entry, full_files)
                        if cache else None)
            full_cached = (cache.get(full_key, read_cols)
                           if cache else None)
            if full_cached is not None:
                batch, seg = full_cached
                self.stats.record("IndexScan(cached)")
                self.stats.bucket_pruned_files += sum(
                    len(by_bucket[x]) for x in wanted_buckets
                    if x != prune_bucket)
                b = prune_bucket
                if b in wanted_buckets:
                    batch = batch.slice(int(seg[b]), int(seg[b + 1]))
                else:
                    batch = batch.slice(0, 0)
                batch = self._apply_excluded(plan, batch)
                return batch.select(plan.columns), None
            # cold: restrict the load to the matching bucket (membership
            # checked against the OWNERSHIP-filtered set so each rank
            # serves only its own buckets at N>1)
            self.stats.bucket_pruned_files += sum(
                len(by_bucket[x]) for x in wanted_buckets
                if x != prune_bucket)
            wanted_buckets = ([prune_bucket]
                              if prune_bucket in wanted_buckets else [])

        cache_files = [p for b in wanted_buckets
                       for p in sorted(by_bucket[b])]
        key = cache.key(entry, cache_files) if cache else None
        cached = cache.get(key, read_cols) if cache else None
        if cached is not None:
            batch, seg = cached
            self.stats.record("IndexScan(cached)")
        else:
            sort_col = (index.indexed_columns[0]
                        if getattr(index, "indexed_columns", None) else None)
            # one batched read of every wanted file (bucket-major order) —
            # the reader's thread pool overlaps disk/PCIe/decode across
            # files; per-bucket segments come from the per-file row counts
            ordered_paths: List[str] = []
            files_per_bucket: List[Tuple[int, int]] = []
            file_ix_per_bucket: List[Tuple[int, int]] = []
            for b in wanted_buckets:
                paths = sorted(by_bucket[b])
                files_per_bucket.append((b, len(paths)))
                file_ix_per_bucket.append(
                    (len(ordered_paths), len(paths)))
                ordered_paths.extend(paths)
            self.stats.scanned_files += len(ordered_paths)
            import time as _time
            _t0 = _time.perf_counter()
            if not ordered_paths:
                batch = ColumnBatch({c: torch.empty(0) for c in read_cols})
                row_counts = []
            elif self.device.type == "cuda":
                batch, row_counts = read_files_batch_device(
                    ordered_paths, self.device, columns=read_cols)
            else:
                batch, row_counts = read_files_batch(
                    ordered_paths, columns=read_cols)
            if os.environ.get("HS_TIMING"):
                import sys as _sys
                print(f"[hs-timing] index scan read: {len(ordered_paths)}"
                      f" files {_time.perf_counter() - _t0:.3f}s",
                      file=_sys.stderr)
            seg_counts = torch.zeros(num_buckets + 1, dtype=torch.int64)
            fi = 0
            for b, nfiles in files_per_bucket:
                seg_counts[b + 1] = sum(row_counts[fi:fi + nfiles])
                fi += nfiles
            seg = torch.cumsum(seg_counts, 0)
            # multi-file buckets: each file is sorted but their
            # concatenation is not — re-sort merged buckets so merge
            # joins keep the sorted-segment contract (Spark re-sorts
            # multi-file buckets inside SortMergeJoinExec the same way).
            # Per-bucket sorts beat one whole-batch (bucket,key) sort
            # here: at multi-billion-row scale the global sort's i64
            # payloads + temporaries double the memory traffic
            # (measured 2.3x slower on a 40 GiB two-group index).
            if plan.use_bucket_spec and sort_col is not None and \
                    any(n > 1 for _, n in files_per_bucket) and \
                    batch.num_rows:
                merged_ok = not batch.has_nulls(sort_col) and \
                    all(n <= 2 for _, n in files_per_bucket)
                if merged_ok:
                    # every merged bucket holds exactly two sorted runs
                    # (incremental refresh / two-group builds): ONE
                    # segmented merge-rank launch (K4b) replaces the
                    # per-bucket sort loop
                    split = seg[1:].clone()
                    for (b, nfiles), (fi0, _) in zip(
                            files_per_bucket, file_ix_per_bucket):
                        if nfiles == 2:
                            split[b] = int(seg[b]) + row_counts[fi0]
                    keys = ops.sql_key(batch.tensor(sort_col))
                    perm = ops.run_merge_perm(keys, seg, split)
                    batch = batch.gather(perm)
                else:
                    pieces: List[ColumnBatch] = []
                    for (b, nfiles), (fi0, _) in zip(files_per_bucket,
                                                     file_ix_per_bucket):
                        lo, hi = int(seg[b]), int(seg[b + 1])
                        sub = batch.slice(lo, hi)
                        if nfiles > 1 and sub.num_rows:
                            perm = ops.sort_perm(
                                ops.sql_key(sub.tensor(sort_col)))
                            sub = sub.gather(perm)
                        pieces.append(sub)
                    batch = ColumnBatch.concat(pieces)
            if cache:
                cache.put(key, batch, seg)

        seg_local = None if eq_prune is not None else seg

        # lineage delete filter (Hybrid Scan deletes, K7)
        if plan.excluded_source_file_ids and batch.num_rows:
            ids = torch.tensor(sorted(plan.excluded_source_file_ids),
                               dtype=torch.int64, device=batch.device)
            lineage = batch.tensor(IndexConstants.DATA_FILE_NAME_ID_COLUMN)
            keep = ~ops.isin_sorted(lineage, ids)
            kept_idx = torch.nonzero(keep, as_tuple=False).flatten()
            # recompute per-bucket counts after the filter
            if seg_local is not None:
                new_counts = torch.zeros(num_buckets + 1, dtype=torch.int64)
                kc = kept_idx.cpu()
                for b in wanted_buckets:
                    lo, hi = int(seg_local[b]), int(seg_local[b + 1])
                    new_counts[b + 1] = int(((kc >= lo) & (kc < hi)).sum())
                seg_local = torch.cumsum(new_counts, 0)
            batch = batch.gather(kept_idx)
            self.stats.record("LineageFilter")
        batch = batch.select(plan.columns)

        if plan.use_bucket_spec and eq_prune is None:
            return batch, seg_local
        return batch, None

    def _apply_excluded(self, plan: IndexScan, batch: ColumnBatch
                        ) -> ColumnBatch:
        """Lineage delete filter for the cached-slice fast path."""
        if not plan.excluded_source_file_ids or batch.num_rows == 0:
            return batch
        ids = torch.tensor(sorted(plan.excluded_source_file_ids),
                           dtype=torch.int64, device=batch.device)
        lineage = batch.tensor(IndexConstants.DATA_FILE_NAME_ID_COLUMN)
        keep = ~ops.isin_sorted(lineage, ids)
        self.stats.record("LineageFilter")
        return batch.gather(torch.nonzero(keep, as_tuple=False).flatten())

    def _zorder_prune(self, cond: Expr, scan: IndexScan):
        """Prune a z-order IndexScan's file list using Parquet column
        stats for every comparison conjunct on an indexed column."""
        from ..plan.expr import split_conjunctive
        index = scan.entry.derivedDataset
        files = [f for f in scan.entry.content.os_files()
                 if f.endswith(".parquet")]
        indexed = {c.lower() for c in index.indexed_columns}
        total_skipped = 0
        for conj in split_conjunctive(cond):
            if isinstance(conj, BinComp) and isinstance(conj.left, Col) \
                    and isinstance(conj.right, Lit) and \
                    conj.left.name.lower() in indexed:
                files, skipped = index.prune_files_by_stats(
                    files, conj.left.name, conj.op, conj.right.value)
                total_skipped += skipped
        if total_skipped == 0:
            return None
        self.stats.bucket_pruned_files += total_skipped
        return IndexScan(scan.entry, scan.columns, False,
                         scan.excluded_source_file_ids,
                         version_files=files)

    def _bucket_of_value(self, index, col_name: str, value,
                         num_buckets: int) -> int:
        """Bucket holding every row SQL-equal to the literal; -1 (no
        bucket) when no value of the column's type equals it."""
        if index.schema.field_type(col_name) == "string":
            from ..ops.string_hash import bucket_of_string_value
            return bucket_of_string_value(str(value), num_buckets)
        t = _value_tensor(index.schema.field_type(col_name), value)
        if t is None:
            return -1
        return int(ops.cpu_ref.murmur3_bucket([t], num_buckets)[0])

    # ------------------------------------------------------------------
    def _exec_filter(self, plan: Filter
                     ) -> Tuple[ColumnBatch, Optional[torch.Tensor]]:
        child = plan.child
        # z-order path: prune index files via their Parquet column stats
        if isinstance(child, IndexScan) and \
                child.entry.derivedDataset.kind == "ZOrderCoveringIndex" \
                and child.version_files is None:
            pruned = self._zorder_prune(plan.condition, child)
            if pruned is not None:
                batch, _ = self._exec_index_scan(pruned)
                self.stats.record("Filter")
                return self._apply_predicate(batch, plan.condition), None
        # bucket pruning: Filter(eq on first indexed col, IndexScan)
        if isinstance(child, IndexScan) and child.use_bucket_spec:
            eq = _single_equality(plan.condition)
            index = child.entry.derivedDataset
            if eq is not None and index.indexed_columns and \
                    eq[0].lower() == index.indexed_columns[0].lower():
                batch, seg = self._exec_index_scan(child, eq_prune=eq)
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
        batch, seg = self._exec(child)
        self.stats.record("Filter")
        return self._apply_predicate(batch, plan.condition), None

    def _apply_predicate(self, batch: ColumnBatch, cond: Expr) -> ColumnBatch:
        if batch.num_rows == 0:
            return batch
        idx = self._predicate_indices(batch, cond)
        return batch.gather(idx)

    def _predicate_indices(self, batch: ColumnBatch,
                           cond: Expr) -> torch.Tensor:
        """Native fast path for a single numeric comparison (select_range
        kernel); general path composes boolean masks."""
        if not any(batch.has_column(c) and batch.has_nulls(c)
                   for c in cond.references()):
            rng = _as_range(cond, batch)
            if rng is not None:
                col, lo, hi = rng
                if lo is None:       # no value of the column can match
                    return torch.empty(0, dtype=torch.int64,
                                       device=batch.device)
                return ops.select_range_u64(ops.sql_key(col), lo, hi,
                                            True, True)
        mask = self._eval_mask(batch, cond)
        return torch.nonzero(mask, as_tuple=False).flatten()

    def _valid_of(self, batch: ColumnBatch, e: Expr
                  ) -> Optional[torch.Tensor]:
        """Conjunction of validity masks over e's referenced columns, or
        None when none of them are nullable."""
        out = None
        for c in e.references():
            if not batch.has_column(c):
                continue
            m = batch.mask(c)
            if m is not None:
                out = m if out is None else out & m
        return out

    def _eval_mask(self, batch: ColumnBatch, e: Expr) -> torch.Tensor:
        if isinstance(e, And):
            return self._eval_mask(batch, e.left) & \
                self._eval_mask(batch, e.right)
        if isinstance(e, Or):
            return self._eval_mask(batch, e.left) | \
                self._eval_mask(batch, e.right)
        if isinstance(e, Not):
            # SQL three-valued logic: NOT(null-involving predicate) is
            # null -> the row is excluded, so AND the child's validity
            m = ~self._eval_mask(batch, e.child)
            v = self._valid_of(batch, e.child)
            return m & v if v is not None else m
        if isinstance(e, IsNotNull):
            m = batch.mask(e.col.name) if batch.has_column(e.col.name) \
                else None
            if m is not None:
                return m.clone()
            return torch.ones(batch.num_rows, dtype=torch.bool,
                              device=batch.device)
        if isinstance(e, IsNull):
            m = batch.mask(e.col.name) if batch.has_column(e.col.name) \
                else None
            if m is not None:
                return ~m
            return torch.zeros(batch.num_rows, dtype=torch.bool,
                               device=batch.device)
        if isinstance(e, In):
            from ..plan.expr import Arith
            if isinstance(e.col, Arith):
                m = _in_mask(_eval_arith(batch, e.col), e.values)
                v = self._valid_of(batch, e)
                return m & v if v is not None else m
            col = batch.column(e.col.name)
            vals = e.values
            if isinstance(col, StringColumn):
                codes = torch.tensor(
                    sorted(c for c in (col.code_of(v) for v in vals)
                           if c >= 0),
                    dtype=torch.int64, device=col.codes.device)
                m = ops.isin_sorted(col.codes.to(torch.int64), codes)
            else:
                m = _in_mask(col, vals)
            v = self._valid_of(batch, e)
            return m & v if v is not None else m
        if isinstance(e, BinComp):
            m = _compare(batch, e)
            v = self._valid_of(batch, e)
            return m & v if v is not None else m
        raise HyperspaceException(f"Cannot evaluate {e!r}")

    # ------------------------------------------------------------------
    def _exec_join(self, plan: Join) -> ColumnBatch:
        pairs = extract_equi_join_keys(plan.condition)
        if not pairs:
            raise HyperspaceException(
                "Only equi-joins are executable in v0")
        lkeys_names = [p[0] for p in pairs]
        rkeys_names = [p[1] for p in pairs]

        left_bucketed = _bucketed_side(plan.left, lkeys_names)
        right_bucketed = _bucketed_side(plan.right, rkeys_names)

        lbatch, lseg = self._exec(plan.left)
        rbatch, rseg = self._exec(plan.right)

        # two indexes are co-bucketed only if equal keys hash alike: an
        # int64 key and a narrower one (or double and float) land in
        # different buckets, so such a pair joins on the shuffled path
        co_bucketed = left_bucketed and right_bucketed and all(
            _same_hash_kind(lbatch.column(ln), rbatch.column(rn))
            for ln, rn in pairs)

        if plan.join_type != "inner":
            return self._exec_typed_join(
                plan.join_type, pairs, lbatch, lseg, rbatch, rseg,
                co_bucketed)

        # inner-join SQL semantics: null join keys never match — drop
        # them up front (bucketed layouts keep NULLS FIRST per bucket,
        # so the segment offsets shift by the per-prefix null count)
        lbatch, lseg = _drop_null_keys(lbatch, lkeys_names[0], lseg)
        rbatch, rseg = _drop_null_keys(rbatch, rkeys_names[0], rseg)

        if (co_bucketed and lseg is not None
                and rseg is not None and lseg.numel() == rseg.numel()):
            # zero-shuffle co-bucketed sort-merge join (K4):
            # both sides already hash-partitioned into the same buckets and
            # sorted by the join key within each bucket at build time.
            self.stats.merge_joins += 1
            self.stats.record("SortMergeJoin(co-bucketed)")
            lk_t, rk_t = _join_key_tensors(lbatch, rbatch,
                                           lkeys_names[0], rkeys_names[0])
            lk = ops.sql_key(lk_t)
            rk = ops.sql_key(rk_t)
            lidx, ridx = ops.merge_join(lk, rk, lseg, rseg)
        else:
            # on-the-fly sort-merge join: shuffle-equivalent (counts as an
            # Exchange in plan-diff tests)
            self.stats.shuffles += 2
            self.stats.hash_joins += 1
            self.stats.record("SortMergeJoin(shuffled)")
            lk_t, rk_t = _join_key_tensors(lbatch, rbatch,
                                           lkeys_names[0], rkeys_names[0])
            lk = ops.sql_key(lk_t)
            rk = ops.sql_key(rk_t)
            lperm = ops.sort_perm(lk)
            rperm = ops.sort_perm(rk)
            lbatch = lbatch.gather(lperm)
            rbatch = rbatch.gather(rperm)
            lk, rk = lk[lperm], rk[rperm]
            one_seg = torch.tensor([0, lk.numel()], dtype=torch.int64)
            one_seg_r = torch.tensor([0, rk.numel()], dtype=torch.int64)
            lidx, ridx = ops.merge_join(lk, rk, one_seg, one_seg_r)

        # secondary key equality check for multi-key joins (null
        # secondary keys never match)
        lidx, ridx = _secondary_key_filter(lbatch, rbatch, pairs, lidx, ridx)
        return _join_columns(lbatch.gather(lidx), rbatch.gather(ridx))

    def _exec_typed_join(self, jt: str, pairs, lbatch: ColumnBatch,
                         lseg: Optional[torch.Tensor], rbatch: ColumnBatch,
                         rseg: Optional[torch.Tensor], both_bucketed: bool
                         ) -> ColumnBatch:
        """Outer, semi and anti joins (``jt`` is the canonical type).

        Same two physical paths as the inner join; the merge-join kernel
        runs in the matching mode.  Null join keys never match: such
        rows leave the kernel's input, and those of a preserved side come
        back as unmatched rows.  A right outer join is the left outer
        join of the swapped sides; a full outer join is left_outer(L, R)
        plus the rows of left_anti(R, L) with null left columns — both
        sides are sorted and co-segmented, so the swap is valid on either
        path."""
        lkey, rkey = pairs[0]
        lbatch, lseg, lnull = _split_null_keys(lbatch, lkey, lseg)
        rbatch, rseg, rnull = _split_null_keys(rbatch, rkey, rseg)
        lk_t, rk_t = _join_key_tensors(lbatch, rbatch, lkey, rkey)
        lk = ops.sql_key(lk_t)
        rk = ops.sql_key(rk_t)
        if (both_bucketed and lseg is not None and rseg is not None
                and lseg.numel() == rseg.numel()):
            self.stats.merge_joins += 1
            self.stats.record(f"SortMergeJoin(co-bucketed, {jt})")
        else:
            self.stats.shuffles += 2
            self.stats.hash_joins += 1
            self.stats.record(f"SortMergeJoin(shuffled, {jt})")
            if lk.numel():
                lperm = ops.sort_perm(lk)
                lbatch, lk = lbatch.gather(lperm), lk[lperm]
            if rk.numel():
                rperm = ops.sort_perm(rk)
                rbatch, rk = rbatch.gather(rperm), rk[rperm]
            lseg = torch.tensor([0, lk.numel()], dtype=torch.int64)
            rseg = torch.tensor([0, rk.numel()], dtype=torch.int64)
        rpairs = [(r, l) for l, r in pairs]

        def from_left(mode):
            return _typed_match(mode, lk, rk, lseg, rseg, lbatch, rbatch,
                                pairs)

        def from_right(mode):
            return _typed_match(mode, rk, lk, rseg, lseg, rbatch, lbatch,
                                rpairs)

        if jt == "left_semi":
            return lbatch.gather(from_left("left_semi")[0])
        if jt == "left_anti":
            out = lbatch.gather(from_left("left_anti")[0])
            return out if lnull is None else ColumnBatch.concat([out, lnull])

        # (left part, right part) row-aligned pieces of the result
        pieces: List[Tuple[ColumnBatch, ColumnBatch]] = []
        if jt in ("left_outer", "full_outer"):
            lidx, ridx = from_left("left_outer")
            pieces.append((lbatch.gather(lidx),
                           _gather_nullable(rbatch, ridx)))
            if lnull is not None:
                pieces.append((lnull, _null_batch(rbatch, lnull.num_rows)))
            if jt == "full_outer":
                ranti = from_right("left_anti")[0]
                pieces.append((_null_batch(lbatch, ranti.numel()),
                               rbatch.gather(ranti)))
        else:  # right_outer
            ridx, lidx = from_right("left_outer")
            pieces.append((_gather_nullable(lbatch, lidx),
                           rbatch.gather(ridx)))
        if jt in ("right_outer", "full_outer") and rnull is not None:
            pieces.append((_null_batch(lbatch, rnull.num_rows), rnull))
        if len(pieces) == 1:
            return _join_columns(*pieces[0])
        return _join_columns(ColumnBatch.concat([p[0] for p in pieces]),
                             ColumnBatch.concat([p[1] for p in pieces]))

    # ------------------------------------------------------------------
    def _exec_aggregate(self, plan: Aggregate) -> ColumnBatch:
        """Group-by as a reduce over adjacent runs (K13).

        Grouped path: the child is bucketed on the single grouping
        column, so every group sits in one bucket with its rows adjacent
        (filters and projections keep row order) — no sort, no
        repartition.  Multi-file buckets are re-sorted on the stored
        placeholder of null rows, so null keys are split off and reduced
        as one group of their own.  Sort path (everything else): sort by
        the grouping columns first, which counts as a shuffle.  A global
        aggregate is one run and needs neither."""
        batch, _ = self._exec(plan.child)
        keys = plan.group_cols
        for k in keys:
            col = batch.column(k)
            if not isinstance(col, StringColumn) and \
                    col.dtype.is_floating_point:
                raise HyperspaceException(
                    f"Grouping on float column {k!r} is not supported: "
                    "-0.0 / +0.0 and NaN need SQL equality rules the "
                    "adjacent-run grouping does not apply yet")
        op = aggregate_operator_name(plan)
        self.stats.sort_aggregates += 1
        self.stats.record(op)
        if not keys:
            return _reduce_runs(batch, [], plan.aggs, global_group=True)
        if op == "SortAggregate(bucketed)":
            if batch.has_nulls(keys[0]):
                rest, _, nulls = _split_null_keys(batch, keys[0], None)
                return ColumnBatch.concat([
                    _reduce_runs(rest, keys, plan.aggs),
                    _reduce_runs(nulls, keys, plan.aggs, one_group=True)])
            return _reduce_runs(batch, keys, plan.aggs)
        self.stats.shuffles += 1
        if batch.num_rows:
            from ..index.covering.index import _multi_key_sort_perm
            # null rows sort on (null flag, key): blank their stored
            # values so equal key tuples end up adjacent
            sort_batch = batch.select(keys)
            for k in keys:
                m = batch.mask(k)
                if m is not None and not bool(m.all()):
                    t = sort_batch.tensor(k)
                    t = torch.where(m, t, torch.zeros((), dtype=t.dtype,
                                                      device=t.device))
                    c = sort_batch.column(k)
                    sort_batch = sort_batch.with_column(
                        sort_batch._stored_key(k),
                        StringColumn(t, c.values)
                        if isinstance(c, StringColumn) else t, m)
            batch = batch.gather(_multi_key_sort_perm(sort_batch, keys))
        return _reduce_runs(batch, keys, plan.aggs)

    # ------------------------------------------------------------------
    def _refuse_distributed_order(self, what: str):
        from ..parallel import dist_context as dc
        if dc.is_distributed() and dc.get_world_size() > 1:
            raise HyperspaceException(
                f"{what} is not supported in a distributed session: every "
                "rank holds a partition of the rows, and a per-rank order "
                "is not a global one")

    def _exec_sort(self, plan: Sort) -> ColumnBatch:
        """Full ORDER BY: gather by the stable multi-column permutation."""
        from .ordering import order_perm
        self._refuse_distributed_order("ORDER BY")
        batch, _ = self._exec(plan.child)
        self.stats.record("Sort")
        self.stats.sorts += 1
        if batch.num_rows > 1:
            batch = batch.gather(order_perm(batch, plan.orders))
        return batch

    def _exec_limit(self, plan: Limit) -> ColumnBatch:
        """LIMIT n: the child's first n rows; over a Sort (directly or
        through one Project) a top-k that never sorts the whole input.

        TopK(bucketed): one order column, and the child is bucketed and
        sorted on it (no nulls in it): the first (last) n rows of every
        bucket are the candidates.  TopK(select): everything else, by
        radix select on the leading order column.  Both sort only their
        candidates."""
        from . import ordering
        self._refuse_distributed_order("LIMIT")
        sort, project = _limit_sort_shape(plan)
        n = plan.n
        if sort is None:
            batch, _ = self._exec(plan.child)
            self.stats.record("Limit")
            return batch.slice(0, min(n, batch.num_rows))
        batch, seg = self._exec(sort.child)
        op = topk_operator_name(plan)
        if op == "TopK(bucketed)" and (
                seg is None or batch.has_nulls(sort.orders[0].column)):
            # multi-file buckets re-sort on the stored placeholder of null
            # rows: nulls are not reliably first there
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
        from ..index.covering.index import sort_by_bucket_and_keys
        from ..ops.string_hash import bucket_hash_keys
        keys = bucket_hash_keys(batch, bucket_cols)
        key_masks = [batch.mask(c) for c in bucket_cols]
        bucket_ids = ops.murmur3_bucket(
            keys, num_buckets,
            key_masks if any(m is not None for m in key_masks) else None)
        return sort_by_bucket_and_keys(batch, bucket_ids, bucket_cols,
                                       num_buckets)


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------

_SPARK_DTYPES = {"long": torch.int64, "integer": torch.int32,
                 "short": torch.int16, "byte": torch.int8,
                 "date": torch.int32,  # days; hashes as int, like Spark
                 "double": torch.float64, "float": torch.float32}


def _join_key_tensors(lbatch: ColumnBatch, rbatch: ColumnBatch,
                      ln: str, rn: str
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Comparable key tensors for one join-key pair.

    String keys from independent indexes carry independent dictionaries,
    so both sides remap onto their merged sorted dictionary.  The remap
    is monotone (sorted dict -> code order == lexicographic order), so
    per-bucket sortedness from the build survives and the merge join
    stays valid (reference joins strings via Spark's UTF8String
    comparisons; here the dictionary merge happens once per join and the
    remap is a device gather)."""
    lcol = lbatch.column(ln)
    rcol = rbatch.column(rn)
    lstr = isinstance(lcol, StringColumn)
    rstr = isinstance(rcol, StringColumn)
    if lstr != rstr:
        raise HyperspaceException(
            f"join key type mismatch: {ln} vs {rn}")
    if not lstr:
        lt, rt = lbatch.tensor(ln), rbatch.tensor(rn)
        if lt.dtype.is_floating_point != rt.dtype.is_floating_point:
            # the u64 keys of an integer and of a float are unrelated:
            # comparing them would silently match nothing
            raise HyperspaceException(
                f"join key type mismatch: {ln} ({lt.dtype}) vs {rn} "
                f"({rt.dtype}): an integer key does not join a float "
                "key, store both sides as one type")
        return lt, rt
    merged = sorted(set(lcol.values) | set(rcol.values))
    vi = {v: i for i, v in enumerate(merged)}
    llut = torch.tensor([vi[v] for v in lcol.values], dtype=torch.int64,
                        device=lcol.codes.device)
    rlut = torch.tensor([vi[v] for v in rcol.values], dtype=torch.int64,
                        device=rcol.codes.device)
    lk = llut[lcol.codes.long()] if len(lcol.values) else \
        lcol.codes.long()
    rk = rlut[rcol.codes.long()] if len(rcol.values) else \
        rcol.codes.long()
    return lk, rk


def _drop_null_keys(batch: ColumnBatch, key_name: str,
                    seg: Optional[torch.Tensor]
                    ) -> Tuple[ColumnBatch, Optional[torch.Tensor]]:
    """Remove rows whose join key is null (inner-join semantics).

    When per-bucket segment offsets accompany the batch, they stay valid
    because every bucketed layout in the engine sorts NULLS FIRST within
    each bucket: each offset shifts down by the number of nulls before
    it."""
    if not batch.has_nulls(key_name):
        return batch, seg
    m = batch.mask(key_name)
    keep = torch.nonzero(m, as_tuple=False).flatten()
    if seg is not None:
        nullcum = torch.cat([
            torch.zeros(1, dtype=torch.int64, device=m.device),
            torch.cumsum((~m).to(torch.int64), 0)])
        seg = (seg.to(m.device) - nullcum[seg.to(m.device)]).cpu()
    return batch.gather(keep), seg


def _split_null_keys(batch: ColumnBatch, key_name: str,
                     seg: Optional[torch.Tensor]
                     ) -> Tuple[ColumnBatch, Optional[torch.Tensor],
                                Optional[ColumnBatch]]:
    """``_drop_null_keys`` that also returns the null-key rows (None when
    there are none) so an outer or anti join can keep them as unmatched."""
    if not batch.has_nulls(key_name):
        return batch, seg, None
    nulls = batch.gather(torch.nonzero(
        ~batch.mask(key_name), as_tuple=False).flatten())
    kept, seg = _drop_null_keys(batch, key_name, seg)
    return kept, seg, nulls


def _secondary_key_filter(lbatch: ColumnBatch, rbatch: ColumnBatch, pairs,
                          lidx: torch.Tensor, ridx: torch.Tensor
                          ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Secondary key equality check for multi-key joins over the
    primary-key pairs (null secondary keys never match)."""
    if len(pairs) > 1 and lidx.numel():
        keep = torch.ones(lidx.numel(), dtype=torch.bool,
                          device=lidx.device)
        for ln, rn in pairs[1:]:
            lv_t, rv_t = _join_key_tensors(lbatch, rbatch, ln, rn)
            lv, rv = lv_t[lidx], rv_t[ridx]
            if lv.dtype.is_floating_point or lv.dtype != rv.dtype:
                # SQL equality (-0.0 = 0.0, NaN = NaN), widths promoted
                lv, rv = ops.sql_key(lv), ops.sql_key(rv)
            keep &= (lv == rv)
            lm, rm = lbatch.mask(ln), rbatch.mask(rn)
            if lm is not None:
                keep &= lm[lidx]
            if rm is not None:
                keep &= rm[ridx]
        sel = torch.nonzero(keep, as_tuple=False).flatten()
        lidx, ridx = lidx[sel], ridx[sel]
    return lidx, ridx


def _typed_match(mode: str, lk: torch.Tensor, rk: torch.Tensor,
                 lseg: torch.Tensor, rseg: torch.Tensor,
                 lbatch: ColumnBatch, rbatch: ColumnBatch, pairs
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lidx, ridx) of a left_outer / left_semi / left_anti match.

    A single-key join is one fused kernel pass in that mode.  With
    secondary keys the kernel cannot see that all of a row's primary
    matches fail the secondary check, so the inner pairs are filtered
    first and the result is derived from the surviving left rows (order
    within the result is then matched rows first; none is promised)."""
    if len(pairs) == 1:
        return ops.merge_join(lk, rk, lseg, rseg, mode)
    lidx, ridx = ops.merge_join(lk, rk, lseg, rseg)
    lidx, ridx = _secondary_key_filter(lbatch, rbatch, pairs, lidx, ridx)
    matched = torch.zeros(lbatch.num_rows, dtype=torch.bool,
                          device=lk.device)
    matched[lidx] = True
    none = torch.empty(0, dtype=torch.int64, device=lk.device)
    if mode == "left_semi":
        return torch.nonzero(matched, as_tuple=False).flatten(), none
    unmatched = torch.nonzero(~matched, as_tuple=False).flatten()
    if mode == "left_anti":
        return unmatched, none
    return (torch.cat([lidx, unmatched]),
            torch.cat([ridx, torch.full_like(unmatched, -1)]))


def _bucketed_group_source(plan: LogicalPlan, key: str) -> bool:
    """True if the subplan, walked down through Project and Filter nodes
    (both keep row order), is a bucketed covering IndexScan whose single
    indexed column is ``key``, or a BucketUnion on exactly that column:
    every group then lies inside one bucket with its rows adjacent."""
    node = plan
    while isinstance(node, (Project, Filter)):
        node = node.child
    if isinstance(node, IndexScan):
        index = node.entry.derivedDataset
        return (node.use_bucket_spec and index.kind == "CoveringIndex" and
                [c.lower() for c in index.indexed_columns] == [key.lower()])
    if isinstance(node, BucketUnionNode):
        return [c.lower() for c in node.bucket_columns] == [key.lower()]
    return False


def aggregate_operator_name(plan: Aggregate) -> str:
    """Physical operator an Aggregate node runs as."""
    if not plan.group_cols:
        return "SortAggregate(global)"
    if len(plan.group_cols) == 1 and \
            _bucketed_group_source(plan.child, plan.group_cols[0]):
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


def _bucketed_order_source(plan: LogicalPlan, key: str) -> bool:
    """Like _bucketed_group_source, walked down through Project only: a
    Filter drops the segment offsets, which the bucket heads come from."""
    node = plan
    while isinstance(node, Project):
        node = node.child
    return not isinstance(node, Filter) and _bucketed_group_source(node, key)


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
            _bucketed_order_source(sort.child, sort.orders[0].column):
        return "TopK(bucketed)"
    return "TopK(select)"


_REDUCE_OUTPUTS = {"sum": ("sum", "count"), "avg": ("sum", "count"),
                   "min": ("min", "count"), "max": ("max", "count"),
                   "count": ("count",)}


def _reduce_runs(batch: ColumnBatch, keys: List[str], aggs,
                 one_group: bool = False, global_group: bool = False
                 ) -> ColumnBatch:
    """Aggregate runs of adjacent equal ``keys`` rows: group offsets from
    adjacency, then one fused segmented reduce per input column.
    ``one_group``: all rows are one group (the null-key rows);
    ``global_group``: likewise, and an empty input still gives one row."""
    n = batch.num_rows
    dev = batch.device
    if global_group or one_group:
        n_groups = 1 if (n or global_group) else 0
        offsets = torch.tensor([0, n] if n_groups else [0],
                               dtype=torch.int64, device=dev)
    elif n == 0:
        offsets = torch.zeros(1, dtype=torch.int64, device=dev)
    else:
        masks = [batch.mask(k) for k in keys]
        offsets = ops.group_offsets(
            [ops.normalize_key(batch.tensor(k)) for k in keys],
            masks if any(m is not None for m in masks) else None)
    n_groups = offsets.numel() - 1
    first = offsets[:-1]
    cols: Dict[str, object] = {}
    masks_out: Dict[str, torch.Tensor] = {}
    for k in keys:
        name = batch._stored_key(k)
        c = batch.column(k)
        cols[name] = c.gather(first) if isinstance(c, StringColumn) \
            else ops.gather_rows(c, first)
        m = batch.mask(k)
        if m is not None:
            masks_out[name] = m[first]

    # one fused reduce per input column, for everything asked of it
    wanted: Dict[str, set] = {}
    for a in aggs:
        if a.column is not None:
            wanted.setdefault(a.column.lower(), set()).update(
                _REDUCE_OUTPUTS[a.func])
    reduced: Dict[str, dict] = {}
    for cname, outs in wanted.items():
        c = batch.column(cname)
        if isinstance(c, StringColumn) and outs & {"sum"}:
            raise HyperspaceException(
                f"sum/avg over string column {cname!r} is not supported")
        want = tuple(o for o in ("sum", "min", "max", "count") if o in outs)
        if n == 0:
            # nothing to read: counts are 0, everything else null
            t = batch.tensor(cname)
            sum_dt = torch.float64 if t.dtype.is_floating_point \
                else torch.int64
            reduced[cname] = {
                o: torch.zeros(n_groups, device=dev, dtype=(
                    sum_dt if o == "sum" else
                    torch.int64 if o == "count" else t.dtype))
                for o in want}
        else:
            reduced[cname] = ops.segmented_reduce(
                batch.tensor(cname), batch.mask(cname), offsets, want)
    for a in aggs:
        name = a.output_name
        if a.column is None:
            cols[name] = offsets[1:] - offsets[:-1]
            continue
        c = batch.column(a.column)
        r = reduced[a.column.lower()]
        cnt = r["count"]
        if a.func == "count":
            cols[name] = cnt
            continue
        if a.func == "sum":
            out = r["sum"]
        elif a.func == "avg":
            out = r["sum"].to(torch.float64) / cnt.to(torch.float64)
        else:
            t = c.codes if isinstance(c, StringColumn) else c
            out = r[a.func].to(t.dtype)
            if isinstance(c, StringColumn):
                out = StringColumn(out, c.values if len(c.values) else [""])
        cols[name] = out
        if batch.mask(a.column) is not None or n == 0:
            masks_out[name] = cnt > 0
    return ColumnBatch(cols, masks_out)


def _null_batch(like: ColumnBatch, n: int) -> ColumnBatch:
    """``n`` all-null rows with the columns and dtypes of ``like``.  The
    value slots hold the fill a null carries elsewhere (0 / the first
    dictionary entry, "" for an empty dictionary)."""
    dev = like.device
    cols: Dict[str, object] = {}
    for k, v in like.columns.items():
        if isinstance(v, StringColumn):
            cols[k] = StringColumn(
                torch.zeros(n, dtype=torch.int32, device=dev),
                v.values if len(v.values) else [""])
        else:
            cols[k] = torch.zeros(n, dtype=v.dtype, device=dev)
    return ColumnBatch(cols, {k: torch.zeros(n, dtype=torch.bool, device=dev)
                              for k in cols})


def _gather_nullable(batch: ColumnBatch, idx: torch.Tensor) -> ColumnBatch:
    """Gather where ``idx == -1`` yields an all-null row.  The -1 never
    reaches the gather: it is clamped to row 0 and masked out; a batch
    with no rows to clamp to is built as nulls directly."""
    if batch.num_rows == 0:
        return _null_batch(batch, idx.numel())
    out = batch.gather(idx.clamp_min(0))
    valid = idx >= 0
    masks = {}
    for k in out.columns:
        m = out.mask(k)
        masks[k] = valid if m is None else (valid & m)
    return ColumnBatch(out.columns, masks)


def _join_columns(lout: ColumnBatch, rout: ColumnBatch) -> ColumnBatch:
    """Left then right columns; a right name already taken gets ``_r``."""
    cols: Dict[str, object] = {}
    masks: Dict[str, torch.Tensor] = {}
    for k, v in lout.columns.items():
        cols[k] = v
        if lout.mask(k) is not None:
            masks[k] = lout.mask(k)
    for k, v in rout.columns.items():
        name = k if k not in cols else f"{k}_r"
        cols[name] = v
        if rout.mask(k) is not None:
            masks[name] = rout.mask(k)
    return ColumnBatch(cols, masks)


def _empty_batch(schema) -> ColumnBatch:
    """Zero-row batch carrying the relation's column structure (empty
    shards in a distributed scan must keep the schema)."""
    cols: Dict[str, object] = {}
    for f in schema.fields:
        if f.type == "string":
            cols[f.name] = StringColumn(
                torch.empty(0, dtype=torch.int32), [])
        else:
            dt = _SPARK_DTYPES.get(f.type, torch.int64)
            cols[f.name] = torch.empty(0, dtype=dt)
    return ColumnBatch(cols)


def _eval_arith(batch: ColumnBatch, e) -> torch.Tensor:
    """Evaluate a scalar arithmetic expression per row (Arith trees over
    Col/Lit; '%' uses Java/Spark remainder = fmod)."""
    from ..plan.expr import Arith
    if isinstance(e, Col):
        col = batch.column(e.name)
        if isinstance(col, StringColumn):
            raise HyperspaceException(
                "arithmetic over string columns is not supported")
        return col
    if isinstance(e, Lit):
        return e.value
    if isinstance(e, Arith):
        lv = _eval_arith(batch, e.left)
        rv = _eval_arith(batch, e.right)
        if e.op == "+":
            return lv + rv
        if e.op == "-":
            return lv - rv
        if e.op == "*":
            return lv * rv
        if e.op == "%":
            return torch.fmod(lv, rv)
        lt = lv.to(torch.float64) if torch.is_tensor(lv) else lv
        return lt / rv
    raise HyperspaceException(f"Cannot evaluate expression {e!r}")


def _compare(batch: ColumnBatch, e: BinComp) -> torch.Tensor:
    """General comparison mask (non-hot path; hot single comparisons lower
    to select_range_u64 in _predicate_indices)."""
    from ..plan.expr import Arith
    if isinstance(e.left, Arith):
        lv = _eval_arith(batch, e.left)
        rv = (_eval_arith(batch, e.right)
              if not isinstance(e.right, Lit) else e.right.value)
        if torch.is_tensor(lv) and isinstance(e.right, Lit) and \
                sql_compare.supported(lv.dtype, rv):
            return sql_compare.literal_mask(lv, e.op, rv)
        return {"=": lv == rv, "!=": lv != rv, "<": lv < rv,
                "<=": lv <= rv, ">": lv > rv, ">=": lv >= rv}[e.op]
    if not isinstance(e.left, Col):
        raise HyperspaceException(f"Unsupported comparison {e!r}")
    col = batch.column(e.left.name)
    if isinstance(e.right, Col):
        rhs = batch.column(e.right.name)
        lv = col.codes if isinstance(col, StringColumn) else col
        rv = rhs.codes if isinstance(rhs, StringColumn) else rhs
    else:
        value = e.right.value
        if isinstance(col, StringColumn):
            # dictionary is sorted, so code order == lexicographic order;
            # an absent literal maps to its insertion point.
            codes = col.codes
            pos = col.searchsorted(str(value))
            exact = (pos < len(col.values) and col.values[pos] == str(value))
            op = e.op
            if op == "=":
                return (codes == pos if exact else
                        torch.zeros(len(col), dtype=torch.bool,
                                    device=codes.device))
            if op == "!=":
                return (codes != pos if exact else
                        torch.ones(len(col), dtype=torch.bool,
                                   device=codes.device))
            if op == "<":
                return codes < pos
            if op == "<=":
                return codes < pos + (1 if exact else 0)
            if op == ">":
                return codes >= pos + (1 if exact else 0)
            return codes >= pos  # >=
        elif sql_compare.supported(col.dtype, value):
            return sql_compare.literal_mask(col, e.op, value)
        else:
            lv = col
            rv = torch.tensor(value, dtype=col.dtype, device=col.device)
    op = e.op
    if op == "=":
        return lv == rv
    if op == "!=":
        return lv != rv
    if op == "<":
        return lv < rv
    if op == "<=":
        return lv <= rv
    if op == ">":
        return lv > rv
    return lv >= rv


def _value_tensor(spark_type: Optional[str], value
                  ) -> Optional[torch.Tensor]:
    """The literal as a one-element tensor of the column's type, for
    hashing to its bucket; None when no value of that type equals it."""
    dt = _SPARK_DTYPES.get(spark_type or "", None)
    if dt is None:
        dt = torch.int64 if isinstance(value, int) else torch.float64
    if sql_compare.supported(dt, value):
        return sql_compare.equality_probe(dt, value)
    return torch.tensor([value], dtype=dt)


def _in_mask(t: torch.Tensor, values) -> torch.Tensor:
    """``t IN (values)`` for a numeric tensor: the OR of SQL ``=``."""
    if all(sql_compare.supported(t.dtype, v) for v in values):
        return sql_compare.in_mask(t, values)
    vs = torch.tensor(sorted(int(v) for v in values), dtype=torch.int64,
                      device=t.device)
    return ops.isin_sorted(t.to(torch.int64), vs)


def _same_hash_kind(lcol, rcol) -> bool:
    """True if SQL-equal values of the two key columns hash to the same
    bucket: murmur3 folds 64-bit integers, narrower integers, doubles
    and floats each their own way."""
    def kind(c):
        if isinstance(c, StringColumn):
            return "string"
        if c.dtype.is_floating_point or c.dtype == torch.int64:
            return c.dtype
        return torch.int32
    return kind(lcol) == kind(rcol)


def _single_equality(cond: Expr) -> Optional[Tuple[str, object]]:
    if isinstance(cond, BinComp) and cond.op == "=" and \
            isinstance(cond.left, Col) and isinstance(cond.right, Lit):
        return cond.left.name, cond.right.value
    return None


def _as_range(cond: Expr, batch: ColumnBatch):
    """Lower a single numeric comparison to the select_range_u64 kernel:
    returns (column, lo, hi) — closed u64 bounds over ``ops.sql_key`` of
    the column, both None when nothing can match — or None when the
    comparison takes the mask path."""
    if not (isinstance(cond, BinComp) and isinstance(cond.left, Col)
            and isinstance(cond.right, Lit)):
        return None
    col = batch.column(cond.left.name)
    if isinstance(col, StringColumn):
        return None
    value = cond.right.value
    if not sql_compare.supported(col.dtype, value):
        return None
    spec = sql_compare.lower(col.dtype, cond.op, value)
    if spec is sql_compare.NONE:
        return col, None, None
    if spec is sql_compare.ALL:
        spec = ("range", sql_compare.S_MIN, sql_compare.S_MAX)
    if spec[0] != "range":
        return None
    # s-space -> the int64-encoded u64 the kernel compares
    return col, spec[1] ^ sql_compare.SIGN, spec[2] ^ sql_compare.SIGN


def _bucketed_side(plan: LogicalPlan, key_names: List[str]) -> bool:
    """True if the subplan yields bucket-partitioned data keyed on
    key_names (IndexScan/BucketUnion with matching indexed columns)."""
    node: LogicalPlan = plan
    while isinstance(node, Project):
        node = node.child
    if isinstance(node, IndexScan):
        idx_cols = [c.lower() for c in node.entry.derivedDataset
                    .indexed_columns]
        return node.use_bucket_spec and \
            idx_cols == [k.lower() for k in key_names]
    if isinstance(node, BucketUnionNode):
        return [c.lower() for c in node.bucket_columns] == \
            [k.lower() for k in key_names]
    return False
