"""CoveringIndex: bucketed + sorted vertical slice of the source.

The flagship index kind (reference: index/covering/CoveringIndex.scala,
CoveringIndexTrait.scala).  Index data = indexed + included columns
[+ lineage column], hash-repartitioned into ``numBuckets`` by Spark-
compatible Murmur3 of the indexed columns, sorted by the indexed columns
within each bucket, stored as uncompressed PLAIN Parquet with the
bucket-id-in-filename contract.

The build pipeline is the device data plane: murmur3 bucketize (K2),
stable radix sort by (bucket, indexed cols) (K3), segmented write.  With
torch.distributed initialized, buckets are exchanged across GPUs via RCCL
all-to-all before the sort (C1, parallel/exchange.py).
"""

from __future__ import annotations

import contextlib
import os
from typing import Any, Dict, List, Optional, Tuple

import torch

from ..base import Index, IndexerContext
from ...config import IndexConstants
from ...exceptions import HyperspaceException
from ...log.entry import (Schema, register_derived_dataset,
                          COVERING_INDEX_TYPE)
from ... import ops
from ...execution.columnar import ColumnBatch, StringColumn
from ...sources.parquet_io import (bucket_file_name, write_batch_parquet,
                                   read_files_batch, bucket_id_of_file)


class CoveringIndex(Index):
    def __init__(self, indexed_columns: List[str],
                 included_columns: List[str], schema: Schema,
                 num_buckets: int, properties: Dict[str, str]):
        self.indexed_columns = list(indexed_columns)
        self.included_columns = list(included_columns)
        self.schema = schema
        self.num_buckets = num_buckets
        self._properties = dict(properties)

    # -- identity ---------------------------------------------------------
    @property
    def kind(self) -> str:
        return "CoveringIndex"

    @property
    def kind_abbr(self) -> str:
        return "CI"

    def indexed_columns_list(self) -> List[str]:
        return list(self.indexed_columns)

    def referenced_columns(self) -> List[str]:
        return self.indexed_columns + self.included_columns

    @property
    def can_handle_deleted_files(self) -> bool:
        return (self._properties.get(IndexConstants.LINEAGE_PROPERTY, "false")
                .lower() == "true")

    @property
    def has_lineage(self) -> bool:
        return self.can_handle_deleted_files

    def with_new_properties(self, props: Dict[str, str]) -> "CoveringIndex":
        return CoveringIndex(self.indexed_columns, self.included_columns,
                             self.schema, self.num_buckets, props)

    # -- json (wire-compatible with the reference) -------------------------
    def to_json(self) -> Dict[str, Any]:
        return {
            "type": COVERING_INDEX_TYPE,
            "indexedColumns": self.indexed_columns,
            "includedColumns": self.included_columns,
            "schema": self.schema.to_json(),
            "numBuckets": self.num_buckets,
            "properties": self._properties,
        }

    @staticmethod
    def from_json(d: Dict[str, Any]) -> "CoveringIndex":
        return CoveringIndex(
            d["indexedColumns"], d["includedColumns"],
            Schema.from_json(d["schema"]), d["numBuckets"],
            d.get("properties", {}))

    # -- build data plane ---------------------------------------------------
    def write(self, ctx: IndexerContext, index_data) -> List[str]:
        """Bucketize + per-bucket sort + bucketed parquet write (K2+K3).

        ``index_data`` is a ColumnBatch or a ScanStream.  Streams are
        processed group by group — read/decode of group g+1 prefetches
        while g bucketizes/sorts and g-1's files flush on write threads —
        bounding memory to O(group) and overlapping disk, PCIe and
        kernels (out-of-core builds of sources larger than HBM).

        With torch.distributed initialized this is the multi-GPU build:
        each rank holds a source shard; bucket rows are exchanged via
        RCCL all-to-all over xGMI so rank r owns buckets
        {b : b % world == r}.
        """
        from ...execution.scan_stream import ScanStream
        os.makedirs(ctx.index_data_path, exist_ok=True)

        import torch.distributed as dist
        distributed = dist.is_available() and dist.is_initialized() and \
            dist.get_world_size() > 1
        task_id = dist.get_rank() if distributed else 0

        if isinstance(index_data, ScanStream):
            batches = index_data.batches()
            n_groups = len(index_data.file_groups())
        else:
            batches = iter([index_data])
            n_groups = 1

        # collective iteration count: every rank must join every
        # all-to-all, so ranks with fewer groups contribute empty batches
        if distributed:
            from ...parallel import dist_context as dc
            t = dc.collective_tensor([n_groups])
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            n_groups = int(t[0])
            written = self._write_distributed(ctx, batches, n_groups,
                                              task_id)
        else:
            written = []
            for g in range(n_groups):
                try:
                    batch = next(batches)
                except StopIteration:
                    batch = self._empty_batch(ctx)
                written.extend(self._write_group(ctx, batch, task_id))
        if n_groups > 1:
            # multi-group (out-of-core) builds: the per-group batches
            # are partial slices of each bucket — not cacheable as-is
            ctx.built_for_cache = None
        return written

    def _bucket_ids(self, batch: ColumnBatch) -> torch.Tensor:
        from ...ops.string_hash import bucket_hash_keys
        keys = bucket_hash_keys(batch, self.indexed_columns)
        key_masks = [batch.mask(c) for c in self.indexed_columns]
        return ops.murmur3_bucket(
            keys, self.num_buckets,
            key_masks if any(m is not None for m in key_masks) else None)

    def _write_distributed(self, ctx, batches, n_groups: int,
                           task_id: int) -> List[str]:
        """Pipelined multi-GPU build: each group is split into chunks;
        chunk k+1's hash/pack and the previous group's sort/write overlap
        chunk k's RCCL all-to-all in flight on the xGMI links
        (SURVEY §7 hard part b; C1)."""
        import torch.distributed as dist
        from ...parallel import dist_context as dc
        from ...parallel.exchange import BucketExchange
        n = self.num_buckets
        ex = BucketExchange(n)
        ctx.exchange_stats = ex
        chunk_bytes = int(ctx.session.conf.get(
            "spark.hyperspace.exchange.chunkBytes", 1 << 30))
        written: List[str] = []
        recv_acc: Dict[int, list] = {}

        def flush_group(g: int) -> None:
            parts = recv_acc.pop(g, [])
            parts = [(b, k) for b, k in parts if b.num_rows]
            if not parts:
                return
            if len(parts) == 1:
                rb, rbk = parts[0]
            else:
                rb = ColumnBatch.concat([p[0] for p in parts])
                rbk = torch.cat([p[1] for p in parts])
            batch, seg = sort_by_bucket_and_keys(
                rb, rbk, self.indexed_columns, n)
            out = write_bucketed(batch, seg, ctx.index_data_path, n,
                                 task_id)
            ctx.built_for_cache = (batch, seg, list(out))
            written.extend(out)

        prev = None  # (pending, group, last-chunk-of-group)
        for g in range(n_groups):
            try:
                batch = next(batches)
            except StopIteration:
                batch = self._empty_batch(ctx)
            # every rank must post the same number of chunk exchanges:
            # agree on max chunk count, short ranks send empty chunks
            local_chunks = 1
            if chunk_bytes > 0 and batch.num_rows:
                local_chunks = max(
                    1, -(-batch.nbytes() // chunk_bytes))
            t = dc.collective_tensor([local_chunks])
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            nchunks = int(t[0])
            rows = batch.num_rows
            for c in range(nchunks):
                lo = rows * c // nchunks
                hi = rows * (c + 1) // nchunks
                sub = batch.slice(lo, hi) if nchunks > 1 else batch
                pend = ex.start(sub, self._bucket_ids(sub))
                if prev is not None:
                    p, pg, plast = prev
                    recv_acc.setdefault(pg, []).append(ex.finish(p))
                    if plast:
                        flush_group(pg)
                prev = (pend, g, c == nchunks - 1)
        if prev is not None:
            p, pg, _ = prev
            recv_acc.setdefault(pg, []).append(ex.finish(p))
            flush_group(pg)
        return written

    def _write_group(self, ctx, batch: ColumnBatch,
                     task_id: int) -> List[str]:
        import time as _time
        timing = os.environ.get("HS_TIMING")
        n = self.num_buckets
        t0 = _time.perf_counter()
        bucket_ids = self._bucket_ids(batch)
        if batch.num_rows == 0:
            return []
        t1 = _time.perf_counter()

        # Bucket-batch pipelined sort+write, OPT-IN: a same-box A/B
        # (profiles/README round 2) measured it 45% SLOWER than the
        # monolithic sort+write at 8 GiB/200 buckets — the extra
        # partition pass + per-batch sort fixed costs outweigh the
        # write overlap.  Kept behind HS_PIPE_WRITE for re-evaluation
        # at other shapes (more buckets, slower storage).
        pipeline = (batch.device.type == "cuda" and n >= 8
                    and batch.num_rows >= 1 << 22
                    and bool(os.environ.get("HS_PIPE_WRITE")))
        if not pipeline:
            batch, seg = sort_by_bucket_and_keys(
                batch, bucket_ids, self.indexed_columns, n)
            if timing:
                import torch as _torch
                if batch.device.type == "cuda":
                    _torch.cuda.synchronize()
            t2 = _time.perf_counter()
            out = write_bucketed(batch, seg, ctx.index_data_path, n,
                                 task_id)
            # build write-through for the HBM index-data cache: the
            # sorted bucket-major batch + segment offsets ARE the
            # index-scan layout, so the first post-build query serves
            # from residency (288 GB HBM3E; the put happens after the
            # action commits — see IndexManagement)
            ctx.built_for_cache = (batch, seg, list(out))
            if timing:
                import sys as _sys
                print(f"[hs-timing] build group: hash {t1-t0:.3f}s "
                      f"sort {t2-t1:.3f}s write "
                      f"{_time.perf_counter()-t2:.3f}s",
                      file=_sys.stderr)
            return out

        # Pipelined sort+write: one stable bucket-partition pass, then
        # bucket BATCHES key-sort on the GPU while earlier batches'
        # D2H + parquet writes drain on worker threads/streams — the
        # write wall-time (the largest build phase) overlaps the sort
        # instead of following it.
        import torch as _torch
        from concurrent.futures import ThreadPoolExecutor
        b64 = bucket_ids.to(_torch.int64)
        perm = ops.sort_perm(ops.normalize_key(b64))
        batch = batch.gather(perm)
        sorted_b = ops.gather_rows(b64, perm)
        seg = _bucket_seg_offsets(sorted_b, n)
        t2 = _time.perf_counter()

        nb_batches = min(8, n)
        bounds = [round(i * n / nb_batches) for i in range(nb_batches + 1)]
        pool = ThreadPoolExecutor(max_workers=2)
        futures = []
        pieces: List[ColumnBatch] = []
        for i in range(nb_batches):
            b_lo, b_hi = bounds[i], bounds[i + 1]
            r_lo, r_hi = int(seg[b_lo]), int(seg[b_hi])
            if r_hi <= r_lo:
                continue
            sub = batch.slice(r_lo, r_hi)
            sub_sorted, lseg = sort_by_bucket_and_keys(
                sub, sorted_b[r_lo:r_hi], self.indexed_columns, n)
            ev = _torch.cuda.Event()
            ev.record()
            pieces.append(sub_sorted)
            futures.append(pool.submit(
                write_bucketed, sub_sorted, lseg, ctx.index_data_path,
                n, task_id, ev))
        out = []
        for f in futures:
            out.extend(f.result())
        pool.shutdown()
        if timing:
            _torch.cuda.synchronize()
        t3 = _time.perf_counter()
        full = (ColumnBatch.concat(pieces) if len(pieces) > 1
                else pieces[0]) if pieces else batch
        ctx.built_for_cache = (full, seg, list(out))
        if timing:
            import sys as _sys
            print(f"[hs-timing] build group: hash {t1-t0:.3f}s "
                  f"partition {t2-t1:.3f}s sort+write(pipe) "
                  f"{t3-t2:.3f}s", file=_sys.stderr)
        return out

    def _empty_batch(self, ctx) -> ColumnBatch:
        """Zero-row batch matching the index schema — ranks that run out
        of file groups still join every collective with the exact same
        packed layout (string fields must be StringColumns, not i64)."""
        import torch as _torch
        dts = {"long": _torch.int64, "integer": _torch.int32,
               "short": _torch.int16, "byte": _torch.int8,
               "date": _torch.int32,
               "double": _torch.float64, "float": _torch.float32,
               "boolean": _torch.bool}
        cols: Dict[str, Any] = {}
        for f in self.schema.fields:
            if f.type == "string":
                cols[f.name] = StringColumn(
                    _torch.empty(0, dtype=_torch.int32,
                                 device=ctx.session.device), [])
            else:
                cols[f.name] = _torch.empty(
                    0, dtype=dts.get(f.type, _torch.int64),
                    device=ctx.session.device)
        return ColumnBatch(cols)

    def optimize(self, ctx: IndexerContext,
                 files_to_optimize: List[str]) -> List[str]:
        """Per-bucket compaction: merge this bucket's small files into one
        (reference: CoveringIndexTrait.optimize + OptimizeAction —
        files are already bucket-pure, so this is a read + re-sort +
        single-file rewrite per bucket)."""
        os.makedirs(ctx.index_data_path, exist_ok=True)
        by_bucket: Dict[int, List[str]] = {}
        for p in files_to_optimize:
            b = bucket_id_of_file(p)
            if b is None:
                raise HyperspaceException(f"Not a bucketed index file: {p}")
            by_bucket.setdefault(b, []).append(p)
        from concurrent.futures import ThreadPoolExecutor

        def compact_one(item):
            b, paths = item
            sub, _ = read_files_batch(sorted(paths))
            if ctx.session.device.type == "cuda":
                sub = sub.to(ctx.session.device)
            perm = _multi_key_sort_perm(sub, self.indexed_columns)
            sub = sub.gather(perm)
            out = os.path.join(ctx.index_data_path, bucket_file_name(0, b))
            write_batch_parquet(sub.to("cpu") if sub.device.type == "cuda"
                                else sub, out)
            return out

        items = sorted(by_bucket.items())
        if len(items) <= 2:
            return [compact_one(i) for i in items]
        with ThreadPoolExecutor(max_workers=8) as pool:
            return list(pool.map(compact_one, items))

    def refresh_incremental(self, ctx: IndexerContext,
                            appended_batch: Optional[ColumnBatch],
                            deleted_file_ids: List[int],
                            previous_files: List[str]
                            ) -> Tuple[List[str], List[str]]:
        """Index appended data into new files; rewrite old files dropping
        rows whose lineage id is deleted
        (reference: CoveringIndexTrait.scala:57-106).

        Returns (new files written, kept previous files).
        """
        written: List[str] = []
        if appended_batch is not None and appended_batch.num_rows:
            written.extend(self.write(ctx, appended_batch))
        kept = list(previous_files)
        if deleted_file_ids:
            if not self.has_lineage:
                raise HyperspaceException(
                    "Index has no lineage column; cannot handle deletes")
            os.makedirs(ctx.index_data_path, exist_ok=True)
            ids = torch.tensor(sorted(deleted_file_ids), dtype=torch.int64)
            kept = []
            lineage_col = IndexConstants.DATA_FILE_NAME_ID_COLUMN
            for p in previous_files:
                b = bucket_id_of_file(p)
                sub, _ = read_files_batch([p])
                lineage = sub.tensor(lineage_col)
                keep_mask = ~ops.isin_sorted(lineage, ids)
                if bool(keep_mask.all()):
                    kept.append(p)
                    continue
                sub = sub.gather(
                    torch.nonzero(keep_mask, as_tuple=False).flatten())
                if sub.num_rows == 0:
                    # every row of this bucket file came from deleted
                    # sources: the file simply disappears (Spark writes
                    # no empty bucket files either)
                    continue
                out = os.path.join(ctx.index_data_path,
                                   bucket_file_name(1, b or 0))
                write_batch_parquet(sub, out)
                written.append(out)
        return written, kept

    def statistics(self) -> Dict[str, Any]:
        return {"indexedColumns": self.indexed_columns,
                "includedColumns": self.included_columns,
                "numBuckets": self.num_buckets}


# ---------------------------------------------------------------------------
# build helpers (shared with zorder)
# ---------------------------------------------------------------------------

def _multi_key_sort_perm(batch: ColumnBatch, key_cols: List[str]
                         ) -> torch.Tensor:
    """Stable multi-column sort permutation: LSD over columns
    (least-significant column first).  Nullable columns order ASC NULLS
    FIRST (Spark's default): a stable partition moves this column's null
    rows ahead after its key sort, giving (null-flag, key) lexicographic
    order per column.  Float columns sort by their SQL key (-0.0 with
    +0.0, every NaN last): that is the key the merge join compares, so
    a bucket sorted by raw bits would not be sorted for it."""
    n = batch.num_rows
    dev = batch.device
    perm = torch.arange(n, dtype=torch.int64, device=dev)
    for c in reversed(key_cols):
        keys = ops.sql_key(batch.tensor(c))[perm]
        _, perm = ops.sort_pairs(keys, perm)
        m = batch.mask(c)
        if m is not None and not bool(m.all()):
            f = m[perm]
            perm = perm[torch.cat([
                torch.nonzero(~f, as_tuple=False).flatten(),
                torch.nonzero(f, as_tuple=False).flatten()])]
    return perm


def _bucket_seg_offsets(sorted_bkeys_u64: torch.Tensor, num_buckets: int
                        ) -> torch.Tensor:
    """Per-bucket segment offsets (num_buckets+1) of a bucket-sorted
    normalized-or-raw int64 bucket column, via device searchsorted."""
    probes = ops.cpu_ref.normalize_key(
        torch.arange(num_buckets + 1, dtype=torch.int64)).to(
            sorted_bkeys_u64.device)
    if sorted_bkeys_u64.numel() and int(sorted_bkeys_u64.max()) >= 0 \
            and int(sorted_bkeys_u64.min()) >= 0:
        # raw (un-normalized) bucket ids sort in plain int64 order
        seg = torch.searchsorted(
            sorted_bkeys_u64,
            torch.arange(num_buckets + 1, dtype=torch.int64,
                         device=sorted_bkeys_u64.device))
        return seg.cpu()
    sortable = sorted_bkeys_u64 ^ (-0x8000000000000000)
    sortable_probes = probes ^ (-0x8000000000000000)
    return torch.searchsorted(sortable, sortable_probes).cpu()


def _fused_bucket_sort(batch: ColumnBatch, bucket_ids: torch.Tensor,
                       key_cols: List[str], num_buckets: int
                       ) -> Optional[Tuple[ColumnBatch, torch.Tensor]]:
    """The common index shape — one integer key column without nulls, on
    the device — sorted by ops.bucket_sort_perm: one composite sort, the
    key column rebuilt from it and every other column gathered once
    through the int32 permutation.  None = not that shape, the caller
    runs the general path.  HS_FUSED_BUCKET_SORT=0 (read per call) turns
    it off."""
    if len(key_cols) != 1 or os.environ.get("HS_FUSED_BUCKET_SORT") == "0":
        return None
    key_name = batch._stored_key(key_cols[0])
    key = batch.columns[key_name]
    if isinstance(key, StringColumn) or batch.has_nulls(key_name):
        return None
    res = ops.bucket_sort_perm(key, bucket_ids, num_buckets)
    if res is None:
        return None
    perm, sorted_key, seg = res
    cols: Dict[str, Any] = {}
    for k, v in batch.columns.items():
        if k == key_name:
            cols[k] = sorted_key
        elif isinstance(v, StringColumn):
            cols[k] = StringColumn(ops.gather_rows(v.codes, perm), v.values)
        else:
            cols[k] = ops.gather_rows(v, perm)
    return ColumnBatch(
        cols, {k: m[perm] for k, m in batch.masks.items()}), seg


def sort_by_bucket_and_keys(batch: ColumnBatch, bucket_ids: torch.Tensor,
                            key_cols: List[str], num_buckets: int
                            ) -> Tuple[ColumnBatch, torch.Tensor]:
    """Stable sort rows by (bucket, key columns); returns the reordered
    batch and per-bucket segment offsets (num_buckets+1)."""
    fused = _fused_bucket_sort(batch, bucket_ids, key_cols, num_buckets)
    if fused is not None:
        return fused
    perm = _multi_key_sort_perm(batch, key_cols)
    b64 = ops.gather_rows(bucket_ids.to(torch.int64), perm)
    sorted_bkeys, perm2 = ops.sort_pairs(ops.normalize_key(b64), perm)
    batch = batch.gather(perm2)
    # segment offsets via searchsorted on the sorted bucket keys (device
    # side; avoids a full-column D2H)
    probes = ops.cpu_ref.normalize_key(
        torch.arange(num_buckets + 1, dtype=torch.int64)).to(
            sorted_bkeys.device)
    sortable = sorted_bkeys ^ (-0x8000000000000000)
    sortable_probes = probes ^ (-0x8000000000000000)
    seg = torch.searchsorted(sortable, sortable_probes).cpu()
    return batch, seg


_NATIVE_WRITE_DTYPES = (torch.int64, torch.int32, torch.float64,
                        torch.float32)
_WRITE_RING_SLOTS = 64


def _native_write_eligible(batch: ColumnBatch) -> bool:
    """The shape the native writer covers: the extension is loaded, every
    column a non-string int64/int32/float64/float32 tensor, no masks.
    HS_NATIVE_WRITE=0 (read per call) turns it off."""
    if os.environ.get("HS_NATIVE_WRITE") == "0" or batch.masks:
        return False
    if not batch.columns or not ops.native.available():
        return False
    return all(not isinstance(c, StringColumn)
               and c.dtype in _NATIVE_WRITE_DTYPES and c.dim() == 1
               and c.device == batch.device
               for c in batch.columns.values())


def _device_stat_unusable(v) -> bool:
    """The float-statistics rule.  The device reduce orders floats by
    normalize_key (-NaN < -inf < -0.0 < +0.0 < +inf < +NaN), numpy's
    min/max propagate NaN and pick between -0.0 and +0.0 by element order.
    A NaN anywhere in a bucket, or a zero at either end of its range,
    shows up as a NaN or a zero in the device min or max: such a (bucket,
    column) pair takes its statistics from numpy on the host instead, so
    the footer bytes stay those of write_parquet_native."""
    return v != v or v == 0


def _bucket_statistics(batch: ColumnBatch, jobs) -> Tuple[list, list]:
    """PLAIN-encoded (min, max) of every (file, column), file-major.
    Device batches: one segmented_reduce and one small D2H per column."""
    from ...sources.native_parquet import _statistics
    ncols = len(batch.columns)
    mins = [b""] * (len(jobs) * ncols)
    maxs = [b""] * (len(jobs) * ncols)
    on_device = batch.device.type == "cuda"
    offsets = torch.tensor([jobs[0][1]] + [j[2] for j in jobs],
                           dtype=torch.int64)
    for c, col in enumerate(batch.columns.values()):
        mm = None
        if on_device:
            # the non-empty buckets tile [lo0, hi_last) with strictly
            # ascending offsets, as the kernel requires
            lo0, hi1 = jobs[0][1], jobs[-1][2]
            red = ops.segmented_reduce(col[lo0:hi1], None, offsets - lo0,
                                       want=("min", "max"))
            mm = torch.stack([red["min"], red["max"]]).cpu().numpy()
        for f, (_, lo, hi, _) in enumerate(jobs):
            if mm is not None and not (
                    col.dtype.is_floating_point
                    and (_device_stat_unusable(mm[0, f])
                         or _device_stat_unusable(mm[1, f]))):
                mn, mx = mm[0, f].tobytes(), mm[1, f].tobytes()
            else:
                mn, mx = _statistics(col[lo:hi].cpu().numpy())
            mins[f * ncols + c] = mn
            maxs[f * ncols + c] = mx
    return mins, maxs


def _write_bucketed_native(batch: ColumnBatch, jobs,
                           after_event: Optional["torch.cuda.Event"]
                           ) -> List[str]:
    """All bucket files of an eligible batch through the extension's
    write_bucket_files: statistics from the device, then one GIL-released
    call that streams chunks through a pinned ring into pwrite (host
    batches: pwrite from the column memory).  HS_WRITE_CHUNK_MB and
    HS_WRITE_THREADS override the chunk size and the writer thread
    count."""
    import time as _time
    import numpy as np
    from ...sources.native_parquet import (ColumnChunkLayout, Page,
                                           _layout_cache_put)
    from ...sources.staging import _pinned_get, _pinned_put
    timing = os.environ.get("HS_TIMING")
    t0 = _time.perf_counter()
    on_device = batch.device.type == "cuda"
    names = list(batch.columns.keys())
    cols = [c.contiguous() for c in batch.columns.values()]
    chunk = max(1, int(float(os.environ.get("HS_WRITE_CHUNK_MB", "8"))
                       * (1 << 20)))
    # copier + writers stay within the 16 CPUs a process is given
    threads = min(15, max(1, int(os.environ.get("HS_WRITE_THREADS", "15"))))
    paths = [j[3] for j in jobs]
    row_lo = [j[1] for j in jobs]
    row_hi = [j[2] for j in jobs]
    ring = None
    streams = (0, 0)
    if on_device:
        if after_event is not None:
            torch.cuda.current_stream(batch.device).wait_event(after_event)
        # no chunk is larger than the largest column payload, and the
        # ring never holds more slots than there are chunks
        esz = max(c.element_size() for c in cols)
        largest = max(hi - lo for lo, hi in zip(row_lo, row_hi)) * esz
        chunk = min(chunk, -(-largest // 4096) * 4096)
        n_chunks = sum(-(-(hi - lo) * c.element_size() // chunk)
                       for lo, hi in zip(row_lo, row_hi) for c in cols)
        ring = _pinned_get(chunk * max(2, min(_WRITE_RING_SLOTS, n_chunks)))
    try:
        with torch.cuda.device(batch.device) if on_device \
                else contextlib.nullcontext():
            mins, maxs = _bucket_statistics(batch, jobs)
            t1 = _time.perf_counter()
            if on_device:
                pool = [torch.cuda.Stream(device=batch.device)
                        for _ in range(2)]
                streams = tuple(s.cuda_stream for s in pool)
            sizes, mtimes, starts, ends = ops.native.ext().write_bucket_files(
                cols, names, paths, row_lo, row_hi, mins, maxs,
                ring if ring is not None
                else torch.empty(0, dtype=torch.uint8),
                chunk, threads, streams[0], streams[1], bool(timing))
    finally:
        if ring is not None:
            _pinned_put(ring)
    ncols = len(cols)
    np_dtypes = [np.dtype(str(c.dtype).replace("torch.", "")) for c in cols]
    for f, path in enumerate(paths):
        rows = row_hi[f] - row_lo[f]
        _layout_cache_put(path, rows, [
            ColumnChunkLayout(
                names[c], np_dtypes[c],
                [Page("plain", starts[f * ncols + c], ends[f * ncols + c],
                      rows)], rows, "plain", None, [None])
            for c in range(ncols)], (sizes[f], mtimes[f]))
    if timing:
        import sys as _sys
        t2 = _time.perf_counter()
        print(f"[hs-timing] native write: stats {t1-t0:.3f}s "
              f"files {t2-t1:.3f}s ({len(paths)} files, chunk {chunk} B, "
              f"{threads} writers)", file=_sys.stderr)
    return paths


def write_bucketed(batch: ColumnBatch, seg: torch.Tensor, out_dir: str,
                   num_buckets: int, task_id: int = 0,
                   after_event: Optional["torch.cuda.Event"] = None
                   ) -> List[str]:
    """Write per-bucket parquet files honoring the bucket-id filename
    contract.  Empty buckets produce no file (as in Spark).

    The common shape (see _native_write_eligible, and more than two
    files) goes through the extension's native writer; the files are the
    same bytes either way.  Everything else runs the Python writer below.

    Files are written by a thread pool: the native encoder's byte
    assembly (numpy tobytes) and os.write both release the GIL, so the
    200-file write overlaps to page-cache speed.  ``after_event``: D2H
    copies wait on it (orders them after the producing sort when the
    caller pipelines sort and write on different streams).
    """
    from concurrent.futures import ThreadPoolExecutor
    from ...execution.columnar import StringColumn
    from ...sources.parquet_io import _pinned_get, _pinned_put
    on_device = batch.device.type == "cuda"
    jobs = []
    for b in range(num_buckets):
        lo, hi = int(seg[b]), int(seg[b + 1])
        if hi <= lo:
            continue
        jobs.append((b, lo, hi,
                     os.path.join(out_dir, bucket_file_name(task_id, b))))

    if len(jobs) > 2 and _native_write_eligible(batch):
        return _write_bucketed_native(batch, jobs, after_event)

    # per-worker HIP streams + pooled pinned staging: pageable D2H runs
    # at ~13 GB/s, pinned at ~53 GB/s, and per-bucket copies on separate
    # streams overlap other workers' os.write calls
    streams = ([torch.cuda.Stream(device=batch.device)
                for _ in range(min(8, max(1, len(jobs))))]
               if on_device else [])

    def write_one(job_i):
        b, lo, hi, out = jobs[job_i]
        piece = batch.slice(lo, hi)
        held = []
        if on_device:
            s = streams[job_i % len(streams)]
            if after_event is not None:
                s.wait_event(after_event)
            cols = {}
            masks = {}
            with torch.cuda.stream(s):
                for name, col in piece.columns.items():
                    if isinstance(col, StringColumn):
                        cols[name] = col.to("cpu")
                        continue
                    nb = col.numel() * col.element_size()
                    bufp = _pinned_get(nb)
                    host = bufp[:nb].view(col.dtype)
                    host.copy_(col, non_blocking=True)
                    cols[name] = host
                    held.append(bufp)
                for name, m in piece.masks.items():
                    masks[name] = m.to("cpu")
            s.synchronize()
            piece = ColumnBatch(cols, masks)
        write_batch_parquet(piece, out)
        for bufp in held:
            _pinned_put(bufp)
        return out

    if len(jobs) <= 2:
        return [write_one(i) for i in range(len(jobs))]
    with ThreadPoolExecutor(max_workers=16) as pool:
        return list(pool.map(write_one, range(len(jobs))))


register_derived_dataset(COVERING_INDEX_TYPE, CoveringIndex)
