"""Parquet read/write for the build pipeline (host path).

Write side keeps the reference's bucket-id-in-filename contract:
``part-<task>-<uuid>_<bucketid>.c000.parquet`` — OptimizeAction groups
files by the bucket id parsed from the name
(reference: actions/OptimizeAction.scala:109-111; Spark bucketed file
naming from saveWithBuckets, index/DataFrameWriterExtensions.scala:50-80).

Index data files are written UNCOMPRESSED with PLAIN encoding so the
device Parquet page-decode kernel (K1) has a direct path; pyarrow handles
footer/metadata assembly.
"""

from __future__ import annotations

import itertools
import os
import re
import sys
import threading
import time
import uuid
from concurrent.futures import ThreadPoolExecutor, as_completed
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from ..exceptions import HyperspaceException
from .device_decode import (DecodeState, convert_logical, decode_chunks,
                            split_row_groups)
from .logical_types import (Conv, check_parquet_file, parquet_convs,
                            to_storage_np)
from .native_parquet import (StrCol, layout_cache_get, merge_string_dicts,
                             read_native_layout, string_remap_tables)
from .staging import _DEV_RATIO, _pinned_get, _pinned_put  # noqa: F401

_BUCKET_RE = re.compile(r".*_(\d+)(?:\.\w+)*\.parquet$")


def bucket_id_of_file(path: str) -> Optional[int]:
    m = _BUCKET_RE.match(os.path.basename(path))
    return int(m.group(1)) if m else None


def bucket_file_name(task_id: int, bucket_id: int, token: str = "") -> str:
    token = token or uuid.uuid4().hex[:8]
    return f"part-{task_id:05d}-{token}_{bucket_id:05d}.c000.parquet"


def write_batch_parquet(batch, path: str, compression: Optional[str] = None,
                        use_dictionary: bool = False) -> Tuple[int, int]:
    """Write a ColumnBatch to one parquet file.  Returns (size, mtime_ms).

    All-numeric batches use the native writer (uncompressed PLAIN pages
    assembled directly from the column buffers — K3 encode side); string
    columns fall back to pyarrow.
    """
    from ..execution.columnar import StringColumn
    if compression is None:
        from .native_parquet import write_parquet_native, _NP_TO_PARQUET
        cols = {name: (StrCol(c.codes.numpy(), c.values)
                       if isinstance(c, StringColumn) else c.numpy())
                for name, c in batch.columns.items()}
        if all(isinstance(a, StrCol) or a.dtype in _NP_TO_PARQUET
               for a in cols.values()):
            masks = {name: m.numpy()
                     for name, m in batch.masks.items()} \
                if batch.masks else None
            return write_parquet_native(cols, path, masks)
    import pyarrow.parquet as pq
    table = batch.to_arrow()
    pq.write_table(table, path, compression=compression or "NONE",
                   use_dictionary=use_dictionary,
                   write_statistics=True,
                   data_page_version="1.0")
    st = os.stat(path)
    return st.st_size, int(st.st_mtime * 1000)


def _resolve_read_columns(p, columns):
    """Map requested column names onto a file schema: a dotted request
    ("a.b.c") may be a nested leaf (read the top-level struct and let
    from_arrow flatten it); flat columns whose NAME contains dots (our
    index data for nested leaves) match the file schema directly."""
    import pyarrow.parquet as pq
    if columns is None:
        return None
    top = {n.lower(): n for n in pq.ParquetFile(p).schema_arrow.names}
    read_cols = []
    for c in columns:
        if c.lower() in top:
            read_cols.append(top[c.lower()])
        elif "." in c and c.split(".")[0].lower() in top:
            root = top[c.split(".")[0].lower()]
            if root not in read_cols:
                read_cols.append(root)
        else:
            read_cols.append(c)
    return read_cols


def _pyarrow_file_dict(p, columns):
    """One non-native file read through pyarrow into the per-file
    (columns, masks) dict shape of read_native_host, so a batch can mix
    native and fallback files."""
    import pyarrow.parquet as pq
    from ..execution.columnar import ColumnBatch, StringColumn
    check_parquet_file(p, columns)  # same refusals as the native walk
    t = pq.read_table(p, columns=_resolve_read_columns(p, columns))
    b = ColumnBatch.from_arrow(t)
    if columns is not None:
        b = b.select(columns)
    cols = {}
    for name, c in b.columns.items():
        cols[name] = (StrCol(c.codes.numpy(), c.values)
                      if isinstance(c, StringColumn) else c.numpy())
    masks = {name: m.numpy() for name, m in (b.masks or {}).items()}
    return cols, masks, t.num_rows


def read_files_batch(paths: List[str], columns: Optional[List[str]] = None):
    """Read parquet files into a single host ColumnBatch, plus per-file row
    counts (for lineage / per-file segmentation).  Native-layout files
    (uncompressed PLAIN numeric) bypass pyarrow; non-native files decode
    per-file through pyarrow and merge with the native ones (a single
    legacy file no longer drops the whole batch to the slow path)."""
    from ..execution.columnar import ColumnBatch
    from .native_parquet import read_native_host

    per_file = []
    per_file_masks = []
    row_counts = []
    native_ok = True
    try:
        for p in paths:
            res = read_native_host(p, columns)
            if res is None:
                cols, fmasks, n = _pyarrow_file_dict(p, columns)
            else:
                cols, fmasks = res
                n = len(next(iter(cols.values()))) if cols else 0
            per_file.append(cols)
            per_file_masks.append(fmasks)
            row_counts.append(n)
    except HyperspaceException:  # a refused logical type
        raise
    except Exception:  # exotic schema mix: whole-batch pyarrow path
        native_ok = False
        row_counts = []
    if native_ok and paths:
        names = list(per_file[0].keys())
        if columns is not None:
            order = {c.lower(): i for i, c in enumerate(columns)}
            names.sort(key=lambda n: order.get(n.lower(), 99))
        from ..execution.columnar import StringColumn
        merged = {}
        merged_masks = {}
        for name in names:
            arrs = [f[name] for f in per_file]
            if any(isinstance(a, StrCol) for a in arrs):
                # merge per-file dictionaries, remap codes (unsorted
                # parquet insertion-order dictionaries force the remap:
                # StringColumn codes must follow lex order)
                dicts = [a.values for a in arrs]
                mvals, remap = merge_string_dicts(dicts)
                parts = [a.codes for a in arrs]
                if remap:
                    parts = [part if lut is None
                             else np.array(lut, dtype=np.int32)[part]
                             for part, lut in zip(
                                 parts, string_remap_tables(mvals, dicts))]
                codes = np.concatenate(parts) if len(parts) > 1 else parts[0]
                merged[name] = StringColumn(
                    torch.from_numpy(np.ascontiguousarray(codes)),
                    list(mvals))
            else:
                merged[name] = torch.from_numpy(
                    np.concatenate(arrs) if len(arrs) > 1 else arrs[0])
            if any(name in fm for fm in per_file_masks):
                mparts = [fm.get(name, np.ones(rc, dtype=bool))
                          for fm, rc in zip(per_file_masks, row_counts)]
                merged_masks[name] = torch.from_numpy(
                    np.concatenate(mparts) if len(mparts) > 1
                    else mparts[0])
        return ColumnBatch(merged, merged_masks), row_counts

    import pyarrow.parquet as pq
    import pyarrow as pa
    tables = []
    row_counts = []
    for p in paths:
        check_parquet_file(p, columns)
        t = pq.read_table(p, columns=_resolve_read_columns(p, columns))
        tables.append(t)
        row_counts.append(t.num_rows)
    if not tables:
        return ColumnBatch({}), []
    table = pa.concat_tables(tables, promote_options="default")
    batch = ColumnBatch.from_arrow(table)
    if columns is not None:
        batch = batch.select(columns)
    return batch, row_counts


_PHYS_TO_NP = {"INT64": np.dtype("int64"), "INT32": np.dtype("int32"),
               "DOUBLE": np.dtype("float64"), "FLOAT": np.dtype("float32")}
_NP_TO_TORCH = {np.dtype("int64"): torch.int64,
                np.dtype("int32"): torch.int32,
                np.dtype("float64"): torch.float64,
                np.dtype("float32"): torch.float32}
_N_STREAMS = 16  # row-group units of a single file fan out too


class _ReadPlan(NamedTuple):
    """What the footers (or the writer's layout cache) say about a batch
    of files, enough to size the output before any file is read."""
    names: List[str]               # output columns, in output order
    dtypes: Dict[str, np.dtype]    # PHYSICAL dtype the decoders write
    convs: Dict[str, Conv]         # columns converted after the decode
    row_counts: List[int]
    nullable_cols: set
    string_cols: set
    layouts: Optional[list]        # per-file chunk layouts (cache hit)
    metas: list                    # per-file footer metadata (cache miss)
    schemas: list


def _plan_from_cache(cached, want) -> _ReadPlan:
    lay0 = cached[0][1]
    return _ReadPlan(
        [c.name for c in lay0 if want is None or c.name.lower() in want],
        {c.name: c.np_dtype for c in lay0},
        {c.name: c.conv for c in lay0 if c.conv is not None},
        [ent[0] for ent in cached],
        {c.name for ent in cached for c in ent[1] if c.has_nulls},
        {c.name for ent in cached for c in ent[1] if c.is_string},
        [[c for c in ent[1] if want is None or c.name.lower() in want]
         for ent in cached], [], [])


def _plan_from_footers(paths, want) -> Optional[_ReadPlan]:
    import pyarrow.parquet as pq
    metas = []
    schemas = []
    for p in paths:
        try:
            pf = pq.ParquetFile(p)
        except Exception:  # noqa: BLE001
            return None
        metas.append(pf.metadata)
        schemas.append(pf.schema)
    # refused logical types raise here: nothing is allocated or launched
    file_convs = [parquet_convs(sch, want) for sch in schemas]
    # column nullability from chunk statistics (sizes the preallocated
    # masks); an OPTIONAL chunk without statistics could hide nulls ->
    # the host path decides instead
    nullable_cols = set()
    for md, sch in zip(metas, schemas):
        for rg_i in range(md.num_row_groups):
            rg = md.row_group(rg_i)
            for ci in range(rg.num_columns):
                col = rg.column(ci)
                st = col.statistics
                if st is None or st.null_count is None:
                    if sch.column(ci).max_definition_level > 0:
                        return None
                elif st.null_count > 0:
                    nullable_cols.add(col.path_in_schema)
    rg0 = metas[0].row_group(0)
    names = []
    dtypes = {}
    convs = {}
    string_cols = set()
    for ci in range(rg0.num_columns):
        col = rg0.column(ci)
        name = col.path_in_schema
        if want is not None and name.lower() not in want:
            continue
        npd = _PHYS_TO_NP.get(col.physical_type)
        if npd is None:
            sch_col = schemas[0].column(ci)
            if col.physical_type == "BYTE_ARRAY":
                # dictionary strings decode to int32 codes; the layout
                # parse validates the encoding (else the worker falls
                # back)
                npd = np.dtype("int32")
                string_cols.add(name)
            elif col.physical_type == "FIXED_LEN_BYTE_ARRAY" and \
                    sch_col.logical_type.type == "DECIMAL" and \
                    sch_col.precision <= 18:
                # FLBA decimal(p<=18): engine representation is the
                # unscaled int64; files carrying it have no native
                # layout and read per file on host workers
                npd = np.dtype("int64")
            elif col.physical_type == "INT96":
                # legacy timestamp: per-file host read -> int64
                npd = np.dtype("int64")
            else:
                return None
        names.append(name)
        dtypes[name] = npd
        if ci in file_convs[0]:
            convs[name] = file_convs[0][ci]
    return _ReadPlan(names, dtypes, convs, [md.num_rows for md in metas],
                     nullable_cols, string_cols, None, metas, schemas)


def _plan_device_read(paths, columns) -> Optional[_ReadPlan]:
    """Footer metadata (cheap) sizes the output tensors up front.  None:
    the batch has to take the host table path."""
    want = {c.lower() for c in columns} if columns is not None else None
    # write-time layout cache: every file our native writer produced in
    # this process skips the footer + page-header parse (the dominant
    # GIL-bound cost of a ~200-file cold load)
    cached = [layout_cache_get(p) for p in paths]
    plan = (_plan_from_cache(cached, want) if None not in cached
            else _plan_from_footers(paths, want))
    if plan is not None and columns is not None:
        order = {c.lower(): i for i, c in enumerate(columns)}
        plan.names.sort(key=lambda n: order.get(n.lower(), 99))
    return plan


class _DeviceRead:
    """The read -> upload -> decode pipeline of one batch.  Each file's
    H2D copy and decode kernels run on their own stream, so copies
    overlap other files' decodes instead of serializing on the default
    stream (xfers are the cold-load bound)."""

    def __init__(self, paths, columns, device, plan: _ReadPlan):
        from ..ops import native as native_ext
        self.paths, self.columns, self.plan = paths, columns, plan
        total_rows = int(sum(plan.row_counts))
        self.st = DecodeState(
            device, native_ext.ext(), plan.names,
            np.concatenate([[0], np.cumsum(plan.row_counts)[:-1]]),
            {n: torch.empty(total_rows, dtype=_NP_TO_TORCH[plan.dtypes[n]],
                            device=device) for n in plan.names},
            {n: torch.ones(total_rows, dtype=torch.bool, device=device)
             for n in plan.names if n in plan.nullable_cols},
            os.environ.get("HS_DECODE_TIMING"))
        self.streams = [torch.cuda.Stream(device=device)
                        for _ in range(_N_STREAMS)]
        # per file: (pinned buffer or None for a host-read file, size,
        # chunk layouts)
        self.infos: List[Optional[tuple]] = [None] * len(paths)
        self.dev_bufs: List[Optional[torch.Tensor]] = [None] * len(paths)
        self.upload_events: list = [None] * len(paths)
        self.upload_lock = threading.Lock()
        self.uids = itertools.count()

    def load_file(self, i):
        """Read + layout-parse one file (no decode)."""
        p = self.paths[i]
        size = os.path.getsize(p)
        buf = _pinned_get(size + 4)
        view = memoryview(buf.numpy())
        with open(p, "rb", buffering=0) as f:
            f.readinto(view[:size])
        if self.plan.layouts is not None:
            return buf, size, self.plan.layouts[i]
        lay = read_native_layout(p, self.columns, data=view[:size],
                                 meta=self.plan.metas[i],
                                 pf_schema=self.plan.schemas[i])
        if lay is None:  # no native layout: per-file pyarrow host read
            _pinned_put(buf)
            return None, 0, None
        return buf, size, lay[1]

    def host_unit(self, i):
        """Non-native file inside a mixed batch: pyarrow-read on this
        worker thread, upload into the preallocated slices (the native
        files around it stay on the device decode path)."""
        st, plan = self.st, self.plan
        cols, fmasks, n = _pyarrow_file_dict(self.paths[i], self.columns)
        assert n == plan.row_counts[i], (self.paths[i], n,
                                         plan.row_counts[i])
        low = {k.lower(): v for k, v in cols.items()}
        mlow = {k.lower(): v for k, v in fmasks.items()}
        base = int(st.file_base[i])
        with torch.cuda.stream(self.streams[i % _N_STREAMS]):
            for name in plan.names:
                arr = low[name.lower()]
                if isinstance(arr, StrCol):
                    st.str_chunks.append((name, base, base + n,
                                          arr.values))
                    arr = arr.codes
                else:
                    # engine representation -> the physical dtype the
                    # batch stores until its convert step (a uint32
                    # column travels as its int32 bit pattern)
                    arr = to_storage_np(arr, plan.dtypes[name])
                st.out[name][base:base + n] = torch.from_numpy(
                    np.ascontiguousarray(arr)).to(st.device,
                                                  non_blocking=True)
                m = mlow.get(name.lower())
                if name in st.out_masks and m is not None:
                    st.out_masks[name][base:base + n] = \
                        torch.from_numpy(m).to(st.device, non_blocking=True)

    def decode_unit(self, uid, i, row_off, chunks):
        buf, size, _ = self.infos[i]
        t0 = time.perf_counter()
        stream = self.streams[uid % _N_STREAMS]
        with torch.cuda.stream(stream):
            with self.upload_lock:
                if self.dev_bufs[i] is None:
                    # upload only the file's bytes (+4B decode slack),
                    # not the whole pooled size class
                    self.dev_bufs[i] = buf[:size + 4].to(
                        self.st.device, non_blocking=True)
                    self.upload_events[i] = torch.cuda.Event()
                    self.upload_events[i].record(stream)
                else:
                    stream.wait_event(self.upload_events[i])
            decode_chunks(self.st, i, buf, self.dev_bufs[i], chunks, row_off)
        if self.st.timing == "2":
            print(f"[hs-unit] u{uid} rows={chunks[0].num_values} chunks="
                  f"{[(c.name, c.encoding, len(c.pages)) for c in chunks]} "
                  f"{time.perf_counter()-t0:.3f}s", file=sys.stderr)

    def units(self, i):
        """The decode calls of loaded file ``i``: one per row group when
        the batch has fewer files than streams, else one per file."""
        chunks = self.infos[i][2]
        if chunks is None:
            return [(self.host_unit, i)]
        groups = (split_row_groups(chunks) if len(self.paths) < _N_STREAMS
                  else [(0, chunks)])
        return [(self.decode_unit, next(self.uids), i, row_off, rg_chunks)
                for row_off, rg_chunks in groups]

    def run(self) -> int:
        """File reads stream into decode units as each read completes (a
        strict all-reads-then-all-decodes barrier left the H2D + decode
        tail serialized after ~0.46 s of source reads).  Returns the
        number of units."""
        n_units = 0
        workers = int(os.environ.get("HS_DECODE_WORKERS", "16"))
        if len(self.paths) > 2 and workers > 1:
            dec_futs = []
            with ThreadPoolExecutor(max_workers=16) as read_pool, \
                    ThreadPoolExecutor(max_workers=workers) as dec_pool:
                read_futs = {read_pool.submit(self.load_file, i): i
                             for i in range(len(self.paths))}
                for fut in as_completed(read_futs):
                    i = read_futs[fut]
                    self.infos[i] = fut.result()
                    dec_futs += [dec_pool.submit(*u) for u in self.units(i)]
                for f in dec_futs:
                    f.result()
            return len(dec_futs)
        for i in range(len(self.paths)):
            self.infos[i] = self.load_file(i)
        for i in range(len(self.paths)):
            for fn, *args in self.units(i):
                fn(*args)
                n_units += 1
        return n_units


def _merge_string_columns(st: DecodeState, string_cols) -> None:
    """One sorted dictionary per string column over all its decoded
    runs; codes of runs under another dictionary remap on device."""
    from ..execution.columnar import StringColumn
    by_name: Dict[str, list] = {}
    for name, lo, hi, vals in st.str_chunks:
        by_name.setdefault(name, []).append((lo, hi, vals))
    for name in string_cols:
        runs = by_name.get(name, [])
        dicts = [v for _, _, v in runs]
        merged, remap = merge_string_dicts(dicts)
        if not dicts:
            merged = [""]  # all-null column: masked 0-codes
        if remap:
            tables = string_remap_tables(merged, dicts)
            for (lo, hi, _), lut in zip(runs, tables):
                if lut is not None:
                    lut = torch.tensor(lut, dtype=torch.int32,
                                       device=st.device)
                    st.out[name][lo:hi] = lut[st.out[name][lo:hi].long()]
        st.out[name] = StringColumn(st.out[name], list(merged))


def read_files_batch_device(paths: List[str], device,
                            columns: Optional[List[str]] = None):
    """Device-decoded parquet read (K1): raw file bytes -> HBM -> the
    unaligned-copy decode kernel assembles each column.  Disk reads, PCIe
    transfers and decode overlap across files.  Falls back to the host
    path + H2D for non-native files.  Returns (ColumnBatch on ``device``,
    per-file row counts)."""
    from ..execution.columnar import ColumnBatch

    def fallback():
        batch, rc = read_files_batch(paths, columns)
        return batch.to(device), rc

    plan = _plan_device_read(paths, columns)
    if plan is None:
        return fallback()
    rd = _DeviceRead(paths, columns, device, plan)
    st = rd.st
    t1 = time.perf_counter()
    n_units = rd.run()
    t2 = time.perf_counter()
    # order the default stream after every worker stream, then host-sync
    # so the pinned buffers can be recycled
    cur = torch.cuda.current_stream()
    for s in rd.streams:
        cur.wait_stream(s)
    cur.synchronize()
    if st.timing:
        print(f"[hs-decode] files={len(paths)} units={n_units} "
              f"read+decode(pipe) {t2-t1:.3f}s "
              f"sync {time.perf_counter()-t2:.3f}s", file=sys.stderr)
    # one device reduction + sync for every chunk's status words (a
    # per-tensor .any() paid ~1.4 ms of sync each across ~50 chunks)
    snappy_bad = bool(torch.cat(st.statuses).ne(0).any().item()) \
        if st.statuses else False
    for b in [inf[0] for inf in rd.infos] + st.keepalive:
        if b is not None:
            _pinned_put(b)
    if snappy_bad:
        return fallback()
    if plan.string_cols:
        _merge_string_columns(st, plan.string_cols)
    for name, conv in plan.convs.items():
        st.out[name] = convert_logical(st.out[name], conv)
    return ColumnBatch(st.out, st.out_masks), plan.row_counts
