"""Group-by as a reduce over adjacent runs (K13): group offsets from
adjacency, then one fused segmented reduce per input column."""

from __future__ import annotations

from typing import Dict, List

import torch

from .columnar import ColumnBatch, StringColumn
from .join import _split_null_keys
from .layout import aggregate_operator_name
from .. import ops
from ..exceptions import HyperspaceException
from ..plan.nodes import Aggregate


def exec_aggregate(ex, plan: Aggregate) -> ColumnBatch:
    """Grouped path: the child is bucketed on the single grouping
    column, so every group sits in one bucket with its rows adjacent
    (filters and projections keep row order) — no sort, no
    repartition.  Multi-file buckets are re-sorted on the stored
    placeholder of null rows, so null keys are split off and reduced
    as one group of their own.  Sort path (everything else): sort by
    the grouping columns first, which counts as a shuffle.  A global
    aggregate is one run and needs neither."""
    batch, _ = ex._exec(plan.child)
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
    ex.stats.sort_aggregates += 1
    ex.stats.record(op)
    if not keys:
        return _reduce_runs(batch, [], plan.aggs, global_group=True)
    if op == "SortAggregate(bucketed)":
        if batch.has_nulls(keys[0]):
            rest, _, nulls = _split_null_keys(batch, keys[0], None)
            return ColumnBatch.concat([
                _reduce_runs(rest, keys, plan.aggs),
                _reduce_runs(nulls, keys, plan.aggs, one_group=True)])
        return _reduce_runs(batch, keys, plan.aggs)
    ex.stats.shuffles += 1
    if batch.num_rows:
        batch = batch.gather(_group_sort_perm(batch, keys))
    return _reduce_runs(batch, keys, plan.aggs)


def _group_sort_perm(batch: ColumnBatch, keys: List[str]) -> torch.Tensor:
    """Permutation that makes equal key tuples adjacent.  Null rows sort
    on (null flag, key): their stored values are blanked first."""
    # the index package imports this one for ColumnBatch
    from ..index.covering.index import _multi_key_sort_perm
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
    return _multi_key_sort_perm(sort_batch, keys)


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
    reduced = _reduce_columns(batch, aggs, offsets)
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


def _reduce_columns(batch: ColumnBatch, aggs, offsets: torch.Tensor
                    ) -> Dict[str, dict]:
    """One fused reduce per input column, for everything asked of it:
    lower-cased column name -> {output name -> per-group tensor}."""
    n_groups = offsets.numel() - 1
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
        if batch.num_rows == 0:
            # nothing to read: counts are 0, everything else null
            t = batch.tensor(cname)
            sum_dt = torch.float64 if t.dtype.is_floating_point \
                else torch.int64
            reduced[cname] = {
                o: torch.zeros(n_groups, device=batch.device, dtype=(
                    sum_dt if o == "sum" else
                    torch.int64 if o == "count" else t.dtype))
                for o in want}
        else:
            reduced[cname] = ops.segmented_reduce(
                batch.tensor(cname), batch.mask(cname), offsets, want)
    return reduced
