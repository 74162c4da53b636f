"""ORDER BY and LIMIT over ColumnBatches (K14).

Values compare by ``ops.sql_key``: NaN above every number and equal to
itself, -0.0 with +0.0, strings by their dictionary codes (the dictionary
is sorted), decimals, dates and timestamps by their stored integers.  A
descending column sorts on the complement of that key, so every sort and
every selection below is an ascending u64 one.

  order_key     the u64 order key of one column
  order_perm    stable multi-column sort permutation (full ORDER BY)
  topk_select   ORDER BY ... LIMIT n by radix select: the rows that can be
                among the first n come from ``ops.topk_rows`` on the
                leading column, and only they are sorted
  topk_bucketed the same over a batch whose buckets are each sorted on the
                single order column: the candidates are the first (last)
                n rows of every bucket, and no kernel reads the column
"""

from __future__ import annotations

import os
from typing import List

import torch

from .columnar import ColumnBatch
from .. import ops
from ..plan.expr import SortOrder


def order_key(col, ascending: bool = True) -> torch.Tensor:
    """u64 key (int64-encoded) whose ascending order is the requested
    order of ``col`` (a tensor or a StringColumn)."""
    t = col.codes if hasattr(col, "codes") else col
    return ops.order_key(t, not ascending)


def order_perm(batch: ColumnBatch, orders: List[SortOrder]) -> torch.Tensor:
    """Stable multi-column sort permutation: LSD over the order columns
    (least significant first) with the stable radix sort, then per
    nullable column one stable partition that puts its null rows first or
    last.  Null rows sort on a blanked key, so rows that tie on every
    column keep the batch's row order."""
    n = batch.num_rows
    dev = batch.device
    perm = torch.arange(n, dtype=torch.int64, device=dev)
    first = True
    for o in reversed(orders):
        keys = order_key(batch.column(o.column), o.ascending)
        m = batch.mask(o.column) if batch.has_nulls(o.column) else None
        if m is not None:
            keys = torch.where(m, keys, torch.zeros_like(keys))
        if not first:
            keys = ops.gather_rows(keys, perm)
        first = False
        _, perm = ops.sort_pairs(keys, perm)
        if m is not None:
            f = m[perm]
            nulls = torch.nonzero(~f, as_tuple=False).flatten()
            vals = torch.nonzero(f, as_tuple=False).flatten()
            perm = perm[torch.cat([nulls, vals] if o.nulls_first
                                  else [vals, nulls])]
    return perm


def select_enabled() -> bool:
    """``HS_TOPK_SELECT=0`` (read per call) sorts the whole input instead
    of selecting: for A/B runs and as a way back."""
    return os.environ.get("HS_TOPK_SELECT", "1") != "0"


def _sorted_head(batch: ColumnBatch, orders: List[SortOrder], n: int
                 ) -> ColumnBatch:
    if batch.num_rows > 1:
        batch = batch.gather(order_perm(batch, orders)[:n])
    return batch.slice(0, min(n, batch.num_rows))


def topk_select(batch: ColumnBatch, orders: List[SortOrder], n: int
                ) -> ColumnBatch:
    """First ``n`` rows of the stable sort of ``batch`` by ``orders``,
    exactly, without sorting the batch: candidates by the leading column,
    then the sort of the candidates alone."""
    rows = batch.num_rows
    if n >= rows or not select_enabled():
        return _sorted_head(batch, orders, n)
    lead = orders[0]
    keep_ties = len(orders) > 1
    key = order_key(batch.column(lead.column), lead.ascending)
    m = batch.mask(lead.column) if batch.has_nulls(lead.column) else None
    if m is None:
        cand = ops.topk_rows(key, n, None, keep_ties)
    else:
        null_rows = torch.nonzero(~m, as_tuple=False).flatten()
        c0 = null_rows.numel()
        nv = rows - c0
        if lead.nulls_first:
            if n <= c0:
                cand = null_rows
            else:
                cand = torch.cat([
                    null_rows, ops.topk_rows(key, n - c0, m, keep_ties)])
        else:
            if n <= nv:
                cand = ops.topk_rows(key, n, m, keep_ties)
            else:
                cand = torch.cat([
                    torch.nonzero(m, as_tuple=False).flatten(), null_rows])
        if not keep_ties:
            # all nulls tie: the first ones in row order are the answer
            if lead.nulls_first and n <= c0:
                cand = cand[:n]
            elif not lead.nulls_first and n > nv:
                cand = cand[:n]
        # a null and a valid row never tie, and each of the two lists is
        # in row order: rows that tie keep the batch's order
    return _sorted_head(batch.gather(cand), orders, n)


def bucket_candidates(seg: torch.Tensor, n: int, ascending: bool
                      ) -> torch.Tensor:
    """Row indices of the first (ascending) or last (descending)
    ``min(n, len)`` rows of every bucket, from the num_buckets + 1 segment
    offsets: at most num_buckets * n rows, in row order."""
    seg = seg.to(torch.int64).cpu()
    lens = seg[1:] - seg[:-1]
    take = lens.clamp(max=n)
    starts = seg[:-1] if ascending else seg[1:] - take
    total = int(take.sum())
    ends = torch.cumsum(take, 0)
    within = torch.arange(total, dtype=torch.int64) - \
        torch.repeat_interleave(ends - take, take)
    return torch.repeat_interleave(starts, take) + within


def topk_bucketed(batch: ColumnBatch, seg: torch.Tensor, order: SortOrder,
                  n: int) -> ColumnBatch:
    """ORDER BY one column LIMIT n over buckets each sorted on that
    column (no nulls in it): the answer lies in the first (last) n rows
    of the buckets."""
    cand = bucket_candidates(seg, n, order.ascending).to(batch.device)
    return _sorted_head(batch.gather(cand), [order], n)
