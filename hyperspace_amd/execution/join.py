"""Equi-joins as per-bucket sort-merge joins (K4).

Two physical paths serve every join type.  Co-bucketed: both sides are
already hash-partitioned into the same buckets and sorted by the join key
within each bucket at build time, so the merge join runs with zero
exchange.  Shuffled: both sides are sorted on the fly into one segment
each (counts as an Exchange in plan-diff tests).  ``_physical_path``
chooses and prepares the path for the inner and the typed joins alike.
"""

from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from .columnar import (ColumnBatch, StringColumn, _gather_nullable,
                       _join_columns, _null_batch)
from .layout import join_side_bucketed
from .. import ops
from ..exceptions import HyperspaceException
from ..plan.expr import extract_equi_join_keys
from ..plan.nodes import Join


def exec_join(ex, plan: Join) -> ColumnBatch:
    pairs = extract_equi_join_keys(plan.condition)
    if not pairs:
        raise HyperspaceException(
            "Only equi-joins are executable in v0")
    left_bucketed = join_side_bucketed(plan.left, [p[0] for p in pairs])
    right_bucketed = join_side_bucketed(plan.right, [p[1] for p in pairs])

    lbatch, lseg = ex._exec(plan.left)
    rbatch, rseg = ex._exec(plan.right)

    # two indexes are co-bucketed only if equal keys hash alike: an
    # int64 key and a narrower one (or double and float) land in
    # different buckets, so such a pair joins on the shuffled path
    co_bucketed = left_bucketed and right_bucketed and all(
        _same_hash_kind(lbatch.column(ln), rbatch.column(rn))
        for ln, rn in pairs)
    if plan.join_type != "inner":
        return _typed_join(ex, plan.join_type, pairs, lbatch, lseg,
                           rbatch, rseg, co_bucketed)
    return _inner_join(ex, pairs, lbatch, lseg, rbatch, rseg, co_bucketed)


def _physical_path(ex, label: str, pairs, co_bucketed: bool,
                   lbatch: ColumnBatch, lseg: Optional[torch.Tensor],
                   rbatch: ColumnBatch, rseg: Optional[torch.Tensor]):
    """Choose the physical path for two inputs already free of null keys,
    count it, and return the aligned ``(lbatch, lk, lseg, rbatch, rk,
    rseg)``: u64 keys of the first key pair, sorted within the segments
    that both sides share.  ``label`` completes the operator name."""
    lk_t, rk_t = _join_key_tensors(lbatch, rbatch, *pairs[0])
    lk = ops.sql_key(lk_t)
    rk = ops.sql_key(rk_t)
    if (co_bucketed and lseg is not None and rseg is not None
            and lseg.numel() == rseg.numel()):
        ex.stats.merge_joins += 1
        ex.stats.record(f"SortMergeJoin(co-bucketed{label})")
        return lbatch, lk, lseg, rbatch, rk, rseg
    ex.stats.shuffles += 2
    ex.stats.hash_joins += 1
    ex.stats.record(f"SortMergeJoin(shuffled{label})")
    if lk.numel():
        lperm = ops.sort_perm(lk)
        lbatch, lk = lbatch.gather(lperm), lk[lperm]
    if rk.numel():
        rperm = ops.sort_perm(rk)
        rbatch, rk = rbatch.gather(rperm), rk[rperm]
    lseg = torch.tensor([0, lk.numel()], dtype=torch.int64)
    rseg = torch.tensor([0, rk.numel()], dtype=torch.int64)
    return lbatch, lk, lseg, rbatch, rk, rseg


def _inner_join(ex, pairs, lbatch: ColumnBatch,
                lseg: Optional[torch.Tensor], rbatch: ColumnBatch,
                rseg: Optional[torch.Tensor], co_bucketed: bool
                ) -> ColumnBatch:
    # inner-join SQL semantics: null join keys never match — drop
    # them up front (bucketed layouts keep NULLS FIRST per bucket,
    # so the segment offsets shift by the per-prefix null count)
    lbatch, lseg = _drop_null_keys(lbatch, pairs[0][0], lseg)
    rbatch, rseg = _drop_null_keys(rbatch, pairs[0][1], rseg)
    lbatch, lk, lseg, rbatch, rk, rseg = _physical_path(
        ex, "", pairs, co_bucketed, lbatch, lseg, rbatch, rseg)
    lidx, ridx = ops.merge_join(lk, rk, lseg, rseg)
    # secondary key equality check for multi-key joins (null
    # secondary keys never match)
    lidx, ridx = _secondary_key_filter(lbatch, rbatch, pairs, lidx, ridx)
    return _join_columns(lbatch.gather(lidx), rbatch.gather(ridx))


def _typed_join(ex, jt: str, pairs, lbatch: ColumnBatch,
                lseg: Optional[torch.Tensor], rbatch: ColumnBatch,
                rseg: Optional[torch.Tensor], co_bucketed: bool
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
    lbatch, lseg, lnull = _split_null_keys(lbatch, pairs[0][0], lseg)
    rbatch, rseg, rnull = _split_null_keys(rbatch, pairs[0][1], rseg)
    lbatch, lk, lseg, rbatch, rk, rseg = _physical_path(
        ex, f", {jt}", pairs, co_bucketed, lbatch, lseg, rbatch, rseg)
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
