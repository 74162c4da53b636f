"""Predicate evaluation over a ColumnBatch: plain functions of
``(batch, expr)``.

A single numeric comparison over null-free columns lowers to the native
``select_range_u64`` kernel (``_as_range``); everything else composes
boolean masks under SQL three-valued logic (``_eval_mask``).
"""

from __future__ import annotations

import operator
from typing import Optional, Tuple

import torch

from .columnar import ColumnBatch, StringColumn, _SPARK_DTYPES
from . import sql_compare
from .. import ops
from ..exceptions import HyperspaceException
from ..plan.expr import (And, Arith, BinComp, Col, Expr, In, IsNotNull,
                         IsNull, Lit, Not, Or)

_COMPARE = {"=": operator.eq, "!=": operator.ne, "<": operator.lt,
            "<=": operator.le, ">": operator.gt, ">=": operator.ge}


def _predicate_indices(batch: ColumnBatch, cond: Expr) -> torch.Tensor:
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
    mask = _eval_mask(batch, cond)
    return torch.nonzero(mask, as_tuple=False).flatten()


def _valid_of(batch: ColumnBatch, e: Expr) -> Optional[torch.Tensor]:
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


def _and_valid(batch: ColumnBatch, e: Expr, m: torch.Tensor) -> torch.Tensor:
    """A comparison involving a null is null: the row does not match."""
    v = _valid_of(batch, e)
    return m & v if v is not None else m


def _eval_mask(batch: ColumnBatch, e: Expr) -> torch.Tensor:
    if isinstance(e, And):
        return _eval_mask(batch, e.left) & _eval_mask(batch, e.right)
    if isinstance(e, Or):
        return _eval_mask(batch, e.left) | _eval_mask(batch, e.right)
    if isinstance(e, Not):
        # SQL three-valued logic: NOT(null-involving predicate) is
        # null -> the row is excluded, so AND the child's validity
        return _and_valid(batch, e.child, ~_eval_mask(batch, e.child))
    if isinstance(e, (IsNotNull, IsNull)):
        m = batch.mask(e.col.name) if batch.has_column(e.col.name) \
            else None
        if m is not None:
            return m.clone() if isinstance(e, IsNotNull) else ~m
        fill = torch.ones if isinstance(e, IsNotNull) else torch.zeros
        return fill(batch.num_rows, dtype=torch.bool, device=batch.device)
    if isinstance(e, In):
        if isinstance(e.col, Arith):
            return _and_valid(batch, e,
                              _in_mask(_eval_arith(batch, e.col), e.values))
        col = batch.column(e.col.name)
        if isinstance(col, StringColumn):
            codes = torch.tensor(
                sorted(c for c in (col.code_of(v) for v in e.values)
                       if c >= 0),
                dtype=torch.int64, device=col.codes.device)
            m = ops.isin_sorted(col.codes.to(torch.int64), codes)
        else:
            m = _in_mask(col, e.values)
        return _and_valid(batch, e, m)
    if isinstance(e, BinComp):
        return _and_valid(batch, e, _compare(batch, e))
    raise HyperspaceException(f"Cannot evaluate {e!r}")


def _eval_arith(batch: ColumnBatch, e) -> torch.Tensor:
    """Evaluate a scalar arithmetic expression per row (Arith trees over
    Col/Lit; '%' uses Java/Spark remainder = fmod)."""
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


def _compare_string_literal(col: StringColumn, op: str,
                            value: str) -> torch.Tensor:
    """The dictionary is sorted, so code order == lexicographic order; an
    absent literal maps to its insertion point."""
    codes = col.codes
    pos = col.searchsorted(value)
    exact = pos < len(col.values) and col.values[pos] == value
    if op in ("=", "!=") and not exact:
        fill = torch.zeros if op == "=" else torch.ones
        return fill(len(col), dtype=torch.bool, device=codes.device)
    if op in ("<=", ">"):
        # strictly below / not below the first code above the literal
        op, pos = ("<" if op == "<=" else ">="), pos + (1 if exact else 0)
    return _COMPARE[op](codes, pos)


def _compare(batch: ColumnBatch, e: BinComp) -> torch.Tensor:
    """General comparison mask (non-hot path; hot single comparisons lower
    to select_range_u64 in _predicate_indices)."""
    if isinstance(e.left, Arith):
        lv = _eval_arith(batch, e.left)
        rv = (_eval_arith(batch, e.right)
              if not isinstance(e.right, Lit) else e.right.value)
        if torch.is_tensor(lv) and isinstance(e.right, Lit) and \
                sql_compare.supported(lv.dtype, rv):
            return sql_compare.literal_mask(lv, e.op, rv)
        return _COMPARE[e.op](lv, rv)
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
            return _compare_string_literal(col, e.op, str(value))
        if sql_compare.supported(col.dtype, value):
            return sql_compare.literal_mask(col, e.op, value)
        lv = col
        rv = torch.tensor(value, dtype=col.dtype, device=col.device)
    return _COMPARE[e.op](lv, rv)


def _in_mask(t: torch.Tensor, values) -> torch.Tensor:
    """``t IN (values)`` for a numeric tensor: the OR of SQL ``=``."""
    if all(sql_compare.supported(t.dtype, v) for v in values):
        return sql_compare.in_mask(t, values)
    vs = torch.tensor(sorted(int(v) for v in values), dtype=torch.int64,
                      device=t.device)
    return ops.isin_sorted(t.to(torch.int64), vs)


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
