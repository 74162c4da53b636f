"""SQL comparison of a numeric column with a numeric literal.

Spark's rules, lowered to integer bounds so that one answer serves every
physical path (select_range fast path, boolean-mask path, bucket prune):

* float / double: every NaN equals every NaN and is greater than every
  other value, +inf included; -0.0 = 0.0.  A float32 column is promoted
  to double before it meets the literal.
* integer column: the comparison is mathematically exact whatever the
  column width — a fractional literal, one outside the column's type or
  outside int64 lowers to integer bounds inside the type (``qty < 2.5``
  is ``qty <= 2``; ``qty = 2.5`` matches nothing).

Bounds live in "s-space": the signed int64 whose order is the SQL order
of the column.  For an integer column that is the value itself; for a
float column it is ``ops.sql_key(col) ^ SIGN``.  ``s ^ SIGN`` is the
int64-encoded u64 key select_range_u64 compares.
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from .. import ops

SIGN = -0x8000000000000000
S_MIN = -0x8000000000000000
S_MAX = 0x7FFFFFFFFFFFFFFF

INT_RANGE = {torch.int8: (-(1 << 7), (1 << 7) - 1),
             torch.int16: (-(1 << 15), (1 << 15) - 1),
             torch.int32: (-(1 << 31), (1 << 31) - 1),
             torch.int64: (S_MIN, S_MAX)}
FLOAT_DTYPES = (torch.float32, torch.float64)

NONE = ("none",)
ALL = ("all",)


def supported(dtype: torch.dtype, value) -> bool:
    return (dtype in INT_RANGE or dtype in FLOAT_DTYPES) and \
        isinstance(value, (int, float))


def float_s(value: float) -> int:
    """s-space image of a double (zeros and NaNs canonical)."""
    key = int(ops.cpu_ref.sql_key(
        torch.tensor([value], dtype=torch.float64))[0])
    return key ^ SIGN


def _float_neighbours(value) -> Tuple[float, float]:
    """(largest double <= value, smallest double >= value), exactly."""
    if isinstance(value, float):
        return value, value
    try:
        f = float(value)
    except OverflowError:
        f = math.inf if value > 0 else -math.inf
    if f == value:
        return f, f
    if f > value:
        return math.nextafter(f, -math.inf), f
    return f, math.nextafter(f, math.inf)


def lower(dtype: torch.dtype, op: str, value):
    """``col <op> value`` as NONE, ALL, ("range", s_lo, s_hi) (closed) or
    ("ne", s).  ALL / "ne" speak of non-null rows only."""
    if dtype in INT_RANGE:
        mn, mx = INT_RANGE[dtype]
        if isinstance(value, float) and math.isnan(value):
            # NaN is above every value
            return ALL if op in ("<", "<=", "!=") else NONE
        if isinstance(value, float) and math.isinf(value):
            fl = ce = mx + 1 if value > 0 else mn - 1
            exact = False
        else:
            fl, ce = math.floor(value), math.ceil(value)
            exact = fl == ce
        point = exact and mn <= fl <= mx
        if op == "=":
            return ("range", fl, fl) if point else NONE
        if op == "!=":
            return ("ne", fl) if point else ALL
        if op in ("<", "<="):
            hi = ce - 1 if op == "<" else fl
            return NONE if hi < mn else ("range", mn, min(hi, mx))
        lo = fl + 1 if op == ">" else ce
        return NONE if lo > mx else ("range", max(lo, mn), mx)
    down, up = _float_neighbours(value)
    exact = down == up or (down != down)      # NaN literal is a point
    if op == "=":
        return ("range", float_s(down), float_s(down)) if exact else NONE
    if op == "!=":
        return ("ne", float_s(down)) if exact else ALL
    if op in ("<", "<="):
        hi = float_s(down) - (1 if exact and op == "<" else 0)
        return NONE if hi < S_MIN else ("range", S_MIN, hi)
    lo = float_s(up) + (1 if exact and op == ">" else 0)
    return NONE if lo > S_MAX else ("range", lo, S_MAX)


def s_values(t: torch.Tensor) -> torch.Tensor:
    """s-space image of a column: the column itself for integers."""
    if t.dtype in INT_RANGE:
        return t
    return ops.sql_key(t) ^ SIGN


def literal_mask(t: torch.Tensor, op: str, value) -> torch.Tensor:
    """Boolean mask of ``t <op> value`` (validity is the caller's)."""
    spec = lower(t.dtype, op, value)
    if spec is NONE or spec is ALL:
        return torch.full((t.numel(),), spec is ALL, dtype=torch.bool,
                          device=t.device)
    s = s_values(t)
    if spec[0] == "ne":
        return s != spec[1]
    _, lo, hi = spec
    if lo == hi:
        return s == lo
    floor = INT_RANGE.get(t.dtype, (S_MIN, S_MAX))
    if lo == floor[0]:
        return s <= hi
    if hi == floor[1]:
        return s >= lo
    return (s >= lo) & (s <= hi)


def in_mask(t: torch.Tensor, values) -> torch.Tensor:
    """``t IN (values)``: the OR of ``=`` under the rules above, as one
    sorted-set probe."""
    points = set()
    for v in values:
        spec = lower(t.dtype, "=", v)
        if spec is not NONE:
            points.add(spec[1])
    if not points:
        return torch.zeros(t.numel(), dtype=torch.bool, device=t.device)
    vs = torch.tensor(sorted(points), dtype=torch.int64, device=t.device)
    return ops.isin_sorted(s_values(t).to(torch.int64), vs)


def equality_probe(dtype: torch.dtype, value) -> Optional[torch.Tensor]:
    """One-element tensor of ``dtype`` that hashes to the bucket of every
    row equal to the literal, or None when no value of the type equals
    it (``qty = 2.5``, an out-of-range integer, ``p32 = 1.7``)."""
    if lower(dtype, "=", value) is NONE:
        return None
    if dtype in INT_RANGE:
        return torch.tensor([math.floor(value)], dtype=dtype)
    t = torch.tensor([float(value)], dtype=dtype)
    if dtype == torch.float32 and not math.isnan(float(value)) and \
            float(t[0]) != float(value):
        return None
    return t
