"""Aggregate functions for ``DataFrame.agg`` / ``GroupedData.agg`` and
sort orders for ``DataFrame.order_by``.

    from hyperspace_amd import functions as F
    df.group_by("k").agg(F.sum("a").alias("total"), F.count())

Each call builds an ``AggExpr``.  Semantics follow Spark with ANSI mode
off: nulls are ignored by every aggregate except ``count()``; a group whose
inputs are all null yields null for sum, min, max and avg, and 0 for
``count(col)``.
"""

from __future__ import annotations

from typing import Optional, Union

from .plan.expr import AggExpr, Col, SortOrder

__all__ = ["count", "sum", "min", "max", "avg",
           "asc", "desc", "asc_nulls_last", "desc_nulls_first"]

_ColLike = Union[str, Col]


def count(col: Optional[_ColLike] = None) -> AggExpr:
    """``count()`` counts rows; ``count(col)`` counts non-null values."""
    return AggExpr("count", col)


def sum(col: _ColLike) -> AggExpr:  # noqa: A001 - pyspark's name
    """Sum: int64 with wrap-around over integer (and decimal, as unscaled
    int64) columns, float64 over float columns."""
    return AggExpr("sum", col)


def min(col: _ColLike) -> AggExpr:  # noqa: A001
    """Minimum, in the input type; strings compare lexicographically and
    floats in sort order (-0.0 < +0.0, NaN outermost)."""
    return AggExpr("min", col)


def max(col: _ColLike) -> AggExpr:  # noqa: A001
    """Maximum; see ``min``."""
    return AggExpr("max", col)


def avg(col: _ColLike) -> AggExpr:
    """Average as float64: sum divided by count.  For a decimal column
    this is the average of the UNSCALED integer values (the scale stays in
    the schema and is not applied)."""
    return AggExpr("avg", col)


def asc(col: _ColLike) -> SortOrder:
    """Ascending, nulls first (Spark's default for ASC)."""
    return SortOrder(col, True)


def desc(col: _ColLike) -> SortOrder:
    """Descending, nulls last (Spark's default for DESC)."""
    return SortOrder(col, False)


def asc_nulls_last(col: _ColLike) -> SortOrder:
    return SortOrder(col, True, False)


def desc_nulls_first(col: _ColLike) -> SortOrder:
    return SortOrder(col, False, True)
