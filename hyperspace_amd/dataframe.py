"""User-facing DataFrame: a logical plan + session.

Mirrors the subset of the Spark DataFrame surface that Hyperspace's API
touches: filter / select / join / group_by / agg / distinct / collect,
plus plan access for
createIndex, explain and whyNot.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Union

from .exceptions import HyperspaceException
from .plan.expr import AggExpr, Col, Expr, col as _col, parse_predicate
from .plan.nodes import Aggregate, Filter, Join, LogicalPlan, Project


class DataFrame:
    def __init__(self, session, plan: LogicalPlan):
        self.session = session
        self.plan = plan

    # -- transforms -------------------------------------------------------
    def filter(self, condition: Union[str, Expr]) -> "DataFrame":
        if isinstance(condition, str):
            condition = parse_predicate(condition)
        condition = _bind_decimal_literals(condition, self.plan)
        return DataFrame(self.session, Filter(condition, self.plan))

    where = filter

    def select(self, *columns: str) -> "DataFrame":
        cols = list(columns)
        return DataFrame(self.session, Project(cols, self.plan))

    def join(self, other: "DataFrame", on: Union[str, Expr, List[str]],
             how: str = "inner") -> "DataFrame":
        """Equi-join with ``other``.

        ``how`` is one of (case-insensitive):
        ``inner``; ``left`` / ``left_outer`` / ``leftouter``;
        ``right`` / ``right_outer`` / ``rightouter``;
        ``full`` / ``outer`` / ``full_outer`` / ``fullouter``;
        ``semi`` / ``left_semi`` / ``leftsemi``;
        ``anti`` / ``left_anti`` / ``leftanti``.
        Outer joins null-extend the unmatched side; semi and anti return
        only this frame's columns.  Null join keys never match."""
        if isinstance(on, str):
            on = [on]
        if isinstance(on, list):
            expr: Optional[Expr] = None
            for name in on:
                e = _col(name) == _col(name)
                expr = e if expr is None else (expr & e)
            condition = expr
        else:
            condition = on
        assert condition is not None
        return DataFrame(self.session,
                         Join(self.plan, other.plan, condition, how))

    def group_by(self, *cols: Union[str, Col]) -> "GroupedData":
        """Group by columns; finish with ``.agg(...)`` or ``.count()``.
        Null keys compare equal and form one group.  Grouping on float
        columns is refused when the query runs."""
        return GroupedData(self, _resolve_columns(self.plan, cols))

    groupBy = group_by

    def agg(self, *aggs: Union[AggExpr, Dict[str, str]]) -> "DataFrame":
        """Global aggregate (no keys): exactly one row, also on empty
        input, where counts are 0 and every other aggregate is null."""
        return GroupedData(self, []).agg(*aggs)

    def distinct(self) -> "DataFrame":
        """Distinct rows: an aggregate over all output columns with no
        aggregate expressions."""
        return DataFrame(self.session, Aggregate(
            self.plan.output_columns(), [], self.plan))

    # -- actions ----------------------------------------------------------
    def optimized_plan(self) -> LogicalPlan:
        """Apply the Hyperspace rewrite rules if enabled."""
        if self.session.is_hyperspace_enabled():
            from .rules.apply_hyperspace import ApplyHyperspace
            return ApplyHyperspace(self.session).apply(self.plan)
        return self.plan

    def collect(self):
        from .execution.executor import Executor
        ex = Executor(self.session)
        batch = ex.execute(self.optimized_plan())
        self._last_stats = ex.stats
        return batch

    def count(self) -> int:
        return self.collect().num_rows

    def to_pandas(self):
        import pandas as pd
        return pd.DataFrame(self.collect().to_numpy())

    def explain_plan(self) -> str:
        return self.optimized_plan().pretty()

    def __repr__(self):
        return f"DataFrame:\n{self.plan.pretty()}"


class GroupedData:
    """``df.group_by(...)``: holds the grouping columns until ``agg``."""

    def __init__(self, df: DataFrame, group_cols: List[str]):
        self._df = df
        self._group_cols = group_cols

    def agg(self, *aggs: Union[AggExpr, Dict[str, str]]) -> DataFrame:
        """Aggregate each group.  Takes ``AggExpr`` objects from
        ``hyperspace_amd.functions`` or the pyspark dict form
        ``{"column": "function"}`` (``{"*": "count"}`` counts rows).
        Output: the grouping columns, then one column per aggregate, in
        unspecified row order."""
        exprs: List[AggExpr] = []
        for a in aggs:
            if isinstance(a, dict):
                exprs.extend(AggExpr(f, c) for c, f in a.items())
            elif isinstance(a, AggExpr):
                exprs.append(a)
            else:
                raise HyperspaceException(
                    f"agg() takes AggExpr objects or a dict, got {a!r}")
        if not exprs:
            raise HyperspaceException("agg() needs at least one aggregate")
        plan = self._df.plan
        resolved = [
            e if e.column is None
            else e.with_column(_resolve_columns(plan, [e.column])[0])
            for e in exprs]
        seen = set()
        for name in self._group_cols + [e.output_name for e in resolved]:
            if name.lower() in seen:
                raise HyperspaceException(
                    f"Duplicate output column {name!r} in aggregate")
            seen.add(name.lower())
        return DataFrame(self._df.session,
                         Aggregate(self._group_cols, resolved, plan))

    def count(self) -> DataFrame:
        return self.agg(AggExpr("count"))


def _resolve_columns(plan: LogicalPlan, cols) -> List[str]:
    """Names as the plan spells them (matched case-insensitively)."""
    have = {c.lower(): c for c in plan.output_columns()}
    out = []
    for c in cols:
        name = c.name if isinstance(c, Col) else c
        if not isinstance(name, str) or name.lower() not in have:
            raise HyperspaceException(
                f"No column {name!r}; have {plan.output_columns()}")
        out.append(have[name.lower()])
    return out


def _bind_decimal_literals(cond: Expr, plan: LogicalPlan) -> Expr:
    """Scale numeric literals compared against decimal(p,s) columns to
    the column's unscaled-int64 representation (decimals ingest as
    unscaled integers with the scale recorded in the schema; Spark's
    analyzer performs the same literal cast)."""
    import decimal as _dec
    from .plan.expr import And, Arith, BinComp, Col, In, Lit, Not, Or
    scales = {}
    for leaf in plan.collect_leaves():
        rel = getattr(leaf, "relation", None)
        if rel is None:
            continue
        try:
            fields = rel.schema.fields
        except Exception:  # noqa: BLE001
            continue
        for f in fields:
            t = f.type or ""
            if t.startswith("decimal("):
                try:
                    scales[f.name.lower()] = int(
                        t[len("decimal("):-1].split(",")[1])
                except (IndexError, ValueError):
                    pass
    if not scales:
        return cond

    def col_scale(e):
        if isinstance(e, Col):
            return scales.get(e.name.lower())
        if isinstance(e, Arith):
            return col_scale(e.left) if col_scale(e.left) is not None \
                else col_scale(e.right)
        return None

    def scale_value(v, s):
        return int(_dec.Decimal(str(v)).scaleb(s))

    def walk(e):
        if isinstance(e, And):
            return And(walk(e.left), walk(e.right))
        if isinstance(e, Or):
            return Or(walk(e.left), walk(e.right))
        if isinstance(e, Not):
            return Not(walk(e.child))
        if isinstance(e, BinComp) and isinstance(e.right, Lit):
            s = col_scale(e.left)
            if s is not None and isinstance(
                    e.right.value, (int, float, _dec.Decimal)):
                return BinComp(e.op, e.left,
                               Lit(scale_value(e.right.value, s)))
        if isinstance(e, In):
            s = col_scale(e.col)
            if s is not None:
                return In(e.col, [
                    scale_value(v, s)
                    if isinstance(v, (int, float, _dec.Decimal)) else v
                    for v in e.values])
        return e

    return walk(cond)
