"""Expression tree for filters and join conditions.

The engine's analog of Catalyst expressions — only what the rule layer
needs: column refs, literals, comparisons, boolean connectives, IN.
"""

from __future__ import annotations

import re
from typing import Any, List, Set, Union

from ..exceptions import HyperspaceException


class Expr:
    def references(self) -> Set[str]:
        raise NotImplementedError

    # sugar so users can write col("a") == 1
    def __and__(self, other):
        return And(self, _wrap(other))

    def __or__(self, other):
        return Or(self, _wrap(other))

    def __invert__(self):
        return Not(self)

    # arithmetic sugar: (col("a") % 10) == 3 — scalar expressions the
    # data-skipping sketches can bind to (reference ExpressionUtils
    # accepts arbitrary deterministic scalar expressions)
    def __add__(self, other):
        return Arith("+", self, _wrap(other))

    def __sub__(self, other):
        return Arith("-", self, _wrap(other))

    def __mul__(self, other):
        return Arith("*", self, _wrap(other))

    def __mod__(self, other):
        return Arith("%", self, _wrap(other))

    def __truediv__(self, other):
        return Arith("/", self, _wrap(other))

    def isin(self, values):
        return In(self, list(values))


class Col(Expr):
    def __init__(self, name: str):
        self.name = name

    def references(self):
        return {self.name}

    def __eq__(self, other):  # type: ignore[override]
        return BinComp("=", self, _wrap(other))

    def __ne__(self, other):  # type: ignore[override]
        return BinComp("!=", self, _wrap(other))

    def __lt__(self, other):
        return BinComp("<", self, _wrap(other))

    def __le__(self, other):
        return BinComp("<=", self, _wrap(other))

    def __gt__(self, other):
        return BinComp(">", self, _wrap(other))

    def __ge__(self, other):
        return BinComp(">=", self, _wrap(other))

    def is_not_null(self):
        return IsNotNull(self)

    def is_null(self):
        return IsNull(self)

    # sort orders (Spark: ASC is NULLS FIRST, DESC is NULLS LAST)
    def asc(self):
        return SortOrder(self.name, True)

    def desc(self):
        return SortOrder(self.name, False)

    def asc_nulls_last(self):
        return SortOrder(self.name, True, False)

    def desc_nulls_first(self):
        return SortOrder(self.name, False, True)

    def __hash__(self):
        return hash(("Col", self.name.lower()))

    def __repr__(self):
        return self.name


class Lit(Expr):
    def __init__(self, value: Any):
        self.value = value

    def references(self):
        return set()

    def __repr__(self):
        return repr(self.value)


class BinComp(Expr):
    """left <op> right with op in =, !=, <, <=, >, >=."""

    OPS = ("=", "!=", "<", "<=", ">", ">=")

    def __init__(self, op: str, left: Expr, right: Expr):
        if op not in self.OPS:
            raise HyperspaceException(f"Bad comparison op {op}")
        self.op = op
        self.left = left
        self.right = right

    def references(self):
        return self.left.references() | self.right.references()

    def __repr__(self):
        return f"({self.left!r} {self.op} {self.right!r})"


class Arith(Expr):
    """Scalar arithmetic over columns/literals: +, -, *, %, /.

    ``%`` follows Java/Spark remainder semantics (sign of the dividend).
    Comparisons on an Arith left-hand side evaluate it per row; the
    data-skipping sketches match predicates whose LHS is structurally
    equal to the sketch's expression."""

    OPS = ("+", "-", "*", "%", "/")

    def __init__(self, op: str, left: Expr, right: Expr):
        if op not in self.OPS:
            raise HyperspaceException(f"Bad arithmetic op {op}")
        self.op = op
        self.left = left
        self.right = right

    def references(self):
        return self.left.references() | self.right.references()

    def __eq__(self, other):  # type: ignore[override]
        if isinstance(other, Arith):
            # structural equality when both sides are expression trees
            # (sketch matching); comparison against anything else builds
            # a predicate like Col.__eq__ does
            return (self.op == other.op and
                    _expr_eq(self.left, other.left) and
                    _expr_eq(self.right, other.right))
        return BinComp("=", self, _wrap(other))

    def __ne__(self, other):  # type: ignore[override]
        return BinComp("!=", self, _wrap(other))

    def __lt__(self, other):
        return BinComp("<", self, _wrap(other))

    def __le__(self, other):
        return BinComp("<=", self, _wrap(other))

    def __gt__(self, other):
        return BinComp(">", self, _wrap(other))

    def __ge__(self, other):
        return BinComp(">=", self, _wrap(other))

    def __hash__(self):
        return hash(("Arith", self.op, repr(self)))

    def __repr__(self):
        return f"({self.left!r} {self.op} {self.right!r})"


def _expr_eq(a: "Expr", b: "Expr") -> bool:
    """Structural expression equality (case-insensitive column names)."""
    if isinstance(a, Col) and isinstance(b, Col):
        return a.name.lower() == b.name.lower()
    if isinstance(a, Lit) and isinstance(b, Lit):
        return a.value == b.value
    if isinstance(a, Arith) and isinstance(b, Arith):
        return (a.op == b.op and _expr_eq(a.left, b.left) and
                _expr_eq(a.right, b.right))
    return False


class And(Expr):
    def __init__(self, left: Expr, right: Expr):
        self.left, self.right = left, right

    def references(self):
        return self.left.references() | self.right.references()

    def __repr__(self):
        return f"({self.left!r} AND {self.right!r})"


class Or(Expr):
    def __init__(self, left: Expr, right: Expr):
        self.left, self.right = left, right

    def references(self):
        return self.left.references() | self.right.references()

    def __repr__(self):
        return f"({self.left!r} OR {self.right!r})"


class Not(Expr):
    def __init__(self, child: Expr):
        self.child = child

    def references(self):
        return self.child.references()

    def __repr__(self):
        return f"(NOT {self.child!r})"


class In(Expr):
    def __init__(self, col: Expr, values: List[Any]):
        self.col = col
        self.values = values

    def references(self):
        return self.col.references()

    def __repr__(self):
        return f"({self.col!r} IN {self.values!r})"


class IsNotNull(Expr):
    def __init__(self, col: Expr):
        self.col = col

    def references(self):
        return self.col.references()

    def __repr__(self):
        return f"({self.col!r} IS NOT NULL)"


class IsNull(Expr):
    def __init__(self, col: Expr):
        self.col = col

    def references(self):
        return self.col.references()

    def __repr__(self):
        return f"({self.col!r} IS NULL)"


AGG_FUNCS = ("count", "sum", "min", "max", "avg")


class AggExpr:
    """One aggregate of a group-by: ``func`` over ``column`` (None only
    for ``count()``, the row count), named ``alias`` in the output.
    Built by ``hyperspace_amd.functions``; not a row-level ``Expr``."""

    def __init__(self, func: str, column: "Union[str, Col, None]" = None,
                 alias: "Union[str, None]" = None):
        key = func.strip().lower() if isinstance(func, str) else None
        if key not in AGG_FUNCS:
            raise HyperspaceException(
                f"Unknown aggregate function {func!r}; expected one of "
                f"{list(AGG_FUNCS)}")
        if isinstance(column, Col):
            column = column.name
        if column in ("*", 1):
            column = None
        if column is None and key != "count":
            raise HyperspaceException(f"{key}() needs a column")
        self.func = key
        self.column = column
        self.alias_name = alias

    def alias(self, name: str) -> "AggExpr":
        return AggExpr(self.func, self.column, name)

    @property
    def default_name(self) -> str:
        return f"{self.func}({self.column if self.column is not None else 1})"

    @property
    def output_name(self) -> str:
        return self.alias_name or self.default_name

    def references(self) -> Set[str]:
        return set() if self.column is None else {self.column}

    def with_column(self, column: str) -> "AggExpr":
        return AggExpr(self.func, column, self.alias_name)

    def __repr__(self):
        if self.alias_name:
            return f"{self.default_name} AS {self.alias_name}"
        return self.default_name


class SortOrder:
    """One ORDER BY term: ``column`` ascending or descending, nulls first
    or last.  ``nulls_first=None`` takes Spark's default: first for ASC,
    last for DESC.  Built by ``Col.asc()`` / ``Col.desc()`` and the
    ``hyperspace_amd.functions`` helpers; not a row-level ``Expr``."""

    def __init__(self, column: "Union[str, Col]", ascending: bool = True,
                 nulls_first: "Union[bool, None]" = None):
        if isinstance(column, Col):
            column = column.name
        if not isinstance(column, str):
            raise HyperspaceException(
                f"SortOrder needs a column name, got {column!r}")
        self.column = column
        self.ascending = bool(ascending)
        self.nulls_first = self.ascending if nulls_first is None \
            else bool(nulls_first)

    def with_column(self, column: str) -> "SortOrder":
        return SortOrder(column, self.ascending, self.nulls_first)

    def references(self) -> Set[str]:
        return {self.column}

    def __repr__(self):
        return (f"{self.column} {'ASC' if self.ascending else 'DESC'} "
                f"NULLS {'FIRST' if self.nulls_first else 'LAST'}")


def col(name: str) -> Col:
    return Col(name)


def lit(value: Any) -> Lit:
    return Lit(value)


def _wrap(v: Union[Expr, Any]) -> Expr:
    return v if isinstance(v, Expr) else Lit(v)


# ---------------------------------------------------------------------------
# Helpers used by the rules
# ---------------------------------------------------------------------------

def split_conjunctive(e: Expr) -> List[Expr]:
    """Flatten nested ANDs into a predicate list (CNF top level)."""
    if isinstance(e, And):
        return split_conjunctive(e.left) + split_conjunctive(e.right)
    return [e]


def extract_equi_join_keys(e: Expr) -> List[tuple]:
    """For a join condition that is a CNF of Col = Col, return
    [(left_name, right_name)] or [] if not an equi-join
    (reference: JoinIndexRule CNF check, index/covering/JoinIndexRule.scala).
    """
    pairs = []
    for p in split_conjunctive(e):
        if isinstance(p, BinComp) and p.op == "=" and \
                isinstance(p.left, Col) and isinstance(p.right, Col):
            pairs.append((p.left.name, p.right.name))
        else:
            return []
    return pairs


_PRED_RE = re.compile(
    r"^\s*([A-Za-z_][A-Za-z0-9_.]*)\s*(=|==|!=|<=|>=|<|>)\s*(.+?)\s*$")
_IN_RE = re.compile(
    r"^\s*([A-Za-z_][A-Za-z0-9_.]*)\s+(?:in|IN)\s*\(([^)]*)\)\s*$")
_NULL_RE = re.compile(
    r"^\s*([A-Za-z_][A-Za-z0-9_.]*)\s+(?:is|IS)\s+"
    r"(?:(not|NOT)\s+)?(?:null|NULL)\s*$")


def _parse_literal(val: str) -> Any:
    if val.startswith("'") or val.startswith('"'):
        return val.strip("'\"")
    try:
        return int(val)
    except ValueError:
        return float(val)


def parse_predicate(s: str) -> Expr:
    """Tiny predicate parser: 'col <op> literal', 'col IN (v, ...)',
    'col IS [NOT] NULL', joined by AND."""
    parts = re.split(r"\s+(?:AND|and)\s+(?![^(]*\))", s)
    exprs: List[Expr] = []
    for part in parts:
        m = _IN_RE.match(part)
        if m:
            name, vals = m.groups()
            exprs.append(In(Col(name),
                            [_parse_literal(v.strip())
                             for v in vals.split(",") if v.strip()]))
            continue
        m = _NULL_RE.match(part)
        if m:
            name, neg = m.groups()
            exprs.append(IsNotNull(Col(name)) if neg
                         else IsNull(Col(name)))
            continue
        m = _PRED_RE.match(part)
        if not m:
            raise HyperspaceException(f"Cannot parse predicate: {part}")
        name, op, val = m.groups()
        if op == "==":
            op = "="
        exprs.append(BinComp(op, Col(name), Lit(_parse_literal(val))))
    out = exprs[0]
    for e in exprs[1:]:
        out = And(out, e)
    return out
