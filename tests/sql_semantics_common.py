"""Shared by the SQL-semantics tests (CPU and GPU): a pure-Python oracle
of Spark's comparison rules over row tuples, the table of special values
in two sizes, and the literal / predicate / join matrices.

The oracle calls nothing from the engine.  Python's mixed int / float
comparison is exact and its signed zeros compare equal, so all it adds is
a total order that puts every NaN above every other value, and SQL's
three-valued logic for nulls (None).  Rows are what pyarrow reads back
from the parquet file that was written; result rows are compared as
multisets of full rows, floats by bit pattern.
"""

import math
import operator
import struct
from collections import Counter

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

import hyperspace_amd as hs
from hyperspace_amd.plan.expr import And, BinComp, Col, In, Lit, Not

# ---------------------------------------------------------------------------
# special values
# ---------------------------------------------------------------------------

NEG_NAN64 = 0xFFF8000000000000      # what x86 produces for 0/0
NEG_NAN32 = 0xFFC00000


def _bits64(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _bits32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


# +0, -0, +NaN, -NaN, payload NaN, +inf, -inf, largest finite, most
# negative finite, smallest normal, a subnormal, 1.5, 1.7, 2.5
F64_BITS = [0x0, 0x8000000000000000, 0x7FF8000000000000, NEG_NAN64,
            0x7FF8000000000123, 0x7FF0000000000000, 0xFFF0000000000000,
            0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, 0x0010000000000000,
            0x1, _bits64(1.5), _bits64(1.7), _bits64(2.5)]
F32_BITS = [0x0, 0x80000000, 0x7FC00000, NEG_NAN32, 0x7FC00123,
            0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000,
            0x1, _bits32(1.5), _bits32(1.7), _bits32(2.5)]
NAN_SLOTS = (2, 3, 4)               # positions of the NaNs above

INT_TYPES = {"i8": (np.int8, pa.int8()), "i16": (np.int16, pa.int16()),
             "i32": (np.int32, pa.int32()), "i64": (np.int64, pa.int64())}


def int_range(name):
    info = np.iinfo(INT_TYPES[name.split("_")[0]][0])
    return int(info.min), int(info.max)


def int_specials(name):
    mn, mx = int_range(name)
    return [mn, mx, -1, 0, 2, 3]


def f64_values(bits=F64_BITS):
    return np.array(bits, dtype=np.uint64).view(np.float64)


def f32_values(bits=F32_BITS):
    return np.array(bits, dtype=np.uint32).view(np.float32)


FLOAT_COLS = ["price", "p32"]
INT_COLS = list(INT_TYPES)
VALUE_COLS = FLOAT_COLS + INT_COLS
ALL_COLS = ["rid"] + [c + s for c in VALUE_COLS for s in ("", "_n")]

N_SPECIAL = 28          # the 14 float specials twice; the 6 ints 4-5 times
N_LARGE = 5000          # crosses every 1,024- and 2,048-row tile boundary


def special_positions(n):
    """Rows of an n-row table that hold the special rows: first, last,
    both sides of every 1,024-row boundary (the 2,048-row ones are among
    them), the rest spread evenly."""
    if n == N_SPECIAL:
        return list(range(n))
    pos = {0, n - 1}
    for b in range(1024, n, 1024):
        pos |= {b - 1, b}
    step = n // (N_SPECIAL + 1)
    i = step // 2
    while len(pos) < N_SPECIAL:
        pos.add(i)
        i += step
    return sorted(pos)


def build_table(n):
    """The special rows dealt into ``n`` rows (``n == N_SPECIAL``: the
    bare special rows).  Column ``c_n`` is the nullable twin of ``c``:
    same values, nulls on a fixed subset of rows that leaves every
    special value non-null at least once."""
    pos = special_positions(n)
    j = np.arange(n)
    fill_f = 3.0 + (j % 997) * 0.125            # exact in float32 too
    fill_i = 4 + j % 97
    special_at = np.full(n, -1)
    special_at[pos] = np.arange(N_SPECIAL)
    sp = special_at >= 0
    # nulls of the twins: every 7th filler row, every special row i with
    # i % 5 == 3 (i and i + 14 never both, so each float special stays)
    null = np.where(sp, special_at % 5 == 3, j % 7 == 0)
    cols = {"rid": pa.array(j, type=pa.int64())}

    def add(name, values, typ):
        cols[name] = pa.array(values, type=typ)
        cols[name + "_n"] = pa.array(values, type=typ, mask=null)

    price = fill_f.copy()
    price[sp] = f64_values()[special_at[sp] % 14]
    add("price", price, pa.float64())
    p32 = fill_f.astype(np.float32)
    p32[sp] = f32_values()[special_at[sp] % 14]
    add("p32", p32, pa.float32())
    for name, (npt, pat) in INT_TYPES.items():
        v = fill_i.astype(npt)
        v[sp] = np.array(int_specials(name), dtype=npt)[special_at[sp] % 6]
        add(name, v, pat)
    return pa.table({c: cols[c] for c in ALL_COLS})


class Bag(Counter):
    """Multiset of rows.  Counts are never zero here, so plain dict
    equality is multiset equality (Counter's own walks both sides in
    Python, element by element)."""
    __eq__ = dict.__eq__
    __ne__ = dict.__ne__
    __hash__ = None


def record_bytes(table, columns):
    """One bytes object per row of an arrow table: for each column its
    validity byte and its value (zero under a null) as an int64 or as
    the bits of a double, whatever width the column has: what matters is
    the value, as with Python ints and floats.  Equal bytes <=> equal
    rows with floats compared by bit pattern."""
    if table.num_rows == 0:
        return []
    arrays = []
    for c in columns:
        col = table.column(c).combine_chunks()
        arrays.append(np.asarray(col.is_valid()))
        vals = col.fill_null(0).to_numpy(zero_copy_only=False)
        if vals.dtype.kind == "f":
            vals = vals.astype(np.float64).view(np.uint64)
        arrays.append(vals.astype(np.int64) if vals.dtype.kind in "iub"
                      else vals)
    rec = np.rec.fromarrays(arrays)
    raw, size = rec.tobytes(), rec.dtype.itemsize
    return [raw[i:i + size] for i in range(0, len(raw), size)]


class Source:
    """A written parquet file as pyarrow reads it back: ``rows`` are
    tuples of Python ints / floats / None for the oracle to judge,
    ``keys`` the same rows as bytes for comparing results."""

    def __init__(self, table, directory, name="part-0.parquet"):
        directory.mkdir(parents=True, exist_ok=True)
        path = str(directory / name)
        # no dictionary pages: a dictionary may merge NaN payloads
        pq.write_table(table, path, use_dictionary=False)
        back = pq.read_table(path)
        self.names = back.column_names
        self.columns = {c: back.column(c).to_pylist() for c in self.names}
        self.rows = list(zip(*self.columns.values()))
        self.keys = np.array(record_bytes(back, self.names), dtype=object)
        self.null_key = bytes(len(self.keys[0]))
        self._dicts = None
        self._value_keys = {}

    def dicts(self):
        if self._dicts is None:
            self._dicts = [dict(zip(self.names, r)) for r in self.rows]
        return self._dicts

    def distinct(self, col):
        """(distinct values of a column by bit pattern, index of each
        row's value among them)."""
        if col not in self._value_keys:
            seen, values, codes = {}, [], []
            for v in self.columns[col]:
                k = row_key((v,))
                if k not in seen:
                    seen[k] = len(values)
                    values.append(v)
                codes.append(seen[k])
            self._value_keys[col] = (values, np.array(codes))
        return self._value_keys[col]

    def __len__(self):
        return len(self.rows)


# ---------------------------------------------------------------------------
# oracle
# ---------------------------------------------------------------------------

def total(v):
    """Total-order key: every NaN is one value above all others."""
    return (1, 0) if isinstance(v, float) and v != v else (0, v)


_OPS = {"=": operator.eq, "!=": operator.ne, "<": operator.lt,
        "<=": operator.le, ">": operator.gt, ">=": operator.ge}


def sql_compare(op, a, b):
    """a <op> b under SQL rules; None (unknown) if either is null."""
    if a is None or b is None:
        return None
    return _OPS[op](total(a), total(b))


def row_key(row):
    """Row tuple with floats replaced by their bit pattern."""
    return tuple(struct.pack("<d", v) if isinstance(v, float) else v
                 for v in row)


def rows_counter(rows):
    return Counter(row_key(r) for r in rows)


class Pred:
    """A predicate as both an engine expression and an oracle function
    ``row dict -> True / False / None``."""

    def __init__(self, expr, fn, label, col=None):
        # col: the one column the answer depends on, if there is one
        self.expr, self.fn, self.label, self.col = expr, fn, label, col

    def __repr__(self):
        return self.label


def cmp_pred(col, op, lit):
    return Pred(BinComp(op, Col(col), Lit(lit)),
                lambda r: sql_compare(op, r[col], lit),
                f"{col} {op} {lit!r}", col)


def _in(value, lits):
    if value is None:
        return None
    return any(sql_compare("=", value, x) for x in lits)


def in_pred(col, lits):
    return Pred(In(Col(col), list(lits)), lambda r: _in(r[col], lits),
                f"{col} IN {list(lits)!r}", col)


def arith_in_pred(expr, value_fn, lits, label):
    """``<arithmetic over columns> IN (lits)``; ``value_fn(row)`` is the
    left side's value in Python (None when an input is null)."""
    return Pred(In(expr, list(lits)), lambda r: _in(value_fn(r), lits),
                f"{label} IN {list(lits)!r}")


def not_pred(p):
    def fn(r):
        v = p.fn(r)
        return None if v is None else not v
    return Pred(Not(p.expr), fn, f"NOT ({p.label})", p.col)


def and_pred(p, q):
    def fn(r):
        a, b = p.fn(r), q.fn(r)
        if a is False or b is False:
            return False
        return None if a is None or b is None else True
    return Pred(And(p.expr, q.expr), fn, f"({p.label}) AND ({q.label})")


def filter_oracle(src, pred):
    """Multiset of the rows for which the predicate is TRUE.  A
    one-column predicate is judged once per distinct value."""
    if pred.col is None:
        hit = np.array([pred.fn(d) is True for d in src.dicts()])
    else:
        values, codes = src.distinct(pred.col)
        hit = np.array([pred.fn({pred.col: v}) is True
                        for v in values])[codes]
    return Bag(src.keys[hit].tolist())


def _key_of(row, idx):
    """Join key of a row: None if any key field is null."""
    k = tuple(row[i] for i in idx)
    return None if any(v is None for v in k) else tuple(total(v) for v in k)


def join_oracle(lsrc, rsrc, lcols, rcols, how):
    """SQL join of two sources on the key columns ``lcols`` / ``rcols``
    under the rules above.  ``how`` is a canonical join type.  Returns a
    multiset of output rows (left fields then right fields).  Keys are
    matched through a dict of their total-order images: equal and equally
    hashed for 0.0 / -0.0, for 2 / 2.0 and for any two NaNs."""
    lidx = [lsrc.names.index(c) for c in lcols]
    ridx = [rsrc.names.index(c) for c in rcols]
    by_key = {}
    for j, r in enumerate(rsrc.rows):
        k = _key_of(r, ridx)
        if k is not None:
            by_key.setdefault(k, []).append(j)
    rmatched = [False] * len(rsrc)
    out = []
    for i, l in enumerate(lsrc.rows):
        lk = _key_of(l, lidx)
        hits = [] if lk is None else by_key.get(lk, [])
        for j in hits:
            rmatched[j] = True
        if how == "left_semi":
            out += [lsrc.keys[i]] if hits else []
        elif how == "left_anti":
            out += [] if hits else [lsrc.keys[i]]
        else:
            out += [lsrc.keys[i] + rsrc.keys[j] for j in hits]
            if not hits and how in ("left_outer", "full_outer"):
                out.append(lsrc.keys[i] + rsrc.null_key)
    if how in ("right_outer", "full_outer"):
        out += [lsrc.null_key + rsrc.keys[j]
                for j in range(len(rsrc)) if not rmatched[j]]
    return Bag(out)


JOIN_TYPES = ("inner", "left_outer", "right_outer", "full_outer",
              "left_semi", "left_anti")


# ---------------------------------------------------------------------------
# literals
# ---------------------------------------------------------------------------

def float_literals(col):
    """Literals a float column is compared with: every special of both
    widths as a double, and integers (exact, inexact, beyond double)."""
    lits = [float(v) for v in f64_values()]
    if col.startswith("p32"):
        lits += [float(v) for v in f32_values()[[7, 10, 12]]]
    return lits + [0, 1, 2, -1, 2 ** 53 + 1, 10 ** 400, -10 ** 400]


def int_literals(col):
    """Literals an integer column is compared with: its specials, the
    values just outside its type, fractional and out-of-range ones."""
    mn, mx = int_range(col)
    return int_specials(col) + [
        mn - 1, mx + 1, 2.5, -0.5, 2.0, -0.0, 127.5, 3000000000,
        -3000000000, 1e30, -1e30, 10 ** 30, 2 ** 63, -2 ** 63 - 1,
        math.nan, math.inf, -math.inf]


def literals(col):
    return float_literals(col) if col.split("_")[0] in FLOAT_COLS \
        else int_literals(col)


def in_lists(col):
    if col.split("_")[0] in FLOAT_COLS:
        neg_nan = float(f64_values()[3])
        return [[1.5, 2.5], [1, 2], [0.0], [-0.0, math.nan],
                [neg_nan, 1.7, 3], [math.inf, -math.inf, 10 ** 400], []]
    mn, mx = int_range(col)
    return [[2.5], [2, 2.5, 3000000000], [-1, 0.0, 1e30],
            [mn, mx, mx + 1, mn - 1], [math.nan, 3.0], [4, 5, 100], []]


def predicates(col):
    """Every predicate of the matrix for one column (plain or twin)."""
    out = [cmp_pred(col, op, lit) for op in _OPS for lit in literals(col)]
    out += [in_pred(col, lits) for lits in in_lists(col)]
    out += [not_pred(in_pred(col, in_lists(col)[1])),
            not_pred(cmp_pred(col, "=", literals(col)[1])),
            not_pred(cmp_pred(col, "<", 2.5))]
    return out


def arith_predicates(suffix=""):
    """IN over an arithmetic left side, plain (``suffix=""``) or over the
    nullable twins (``"_n"``)."""
    i32, price = "i32" + suffix, "price" + suffix

    def half(r):
        return None if r[i32] is None else r[i32] / 2

    def plus_zero(r):
        return None if r[price] is None else r[price] + 0.0

    return [
        arith_in_pred(Col(i32) / 2, half, [1.0, 1.5, -0.5, 1],
                      f"({i32} / 2)"),
        arith_in_pred(Col(i32) / 2, half, [2 ** 30, -2 ** 30, 0.75],
                      f"({i32} / 2)"),
        arith_in_pred(Col(price) + 0.0, plus_zero,
                      [-0.0, math.nan, 2.5, 2], f"({price} + 0.0)"),
    ]


TAUTOLOGY = cmp_pred("rid", ">=", 0)


# ---------------------------------------------------------------------------
# engine side
# ---------------------------------------------------------------------------

FILTER_MODES = ("plain", "index", "bucketspec_cold", "bucketspec_warm")
NUM_BUCKETS = 8


def new_session(root, device):
    session = hs.HyperspaceSession(device=device)
    session.conf.set(hs.IndexConstants.INDEX_SYSTEM_PATH,
                     str(root / "indexes"))
    session.conf.set(hs.IndexConstants.INDEX_NUM_BUCKETS, NUM_BUCKETS)
    return session


def filter_env(root, device, n):
    """Session over the n-row table with one covering index per value
    column (plain and twin), each led by that column and including every
    other one.  Returns (session, dataframe, rows read back)."""
    rows = Source(build_table(n), root / "data")
    session = new_session(root, device)
    df = session.read_parquet(str(root / "data"))
    h = hs.Hyperspace(session)
    for c in ALL_COLS[1:]:
        h.create_index(df, hs.CoveringIndexConfig(
            f"ix_{c}", [c], [x for x in ALL_COLS if x != c]))
    return session, df, rows


def set_filter_mode(session, mode):
    if mode == "plain":
        session.disable_hyperspace()
    else:
        session.enable_hyperspace()
    session.conf.set(hs.IndexConstants.INDEX_FILTER_RULE_USE_BUCKET_SPEC,
                     mode.startswith("bucketspec"))


def batch_counter(batch, columns):
    """Multiset of a result batch's rows in ``columns`` order."""
    return Bag(record_bytes(batch.to_arrow(), columns))


def run_filter(session, df, pred, mode):
    """(result multiset, physical operators) of one filter query."""
    if mode == "bucketspec_cold":
        session.index_data_cache().clear()
    q = df.filter(pred.expr).select(*ALL_COLS)
    out = q.collect()
    return batch_counter(out, ALL_COLS), q._last_stats.operators


def describe_diff(got, want, limit=3):
    # a row shows as its first column (validity byte + 8 value bytes)
    extra = [k[:9].hex() for k in list((got - want).elements())[:limit]]
    missing = [k[:9].hex() for k in list((want - got).elements())[:limit]]
    return (f"got {sum(got.values())} rows, want {sum(want.values())}; "
            f"extra {extra} missing {missing}")


WAYS = ("fast", "mask", "twin")


def check_filter_column(session, df, rows, col, mode, which=WAYS):
    """Run the whole matrix of one column three ways — "fast": P alone
    (select_range path), "mask": P AND tautology (mask path), "twin": P
    on the nullable twin — and return the list of failures (empty =
    pass)."""
    set_filter_mode(session, mode)
    failures = []
    # the tautology holds on every row (checked), so P AND tautology has
    # P's answer: the oracle judges P once for both
    assert all(TAUTOLOGY.fn(d) is True for d in rows.dicts())
    ways = []
    if "fast" in which:
        ways += [(p, p) for p in predicates(col)]
    if "mask" in which:
        ways += [(and_pred(p, TAUTOLOGY), p) for p in predicates(col)]
    if "twin" in which:
        ways += [(p, p) for p in predicates(col + "_n")]
    wants = {}
    for pred, judged in ways:
        if judged.label not in wants:
            wants[judged.label] = filter_oracle(rows, judged)
        want = wants[judged.label]
        try:
            got, _ops = run_filter(session, df, pred, mode)
        except Exception as e:  # noqa: BLE001 - reported as a failure
            failures.append(f"{pred!r}: raised {type(e).__name__}: {e}")
            continue
        if got != want:
            failures.append(f"{pred!r}: {describe_diff(got, want)}")
    return failures


# ---------------------------------------------------------------------------
# filter cases (shared bodies of the CPU and GPU tests)
# ---------------------------------------------------------------------------

def filter_matrix(env, col, mode, which=WAYS):
    session, df, rows = env
    failures = check_filter_column(session, df, rows, col, mode, which)
    assert not failures, f"{len(failures)} wrong answers:\n" + \
        "\n".join(failures[:12])


def filter_arith_in(env, mode):
    session, df, rows = env
    set_filter_mode(session, mode)
    for pred in arith_predicates() + arith_predicates("_n"):
        got, _ = run_filter(session, df, pred, mode)
        want = filter_oracle(rows, pred)
        assert got == want, f"{pred!r}: {describe_diff(got, want)}"


def _is_nan(v):
    return v != v


# name -> (predicate, mode, filtered column, hand-written truth of the
# predicate for a non-null Python value of that column).  The truth
# functions use IEEE / integer comparisons only, so they check the oracle
# as well as the engine.
ISSUE_TABLE_FILTERS = {
    "price_eq_zero_fast":
        (cmp_pred("price", "=", 0.0), "plain", "price",
         lambda v: v == 0.0),
    "price_eq_zero_mask":
        (and_pred(cmp_pred("price", "=", 0.0), TAUTOLOGY), "plain",
         "price", lambda v: v == 0.0),
    "price_lt_zero":
        (cmp_pred("price", "<", 0.0), "plain", "price",
         lambda v: v < 0.0),
    "price_gt_one_fast":
        (cmp_pred("price", ">", 1.0), "plain", "price",
         lambda v: _is_nan(v) or v > 1.0),
    "price_gt_one_mask":
        (and_pred(cmp_pred("price", ">", 1.0), TAUTOLOGY), "plain",
         "price", lambda v: _is_nan(v) or v > 1.0),
    "price_in_fractions":
        (in_pred("price", [1.5, 2.5]), "plain", "price",
         lambda v: v in (1.5, 2.5)),
    "price_in_integers":
        (in_pred("price", [1, 2]), "plain", "price", lambda v: False),
    "qty_lt_fraction":
        (cmp_pred("i32", "<", 2.5), "plain", "i32", lambda v: v <= 2),
    "qty_eq_fraction":
        (cmp_pred("i32", "=", 2.5), "plain", "i32", lambda v: False),
    "qty_in_fraction":
        (in_pred("i32", [2.5]), "plain", "i32", lambda v: False),
    "qty_lt_beyond_int32":
        (cmp_pred("i32", "<", 3000000000), "plain", "i32",
         lambda v: True),
    "price_eq_zero_bucket_prune":
        (cmp_pred("price", "=", 0.0), "bucketspec_cold", "price",
         lambda v: v == 0.0),
}


def issue_table_filter(env, name):
    session, df, rows = env
    pred, mode, col, truth = ISSUE_TABLE_FILTERS[name]
    by_hand = Bag(k for k, v in zip(rows.keys.tolist(),
                                        rows.columns[col]) if truth(v))
    assert filter_oracle(rows, pred) == by_hand, "oracle is off"
    set_filter_mode(session, mode)
    got, _ = run_filter(session, df, pred, mode)
    assert got == by_hand, f"{pred!r}: {describe_diff(got, by_hand)}"


def equality_prune_reads_one_bucket(env):
    """The bucketspec modes do take the pruned-bucket and cached-slice
    branches (else the matrix would pass without testing them)."""
    session, df, rows = env
    pred = cmp_pred("price", "=", 0.0)
    want = filter_oracle(rows, pred)
    assert sum(want.values()) >= 2          # +0.0 and -0.0 rows
    set_filter_mode(session, "bucketspec_cold")
    session.index_data_cache().clear()
    q = df.filter(pred.expr).select(*ALL_COLS)
    assert batch_counter(q.collect(), ALL_COLS) == want
    assert q._last_stats.bucket_pruned_files > 0
    assert "IndexScan(cached)" not in q._last_stats.operators
    # a range query loads the whole index; the equality then slices it
    set_filter_mode(session, "bucketspec_warm")
    df.filter(cmp_pred("price", ">=", -1.0).expr).select(*ALL_COLS) \
        .collect()
    q = df.filter(pred.expr).select(*ALL_COLS)
    assert batch_counter(q.collect(), ALL_COLS) == want
    assert "IndexScan(cached)" in q._last_stats.operators
    assert q._last_stats.bucket_pruned_files > 0


# ---------------------------------------------------------------------------
# join cases
# ---------------------------------------------------------------------------

L_COLS = ["lid", "f", "g", "k", "k32"]
R_COLS = ["rid2", "f", "g", "k", "w64", "w16", "d64"]
N_LEFT, N_RIGHT = 2300, 2100    # both cross the 1,024 and 2,048 tiles

# name -> (left key columns, right key columns, buckets hash alike,
# index set).  The (k, f) indexes live in an index set of their own: next
# to the (f, k) ones the join rule may pick either pair for either order.
JOIN_KEYS = {
    "f64": (["f"], ["f"], True, 0),
    "f32": (["g"], ["g"], True, 0),
    "f64_k": (["f", "k"], ["f", "k"], True, 0),
    "k_f64": (["k", "f"], ["k", "f"], True, 1),
    "i32_i64": (["k32"], ["w64"], False, 0),
    "i32_i16": (["k32"], ["w16"], True, 0),
    "f32_f64": (["g"], ["d64"], False, 0),
}


def _join_positions(n):
    pos = {0, n - 1}
    for b in range(1024, n, 1024):
        pos |= {b - 1, b}
    i = 37
    while len(pos) < N_SPECIAL:
        pos.add(i)
        i += n // N_SPECIAL
    return sorted(pos)


def _join_side(n, right):
    j = np.arange(n)
    special_at = np.full(n, -1)
    special_at[_join_positions(n)] = np.arange(N_SPECIAL)
    sp = special_at >= 0
    # the right side deals the specials in another order
    slot = (special_at * (3 if right else 1)) % 14
    f = 100.0 + (j % (700 if right else 600)) * 0.5
    g = f.astype(np.float32)
    f[sp] = f64_values()[slot[sp]]
    g[sp] = f32_values()[slot[sp]]
    k = np.where(sp, special_at % 3, j % (4 if right else 5))
    fnull = ~sp & (j % 11 == 5) | sp & (special_at % 9 == 8)
    gnull = ~sp & (j % 13 == 6) | sp & (special_at % 9 == 8)
    knull = j % 17 == 3
    if not right:
        return pa.table({
            "lid": pa.array(j, type=pa.int64()),
            "f": pa.array(f, mask=fnull),
            "g": pa.array(g, mask=gnull),
            "k": pa.array(k, type=pa.int64(), mask=knull),
            "k32": pa.array(j % 500 - 10, type=pa.int32())})
    w = j % 600 - 15
    return pa.table({
        "rid2": pa.array(j, type=pa.int64()),
        "f": pa.array(f, mask=fnull),
        "g": pa.array(g, mask=gnull),
        "k": pa.array(k, type=pa.int64(), mask=knull),
        "w64": pa.array(w, type=pa.int64()),
        "w16": pa.array(w, type=pa.int16()),
        "d64": pa.array(g.astype(np.float64), mask=gnull)})


class JoinEnv:
    def __init__(self, root, device, num_buckets=NUM_BUCKETS):
        self.lsrc = Source(_join_side(N_LEFT, False), root / "left")
        self.rsrc = Source(_join_side(N_RIGHT, True), root / "right")
        self.sets = {}
        done = set()
        for lk, rk, _, group in JOIN_KEYS.values():
            if group not in self.sets:
                session = new_session(root / f"set{group}", device)
                session.conf.set(hs.IndexConstants.INDEX_NUM_BUCKETS,
                                 num_buckets)
                self.sets[group] = (
                    session, session.read_parquet(str(root / "left")),
                    session.read_parquet(str(root / "right")))
            session, left, right = self.sets[group]
            h = hs.Hyperspace(session)
            for side, df, keys, cols in (("l", left, lk, L_COLS),
                                         ("r", right, rk, R_COLS)):
                name = f"jx_{side}_" + "_".join(keys)
                if name not in done:
                    done.add(name)
                    h.create_index(df, hs.CoveringIndexConfig(
                        name, keys, [c for c in cols if c not in keys]))
        self.session, self.left, self.right = self.sets[0]
        self._oracle = {}

    def oracle(self, keys, how):
        if (keys, how) not in self._oracle:
            lk, rk = JOIN_KEYS[keys][:2]
            self._oracle[keys, how] = join_oracle(
                self.lsrc, self.rsrc, lk, rk, how)
        return self._oracle[keys, how]

    def query(self, keys, how, indexed=True):
        lk, rk, _, group = JOIN_KEYS[keys]
        session, left, right = self.sets[group]
        if indexed:
            session.enable_hyperspace()
        else:
            session.disable_hyperspace()
        cond = None
        for a, b in zip(lk, rk):
            e = BinComp("=", Col(a), Col(b))
            cond = e if cond is None else And(cond, e)
        return left.join(right, on=cond, how=how)

    def run(self, keys, how, physical):
        """(result multiset, operators) of one join on one path."""
        q = self.query(keys, how, physical == "co_bucketed")
        out = q.collect()
        names = list(out.columns)
        return batch_counter(out, names), q._last_stats.operators


def join_env(root, device):
    return JoinEnv(root, device)


def join_matrix(env, keys, physical, how):
    got, operators = env.run(keys, how, physical)
    want = env.oracle(keys, how)
    assert got == want, f"{keys} {how} {physical}: " + \
        describe_diff(got, want)
    joins = [o for o in operators if o.startswith("SortMergeJoin")]
    # equal keys of unlike hash kinds sit in different buckets: such a
    # pair must not take the co-bucketed path even when both are indexed
    co = physical == "co_bucketed" and JOIN_KEYS[keys][2]
    assert len(joins) == 1 and \
        joins[0].startswith("SortMergeJoin(co-bucketed" if co
                            else "SortMergeJoin(shuffled"), operators


def join_int_float_key_is_refused(env, physical):
    """An integer key against a float key raises; it never returns the
    silent empty result the unrelated u64 keys would give."""
    import pytest
    from hyperspace_amd.exceptions import HyperspaceException
    if physical == "co_bucketed":
        env.session.enable_hyperspace()
    else:
        env.session.disable_hyperspace()
    for how in JOIN_TYPES:
        with pytest.raises(HyperspaceException, match="join key type"):
            env.left.join(env.right,
                          on=BinComp("=", Col("k32"), Col("d64")),
                          how=how).collect()
        with pytest.raises(HyperspaceException, match="join key type"):
            env.left.join(env.right,
                          on=And(BinComp("=", Col("f"), Col("f")),
                                 BinComp("=", Col("k32"), Col("d64"))),
                          how=how).collect()


ISSUE_TABLE_JOINS = {"f": ["f"], "f_k": ["f", "k"], "k_f": ["k", "f"]}


def issue_table_joins(root, device, name):
    """Left and right hold {0.0, -0.0, NaN, -NaN, 1.5, 2.0}: 10 pairs on
    f; with k as a further key the same pairs in either key order."""
    vals = np.concatenate([f64_values()[[0, 1, 2, 3]], [1.5, 2.0]])
    ks = [0, 0, 1, 1, 2, 2]
    src = {}
    for side, kk in (("left", ks), ("right", ks[::-1])):
        src[side] = Source(pa.table({
            "f": pa.array(vals), "k": pa.array(kk, type=pa.int64()),
            side[0] + "id": pa.array(range(6), type=pa.int64())}),
            root / side)
    session = new_session(root, device)
    left = session.read_parquet(str(root / "left"))
    right = session.read_parquet(str(root / "right"))
    # by hand: zeros x zeros and NaNs x NaNs give 4 pairs each, 1.5 and
    # 2.0 one each.  k is reversed on the right, so with k as a second
    # key only the NaN rows (k = 1 on both sides) still pair up
    want_f = join_oracle(src["left"], src["right"], ["f"], ["f"], "inner")
    assert sum(want_f.values()) == 10
    want_fk = join_oracle(src["left"], src["right"], ["f", "k"],
                          ["f", "k"], "inner")
    assert sum(want_fk.values()) == 4
    on = ISSUE_TABLE_JOINS[name]
    want = want_f if on == ["f"] else want_fk
    out = left.join(right, on=on).collect()
    got = batch_counter(out, ["f", "k", "lid", "f_r", "k_r", "rid"])
    assert got == want, f"join on {on}: {describe_diff(got, want)}"


def _index_scans(plan):
    from hyperspace_amd.plan.nodes import IndexScan
    if isinstance(plan, IndexScan):
        return [plan]
    return [s for c in plan.children for s in _index_scans(c)]


def assert_buckets_sorted(session, plan, key):
    """Every bucket of every bucketed IndexScan under ``plan`` is
    non-decreasing in the canonical key (nulls first): the order the
    merge join relies on.  Checked in Python on the scanned values."""
    from hyperspace_amd.execution.executor import Executor
    scans = [s for s in _index_scans(plan) if s.use_bucket_spec]
    assert scans
    for scan in scans:
        batch, seg = Executor(session)._exec(scan)
        vals = batch.to_arrow().column(key).to_pylist()
        seg = seg.tolist()
        assert seg[-1] == len(vals)
        for b in range(len(seg) - 1):
            run = vals[seg[b]:seg[b + 1]]
            nn = [total(v) for v in run if v is not None]
            assert run[:len(run) - len(nn)] == [None] * (len(run) - len(nn))
            assert all(a <= c for a, c in zip(nn, nn[1:])), \
                f"bucket {b} of {scan.entry.name} is not sorted: {run}"
    return scans


def index_buckets_sorted_by_canonical_key(root, device):
    """One bucket holding -NaN, -0.0 and +0.0: sorted by raw bits, -NaN
    would come first, but its canonical key is the largest.  The build
    sorts by the canonical key and keeps the stored bits."""
    env = JoinEnv(root, device, num_buckets=1)
    env.session.enable_hyperspace()
    for keys in ("f64", "f32"):
        key = JOIN_KEYS[keys][0][0]
        plan = env.query(keys, "inner").optimized_plan()
        scans = assert_buckets_sorted(env.session, plan, key)
        assert len(scans) == 2
        for how in JOIN_TYPES:
            join_matrix(env, keys, "co_bucketed", how)
    # the stored values keep their bits: -NaN, the payload NaN and -0.0
    # all come back from the index as written
    from hyperspace_amd.execution.executor import Executor
    scan = _index_scans(env.query("f64", "inner").optimized_plan())[0]
    batch, _ = Executor(env.session)._exec(scan)
    stored = rows_counter((v,) for v in
                          batch.to_arrow().column("f").to_pylist())
    src = env.lsrc if "lid" in batch.columns else env.rsrc
    assert stored == rows_counter((v,) for v in src.columns["f"])


def one_answer_on_every_physical_path(fenv, jenv):
    """One filter and one join, each on every physical path it can take:
    the answers are identical (and the oracle's)."""
    session, df, rows = fenv
    pred = cmp_pred("price", "=", 0.0)
    want = filter_oracle(rows, pred)
    answers = {}
    set_filter_mode(session, "plain")
    answers["fast"], _ = run_filter(session, df, pred, "plain")
    answers["mask"], _ = run_filter(session, df,
                                    and_pred(pred, TAUTOLOGY), "plain")
    set_filter_mode(session, "index")
    answers["index"], ops_ix = run_filter(session, df, pred, "index")
    assert "IndexScan" in ops_ix
    set_filter_mode(session, "bucketspec_cold")
    answers["pruned bucket"], ops_cold = run_filter(
        session, df, pred, "bucketspec_cold")
    assert "IndexScan(cached)" not in ops_cold
    run_filter(session, df, cmp_pred("price", ">=", -1.0),
               "bucketspec_warm")
    answers["cached slice"], ops_warm = run_filter(
        session, df, pred, "bucketspec_warm")
    assert "IndexScan(cached)" in ops_warm
    for path, got in answers.items():
        assert got == want, f"{path}: {describe_diff(got, want)}"
    for keys in ("f64", "k_f64"):
        co, ops_co = jenv.run(keys, "inner", "co_bucketed")
        sh, ops_sh = jenv.run(keys, "inner", "shuffled")
        assert "SortMergeJoin(co-bucketed)" in ops_co
        assert "SortMergeJoin(shuffled)" in ops_sh
        assert co == sh == jenv.oracle(keys, "inner")


# ---------------------------------------------------------------------------
# op-level pins: float keys hash and key by their canonical bits
# ---------------------------------------------------------------------------

EDGE_SIZES = (1, 255, 256, 257, 1025)


def canonical_bits(bits, width):
    """Expected canonical bit pattern, in plain Python: -0.0 -> +0.0,
    any NaN -> 0x7ff8000000000000 / 0x7fc00000."""
    sign, inf, nan = ((1 << 63, 0x7FF0000000000000, 0x7FF8000000000000)
                      if width == 64 else
                      (1 << 31, 0x7F800000, 0x7FC00000))
    if bits & (sign - 1) > inf:
        return nan
    return 0 if bits == sign else bits


def float_key_column(width, n=None):
    """(float tensor, integer tensor holding each value's expected
    canonical bits).  ``n=None``: the specials once.  Otherwise n values
    with the specials on the first, last and 256 / 1,024-row edges and
    random finite filler between."""
    import torch
    special = F64_BITS if width == 64 else F32_BITS
    ut, it = (np.uint64, np.int64) if width == 64 else (np.uint32, np.int32)
    ft = np.float64 if width == 64 else np.float32
    if n is None:
        bits = np.array(special, dtype=ut)
    else:
        rng = np.random.default_rng(width + n)
        bits = (rng.standard_normal(n) * 1e3).astype(ft).view(ut)
        edges = [i for i in (0, 1, 254, 255, 256, 257, 1022, 1023, 1024,
                             n - 2, n - 1) if 0 <= i < n]
        for j, i in enumerate(sorted(set(edges))):
            bits[i] = special[(j + n) % len(special)]
    want = np.array([canonical_bits(int(b), width) for b in bits], dtype=ut)
    return (torch.from_numpy(bits.view(ft).copy()),
            torch.from_numpy(want.view(it).copy()))


def check_float_hash_pins(bucket):
    """``bucket(keys, num_buckets, masks)`` is the murmur3_bucket under
    test, returning a CPU tensor.  The integer path hashes raw bits, so
    hashing the expected canonical bits as integers is the yardstick."""
    import torch
    for width in (64, 32):
        ft = torch.float64 if width == 64 else torch.float32
        for n in (None,) + EDGE_SIZES:
            f, want = float_key_column(width, n)
            rows = f.numel()
            lead = torch.arange(rows, dtype=torch.int64) * 7 - 3
            mask = torch.arange(rows) % 3 != 1
            for nb in (8, 200):
                assert torch.equal(bucket([f], nb, None),
                                   bucket([want], nb, None))
                assert torch.equal(bucket([lead, f], nb, None),
                                   bucket([lead, want], nb, None))
                assert torch.equal(bucket([f], nb, [mask]),
                                   bucket([want], nb, [mask]))
                assert torch.equal(bucket([lead, f], nb, [None, mask]),
                                   bucket([lead, want], nb, [None, mask]))
        # spelled out: the zeros share a bucket, and so do all NaNs
        f, _ = float_key_column(width)
        canon_nan = f[2:3]
        for nb in (8, 200, 1 << 20):
            assert torch.equal(bucket([torch.tensor([-0.0], dtype=ft)], nb,
                                      None),
                               bucket([torch.tensor([0.0], dtype=ft)], nb,
                                      None))
            for i in NAN_SLOTS:
                assert torch.equal(bucket([f[i:i + 1]], nb, None),
                                   bucket([canon_nan], nb, None))


def check_sql_key_pins(sql_key, normalize_key):
    """sql_key is normalize_key of the canonical value; normalize_key
    itself keeps its order (-0.0 below +0.0)."""
    import torch
    for width in (64, 32):
        for n in (None,) + EDGE_SIZES:
            f, want = float_key_column(width, n)
            canon = want.view(torch.float64 if width == 64
                              else torch.float32)
            assert torch.equal(sql_key(f), normalize_key(canon))
    z = torch.tensor([-0.0, 0.0], dtype=torch.float64)
    nk = normalize_key(z) ^ (-0x8000000000000000)
    assert int(nk[0]) < int(nk[1])
    ints = torch.tensor([-5, 0, 7], dtype=torch.int32)
    assert torch.equal(sql_key(ints), normalize_key(ints))
