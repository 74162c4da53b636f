"""Shared builders for the ORDER BY / LIMIT tests (CPU and GPU): the
top-k input shapes aimed at the kernel's tile size, the brute-force oracles
over Python values, and the ordered-query dataset."""

import decimal
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import torch

import hyperspace_amd as hs

from aggregate_common import sort_key

TILE = 2048  # rows per tile of the device kernels (checked on the GPU)
MAX_BLOCKS = 2048  # grid cap of the device kernels


# ---------------------------------------------------------------------------
# topk_rows: brute force
# ---------------------------------------------------------------------------

def u64_list(t):
    """int64 tensor of u64 bit patterns -> Python ints in [0, 2**64)."""
    return t.numpy().view(np.uint64).tolist()


def from_u64(values):
    return torch.from_numpy(
        np.asarray(values, dtype=np.uint64).view(np.int64).copy())


class BruteTopK:
    """Brute-force topk_rows over Python ints: one sort per input, any
    number of (k, keep_ties) questions."""

    def __init__(self, keys, valid=None):
        self.keys = u64_list(keys)
        ok = [True] * len(self.keys) if valid is None else valid.tolist()
        self.rows = [i for i, v in enumerate(ok) if v]
        self.ordered = sorted(self.keys[i] for i in self.rows)

    @property
    def n_valid(self):
        return len(self.rows)

    def __call__(self, k, keep_ties):
        if k <= 0:
            return []
        if k >= len(self.rows):
            return list(self.rows)
        t = self.ordered[k - 1]
        less = [i for i in self.rows if self.keys[i] < t]
        ties = [i for i in self.rows if self.keys[i] == t]
        if not keep_ties:
            ties = ties[:k - len(less)]
        return sorted(less + ties)


def k_values(n_valid, T=TILE):
    ks = [0, 1, 2, 64, T + 1, n_valid - 1, n_valid, n_valid + 1]
    return sorted(set(ks))


# ---------------------------------------------------------------------------
# topk_rows: shapes
# ---------------------------------------------------------------------------

def _random_u64(n, rng):
    """Distinct full-width keys that include 0 and 2**64 - 1."""
    vals = set([0, 2**64 - 1][:n])
    while len(vals) < n:
        vals.update(int(v) for v in rng.integers(
            0, 2**64, n - len(vals), dtype=np.uint64))
    vals = sorted(vals)
    return from_u64([vals[i] for i in rng.permutation(n)])


def key_patterns():
    """name -> f(n, rng) -> int64 tensor of u64 bit patterns."""
    base = 0x1234_5600_0078_9A00

    def byte_at(shift):
        def f(n, rng):
            d = rng.integers(0, 256, n, dtype=np.uint64)
            return from_u64((np.uint64(base) & ~(np.uint64(0xFF)
                                                << np.uint64(shift)))
                            | (d << np.uint64(shift)))
        return f

    def two_bytes(n, rng):
        # bytes 1 and 5 vary, the three passes in between are skipped
        lo = rng.integers(0, 7, n, dtype=np.uint64) << np.uint64(8)
        hi = rng.integers(0, 5, n, dtype=np.uint64) << np.uint64(40)
        return from_u64(np.uint64(0x7700_0000_0000_0011) | lo | hi)

    return {
        "all_equal": lambda n, rng: from_u64([0xDEAD_BEEF_0000_0001] * n),
        "two_values": lambda n, rng: from_u64(
            np.where(rng.random(n) < 0.5, np.uint64(5),
                     np.uint64(2**63 + 9))),
        "random_u64": _random_u64,
        "low_byte": byte_at(0),
        "high_byte": byte_at(56),
        "two_bytes": two_bytes,
        "ascending": lambda n, rng: from_u64(
            np.arange(n, dtype=np.uint64) * np.uint64(3)),
        "descending": lambda n, rng: from_u64(
            (np.uint64(2**64 - 1)
             - np.arange(n, dtype=np.uint64) * np.uint64(2**40 + 1))),
    }


SIZES = lambda T=TILE: (1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17)


def validity_variants(keys, rng):
    """name -> (keys, valid): the validity shapes of one key column."""
    n = keys.numel()
    out = {"all_valid": (keys, torch.ones(n, dtype=torch.bool)),
           "all_null": (keys, torch.zeros(n, dtype=torch.bool)),
           "fifth_null": (keys, torch.arange(n) % 5 != 2)}
    # null rows store keys below every valid key: must be ignored
    valid = torch.from_numpy(rng.random(n) < 0.6)
    raised = from_u64(
        [k | (1 << 63) if v else k >> 1
         for k, v in zip(u64_list(keys), valid.tolist())])
    out["nulls_hold_small_keys"] = (raised, valid)
    return out


def op_cases(T=TILE):
    """name -> (keys, valid or None)."""
    rng = np.random.default_rng(41)
    cases = {}
    pats = key_patterns()
    for n in SIZES(T):
        for pname, f in pats.items():
            cases[f"{pname}-n={n}"] = (f(n, rng), None)
        for pname in ("random_u64", "two_values", "low_byte"):
            for vname, kv in validity_variants(pats[pname](n, rng),
                                               rng).items():
                cases[f"{pname}-{vname}-n={n}"] = kv
    return cases


def tie_cases(T=TILE):
    """name -> (keys, valid, ks): a tie group at the threshold that
    straddles a tile edge, with the quota ending inside it."""
    cases = {}
    n = 3 * T
    keys = np.full(n, 900, dtype=np.uint64)
    keys[:40] = np.arange(40)            # 40 rows below the ties
    keys[T - 30:T + 30] = 500            # the tie group, across the edge
    keys[2 * T + 5] = 500                # and one more, a tile later
    cases["ties_across_tile_edge"] = (
        from_u64(keys), None, [40, 41, 69, 70, 71, 99, 100, 101, 102])
    m = torch.ones(n, dtype=torch.bool)
    m[T - 3:T + 3] = False               # nulls inside the tie group
    cases["ties_across_tile_edge_nulls"] = (
        from_u64(keys), m, [41, 60, 67, 68, 93, 94, 95, 96])
    return cases


def grid_case(T=TILE):
    """More tiles than blocks, so every block walks two tiles: the tie
    group straddles the border between two blocks' tile ranges and the
    quota ends inside it."""
    n = MAX_BLOCKS * T + T + 5
    rng = np.random.default_rng(43)
    keys = rng.integers(2**20, 2**40, n, dtype=np.uint64)
    edge = 2 * T * 700                   # first row of block 700's range
    keys[edge - 50:edge + 50] = 1000     # ties below every other key ...
    keys[5:n:T * 64] = 7                 # ... except these
    valid = torch.arange(n) % 5 != 2
    return from_u64(keys), valid, edge


# ---------------------------------------------------------------------------
# order keys
# ---------------------------------------------------------------------------

def order_key_columns():
    """name -> column with the values order_key must get right."""
    nan = float("nan")
    inf = float("inf")
    f64 = torch.tensor([1.5, -0.0, 0.0, nan, -inf, inf, -2.0, 5e-324,
                        -5e-324, 3.0], dtype=torch.float64)
    # NaNs with other payloads and signs
    bits = torch.tensor([0x7FF0000000000001, -0x0008000000000000 + 5,
                         0x7FF8000000000123], dtype=torch.int64)
    f64 = torch.cat([f64, bits.view(torch.float64)])
    f32 = torch.tensor([1.5, -0.0, 0.0, nan, -inf, inf, -2.0, 1e-45, 3.0],
                       dtype=torch.float32)
    bits32 = torch.tensor([0x7F800001, -0x00400000 + 7], dtype=torch.int32)
    f32 = torch.cat([f32, bits32.view(torch.float32)])
    out = {"float64": f64, "float32": f32,
           "bool": torch.tensor([True, False, True])}
    for dt in (torch.int8, torch.int16, torch.int32, torch.int64):
        info = torch.iinfo(dt)
        out[str(dt).split(".")[1]] = torch.tensor(
            [info.min, -1, 0, 1, info.max, 17], dtype=dt)
    return out


# ---------------------------------------------------------------------------
# ordered queries
# ---------------------------------------------------------------------------

N_ROWS = 5003
N_FILES = 4
COLUMNS = ["rid", "i", "u", "f", "s", "n32", "d"]


def _table(rows):
    cols = list(zip(*rows)) if rows else [[] for _ in COLUMNS]
    return pa.table({
        "rid": pa.array(cols[0], type=pa.int64()),
        "i": pa.array(cols[1], type=pa.int64()),
        "u": pa.array(cols[2], type=pa.int64()),
        "f": pa.array(cols[3], type=pa.float64()),
        "s": pa.array(cols[4], type=pa.string()),
        "n32": pa.array(cols[5], type=pa.int32()),
        "d": pa.array(cols[6], type=pa.decimal128(10, 2)),
    })


def make_order_rows(n=N_ROWS, seed=11, rid0=0):
    """Row tuples (rid, i, u, f, s, n32, d): rid a unique payload, i with
    duplicates, u unique, f with NaN, both zeros and nulls, s strings
    with nulls, n32 a nullable int32, d a decimal with duplicates."""
    rng = np.random.default_rng(seed)
    specials = [float("nan"), -0.0, 0.0, float("inf"), float("-inf")]
    u = rng.permutation(n) * 7 - 3 * n
    rows = []
    for r in range(n):
        x = rng.random()
        f = None if x < 0.1 else (
            specials[int(rng.integers(0, 5))] if x < 0.3
            else float(rng.integers(-50, 50)) / 4)
        s = None if rng.random() < 0.05 else \
            "".join("abcXY z"[int(c)] for c in rng.integers(
                0, 7, int(rng.integers(0, 4))))
        n32 = None if rng.random() < 0.2 else int(rng.integers(-40, 40))
        d = decimal.Decimal(int(rng.integers(-300, 300))).scaleb(-2)
        rows.append((rid0 + r, int(rng.integers(0, 300)), int(u[r]) + rid0,
                     f, s, n32, d))
    return rows


def write_order_dataset(root, rows, n_files=N_FILES, prefix="part"):
    os.makedirs(root, exist_ok=True)
    per = (len(rows) + n_files - 1) // n_files
    for i in range(n_files):
        pq.write_table(_table(rows[i * per:(i + 1) * per]),
                       os.path.join(root, f"{prefix}-{i}.parquet"))


def order_session(root, device, num_buckets=8):
    """Session over the ordered-query dataset: (session, hyperspace, df,
    data dir)."""
    data = os.path.join(str(root), "data")
    write_order_dataset(data, make_order_rows())
    session = hs.HyperspaceSession(device=device)
    session.conf.set(hs.IndexConstants.INDEX_NUM_BUCKETS, num_buckets)
    return session, hs.Hyperspace(session), session.read_parquet(data), data


def batch_row_list(batch):
    """ColumnBatch -> (names, list of row tuples in row order, nulls as
    None)."""
    table = batch.to_arrow()
    names = table.column_names
    cols = [table.column(n).to_pylist() for n in names]
    return names, list(zip(*cols)) if cols else []


def value_key(v):
    """The engine's comparison over Python values: sql_key order for
    numbers (NaN above everything and equal to itself, -0.0 with +0.0),
    code point order for strings.  Not defined for None."""
    if isinstance(v, str):
        return v
    if isinstance(v, float):
        if v != v:
            return 2**64 - 1
        if v == 0.0:
            v = 0.0
        return sort_key(v)
    if isinstance(v, decimal.Decimal):
        v = int(v.scaleb(2))
    return sort_key(int(v))


def oracle_sort(names, rows, orders):
    """Stable multi-column sort of row tuples by brute force.  orders:
    list of (column, ascending, nulls_first).  LSD over the columns; per
    column the nulls are split off, the rest sorted by value_key (Python's
    sort is stable, also reversed) and the nulls put first or last."""
    out = list(rows)
    for col, asc, nulls_first in reversed(orders):
        ix = [n.lower() for n in names].index(col.lower())
        nulls = [r for r in out if r[ix] is None]
        vals = sorted((r for r in out if r[ix] is not None),
                      key=lambda r: value_key(r[ix]), reverse=not asc)
        out = nulls + vals if nulls_first else vals + nulls
    return out


def order_tuple(names, row, orders):
    """The order columns of a row, floats as their comparison key."""
    low = [n.lower() for n in names]
    return tuple(None if row[low.index(c.lower())] is None
                 else value_key(row[low.index(c.lower())])
                 for c, _, _ in orders)


def to_sort_orders(orders):
    from hyperspace_amd.plan.expr import SortOrder
    return [SortOrder(c, a, nf) for c, a, nf in orders]


DIRECTIONS = [(True, True), (True, False), (False, True), (False, False)]
ORDER_COLUMNS = ["i", "f", "s", "n32", "d"]
MULTI_ORDERS = {
    "i_asc-f_desc": [("i", True, True), ("f", False, False)],
    "s_desc-n32_asc_nulls_last-u_desc": [
        ("s", False, False), ("n32", True, False), ("u", False, False)],
    "n32_desc_nulls_first-d_asc-f_asc_nulls_last": [
        ("n32", False, True), ("d", True, True), ("f", True, False)],
}


def limits(n_rows):
    return [0, 1, 7, n_rows, n_rows + 5]


def check_topk(q, names, scan_rows, orders, n, unique=False, source=None):
    """Run ``q`` (an order_by(...).limit(n) frame, possibly with a select
    between) and hold it against the brute-force sort of ``scan_rows``."""
    out_names, got = batch_row_list(q.collect())
    want = oracle_sort(names, scan_rows, orders)[:n]
    assert len(got) == len(want)
    keep = [[x.lower() for x in names].index(c.lower()) for c in out_names]
    rid_out = [x.lower() for x in out_names].index("rid")
    by_rid = {r[0]: r for r in (source or scan_rows)}
    have_order = all(c.lower() in [x.lower() for x in out_names]
                     for c, _, _ in orders)
    for g, w in zip(got, want):
        # every returned row is an input row
        src = by_rid[g[rid_out]]
        assert _same_row(g, tuple(src[i] for i in keep)), (g, src)
        if have_order:
            assert order_tuple(out_names, g, orders) == \
                order_tuple(names, w, orders), (g, w)
        else:
            assert order_tuple(names, src, orders) == \
                order_tuple(names, w, orders), (g, w)
        if unique:
            assert _same_row(g, tuple(w[i] for i in keep)), (g, w)
    assert len({g[rid_out] for g in got}) == len(got)
    return got


def _same_row(a, b):
    def norm(v):
        if isinstance(v, float):
            return ("f", np.float64(v).view(np.uint64).item()
                    if v == v else "nan")
        if isinstance(v, decimal.Decimal):
            return int(v.scaleb(2))
        return v
    return tuple(norm(x) for x in a) == tuple(norm(x) for x in b)


# ---------------------------------------------------------------------------
# query scenarios (the CPU and GPU test files run the same ones)
# ---------------------------------------------------------------------------

class OrderEnv:
    """The dataset read through one session, and its rows in scan order
    (what a stable sort's ties are held against)."""

    def __init__(self, root, device, num_buckets=8):
        self.session, self.h, self.df, self.data = order_session(
            root, device, num_buckets)
        self.root = str(root)
        self.reload()

    def reload(self):
        self.df = self.session.read_parquet(self.data)
        was = self.session.is_hyperspace_enabled()
        self.session.disable_hyperspace()
        self.names, self.rows = batch_row_list(self.df.collect())
        if was:
            self.session.enable_hyperspace()

    def index(self, name, col):
        self.h.create_index(self.df, hs.CoveringIndexConfig(
            name, [col], [c for c in COLUMNS if c != col]))


def ops_of(q):
    return q._last_stats.operators


def scenario_single_column(env, col, monkeypatch):
    n_rows = len(env.rows)
    for asc, nulls_first in DIRECTIONS:
        orders = [(col, asc, nulls_first)]
        for n in limits(n_rows):
            q = env.df.order_by(*to_sort_orders(orders)).limit(n)
            check_topk(q, env.names, env.rows, orders, n)
            assert "TopK(select)" in ops_of(q)
            assert "Sort" not in ops_of(q) and q._last_stats.sorts == 0
        # the way back: full sort plus slice gives the same rows
        q = env.df.order_by(*to_sort_orders(orders)).limit(7)
        a = batch_row_list(q.collect())[1]
        monkeypatch.setenv("HS_TOPK_SELECT", "0")
        b = batch_row_list(q.collect())[1]
        monkeypatch.delenv("HS_TOPK_SELECT")
        assert "TopK(select)" in ops_of(q)
        assert [_norm_row(r) for r in a] == [_norm_row(r) for r in b]


def _norm_row(r):
    return tuple("nan" if isinstance(v, float) and v != v else
                 (np.float64(v).view(np.uint64).item()
                  if isinstance(v, float) else v) for v in r)


def scenario_multi_column(env, name):
    orders = MULTI_ORDERS[name]
    for n in limits(len(env.rows)):
        q = env.df.order_by(*to_sort_orders(orders)).limit(n)
        check_topk(q, env.names, env.rows, orders, n)
        assert "TopK(select)" in ops_of(q)


def scenario_unique_column(env):
    """Unique order column: the whole rows are the oracle's."""
    for asc in (True, False):
        orders = [("u", asc, asc)]
        for n in (1, 7, 100):
            q = env.df.order_by("u", ascending=asc).limit(n)
            check_topk(q, env.names, env.rows, orders, n, unique=True)


def scenario_order_by_alone(env):
    """A full Sort is stable: ties keep the scan's row order, so the whole
    output equals the oracle's, row for row."""
    for orders in ([("i", False, False)], [("n32", True, False)],
                   MULTI_ORDERS["i_asc-f_desc"]):
        q = env.df.order_by(*to_sort_orders(orders))
        names, got = batch_row_list(q.collect())
        want = oracle_sort(env.names, env.rows, orders)
        assert [r[0] for r in got] == [r[0] for r in want]
        assert all(_same_row(g, w) for g, w in zip(got, want))
        assert ops_of(q)[-1] == "Sort" and q._last_stats.sorts == 1


def scenario_limit_alone(env):
    for n in limits(len(env.rows)):
        q = env.df.limit(n)
        names, got = batch_row_list(q.collect())
        assert names == env.names
        assert [r[0] for r in got] == [r[0] for r in env.rows[:n]]
        assert ops_of(q)[-1] == "Limit"
    # a Limit over a Limit, and a Sort over a Limit, stay what they are
    q = env.df.limit(50).order_by("i").limit(5)
    orders = [("i", True, True)]
    check_topk(q, env.names, env.rows[:50], orders, 5)
    assert ops_of(q)[-2:] == ["Limit", "TopK(select)"]


def scenario_select_between(env):
    orders = [("f", False, False), ("i", True, True)]
    q = env.df.order_by(*to_sort_orders(orders)).select("rid", "s") \
        .limit(11)
    got = check_topk(q, env.names, env.rows, orders, 11)
    assert len(got[0]) == 2
    assert ops_of(q)[-2:] == ["TopK(select)", "Project"]
    assert q.plan.pretty().splitlines()[0] == "Limit(11)"


def scenario_over_aggregate(env):
    from collections import Counter
    from hyperspace_amd import functions as F
    from hyperspace_amd.plan.expr import col
    q = env.df.group_by("i").agg(F.count().alias("c"),
                                 F.max("u").alias("mu")) \
        .order_by(col("c").desc(), "i").limit(10)
    cnt = Counter(r[1] for r in env.rows)
    mx = {}
    for r in env.rows:
        mx[r[1]] = max(mx.get(r[1], r[2]), r[2])
    want = sorted(((i, c, mx[i]) for i, c in cnt.items()),
                  key=lambda t: (-t[1], t[0]))[:10]
    assert batch_row_list(q.collect())[1] == want
    assert ops_of(q)[-1] == "TopK(select)"


def scenario_over_join(env, tmp):
    right_dir = os.path.join(str(tmp), "right")
    os.makedirs(right_dir)
    pq.write_table(pa.table({
        "i": pa.array(list(range(0, 300, 3)), type=pa.int64()),
        "w": pa.array([x * 10 for x in range(0, 300, 3)],
                      type=pa.int64())}),
        os.path.join(right_dir, "part-0.parquet"))
    right = env.session.read_parquet(right_dir)
    q = env.df.join(right, "i").order_by("u", ascending=False).limit(9)
    names, got = batch_row_list(q.collect())
    want = sorted((r for r in env.rows if r[1] % 3 == 0),
                  key=lambda r: -r[2])[:9]
    rid, w = names.index("rid"), names.index("w")
    assert [g[rid] for g in got] == [r[0] for r in want]
    assert [g[w] for g in got] == [r[1] * 10 for r in want]
    assert ops_of(q)[-1] == "TopK(select)"


def scenario_bucketed(env, index_col="i"):
    """Rule on: the first / last n rows of every bucket answer the query;
    n runs past the size of some buckets too."""
    env.session.enable_hyperspace()
    n_rows = len(env.rows)
    for asc in (True, False):
        orders = [(index_col, asc, asc)]
        for n in (0, 1, 7, 700, n_rows + 5):
            q = env.df.order_by(index_col, ascending=asc).limit(n)
            check_topk(q, env.names, env.rows, orders, n)
            st = q._last_stats
            assert "TopK(bucketed)" in st.operators, st.operators
            assert st.shuffles == 0 and st.sorts == 0
    # through a projection under and over the sort
    orders = [(index_col, False, False)]
    q = env.df.select("rid", index_col, "s").order_by(
        *to_sort_orders(orders)).limit(7)
    check_topk(q, env.names, env.rows, orders, 7)
    assert "TopK(bucketed)" in ops_of(q)
    q = env.df.order_by(*to_sort_orders(orders)).select("rid", "d").limit(7)
    check_topk(q, env.names, env.rows, orders, 7)
    assert "TopK(bucketed)" in ops_of(q)
    # a filter below drops the segment offsets: the select serves it
    q = env.df.filter("u >= 0").order_by(index_col).limit(7)
    check_topk(q, env.names, [r for r in env.rows if r[2] >= 0],
               [(index_col, True, True)], 7)
    assert "TopK(select)" in ops_of(q)


def scenario_bucketed_nullable_key(env):
    """An index on a key with nulls: planned as TopK(bucketed), run as
    TopK(select), and right."""
    from hyperspace_amd.execution.layout import topk_operator_name
    env.session.enable_hyperspace()
    for asc, nulls_first in DIRECTIONS:
        orders = [("n32", asc, nulls_first)]
        q = env.df.order_by(*to_sort_orders(orders)).limit(40)
        assert topk_operator_name(q.optimized_plan()) == "TopK(bucketed)"
        check_topk(q, env.names, env.rows, orders, 40)
        assert "TopK(select)" in ops_of(q)
        assert "TopK(bucketed)" not in ops_of(q)


def hybrid_conf(session):
    c = hs.IndexConstants
    session.conf.set(c.INDEX_HYBRID_SCAN_ENABLED, True)
    session.conf.set(c.INDEX_HYBRID_SCAN_APPENDED_RATIO_THRESHOLD, 0.9)
    session.conf.set(c.INDEX_HYBRID_SCAN_DELETED_RATIO_THRESHOLD, 0.9)


def scenario_bucketed_hybrid(env):
    """A file appended after the build: the rule yields a BucketUnion, and
    the union's buckets serve the top-k."""
    from hyperspace_amd.plan.nodes import BucketUnionNode
    from aggregate_common import plan_nodes
    hybrid_conf(env.session)
    extra = make_order_rows(60, seed=99, rid0=10**6)
    # keys below and above everything the index holds
    extra[0] = extra[0][:1] + (-5,) + extra[0][2:]
    extra[1] = extra[1][:1] + (10**6,) + extra[1][2:]
    write_order_dataset(env.data, extra, n_files=1, prefix="zz-appended")
    env.reload()
    env.session.enable_hyperspace()
    assert len(env.rows) == N_ROWS + 60
    for asc in (True, False):
        q = env.df.order_by("i", ascending=asc).limit(12)
        unions = plan_nodes(q.optimized_plan(), BucketUnionNode)
        assert unions and unions[0].bucket_columns == ["i"]
        got = check_topk(q, env.names, env.rows, [("i", asc, asc)], 12)
        assert got[0][1] == (-5 if asc else 10**6)
        assert "TopK(bucketed)" in ops_of(q)
