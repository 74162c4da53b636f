"""Builders and an independent oracle for the logical-type tests (CPU and
GPU).

The oracle maps an arrow array to the numpy array the engine must hold
for it (docs/DESIGN.md, "Logical types"), written directly with numpy
casts and ``Decimal.scaleb`` — it imports nothing from the read paths
under test.

Every layout file holds every accepted column and its nullable twin
(``n_<name>``): N = 3000 rows in row groups of 1250 (three row groups,
the last one short), ``data_page_size=1024`` so every chunk has several
pages.  Edge values sit at the first rows, the last row and across the
row-group boundaries.
"""

import datetime
import decimal
from collections import Counter

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

N = 3000
ROW_GROUP = 1250
NUM_BUCKETS = 200
EPOCH = datetime.date(1970, 1, 1)

# column -> (arrow type, edge values as python ints, inclusive draw range)
# decimals and dates are drawn as integers (unscaled value / day number)
_SPEC = {
    "i32": (pa.int32(), [-2**31, 2**31 - 1, 0, -1], (-10**6, 10**6)),
    "i64": (pa.int64(), [-2**63, 2**63 - 1, 0, -1], (-10**12, 10**12)),
    "i8": (pa.int8(), [-128, 127, 0, -1], (-128, 127)),
    "i16": (pa.int16(), [-32768, 32767, 0, -1], (-32768, 32767)),
    "u8": (pa.uint8(), [0, 255, 128, 127], (0, 255)),
    "u16": (pa.uint16(), [0, 65535, 32768, 32767], (0, 65535)),
    "u32": (pa.uint32(), [0, 2**31 - 1, 2**31, 2**32 - 1],
            (2**31 - 500, 2**31 + 500)),
    "d": (pa.date32(), [-25567, -1, 0, 1, 19999], (-400, 400)),
    "dec32": (pa.decimal128(7, 2), [-9999999, 9999999, -1, 0, -150],
              (-50000, 50000)),
    "dec64": (pa.decimal128(18, 4), [-(10**18 - 1), 10**18 - 1, -1, 0],
              (-10**9, 10**9)),
    "ts_ms": (pa.timestamp("ms"), [-1, 0, 1, 1_700_000_000_000],
              (-10**6, 10**6)),
    "ts_us": (pa.timestamp("us"), [-1, 0, 1, 1_700_000_000_000_000],
              (-10**6, 10**6)),
    "ts_ns": (pa.timestamp("ns"), [-1, 0, 1, 2**62], (-10**6, 10**6)),
}
INT_LIKE = list(_SPEC)                     # every integer-backed column
CONTROLS = ["f32", "f64", "s", "b"]
BASE_COLUMNS = INT_LIKE + CONTROLS
# BOOLEAN has no native decoder: a read that asks for it sends the whole
# file to pyarrow, so the native checks project it away
NATIVE_COLUMNS = [c for c in BASE_COLUMNS if c != "b"]

# the engine dtype of each accepted arrow type: the table of
# docs/DESIGN.md, restated here on purpose (not imported from the code
# under test)
_ENGINE_DTYPE = {
    pa.int8(): np.int8, pa.int16(): np.int16, pa.int32(): np.int32,
    pa.int64(): np.int64, pa.uint8(): np.int32, pa.uint16(): np.int32,
    pa.uint32(): np.int64, pa.date32(): np.int32,
    pa.float32(): np.float32, pa.float64(): np.float64,
    pa.bool_(): np.bool_,
}


def _ints_to_arrow(typ, ints, null_every=0):
    """Python ints (None = null) -> arrow array of ``typ``."""
    vals = [None if null_every and i % null_every == null_every - 1 else v
            for i, v in enumerate(ints)]
    if pa.types.is_decimal(typ):
        vals = [None if v is None
                else decimal.Decimal(v).scaleb(-typ.scale) for v in vals]
        return pa.array(vals, type=typ)
    if pa.types.is_date(typ) or pa.types.is_timestamp(typ):
        store = pa.int32() if pa.types.is_date(typ) else pa.int64()
        return pa.array(vals, type=store).cast(typ)
    return pa.array(vals, type=typ)


def _draw(name, seed, n=N):
    """n python ints for column ``name``: a pool of ~150 distinct values
    (so a dictionary survives) with the edge values at both ends and on
    the row-group boundaries."""
    typ, edges, (lo, hi) = _SPEC[name]
    rng = np.random.default_rng(seed)
    span = hi - lo + 1
    pool = [lo + int(x) for x in rng.integers(0, span, 150)] + edges
    vals = [pool[int(i)] for i in rng.integers(0, len(pool), n)]
    for k, e in enumerate(edges):
        vals[k] = e
        vals[(ROW_GROUP - 2 + k) % n] = e
    vals[-1] = edges[1]
    return vals


def base_table(seed=0, nullable=True, n=N):
    """All accepted columns (+ nullable twins) as one arrow table."""
    rng = np.random.default_rng(1000 + seed)
    cols = {}
    for j, name in enumerate(INT_LIKE):
        cols[name] = _ints_to_arrow(_SPEC[name][0],
                                    _draw(name, seed * 100 + j, n))
    f64 = rng.standard_normal(n)
    f64[:4] = [0.0, -0.0, np.inf, np.nan]
    cols["f32"] = pa.array(f64.astype(np.float32))
    cols["f64"] = pa.array(f64)
    cols["s"] = pa.array([f"v{(i * 7) % 211:03d}" for i in range(n)],
                         type=pa.string())
    cols["b"] = pa.array((rng.integers(0, 2, n) == 1).tolist(),
                         type=pa.bool_())
    if nullable:
        for j, name in enumerate(INT_LIKE):
            cols["n_" + name] = _ints_to_arrow(
                _SPEC[name][0], _draw(name, seed * 100 + 50 + j, n),
                null_every=3 + j % 5)
        for name in CONTROLS:
            py = cols[name].to_pylist()
            cols["n_" + name] = pa.array(
                [None if i % 6 == 2 else v for i, v in enumerate(py)],
                type=cols[name].type)
    return pa.table(cols)


def _delta_encoding(table):
    return {f.name: "DELTA_BINARY_PACKED" for f in table.schema
            if f.name.replace("n_", "", 1) in INT_LIKE}


# layout -> pq.write_table keyword arguments (beyond the common ones)
LAYOUTS = {
    "plain": dict(compression="NONE", use_dictionary=False,
                  data_page_version="1.0"),
    "snappy_dict": dict(compression="SNAPPY", use_dictionary=True,
                        data_page_version="1.0"),
    "zstd_v2": dict(compression="ZSTD", use_dictionary=False,
                    data_page_version="2.0"),
    # DELTA_BINARY_PACKED has no native decoder: always the fallback
    "delta": dict(compression="NONE", use_dictionary=False,
                  data_page_version="1.0"),
    # uncompressed dictionary pages: the only dictionary layout the HOST
    # native read decodes (compressed chunks decode on the device)
    "dict": dict(compression="NONE", use_dictionary=True,
                 data_page_version="1.0"),
}
# layouts the device read decodes without pyarrow / the host native read
# returns a result for (BOOLEAN projected away)
DEVICE_NATIVE = ["plain", "snappy_dict", "zstd_v2", "dict"]
HOST_NATIVE = ["plain", "dict"]


def write_layout(table, path, layout, row_group_size=ROW_GROUP):
    kw = dict(LAYOUTS[layout])
    if layout == "delta":
        kw["column_encoding"] = _delta_encoding(table)
    pq.write_table(table, str(path), row_group_size=row_group_size,
                   data_page_size=1024, write_batch_size=128,
                   store_decimal_as_integer=True, **kw)
    return str(path)


def write_all_layouts(directory, seed=0):
    """{layout: (path, arrow table)} — every layout holds the same table."""
    table = base_table(seed)
    return {lay: (write_layout(table, directory / f"lt_{lay}.parquet", lay),
                  table) for lay in LAYOUTS}


def flba_decimal_file(directory):
    """decimal(12,2) as FIXED_LEN_BYTE_ARRAY (what pyarrow writes without
    store_decimal_as_integer, and Spark's legacy format): its own file,
    because the integer/FLBA choice is per file."""
    ints = _draw("dec32", 77)
    typ = pa.decimal128(12, 2)
    table = pa.table({"decf": _ints_to_arrow(typ, ints),
                      "n_decf": _ints_to_arrow(typ, ints, null_every=4)})
    p = str(directory / "lt_flba.parquet")
    pq.write_table(table, p, row_group_size=ROW_GROUP, data_page_size=1024,
                   compression="NONE", use_dictionary=False)
    return p, table


# refused type -> (column name, arrow array)
REFUSED = {
    "uint64": ("u64col", pa.array([0, 2**63 + 5, 2**64 - 1],
                                  type=pa.uint64())),
    "time32": ("t32col", pa.array([0, 1, 86_399_999],
                                  type=pa.time32("ms"))),
    "time64": ("t64col", pa.array([0, 1, 86_399_999_999],
                                  type=pa.time64("us"))),
    "binary": ("bincol", pa.array([b"\xff\xfe", b"ok", b"\x80"],
                                  type=pa.binary())),
    "decimal20": ("bigdec", pa.array(
        [decimal.Decimal(10**19), decimal.Decimal(-1), decimal.Decimal(0)],
        type=pa.decimal128(20, 0))),
}


def write_refused(directory):
    """{kind: (path, column name)}: one single-column file per refused
    type, uncompressed PLAIN so that nothing but the type declines it."""
    out = {}
    for kind, (name, arr) in REFUSED.items():
        p = str(directory / f"refused_{kind}.parquet")
        pq.write_table(pa.table({name: arr}), p, compression="NONE",
                       use_dictionary=False)
        out[kind] = (p, name)
    return out


# ---------------------------------------------------------------------------
# oracle
# ---------------------------------------------------------------------------

def oracle(arr):
    """arrow array / chunked array -> (engine numpy array, validity).
    Null slots hold 0 / "" / False and are never compared.  Strings come
    back as an object array of python str."""
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks()
    typ = arr.type
    if pa.types.is_timestamp(typ):
        # the file's unit, as stored: arrow's own int64 view
        py = arr.cast(pa.int64()).to_pylist()
        dtype = np.int64
    else:
        py = arr.to_pylist()
        dtype = None
    valid = np.array([v is not None for v in py], dtype=bool)
    if pa.types.is_string(typ):
        return np.array(["" if v is None else v for v in py],
                        dtype=object), valid
    if pa.types.is_decimal(typ):
        assert typ.precision <= 18
        ints = [0 if v is None else int(v.scaleb(typ.scale)) for v in py]
        return np.array(ints, dtype=np.int64), valid
    if pa.types.is_date32(typ):
        ints = [0 if v is None else (v - EPOCH).days for v in py]
        return np.array(ints, dtype=np.int32), valid
    dtype = dtype or _ENGINE_DTYPE[typ]
    return np.array([0 if v is None else v for v in py],
                    dtype=dtype), valid


def oracle_concat(tables, name):
    parts = [oracle(t.column(name)) for t in tables]
    return (np.concatenate([p[0] for p in parts]),
            np.concatenate([p[1] for p in parts]))


def assert_column(name, got, got_mask, want, valid):
    """``got`` (numpy array, or object array of str) equals the oracle:
    dtype exactly, bytes exactly on the valid rows, validity in full."""
    assert len(got) == len(want), name
    if valid.all():
        assert got_mask is None or bool(np.asarray(got_mask).all()), name
    else:
        assert got_mask is not None, f"{name}: nulls lost"
        assert np.array_equal(np.asarray(got_mask), valid), name
    if want.dtype == object:
        assert got.dtype == object, name
        assert list(got[valid]) == list(want[valid]), name
        return
    assert got.dtype == want.dtype, (name, got.dtype, want.dtype)
    assert np.ascontiguousarray(got[valid]).tobytes() == \
        np.ascontiguousarray(want[valid]).tobytes(), name


def host_columns(cols, masks):
    """The (columns, masks) dicts of read_native_host / _pyarrow_file_dict
    -> {name: (numpy array, mask or None)}; a dictionary-coded string
    column (``codes`` + ``values``) decodes to an object array."""
    out = {}
    for name, c in cols.items():
        if hasattr(c, "codes"):
            c = np.array(c.values, dtype=object)[np.asarray(c.codes)]
        out[name] = (np.asarray(c), masks.get(name))
    return out


def batch_columns(batch):
    """ColumnBatch (any device) -> the same shape as host_columns."""
    out = {}
    for name, c in batch.columns.items():
        if hasattr(c, "codes"):
            arr = np.array(c.values, dtype=object)[c.codes.cpu().numpy()]
        else:
            arr = c.cpu().numpy()
        m = batch.mask(name)
        out[name] = (arr, None if m is None else m.cpu().numpy())
    return out


def assert_table(got, tables, names):
    """``got`` ({name: (array, mask)}) equals the oracle of ``tables``
    concatenated, for exactly ``names`` in that order."""
    assert list(got) == list(names)
    for name in names:
        want, valid = oracle_concat(tables, name)
        assert_column(name, got[name][0], got[name][1], want, valid)


def round_trip_columns(n=2500):
    """(columns, validity mask) of an index batch whose dtypes the native
    writer does not know (int8, int16: written by pyarrow with an INT
    annotation) next to date-as-int32 and decimal-as-int64 columns."""
    import torch
    rng = np.random.default_rng(4)
    cols = {
        "i8": torch.from_numpy(rng.integers(-128, 128, n).astype(np.int8)),
        "i16": torch.from_numpy(
            rng.integers(-32768, 32768, n).astype(np.int16)),
        "d": torch.from_numpy(rng.integers(-400, 20000, n)
                              .astype(np.int32)),
        "dec": torch.from_numpy(rng.integers(-10**17, 10**17, n)),
    }
    cols["i8"][:2] = torch.tensor([-128, 127], dtype=torch.int8)
    cols["i16"][:2] = torch.tensor([-32768, 32767], dtype=torch.int16)
    return cols, torch.from_numpy(rng.random(n) > 0.2)


def assert_round_trip(got, cols, masks):
    """``got`` ({name: (array, mask)}) holds exactly what went in."""
    assert list(got) == list(cols)
    for name, want in cols.items():
        m = masks.get(name)
        valid = (np.ones(len(want), dtype=bool) if m is None
                 else m.numpy())
        assert_column(name, got[name][0], got[name][1], want.numpy(),
                      valid)


# ---------------------------------------------------------------------------
# end-to-end scenario: filters over a mixed-layout table, a join between
# an all-PLAIN and an all-DELTA table
# ---------------------------------------------------------------------------

E2E_ROWS = 1500


def _e2e_table(seed, payload):
    rng = np.random.default_rng(seed)
    days = [-3, -1, 0, 1, 18262] + \
        [int(x) for x in rng.integers(-40, 40, E2E_ROWS - 5)]
    u = [0, 2**31 - 1, 2**31, 2**32 - 1, 2**32 - 1] + \
        [2**31 - 300 + int(x) for x in rng.integers(0, 600, E2E_ROWS - 5)]
    return pa.table({
        "d": _ints_to_arrow(pa.date32(), days),
        "u": _ints_to_arrow(pa.uint32(), u),
        payload: pa.array(rng.integers(0, 10**9, E2E_ROWS)),
    })


def write_e2e(root):
    """Three source directories, two files each:
    ``mixed`` one PLAIN + one DELTA file (filters), ``lplain`` all PLAIN
    and ``rdelta`` all DELTA (the join: the two sides reach the engine
    through opposite read paths).  -> {dir name: (dir, [tables])}"""
    out = {}
    for dname, payload, layouts, seed in (
            ("mixed", "a", ("plain", "delta"), 10),
            ("lplain", "a", ("plain", "plain"), 20),
            ("rdelta", "b", ("delta", "delta"), 30)):
        d = root / dname
        d.mkdir()
        tables = []
        for i, lay in enumerate(layouts):
            t = _e2e_table(seed + i, payload)
            kw = dict(LAYOUTS[lay])
            if lay == "delta":
                kw["column_encoding"] = {"d": "DELTA_BINARY_PACKED",
                                         "u": "DELTA_BINARY_PACKED"}
            pq.write_table(t, str(d / f"part-{i}.parquet"),
                           row_group_size=600, data_page_size=1024, **kw)
            tables.append(t)
        out[dname] = (str(d), tables)
    return out


def e2e_rows(tables, names):
    """Row tuples of the oracle arrays of ``names`` over ``tables``."""
    cols = [oracle_concat(tables, n)[0].tolist() for n in names]
    return list(zip(*cols))


def run_e2e(root, device):
    """Build the indexes and run the filter and join scenario on
    ``device``, every result against the numpy oracle."""
    import hyperspace_amd as hs
    from hyperspace_amd.plan.nodes import IndexScan
    from join_types_common import batch_rows, join_rows_oracle

    src = write_e2e(root)
    session = hs.HyperspaceSession(device=device)
    session.conf.set(hs.IndexConstants.INDEX_NUM_BUCKETS, 16)
    h = hs.Hyperspace(session)
    mixed = session.read_parquet(src["mixed"][0])
    left = session.read_parquet(src["lplain"][0])
    right = session.read_parquet(src["rdelta"][0])
    h.create_index(mixed, hs.CoveringIndexConfig("lt_d", ["d"], ["a"]))
    h.create_index(mixed, hs.CoveringIndexConfig("lt_u", ["u"], ["a"]))
    h.create_index(left, hs.CoveringIndexConfig("lt_jl", ["d"], ["a"]))
    h.create_index(right, hs.CoveringIndexConfig("lt_jr", ["d"], ["b"]))
    session.enable_hyperspace()

    def index_leaves(df):
        return [leaf for leaf in df.optimized_plan().collect_leaves()
                if isinstance(leaf, IndexScan)]

    rows_ua = e2e_rows(src["mixed"][1], ["u", "a"])
    rows_da = e2e_rows(src["mixed"][1], ["d", "a"])
    assert sum(1 for r in rows_ua if r[0] >= 2**31) < len(rows_ua)

    def check(q, index_name, want, pruned):
        assert len(index_leaves(q)) == 1, q.explain_plan()
        assert index_name in h.explain(q)
        assert sum(want.values()) > 0
        assert batch_rows(q.collect())[1] == want, q.explain_plan()
        # with the bucket spec on, an equality opens one bucket of 16:
        # the literal must hash as the column does, or it is the wrong one
        assert (q._last_stats.bucket_pruned_files > 0) == pruned

    for bucket_spec in (False, True):
        session.conf.set(
            hs.IndexConstants.INDEX_FILTER_RULE_USE_BUCKET_SPEC, bucket_spec)
        check(mixed.filter("u >= 2147483648").select("u", "a"), "lt_u",
              Counter(r for r in rows_ua if r[0] >= 2**31), False)
        check(mixed.filter("u = 4294967295").select("u", "a"), "lt_u",
              Counter(r for r in rows_ua if r[0] == 2**32 - 1),
              bucket_spec)
        for day in (-1, 0, 18262, 7):
            check(mixed.filter(f"d = {day}").select("d", "a"), "lt_d",
                  Counter(r for r in rows_da if r[0] == day), bucket_spec)
    session.conf.set(
        hs.IndexConstants.INDEX_FILTER_RULE_USE_BUCKET_SPEC, False)

    q = left.select("d", "a").join(right.select("d", "b"), on="d")
    assert len(index_leaves(q)) == 2, q.explain_plan()
    out = q.collect()
    assert q._last_stats.merge_joins == 1 and q._last_stats.shuffles == 0
    lrows = e2e_rows(src["lplain"][1], ["d", "a"])
    rrows = e2e_rows(src["rdelta"][1], ["d", "b"])
    names, got = batch_rows(out)
    assert names == ["d", "a", "d_r", "b"]
    assert {str(out.tensor(k).dtype) for k in ("d", "d_r")} == \
        {"torch.int32"}
    want = join_rows_oracle(lrows, rrows, "inner")
    assert sum(want.values()) > len(lrows)
    assert got == want
    return session
