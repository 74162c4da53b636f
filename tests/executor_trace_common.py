"""Operator-trace replay for the executor (CPU and GPU tests share it).

A fixed list of small hand-built plans runs in a fixed order over generated
tables (a few thousand rows, 4 buckets, fixed seeds).  For each plan the
trace holds ``stats.operators``, the eight counters of ``PhysicalStats``
and the result: one digest per column over its sorted values, and one
over the rows in the order they came out.  Every value is an integer, a
string or a multiple of 1/4, so host and device agree bitwise.

``tests/golden/executor_traces.json`` is the recorded trace of the commit
before the executor was split into modules; the tests hold every later
executor against it.  ``python tests/executor_trace_common.py --record``
writes it and is not meant to be run again: a change of behaviour shows
as a failing test, not as a new golden file.
"""

import argparse
import hashlib
import json
import os
import sys
import tempfile

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hyperspace_amd as hs  # noqa: E402
from hyperspace_amd import functions as F  # noqa: E402
from hyperspace_amd.execution.executor import Executor  # noqa: E402
from hyperspace_amd.plan.expr import (And, In, Not, Or, SortOrder,  # noqa: E402
                                      col)
from hyperspace_amd.plan.nodes import (Aggregate, BucketUnionNode,  # noqa: E402
                                       Filter, IndexScan, Join, Limit,
                                       Project, Sort)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                      "golden", "executor_traces.json")
NUM_BUCKETS = 4
COUNTERS = ("scanned_files", "scanned_bytes", "shuffles", "merge_joins",
            "hash_joins", "sort_aggregates", "sorts", "bucket_pruned_files")
JOIN_TYPES = ("inner", "left_outer", "right_outer", "full_outer",
              "left_semi", "left_anti")


# ---------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------

def _left(rng, n, rid0=0):
    """rid unique; k with ~5 rows a value; k2 in 0..2; f multiples of 1/4;
    nk a nullable int32 with many rows a value; s short strings."""
    nk = rng.integers(0, 50, n).astype(np.int32)
    return pa.table({
        "rid": pa.array(np.arange(rid0, rid0 + n, dtype=np.int64)),
        "k": pa.array(rng.integers(0, 600, n).astype(np.int64)),
        "k2": pa.array(rng.integers(0, 3, n).astype(np.int64)),
        "f": pa.array(rng.integers(-40, 40, n) / 4.0),
        "nk": pa.array(nk, mask=rng.random(n) < 0.15),
        "s": pa.array(["abcXY z"[int(c)] * int(m) for c, m in zip(
            rng.integers(0, 7, n), rng.integers(0, 3, n))]),
    })


def _right(rng, n):
    """k unique (half of them above every left k); w unique."""
    nk = rng.integers(0, 60, n).astype(np.int32)
    return pa.table({
        "k": pa.array(rng.permutation(2 * n)[:n].astype(np.int64)),
        "k2": pa.array(rng.integers(0, 3, n).astype(np.int64)),
        "nk": pa.array(nk, mask=rng.random(n) < 0.1),
        "w": pa.array(rng.permutation(n).astype(np.int64) * 3 - n),
    })


def _write(table, root, name):
    os.makedirs(root, exist_ok=True)
    pq.write_table(table, os.path.join(root, name))


class TraceEnv:
    """The tables, their indexes and one session on ``device``."""

    def __init__(self, root, device):
        os.environ["HYPERSPACE_SYSTEM_PATH"] = os.path.join(root, "indexes")
        rng = np.random.default_rng(20240607)
        ldir, rdir, mdir = (os.path.join(root, d) for d in "LRM")
        _write(_left(rng, 1500), ldir, "part-0.parquet")
        _write(_left(rng, 1500, 1500), ldir, "part-1.parquet")
        _write(_right(rng, 1200), rdir, "part-0.parquet")
        _write(_left(rng, 1000), mdir, "part-0.parquet")
        s = self.session = hs.HyperspaceSession(device=device)
        s.conf.set(hs.IndexConstants.INDEX_NUM_BUCKETS, NUM_BUCKETS)
        s.conf.set(hs.IndexConstants.INDEX_LINEAGE_ENABLED, True)
        h = hs.Hyperspace(s)
        self.L, self.R = s.read_parquet(ldir), s.read_parquet(rdir)
        M = s.read_parquet(mdir)
        cfg = hs.CoveringIndexConfig
        h.create_index(self.L, cfg("lk", ["k"], ["rid", "k2", "f", "nk"]))
        h.create_index(self.R, cfg("rk", ["k"], ["k2", "w"]))
        h.create_index(self.L, cfg("lnk", ["nk"], ["rid", "k"]))
        h.create_index(self.R, cfg("rnk", ["nk"], ["w"]))
        h.create_index(self.L, cfg("lkk", ["k", "k2"], ["rid"]))
        h.create_index(self.R, cfg("rkk", ["k", "k2"], ["w"]))
        h.create_index(M, cfg("mk", ["k"], ["rid"]))
        h.create_index(M, cfg("mnk", ["nk"], ["rid"]))
        # a second sorted run in every bucket of the M indexes
        _write(_left(rng, 500, 1000), mdir, "part-1.parquet")
        h.refresh_index("mk", "incremental")
        h.refresh_index("mnk", "incremental")

    def ix(self, name, columns, bucketed=True, excluded=None):
        entry = self.session.index_manager().get_index(name)
        return IndexScan(entry, list(columns), bucketed, excluded)

    def clear_cache(self):
        self.session.index_data_cache().clear()


# ---------------------------------------------------------------------------
# queries: (name, plan builder, clear the index data cache first)
# ---------------------------------------------------------------------------

def _eq(a, b):
    return col(a) == col(b)


def _join_sides(env, bucketed, key):
    """Co-bucketed: both sides read the index on ``key``.  Shuffled: both
    sides scan their source files."""
    lcols = ["rid", key] if key == "nk" else ["rid", "k", "k2"]
    rcols = [key, "w"] if key == "nk" else ["k", "k2", "w"]
    if not bucketed:
        return Project(lcols, env.L.plan), Project(rcols, env.R.plan)
    if key == "nk":
        return env.ix("lnk", lcols), env.ix("rnk", rcols)
    if key == "kk":
        return env.ix("lkk", lcols), env.ix("rkk", rcols)
    return env.ix("lk", lcols), env.ix("rk", rcols)


def _join(jt, bucketed, key):
    def build(env):
        left, right = _join_sides(env, bucketed, key)
        cond = _eq("nk", "nk") if key == "nk" else _eq("k", "k")
        if key == "kk":
            cond = And(cond, _eq("k2", "k2"))
        return Join(left, right, cond, jt)
    return build


LK_COLS = ["rid", "k", "k2", "f", "nk"]


def _queries():
    q = []

    def add(name, build, clear=False):
        q.append((name, build, clear))

    def lk_filter(cond, **kw):
        return lambda env: Project(["rid", "k", "f"], Filter(
            cond, env.ix("lk", LK_COLS, **kw)))

    # index scan: the equality-pruned read and the whole-index read
    add("filter_eq_cold", lk_filter(col("k") == 77), clear=True)
    add("filter_eq_bucket_cached", lk_filter(col("k") == 77))
    add("filter_range", lk_filter((col("k") >= 100) & (col("k") < 140)))
    add("filter_eq_index_cached", lk_filter(col("k") == 77))
    add("filter_eq_absent_value", lk_filter(col("k") == -5))
    add("filter_compound", lambda env: Filter(
        Or(And(col("s") >= "b", Not(In(col("nk"), [1, 2, 3]))),
           And(col("k2") != 1, col("f") < col("k2"))),
        env.L.plan))
    add("filter_null_column_range", lambda env: Filter(
        col("nk") > 40, env.ix("lk", LK_COLS)))
    # lineage exclusions on both exits of the index scan
    add("lineage_eq_cold", lk_filter(col("k") == 77, excluded=[0]),
        clear=True)
    add("lineage_scan_segments", lambda env: Join(
        env.ix("lk", ["rid", "k"], excluded=[0]), env.ix("rk", ["k", "w"]),
        _eq("k", "k")))
    add("lineage_eq_index_cached", lk_filter(col("k") == 77, excluded=[1]))
    # multi-file buckets
    add("multifile_two_run_merge",
        lambda env: env.ix("mk", ["rid", "k"]), clear=True)
    add("multifile_nullable_bucket_sort",
        lambda env: env.ix("mnk", ["rid", "nk"]), clear=True)
    add("multifile_join", lambda env: Join(
        env.ix("mk", ["rid", "k"]), env.ix("rk", ["k", "w"]),
        _eq("k", "k")))
    # joins on a nullable key with many rows a value, both physical paths
    for jt in JOIN_TYPES:
        add(f"join_{jt}_cobucketed", _join(jt, True, "nk"))
        add(f"join_{jt}_shuffled", _join(jt, False, "nk"))
    add("join_inner_unique_key_cobucketed", _join("inner", True, "k"))
    add("join_inner_two_keys_cobucketed", _join("inner", True, "kk"))
    add("join_left_outer_two_keys_shuffled", _join("left_outer", False, "kk"))
    add("join_left_anti_two_keys_cobucketed", _join("left_anti", True, "kk"))
    # one side bucketed only: the shuffled path with segments at hand
    add("join_inner_one_side_bucketed", lambda env: Join(
        env.ix("lk", ["rid", "k"]), Project(["k", "w"], env.R.plan),
        _eq("k", "k")))
    # aggregates
    aggs = [F.count().alias("c"), F.sum("f").alias("sf"),
            F.min("rid").alias("lo"), F.max("nk").alias("hi"),
            F.avg("k2").alias("a")]
    add("aggregate_global", lambda env: Aggregate(
        [], aggs, env.ix("lk", LK_COLS)))
    add("aggregate_bucketed", lambda env: Aggregate(
        ["k"], aggs, Filter(col("k2") < 2, env.ix("lk", LK_COLS))))
    add("aggregate_bucketed_null_key", lambda env: Aggregate(
        ["nk"], [F.count().alias("c"), F.sum("k").alias("sk")],
        env.ix("lnk", ["rid", "nk", "k"])))
    add("aggregate_shuffled", lambda env: Aggregate(
        ["k2", "nk"], aggs, env.L.plan))
    # ORDER BY / LIMIT
    add("limit", lambda env: Limit(9, env.ix("rk", ["k", "w"])))
    add("sort", lambda env: Sort(
        [SortOrder("k2"), SortOrder("w", False)], env.R.plan))
    for asc in (True, False):
        d = "asc" if asc else "desc"
        add(f"topk_bucketed_{d}", lambda env, asc=asc: Limit(7, Sort(
            [SortOrder("k", asc)], env.ix("rk", ["k", "w"]))))
        add(f"topk_select_{d}", lambda env, asc=asc: Limit(7, Project(
            ["w", "k"], Sort([SortOrder("w", asc)], env.R.plan))))
    add("topk_filter_drops_segments", lambda env: Limit(7, Sort(
        [SortOrder("k")], Filter(col("w") >= 0, env.ix("rk", ["k", "w"])))))
    add("topk_bucketed_null_key_falls_back", lambda env: Limit(40, Sort(
        [SortOrder("nk")], env.ix("lnk", ["rid", "nk"]))))
    # bucket union with an unbucketed child, under each consumer
    def union(env):
        cols = ["rid", "k"]
        return BucketUnionNode(
            [env.ix("lk", cols), Project(cols, env.L.plan)], NUM_BUCKETS,
            ["k"])
    add("bucket_union", union)
    add("bucket_union_join", lambda env: Join(
        union(env), env.ix("rk", ["k", "w"]), _eq("k", "k")))
    add("bucket_union_aggregate", lambda env: Aggregate(
        ["k"], [F.count().alias("c"), F.sum("rid").alias("sr")], union(env)))
    add("bucket_union_topk", lambda env: Limit(5, Sort(
        [SortOrder("k", False)], union(env))))
    return q


QUERIES = _queries()
QUERY_NAMES = [name for name, _, _ in QUERIES]


# ---------------------------------------------------------------------------
# tracing
# ---------------------------------------------------------------------------

def _digest(values):
    return hashlib.sha256(
        json.dumps(values, allow_nan=True).encode()).hexdigest()[:24]


def _null_low(v):
    return (v is not None, v if v is not None else 0)


def trace_batch(batch):
    table = batch.to_arrow()
    names = table.column_names
    cols = [table.column(n).to_pylist() for n in names]
    return {
        "columns": names,
        "num_rows": table.num_rows,
        "sorted": {n: _digest(sorted(c, key=_null_low))
                   for n, c in zip(names, cols)},
        "nulls": {n: sum(v is None for v in c) for n, c in zip(names, cols)},
        "row_order": _digest([list(r) for r in zip(*cols)]),
    }


def run_traces(device):
    """name -> trace, for every query, in the fixed order."""
    out = {}
    with tempfile.TemporaryDirectory() as root:
        env = TraceEnv(root, device)
        for name, build, clear in QUERIES:
            if clear:
                env.clear_cache()
            ex = Executor(env.session)
            batch = ex.execute(build(env))
            trace = {"operators": list(ex.stats.operators)}
            trace.update({c: getattr(ex.stats, c) for c in COUNTERS})
            trace["result"] = trace_batch(batch)
            out[name] = trace
    return out


def load_golden(device):
    """The recorded traces for ``device`` ('cpu' or 'cuda'): its own
    section where the two legitimately differ, else the common one."""
    with open(GOLDEN) as f:
        g = json.load(f)
    return g.get(device, g.get("common"))


def check_recorded_paths(traces):
    """The queries take the paths their names promise (checked when the
    golden file is recorded, so that it pins what it says it pins)."""
    def ops(name):
        return traces[name]["operators"]
    assert "IndexScan(cached)" not in ops("filter_eq_cold")
    assert traces["filter_eq_cold"]["scanned_files"] == 1
    assert traces["filter_eq_cold"]["bucket_pruned_files"] == 3
    for name in ("filter_eq_bucket_cached", "filter_eq_index_cached"):
        assert "IndexScan(cached)" in ops(name), name
        assert traces[name]["scanned_files"] == 0
        assert traces[name]["result"] == traces["filter_eq_cold"]["result"]
    rows = traces["filter_eq_cold"]["result"]["num_rows"]
    for name in ("lineage_eq_cold", "lineage_eq_index_cached"):
        assert "LineageFilter" in ops(name), name
        assert 0 < traces[name]["result"]["num_rows"] < rows, name
    assert "IndexScan(cached)" not in ops("lineage_eq_cold")
    assert "IndexScan(cached)" in ops("lineage_eq_index_cached")
    assert "LineageFilter" in ops("lineage_scan_segments")
    assert traces["lineage_scan_segments"]["merge_joins"] == 1
    for name in ("multifile_two_run_merge", "multifile_nullable_bucket_sort"):
        assert traces[name]["scanned_files"] == 2 * NUM_BUCKETS, name
        assert traces[name]["result"]["num_rows"] == 1500
    assert traces["multifile_nullable_bucket_sort"]["result"]["nulls"]["nk"]
    for jt in JOIN_TYPES:
        suffix = "" if jt == "inner" else f", {jt}"
        assert ops(f"join_{jt}_cobucketed")[-1] == \
            f"SortMergeJoin(co-bucketed{suffix})"
        assert ops(f"join_{jt}_shuffled")[-1] == \
            f"SortMergeJoin(shuffled{suffix})"
        assert traces[f"join_{jt}_cobucketed"]["result"]["sorted"] == \
            traces[f"join_{jt}_shuffled"]["result"]["sorted"], jt
    assert ops("join_inner_two_keys_cobucketed")[-1] == \
        "SortMergeJoin(co-bucketed)"
    assert ops("join_inner_one_side_bucketed")[-1] == \
        "SortMergeJoin(shuffled)"
    for kind in ("global", "bucketed", "shuffled"):
        assert ops(f"aggregate_{kind}")[-1] == f"SortAggregate({kind})"
    assert ops("aggregate_bucketed_null_key")[-1] == "SortAggregate(bucketed)"
    assert ops("limit")[-1] == "Limit" and ops("sort")[-1] == "Sort"
    for d in ("asc", "desc"):
        assert ops(f"topk_bucketed_{d}")[-1] == "TopK(bucketed)"
        assert ops(f"topk_select_{d}")[-2:] == ["TopK(select)", "Project"]
    assert ops("topk_filter_drops_segments")[-1] == "TopK(select)"
    assert ops("topk_bucketed_null_key_falls_back")[-1] == "TopK(select)"
    assert traces["bucket_union"]["shuffles"] == 1
    assert ops("bucket_union_join")[-1] == "SortMergeJoin(co-bucketed)"
    assert ops("bucket_union_aggregate")[-1] == "SortAggregate(bucketed)"
    assert ops("bucket_union_topk")[-1] == "TopK(bucketed)"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--record", action="store_true",
                    help="write the traces of this checkout")
    ap.add_argument("--device", default="cpu", choices=("cpu", "cuda"))
    ap.add_argument("--section", default="common",
                    help="section of the golden file to write")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    traces = run_traces(args.device)
    check_recorded_paths(traces)
    if not args.record:
        want = load_golden(args.device)
        bad = [n for n in QUERY_NAMES if traces[n] != want[n]]
        print("differing:", bad)
        sys.exit(1 if bad else 0)
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc[args.section] = traces
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(traces)} traces to {args.out} [{args.section}]")


if __name__ == "__main__":
    main()
