"""Group-by micro-benchmark (GPU box): the HIP group_offsets +
segmented_reduce against the same result composed from torch device ops
on the same sorted input, and the bucketed aggregate query end to end
against the same query with the rule switched off.

    python tests/bench_aggregate.py [--rows N] [--e2e-rows N] [--out FILE]

Both sides of each comparison run alternately in one process after a
warm-up; the table gives medians with the min..max spread.  Bytes per
second are the bytes the algorithm has to read (8-byte key, int64 value,
float64 value = 24 B/row) over the median time, beside the measured HBM
copy rate of the MI355X (6.29 TB/s).
"""
import argparse
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import hyperspace_amd as hs
import hyperspace_amd.ops as ops
from hyperspace_amd import functions as F

HBM_MEASURED_TBS = 6.29
BYTES_PER_ROW = 24


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), \
        torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def hip_path(keys, ivals, fvals):
    off = ops.group_offsets([ops.normalize_key(keys)])
    return off, ops.segmented_reduce(ivals, None, off), \
        ops.segmented_reduce(fvals, None, off)


def _torch_reduce(vals, counts, gid, how):
    try:
        return torch.segment_reduce(vals, how, lengths=counts)
    except RuntimeError:
        name = {"sum": "sum", "min": "amin", "max": "amax"}[how]
        out = torch.empty(counts.numel(), dtype=vals.dtype,
                          device=vals.device)
        return out.scatter_reduce_(0, gid, vals, name, include_self=False)


def torch_path(keys, ivals, fvals):
    _, counts = torch.unique_consecutive(keys, return_counts=True)
    gid = torch.repeat_interleave(
        torch.arange(counts.numel(), device=keys.device), counts)
    res = []
    for vals in (ivals, fvals):
        res.append({h: _torch_reduce(vals, counts, gid, h)
                    for h in ("sum", "min", "max")})
    return counts, res[0], res[1]


def make_keys(n, mean_len):
    if mean_len is None:
        return torch.zeros(n, dtype=torch.int64, device="cuda")
    if mean_len == 1:
        return torch.arange(n, dtype=torch.int64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(7)
    steps = torch.rand(n, device="cuda", generator=g) < 1.0 / mean_len
    return torch.cumsum(steps.to(torch.int64), 0)


def summary(ms):
    return (f"{statistics.median(ms):.2f} ms "
            f"({min(ms):.2f}..{max(ms):.2f})")


def bench_ops(n, iters, warmup, lines):
    g = torch.Generator(device="cuda").manual_seed(11)
    ivals = torch.randint(-10**6, 10**6, (n,), device="cuda", generator=g)
    fvals = torch.randn(n, device="cuda", generator=g, dtype=torch.float64)
    lines.append(f"### ops, {n} rows ({iters} alternating runs after "
                 f"{warmup} warm-ups)")
    lines.append("")
    lines.append("| mean group length | groups | HIP | torch composition |"
                 " torch / HIP | HIP algorithmic read rate |")
    lines.append("|---|---|---|---|---|---|")
    for label, mean_len in (("1", 1), ("16", 16), ("4096", 4096),
                            ("single group", None)):
        keys = make_keys(n, mean_len)
        # same answer first
        off, hi, hf = hip_path(keys, ivals, fvals)
        counts, ti, tf = torch_path(keys, ivals, fvals)
        assert torch.equal(off[1:] - off[:-1], counts), label
        for o in ("sum", "min", "max"):
            assert torch.equal(hi[o], ti[o]), (label, o)
        assert torch.equal(hf["min"], tf["min"]), label
        assert torch.equal(hf["max"], tf["max"]), label
        assert torch.allclose(hf["sum"], tf["sum"], rtol=1e-9, atol=1e-6)
        del off, hi, hf, counts, ti, tf
        for _ in range(warmup):
            hip_path(keys, ivals, fvals)
            torch_path(keys, ivals, fvals)
        torch.cuda.synchronize()
        h_ms, t_ms = [], []
        n_groups = 0
        for _ in range(iters):
            ms, out = timed(lambda: hip_path(keys, ivals, fvals))
            h_ms.append(ms)
            n_groups = out[0].numel() - 1
            del out
            ms, out = timed(lambda: torch_path(keys, ivals, fvals))
            t_ms.append(ms)
            del out
        hm, tm = statistics.median(h_ms), statistics.median(t_ms)
        rate = n * BYTES_PER_ROW / (hm * 1e-3) / 1e12
        lines.append(
            f"| {label} | {n_groups} | {summary(h_ms)} | {summary(t_ms)} | "
            f"{tm / hm:.2f}x | {rate:.2f} TB/s "
            f"({100 * rate / HBM_MEASURED_TBS:.0f}% of "
            f"{HBM_MEASURED_TBS} TB/s) |")
        print(lines[-1], flush=True)
    lines.append("")


def bench_query(n, iters, warmup, lines):
    import pyarrow as pa
    import pyarrow.parquet as pq
    tmp = tempfile.mkdtemp()
    os.environ["HYPERSPACE_SYSTEM_PATH"] = os.path.join(tmp, "indexes")
    data = os.path.join(tmp, "data")
    os.makedirs(data)
    rng = np.random.default_rng(3)
    parts = 8
    for i in range(parts):
        m = n // parts
        pq.write_table(pa.table({
            "k": rng.integers(0, max(1, n // 16), m),
            "a": rng.integers(-10**6, 10**6, m),
            "f": rng.standard_normal(m)}),
            os.path.join(data, f"part-{i}.parquet"))
    session = hs.HyperspaceSession(device="cuda")
    session.conf.set(hs.IndexConstants.INDEX_NUM_BUCKETS, 64)
    h = hs.Hyperspace(session)
    df = session.read_parquet(data)
    h.create_index(df, hs.CoveringIndexConfig("agg_ix", ["k"], ["a", "f"]))
    session.enable_hyperspace()
    q = df.group_by("k").agg(F.count(), F.sum("a"), F.sum("f"), F.max("a"))
    key = hs.IndexConstants.INDEX_AGGREGATE_RULE_ENABLED

    def run(rule_on):
        session.conf.set(key, rule_on)
        out = q.collect()
        want = "SortAggregate(bucketed)" if rule_on \
            else "SortAggregate(shuffled)"
        assert want in q._last_stats.operators, q._last_stats.operators
        return out

    a, b = run(True), run(False)
    assert a.num_rows == b.num_rows
    sa = torch.sort(a.tensor("k"))
    sb = torch.sort(b.tensor("k"))
    assert torch.equal(sa.values, sb.values)
    assert torch.equal(a.tensor("sum(a)")[sa.indices],
                       b.tensor("sum(a)")[sb.indices])
    for _ in range(warmup):
        run(True)
        run(False)
    on_ms, off_ms = [], []
    for _ in range(iters):
        on_ms.append(timed(lambda: run(True))[0])
        off_ms.append(timed(lambda: run(False))[0])
    lines.append(f"### query, {n} rows, 64 buckets, {a.num_rows} groups "
                 f"({iters} alternating runs after {warmup} warm-ups)")
    lines.append("")
    lines.append("| plan | time |")
    lines.append("|---|---|")
    lines.append(f"| bucketed (rule on, index resident) | {summary(on_ms)} |")
    lines.append(f"| sort path (rule off, source scan + sort) | "
                 f"{summary(off_ms)} |")
    lines.append(f"| sort path / bucketed | "
                 f"{statistics.median(off_ms) / statistics.median(on_ms):.2f}x"
                 " |")
    lines.append("")
    print("\n".join(lines[-6:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2**26)
    ap.add_argument("--e2e-rows", type=int, default=2**24)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_aggregate needs a GPU"
    lines = []
    bench_ops(args.rows, args.iters, args.warmup, lines)
    if args.e2e_rows:
        bench_query(args.e2e_rows, max(3, args.iters // 3), 1, lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
