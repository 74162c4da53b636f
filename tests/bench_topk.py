"""ORDER BY ... LIMIT micro-benchmark (GPU box): the HIP radix select
(ops.topk_rows plus the sort of its k candidates) against the full stable
radix sort cut to k rows, and the indexed top-k query end to end against
the same query with the rule switched off.

    python tests/bench_topk.py [--rows N] [--e2e-rows N] [--out FILE]

Both sides of each comparison run alternately in one process after a
warm-up; the table gives medians with the min..max spread.  The select's
algorithmic read rate counts 8 B/row for every pass it executes over the
keys (the varying-bit reduce, one histogram pass per key byte that varies,
the count pass; the emit pass stops early and is not counted) over the
median time, beside the measured HBM copy rate of the MI355X (6.29 TB/s).
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

HBM_MEASURED_TBS = 6.29
KS = (1, 100, 2**16)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), \
        torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def summary(ms):
    return (f"{statistics.median(ms):.2f} ms "
            f"({min(ms):.2f}..{max(ms):.2f})")


def make_keys(kind, n):
    """int64 values; the benchmark orders their sql_key."""
    g = torch.Generator(device="cuda").manual_seed(5)
    if kind == "uniform 64-bit":
        return torch.randint(-2**63, 2**63 - 1, (n,), device="cuda",
                             generator=g)
    if kind == "bench-shaped (20 bits vary)":
        return torch.randint(0, 2**20, (n,), device="cuda", generator=g)
    # skewed: 99 % of the rows share the top varying byte, so the first
    # histogram pass is not skipped and nearly every lane hits one bin
    low = torch.randint(0, 2**16, (n,), device="cuda", generator=g)
    top = torch.randint(0, 256, (n,), device="cuda", generator=g)
    common = torch.rand(n, device="cuda", generator=g) < 0.99
    top = torch.where(common, torch.full_like(top, 0x11), top)
    return (top << 16) | low


def select_path(keys, k):
    cand = ops.topk_rows(keys, k)
    sub = ops.gather_rows(keys, cand)
    return ops.gather_rows(sub, ops.sort_perm(sub))


def sort_path(keys, k):
    return ops.gather_rows(keys, ops.sort_perm(keys)[:k].contiguous())


def executed_passes(keys):
    """Passes over the keys the select executes: the varying-bit reduce,
    one histogram pass per key byte that varies, the count pass."""
    x = keys ^ keys[0]
    varying = sum(1 for b in range(8)
                  if bool(((x >> (8 * b)) & 0xFF).any()))
    return 2 + varying


def bench_ops(n, iters, warmup, lines):
    lines.append(f"### ops, {n} int64 keys ({iters} alternating runs after "
                 f"{warmup} warm-ups)")
    lines.append("")
    lines.append("| keys | k | select + sort of k | full sort, first k | "
                 "sort / select | slowest select < fastest sort | passes | "
                 "select algorithmic read rate |")
    lines.append("|---|---|---|---|---|---|---|---|")
    met = True
    for kind in ("uniform 64-bit", "bench-shaped (20 bits vary)",
                 "skewed (99 % share the top varying byte)"):
        keys = ops.sql_key(make_keys(kind, n))
        passes = executed_passes(keys)
        for k in KS:
            # same key sequence first
            assert torch.equal(select_path(keys, k), sort_path(keys, k)), \
                (kind, k)
            for _ in range(warmup):
                select_path(keys, k)
                sort_path(keys, k)
            torch.cuda.synchronize()
            s_ms, f_ms = [], []
            for _ in range(iters):
                s_ms.append(timed(lambda: select_path(keys, k))[0])
                f_ms.append(timed(lambda: sort_path(keys, k))[0])
            sm, fm = statistics.median(s_ms), statistics.median(f_ms)
            ok = max(s_ms) < min(f_ms)
            if k == 100:
                met = met and ok
            rate = n * 8 * passes / (sm * 1e-3) / 1e12
            lines.append(
                f"| {kind} | {k} | {summary(s_ms)} | {summary(f_ms)} | "
                f"{fm / sm:.2f}x | {'yes' if ok else 'NO'} | {passes} | "
                f"{rate:.2f} TB/s ({100 * rate / HBM_MEASURED_TBS:.0f}% of "
                f"{HBM_MEASURED_TBS} TB/s) |")
            print(lines[-1], flush=True)
        del keys
    lines.append("")
    lines.append("Acceptance (k = 100: the slowest select run is faster "
                 "than the fastest sort run on every distribution): "
                 + ("met" if met else "NOT met"))
    lines.append("")
    print(lines[-2], flush=True)


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
            "k": rng.integers(0, 2**40, m),
            "a": rng.integers(-10**6, 10**6, m),
            "f": rng.standard_normal(m)}),
            os.path.join(data, f"part-{i}.parquet"))
    session = hs.HyperspaceSession(device="cuda")
    session.conf.set(hs.IndexConstants.INDEX_NUM_BUCKETS, 64)
    h = hs.Hyperspace(session)
    df = session.read_parquet(data)
    h.create_index(df, hs.CoveringIndexConfig("topk_ix", ["k"], ["a", "f"]))
    session.enable_hyperspace()
    q = df.order_by("k").limit(100)
    key = hs.IndexConstants.INDEX_TOPK_RULE_ENABLED

    def run(rule_on):
        session.conf.set(key, rule_on)
        out = q.collect()
        want = "TopK(bucketed)" if rule_on else "TopK(select)"
        assert want in q._last_stats.operators, q._last_stats.operators
        return out

    a, b = run(True), run(False)
    assert torch.equal(a.tensor("k"), b.tensor("k"))
    for _ in range(warmup):
        run(True)
        run(False)
    on_ms, off_ms = [], []
    for _ in range(iters):
        on_ms.append(timed(lambda: run(True))[0])
        off_ms.append(timed(lambda: run(False))[0])
    lines.append(f"### query order_by(k).limit(100), {n} rows, 64 buckets "
                 f"({iters} alternating runs after {warmup} warm-ups)")
    lines.append("")
    lines.append("| plan | time |")
    lines.append("|---|---|")
    lines.append(f"| TopK(bucketed) (rule on, index resident) | "
                 f"{summary(on_ms)} |")
    lines.append(f"| TopK(select) (rule off, source scan + select) | "
                 f"{summary(off_ms)} |")
    lines.append("")
    print("\n".join(lines[-6:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2**26,
                    help="keys of the op comparison (up to 2**28)")
    ap.add_argument("--e2e-rows", type=int, default=2**24)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_topk needs a GPU"
    assert args.rows <= 2**28
    lines = []
    bench_ops(args.rows, args.iters, args.warmup, lines)
    if args.e2e_rows:
        bench_query(args.e2e_rows, max(3, args.iters // 3), 1, lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
