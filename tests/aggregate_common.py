"""Shared builders for the group-by tests (CPU and GPU): brute-force
oracles over Python values, the input shapes aimed at the kernel's tile
size, and the grouped-query oracle over row tuples."""

import math
import struct
from collections import Counter

import numpy as np
import torch

import hyperspace_amd as hs
from hyperspace_amd import functions as F
from hyperspace_amd.ops import cpu_ref

from join_types_common import make_dataset

TILE = 2048  # rows per tile of the device kernels (checked on the GPU)
I64_MIN = -2**63


# ---------------------------------------------------------------------------
# brute force
# ---------------------------------------------------------------------------

def brute_group_offsets(keys, masks=None):
    """keys: list of int lists (u64 bit patterns); masks: None or list of
    bool lists / None.  A null compares equal to a null whatever it
    stores."""
    n = len(keys[0])

    def cell(c, i):
        if masks is not None and masks[c] is not None and not masks[c][i]:
            return None
        return keys[c][i]

    out = [i for i in range(n) if i == 0 or any(
        cell(c, i) != cell(c, i - 1) for c in range(len(keys)))]
    return out + [n] if n else [0]


def _wrap64(v):
    return (v + 2**63) % 2**64 - 2**63


def sort_key(x):
    """Total order of cpu_ref.normalize_key over Python numbers (the u64
    it maps to; the CPU tests pin the two together)."""
    if isinstance(x, float):
        b = struct.unpack("<Q", struct.pack("<d", x))[0]
        return b ^ (2**64 - 1 if b >> 63 else 2**63)
    return x + 2**63


def brute_segmented_reduce(values, valid, offsets, is_float):
    """Per group: (count, sum, min, max) over the valid rows; ints wrap
    to int64, float sums are math.fsum (the exactly rounded sum)."""
    out = []
    for g in range(len(offsets) - 1):
        rows = [values[i] for i in range(offsets[g], offsets[g + 1])
                if valid is None or valid[i]]
        if not rows:
            out.append((0, 0, 0, 0))
            continue
        if is_float:
            try:
                s = math.fsum(rows)
            except (OverflowError, ValueError):
                s = float("nan")
        else:
            s = _wrap64(sum(rows))
        out.append((len(rows), s, min(rows, key=sort_key),
                    max(rows, key=sort_key)))
    return out


# ---------------------------------------------------------------------------
# group_offsets shapes
# ---------------------------------------------------------------------------

def _runs(n, rng, mean_len=7):
    """n sorted int64 keys in runs of random length."""
    if n == 0:
        return torch.empty(0, dtype=torch.int64)
    steps = (rng.random(n) < 1.0 / mean_len).astype(np.int64)
    return torch.from_numpy(np.cumsum(steps) * 3 - 11)


def _norm(t):
    return cpu_ref.normalize_key(t)


def offset_cases(T=TILE):
    """name -> (normalized key columns, masks or None)."""
    rng = np.random.default_rng(3)
    cases = {}
    for n in (0, 1, T - 1, T, T + 1, 3 * T + 17):
        cases[f"n={n}"] = ([_norm(_runs(n, rng))], None)
    cases["one_group_5T+3"] = (
        [_norm(torch.full((5 * T + 3,), 42, dtype=torch.int64))], None)
    cases["singletons_3T+1"] = (
        [_norm(torch.arange(3 * T + 1, dtype=torch.int64))], None)
    cases["tile_edge_boundaries"] = (
        [_norm(torch.arange(3).repeat_interleave(T))], None)
    # group 1 starts on tile 0's last row and ends on tile 2's first row
    lens = torch.tensor([T - 1, T + 2, T - 1])
    cases["straddling_group"] = (
        [_norm(torch.arange(3).repeat_interleave(lens))], None)
    b = [0, 1, 1 | (1 << 32), -(2**63) | 1 | (1 << 32)]
    cases["bit_0_32_63"] = (
        [torch.tensor(b, dtype=torch.int64).repeat_interleave(3)], None)
    # u64 0, 2**63 and 2**64 - 1 as int64 bit patterns
    cases["u64_extremes"] = (
        [torch.tensor([0, 0, I64_MIN, I64_MIN, -1, -1],
                      dtype=torch.int64)], None)
    n = T + 9
    last = _norm(_runs(n, rng, 3))
    for ncols in (2, 3, 8):
        const = [_norm(torch.full((n,), c, dtype=torch.int64))
                 for c in range(ncols - 1)]
        cases[f"{ncols}_cols_last_changes"] = (const + [last], None)
    vals = _norm(_runs(40, rng, 4))
    cases["null_run_ahead"] = (
        [vals], [torch.tensor([False] * 13 + [True] * 27)])
    first = _norm(torch.tensor([1] * 20 + [2] * 20))
    m2 = torch.ones(40, dtype=torch.bool)
    m2[5:9] = False
    m2[30] = False
    cases["null_in_second_col"] = (
        [first, _norm(torch.full((40,), 7, dtype=torch.int64))], [None, m2])
    m = torch.ones(T + 40, dtype=torch.bool)
    m[T - 5:T + 6] = False  # a null run across the tile edge
    cases["nulls_store_different_values"] = (
        [_norm(torch.arange(T + 40, dtype=torch.int64) // 4)], [m])
    return cases


def offsets_of_lengths(lens):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int64)


# ---------------------------------------------------------------------------
# segmented_reduce shapes
# ---------------------------------------------------------------------------

def _random_lengths(total, rng, T):
    """Group lengths from 1 to 3T summing to ``total``: mostly short with
    a few long ones, the mix 64 buckets of real data give."""
    lens = []
    left = total
    while left > 0:
        r = rng.random()
        hi = 3 * T if r < 0.03 else (64 if r < 0.5 else 4)
        n = int(min(left, rng.integers(1, hi + 1)))
        lens.append(n)
        left -= n
    return lens


_NP = {torch.int64: np.int64, torch.int32: np.int32,
       torch.float64: np.float64, torch.float32: np.float32}


def _values(n, dtype, rng, exact):
    if dtype in (torch.int64, torch.int32):
        return torch.from_numpy(
            rng.integers(-10**6, 10**6, n).astype(_NP[dtype]))
    if exact:
        # integer-valued, |sum| far below 2**53: exact in any order
        return torch.from_numpy(
            rng.integers(-2**20, 2**20, n).astype(_NP[dtype]))
    return torch.from_numpy(
        (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n))
        .astype(_NP[dtype]))


def reduce_cases(dtype, T=TILE, exact=True):
    """name -> (values, valid or None, offsets) for one dtype."""
    rng = np.random.default_rng(17)
    cases = {}
    for n in (1, T - 1, T, T + 1, 3 * T + 17):
        lens = _random_lengths(n, rng, T)
        cases[f"n={n}"] = (_values(n, dtype, rng, exact), None,
                           offsets_of_lengths(lens))
    n = 5 * T + 3
    cases["one_group_5T+3"] = (_values(n, dtype, rng, exact), None,
                               torch.tensor([0, n]))
    n = 3 * T + 1
    cases["singletons_3T+1"] = (_values(n, dtype, rng, exact), None,
                                torch.arange(n + 1))
    cases["straddling_group"] = (
        _values(3 * T, dtype, rng, exact), None,
        offsets_of_lengths([T - 1, T + 2, T - 1]))
    n = 6 * T
    lens = _random_lengths(n, rng, T)
    off = offsets_of_lengths(lens)
    v = _values(n, dtype, rng, exact)
    cases["random_64_buckets"] = (v, None, off)
    cases["random_64_buckets_valid"] = (
        v, torch.from_numpy(rng.random(n) < 0.7), off)
    alt = torch.arange(n) % 2 == 0
    cases["alternating_nulls"] = (v, alt, off)
    # every third group entirely null, one of them crossing tiles
    allnull = torch.ones(n, dtype=torch.bool)
    for g in range(0, len(lens), 3):
        allnull[int(off[g]):int(off[g + 1])] = False
    cases["all_null_groups"] = (v, allnull, off)
    return cases


def special_reduce_cases(T=TILE):
    """name -> (values, valid, offsets): overflow and float-order
    cases."""
    cases = {}
    big = torch.full((T + 5,), 2**62, dtype=torch.int64)
    cases["int64_wrap"] = (big, None, offsets_of_lengths([3, T, 2]))
    cases["int32_past_2_31"] = (
        torch.full((2 * T,), 2**31 - 1, dtype=torch.int32), None,
        offsets_of_lengths([5, 2 * T - 5]))
    nan, inf = float("nan"), float("inf")
    pattern = [1.5, -0.0, 0.0, nan, -inf, inf, -2.0, 0.0, -0.0, inf, -nan,
               3.0]
    lens = [3, 2, 1, 2, 2, 2]
    for dt in (torch.float64, torch.float32):
        cases[f"float_order_{str(dt).split('.')[1]}"] = (
            torch.tensor(pattern, dtype=dt), None, offsets_of_lengths(lens))
    return cases


def big_reduce_case(dtype):
    """More tiles than blocks, so a block walks several tiles and carries
    the open group across them: 2 * 2048 + 1 tiles.  Long groups, runs of
    singletons and a group that spans many blocks."""
    n = (2 * 2048 + 1) * TILE + 5
    rng = np.random.default_rng(23)
    lens, left = [], n
    plan = [7 * TILE + 3, 1, 1, 1, 900 * TILE + 11, 2, TILE, TILE - 1, 1]
    i = 0
    while left > 0:
        m = min(left, plan[i % len(plan)] if i < 4 * len(plan)
                else int(rng.integers(1, 50 * TILE)))
        lens.append(m)
        left -= m
        i += 1
    return (_values(n, dtype, rng, True), None, offsets_of_lengths(lens))


def fsum_bound(values, valid, offsets):
    """Per group ((n - 1) * 2**-53 * sum|x|, math.fsum): the worst-case
    error of summing n doubles in any order."""
    out = []
    v = values.to(torch.float64).tolist()
    ok = None if valid is None else valid.tolist()
    off = offsets.tolist()
    for g in range(len(off) - 1):
        rows = [v[i] for i in range(off[g], off[g + 1])
                if ok is None or ok[i]]
        out.append((max(len(rows) - 1, 0) * 2.0**-53
                    * math.fsum(abs(x) for x in rows), math.fsum(rows)))
    return out


# ---------------------------------------------------------------------------
# grouped queries over row tuples
# ---------------------------------------------------------------------------

def group_oracle(rows, nkeys, specs):
    """Brute-force GROUP BY over row tuples whose first ``nkeys`` fields
    are the keys (None = null, nulls group together).  ``specs``: list of
    (func, field index or None).  Spark semantics: nulls ignored except
    by count(*); all-null inputs give None (0 for count).  Returns a
    Counter of output tuples."""
    groups = {}
    for r in rows:
        groups.setdefault(r[:nkeys], []).append(r)
    out = Counter()
    for key, members in groups.items():
        res = []
        for func, ix in specs:
            if ix is None:
                res.append(len(members))
                continue
            vals = [m[ix] for m in members if m[ix] is not None]
            if func == "count":
                res.append(len(vals))
            elif not vals:
                res.append(None)
            elif func == "sum":
                res.append(sum(vals))
            elif func == "min":
                res.append(min(vals))
            elif func == "max":
                res.append(max(vals))
            else:
                res.append(sum(vals) / len(vals))
        out[key + tuple(res)] += 1
    return out


def standard_aggs():
    """count(), sum(a), min(s), max(s), avg(a) over left(k, a, s) and the
    matching oracle specs."""
    return ([F.count(), F.sum("a"), F.min("s"), F.max("s"), F.avg("a")],
            [("count", None), ("sum", 1), ("min", 2), ("max", 2),
             ("avg", 1)])


def agg_session(root, device, num_buckets=4, n_left=400, n_right=300,
                lineage=False):
    """The join-types dataset with co-bucketed single-column indexes on k
    (jt_l covers a and s, jt_r covers b and t)."""
    ldir, rdir, lrows, rrows = make_dataset(root, n_left, n_right)
    session = hs.HyperspaceSession(device=device)
    session.conf.set(hs.IndexConstants.INDEX_NUM_BUCKETS, num_buckets)
    if lineage:
        session.conf.set(hs.IndexConstants.INDEX_LINEAGE_ENABLED, True)
    h = hs.Hyperspace(session)
    left = session.read_parquet(ldir)
    right = session.read_parquet(rdir)
    h.create_index(left, hs.CoveringIndexConfig("jt_l", ["k"], ["a", "s"]))
    h.create_index(right, hs.CoveringIndexConfig("jt_r", ["k"], ["b", "t"]))
    return session, h, left, right, lrows, rrows, ldir


def plan_nodes(plan, cls):
    out = []

    def walk(n):
        if isinstance(n, cls):
            out.append(n)
        for c in n.children:
            walk(c)

    walk(plan)
    return out
