"""CPU reference implementations of the data-plane ops.

These are the numerics oracles for the HIP kernels (tests compare the
device kernels against these) and the execution path on machines without a
GPU.  They intentionally use plain torch ops — clarity over speed.

Spark-compatible Murmur3 (seed 42) is implemented here bit-exactly so that
bucket assignment matches Spark's HashPartitioning for int/long columns
(reference data plane K2: index/covering/CoveringIndex.scala:58-61).
"""

from __future__ import annotations

from typing import List, Optional, Tuple

import torch

MASK32 = 0xFFFFFFFF
SPARK_HASH_SEED = 42


def _rotl32(x: torch.Tensor, r: int) -> torch.Tensor:
    return ((x << r) | (x >> (32 - r))) & MASK32


def _mix_k1(k1: torch.Tensor) -> torch.Tensor:
    k1 = (k1 * 0xCC9E2D51) & MASK32
    k1 = _rotl32(k1, 15)
    k1 = (k1 * 0x1B873593) & MASK32
    return k1


def _mix_h1(h1: torch.Tensor, k1: torch.Tensor) -> torch.Tensor:
    h1 = h1 ^ k1
    h1 = _rotl32(h1, 13)
    h1 = (h1 * 5 + 0xE6546B64) & MASK32
    return h1


def _fmix(h1: torch.Tensor, length: int) -> torch.Tensor:
    h1 = h1 ^ length
    h1 = h1 ^ (h1 >> 16)
    h1 = (h1 * 0x85EBCA6B) & MASK32
    h1 = h1 ^ (h1 >> 13)
    h1 = (h1 * 0xC2B2AE35) & MASK32
    h1 = h1 ^ (h1 >> 16)
    return h1


def murmur3_hash_int32(x: torch.Tensor, seed) -> torch.Tensor:
    """Spark Murmur3_x86_32 hashInt.  x: any int tensor (uses low 32 bits).
    seed: int or int tensor.  Returns uint32 values in an int64 tensor."""
    v = x.to(torch.int64) & MASK32
    if isinstance(seed, int):
        seed = torch.full_like(v, seed)
    h1 = _mix_h1(seed & MASK32, _mix_k1(v))
    return _fmix(h1, 4)


def murmur3_hash_int64(x: torch.Tensor, seed) -> torch.Tensor:
    """Spark Murmur3 hashLong: mixes low then high 32-bit halves."""
    v = x.to(torch.int64)
    low = v & MASK32
    high = (v >> 32) & MASK32
    if isinstance(seed, int):
        seed = torch.full_like(v, seed)
    h1 = _mix_h1(seed & MASK32, _mix_k1(low))
    h1 = _mix_h1(h1, _mix_k1(high))
    return _fmix(h1, 8)


def murmur3_bucket(keys: List[torch.Tensor], num_buckets: int,
                   masks: Optional[List[Optional[torch.Tensor]]] = None
                   ) -> torch.Tensor:
    """Bucket id per row: Spark HashPartitioning semantics —
    h = seed 42 folded over columns, bucket = pmod(h, n).  A null key
    column leaves the running hash unchanged (Murmur3Hash skips null
    children, so an all-null single-key row lands in pmod(42, n)).
    Float keys hash their canonical bits (-0.0 as +0.0, one NaN), so
    SQL-equal keys share a bucket.
    ``masks[i]`` is a bool validity tensor or None.  Returns int32."""
    h: Optional[torch.Tensor] = None
    for ci, k in enumerate(keys):
        seed = SPARK_HASH_SEED if h is None else h
        if k.dtype in (torch.int64, torch.float64):
            if k.dtype == torch.float64:
                k = canonical_float_bits(k)
            nh = murmur3_hash_int64(k, seed)
        else:
            if k.dtype == torch.float32:
                k = canonical_float_bits(k)
            nh = murmur3_hash_int32(k, seed)
        mask = masks[ci] if masks is not None else None
        if mask is not None and mask.numel():
            seed_t = (torch.full_like(nh, SPARK_HASH_SEED)
                      if h is None else h)
            nh = torch.where(mask.to(torch.bool), nh, seed_t)
        h = nh
    assert h is not None
    signed = h.to(torch.int64)
    signed = torch.where(signed > 0x7FFFFFFF, signed - (1 << 32), signed)
    return ((signed % num_buckets + num_buckets) % num_buckets).to(torch.int32)


# ---------------------------------------------------------------------------
# Order-preserving u64 key normalization
# ---------------------------------------------------------------------------

def normalize_key(col: torch.Tensor) -> torch.Tensor:
    """Map a column to u64 (stored in int64) such that unsigned comparison
    of the result == natural ordering of the values."""
    if col.dtype in (torch.int8, torch.int16, torch.int32, torch.int64):
        return col.to(torch.int64) ^ (-0x8000000000000000)
    if col.dtype == torch.float64:
        bits = col.view(torch.int64)
        mask = torch.where(bits < 0,
                           torch.full_like(bits, -1),
                           torch.full_like(bits, -0x8000000000000000))
        return bits ^ mask
    if col.dtype == torch.float32:
        return normalize_key(col.to(torch.float64))
    if col.dtype == torch.bool:
        return col.to(torch.int64) ^ (-0x8000000000000000)
    raise ValueError(f"Unsupported dtype for sort key: {col.dtype}")


def canonical_float_bits(col: torch.Tensor) -> torch.Tensor:
    """Bit pattern (int64 / int32) of a float64 / float32 column under SQL
    equality: -0.0 becomes +0.0 and every NaN, whatever its sign or
    payload, the canonical quiet NaN 0x7ff8000000000000 / 0x7fc00000 —
    what Java's doubleToLongBits / floatToIntBits hand to Spark's hash."""
    if col.dtype == torch.float64:
        bits = col.contiguous().view(torch.int64)
        mag, inf, nan = 0x7FFFFFFFFFFFFFFF, 0x7FF0000000000000, \
            0x7FF8000000000000
        neg_zero = -0x8000000000000000
    elif col.dtype == torch.float32:
        bits = col.contiguous().view(torch.int32)
        mag, inf, nan, neg_zero = 0x7FFFFFFF, 0x7F800000, 0x7FC00000, \
            -0x80000000
    else:
        raise ValueError(f"not a float column: {col.dtype}")
    bits = torch.where((bits & mag) > inf, torch.full_like(bits, nan), bits)
    return torch.where(bits == neg_zero, torch.zeros_like(bits), bits)


def sql_key(col: torch.Tensor) -> torch.Tensor:
    """``normalize_key`` under SQL equality and ordering: equal keys <=>
    SQL-equal values.  Float zeros share one key and all NaNs share the
    largest one (above +inf); integer columns are unchanged."""
    if col.dtype == torch.float32:
        col = col.to(torch.float64)
    if col.dtype == torch.float64:
        col = canonical_float_bits(col).view(torch.float64)
    return normalize_key(col)


def _as_unsigned_sortable(u64: torch.Tensor) -> torch.Tensor:
    """int64-storing-u64 -> int64 whose signed order == the u64 order."""
    return u64 ^ (-0x8000000000000000)


def stable_sort_u64(keys_u64: torch.Tensor,
                    payload: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Stable sort of (u64 key, payload) by key.  Returns sorted keys and
    correspondingly permuted payload."""
    sortable = _as_unsigned_sortable(keys_u64)
    _, perm = torch.sort(sortable, stable=True)
    return keys_u64[perm], payload[perm]


def sort_perm_u64(keys_u64: torch.Tensor) -> torch.Tensor:
    sortable = _as_unsigned_sortable(keys_u64)
    _, perm = torch.sort(sortable, stable=True)
    return perm


# ---------------------------------------------------------------------------
# Segmented sorted merge join (K4)
# ---------------------------------------------------------------------------

MERGE_JOIN_MODES = {"inner": 0, "left_outer": 1, "left_semi": 2,
                    "left_anti": 3}


def merge_join_mode_code(mode: str) -> int:
    """Kernel mode code for a merge-join mode name."""
    try:
        return MERGE_JOIN_MODES[mode]
    except KeyError:
        raise ValueError(
            f"merge_join mode {mode!r} not in {sorted(MERGE_JOIN_MODES)}")


def merge_join(lkeys: torch.Tensor, rkeys: torch.Tensor,
               lseg: torch.Tensor, rseg: torch.Tensor,
               mode: str = "inner"
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Join two segment-partitioned sorted key arrays.

    ``lseg``/``rseg`` are segment offset arrays of equal length S+1; segment
    s spans [lseg[s], lseg[s+1]).  Keys are u64 values stored in int64,
    sorted in u64 order within each segment.
    Returns (left_idx, right_idx) global row-index pairs of all equal-key
    matches, segment-aligned (only same-segment rows join — this is the
    zero-exchange co-bucketed join).

    With c = a left row's match count, ``mode`` selects how many output
    slots e the row takes: ``inner`` c; ``left_outer`` max(c, 1), the
    single pair (i, -1) when c == 0; ``left_semi`` c > 0; ``left_anti``
    c == 0.  Semi and anti return an empty right_idx.  Output is
    ascending by left row, a row's matches ascending by right index.
    """
    assert lseg.numel() == rseg.numel()
    code = merge_join_mode_code(mode)
    pairs = code in (0, 1)
    louts, routs = [], []
    S = lseg.numel() - 1
    for s in range(S):
        l0, l1 = int(lseg[s]), int(lseg[s + 1])
        r0, r1 = int(rseg[s]), int(rseg[s + 1])
        if l1 <= l0:
            continue
        # an empty right segment searches to lo == hi == 0: every left
        # row of the segment is unmatched
        lk = _as_unsigned_sortable(lkeys[l0:l1]).contiguous()
        rk = _as_unsigned_sortable(rkeys[r0:max(r0, r1)]).contiguous()
        lo = torch.searchsorted(rk, lk, side="left")
        hi = torch.searchsorted(rk, lk, side="right")
        counts = (hi - lo).clamp(min=0)
        if code == 0:
            emit = counts
        elif code == 1:
            emit = counts.clamp(min=1)
        elif code == 2:
            emit = (counts > 0).to(torch.int64)
        else:
            emit = (counts == 0).to(torch.int64)
        total = int(emit.sum())
        if total == 0:
            continue
        louts.append(torch.repeat_interleave(
            torch.arange(l0, l1, dtype=torch.int64), emit))
        if not pairs:
            continue
        starts = torch.repeat_interleave(lo, emit)
        offs = torch.arange(total, dtype=torch.int64) - \
            torch.repeat_interleave(torch.cumsum(emit, 0) - emit, emit)
        ridx = r0 + starts + offs
        if code == 1:
            matched = torch.repeat_interleave(counts, emit) > 0
            ridx = torch.where(matched, ridx, torch.full_like(ridx, -1))
        routs.append(ridx)
    e = torch.empty(0, dtype=torch.int64)
    if not louts:
        return e, e.clone()
    return torch.cat(louts), (torch.cat(routs) if pairs else e)


# ---------------------------------------------------------------------------
# Filters (K7 + filter scan)
# ---------------------------------------------------------------------------

def select_range_u64(keys_u64: torch.Tensor, lo: int, hi: int,
                     lo_incl: bool, hi_incl: bool) -> torch.Tensor:
    """Indices i where lo <?< keys[i] <?< hi under u64 ordering.
    lo/hi are normalized u64 (int64-encoded)."""
    s = _as_unsigned_sortable(keys_u64)
    slo = lo ^ -0x8000000000000000
    shi = hi ^ -0x8000000000000000
    m_lo = (s >= slo) if lo_incl else (s > slo)
    m_hi = (s <= shi) if hi_incl else (s < shi)
    return torch.nonzero(m_lo & m_hi, as_tuple=False).flatten()


def topk_rows(keys_u64: torch.Tensor, k: int,
              valid: Optional[torch.Tensor] = None,
              keep_ties: bool = False) -> torch.Tensor:
    """Rows of the k smallest keys (u64 order) among the valid rows, in
    ascending row index.  With T the k-th smallest valid key: every valid
    row below T, then of the rows equal to T all of them (``keep_ties``)
    or the first k - #below in row order.  k <= 0 gives no row, k >=
    n_valid every valid row; the stored key of an invalid row is ignored."""
    n = keys_u64.numel()
    if valid is None:
        valid = torch.ones(n, dtype=torch.bool, device=keys_u64.device)
    valid = valid.to(torch.bool)
    rows = torch.nonzero(valid, as_tuple=False).flatten()
    if k <= 0 or rows.numel() == 0:
        return rows[:0]
    if k >= rows.numel():
        return rows
    s = _as_unsigned_sortable(keys_u64)
    ordered, _ = torch.sort(s[rows], stable=True)
    t = ordered[k - 1]
    below = valid & (s < t)
    ties = torch.nonzero(valid & (s == t), as_tuple=False).flatten()
    if not keep_ties:
        ties = ties[:k - int(below.sum())]
    take = below.clone()
    take[ties] = True
    return torch.nonzero(take, as_tuple=False).flatten()


def isin_sorted(values: torch.Tensor,
                sorted_set: torch.Tensor) -> torch.Tensor:
    """Boolean mask: values ∈ sorted_set (both int64)."""
    if sorted_set.numel() == 0:
        return torch.zeros_like(values, dtype=torch.bool)
    pos = torch.searchsorted(sorted_set, values)
    pos = pos.clamp(max=sorted_set.numel() - 1)
    return sorted_set[pos] == values


# ---------------------------------------------------------------------------
# Sketches (K8)
# ---------------------------------------------------------------------------

def segmented_minmax(vals: torch.Tensor, seg_off: torch.Tensor
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-segment min/max.  seg_off: S+1 offsets.  Returns (mins, maxs)."""
    S = seg_off.numel() - 1
    mins = torch.empty(S, dtype=vals.dtype)
    maxs = torch.empty(S, dtype=vals.dtype)
    for s in range(S):
        a, b = int(seg_off[s]), int(seg_off[s + 1])
        seg = vals[a:b]
        mins[s] = seg.min() if b > a else 0
        maxs[s] = seg.max() if b > a else 0
    return mins, maxs


def _bloom_hashes(vals: torch.Tensor, k: int, m_bits: int) -> torch.Tensor:
    """k bit positions per value, shape [N, k].  Double hashing with the
    Spark-style (h1 + i*h2) scheme over Murmur3."""
    h1 = murmur3_hash_int64(vals, 0)
    h2 = murmur3_hash_int64(vals, h1)
    idx = []
    for i in range(k):
        combined = (h1 + i * h2) & 0x7FFFFFFFFFFFFFFF
        idx.append(combined % m_bits)
    return torch.stack(idx, dim=1)


def bloom_build(vals: torch.Tensor, m_bits: int, k: int) -> torch.Tensor:
    """Build a bloom filter (int64 word array of ceil(m/64) words)."""
    words = torch.zeros((m_bits + 63) // 64, dtype=torch.int64)
    pos = _bloom_hashes(vals.to(torch.int64), k, m_bits).flatten()
    w = (pos // 64).long()
    b = (pos % 64).long()
    np_words = words.numpy()
    import numpy as np
    np.bitwise_or.at(np_words, w.numpy(),
                     (np.int64(1) << b.numpy().astype(np.int64)))
    return torch.from_numpy(np_words)


def bloom_probe(vals: torch.Tensor, words: torch.Tensor, m_bits: int,
                k: int) -> torch.Tensor:
    pos = _bloom_hashes(vals.to(torch.int64), k, m_bits)
    w = (pos // 64).long()
    b = pos % 64
    bits = (words[w] >> b) & 1
    return bits.all(dim=1)


# ---------------------------------------------------------------------------
# Z-order (K10)
# ---------------------------------------------------------------------------

def zorder_key(cols_u64: List[torch.Tensor], bits_per_col: int
               ) -> torch.Tensor:
    """Interleave the top ``bits_per_col`` bits of each normalized column
    into a single u64 z-address.  cols are normalize_key() outputs."""
    n_cols = len(cols_u64)
    assert n_cols * bits_per_col <= 64
    z = torch.zeros_like(cols_u64[0])
    for b in range(bits_per_col):
        # bit (63 - b) of each column, MSB-first round-robin
        for c, col in enumerate(cols_u64):
            bit = (col >> (63 - b)) & 1
            out_pos = 63 - (b * n_cols + c)
            z = z | (bit << out_pos)
    return z


def run_merge_perm(keys_u64: torch.Tensor, seg: torch.Tensor,
                   split: torch.Tensor) -> torch.Tensor:
    """Segmented two-sorted-run merge permutation (K4b reference).

    Each segment b's rows [seg[b], seg[b+1]) hold two sorted runs split
    at split[b] (== seg[b+1] when the segment is a single run); returns
    perm such that gathering by it sorts each segment, with A-rows
    stably preceding equal B-rows."""
    sortable = _as_unsigned_sortable(keys_u64)
    n = keys_u64.numel()
    perm = torch.empty(n, dtype=torch.int64)
    for b in range(seg.numel() - 1):
        a0, b1, sp = int(seg[b]), int(seg[b + 1]), int(split[b])
        ka, kb = sortable[a0:sp], sortable[sp:b1]
        pos_a = torch.arange(sp - a0) + torch.searchsorted(
            kb, ka, right=False)
        pos_b = torch.arange(b1 - sp) + torch.searchsorted(
            ka, kb, right=True)
        perm[a0 + pos_a] = torch.arange(a0, sp)
        perm[a0 + pos_b] = torch.arange(sp, b1)
    return perm


# ---------------------------------------------------------------------------
# Group-by over adjacent runs (K13)
# ---------------------------------------------------------------------------

def denormalize_key(keys_u64: torch.Tensor, dtype: torch.dtype
                    ) -> torch.Tensor:
    """Inverse of ``normalize_key`` for int32/int64/float32/float64."""
    sign = -0x8000000000000000
    if dtype in (torch.int32, torch.int64):
        return (keys_u64 ^ sign).to(dtype)
    # a set top bit marks a non-negative float (only its sign was flipped)
    bits = torch.where(keys_u64 < 0, keys_u64 ^ sign, ~keys_u64)
    return bits.view(torch.float64).to(dtype)


def group_offsets(keys: List[torch.Tensor],
                  masks: Optional[List[Optional[torch.Tensor]]] = None
                  ) -> torch.Tensor:
    """Offsets [n_groups + 1] of runs of adjacent equal rows.

    ``keys`` are normalize_key() columns; ``masks[i]`` is a validity
    tensor or None.  Row i starts a group if i == 0 or any column's
    (null flag, key) differs from row i - 1; the stored key of a null row
    is ignored, so adjacent nulls of a column compare equal."""
    n = keys[0].numel()
    if n == 0:
        return torch.zeros(1, dtype=torch.int64)
    head = torch.zeros(n, dtype=torch.bool)
    head[0] = True
    for ci, k in enumerate(keys):
        m = masks[ci] if masks is not None else None
        diff = k[1:] != k[:-1]
        if m is not None and m.numel():
            mb = m.to(torch.bool)
            diff = (mb[1:] != mb[:-1]) | (mb[1:] & diff)
        head[1:] |= diff
    starts = torch.nonzero(head, as_tuple=False).flatten()
    return torch.cat([starts, torch.tensor([n], dtype=torch.int64)])


SEGMENTED_REDUCE_OUTPUTS = ("sum", "min", "max", "count")


def segmented_reduce(values: torch.Tensor, valid: Optional[torch.Tensor],
                     offsets: torch.Tensor,
                     want=SEGMENTED_REDUCE_OUTPUTS) -> dict:
    """Per group [offsets[g], offsets[g+1]): ``sum`` (int64 with
    wrap-around for integers, float64 for floats), ``min`` / ``max`` (input
    dtype, normalize_key order, so -0.0 < +0.0 and NaN sorts outermost)
    and ``count`` of the valid rows.  Null rows (valid False) take no part;
    a group without a valid row has count 0 and zeros elsewhere.  A float
    sum starts from +0.0.  Returns a dict with the names in ``want``."""
    offsets = offsets.to(torch.int64)
    G = offsets.numel() - 1
    n = values.numel()
    is_float = values.dtype.is_floating_point
    acc = torch.float64 if is_float else torch.int64
    gid = torch.repeat_interleave(torch.arange(G, dtype=torch.int64),
                                  offsets[1:] - offsets[:-1])
    v = (valid.to(torch.bool) if valid is not None and valid.numel()
         else torch.ones(n, dtype=torch.bool))
    out = {}
    cnt = torch.zeros(G, dtype=torch.int64).index_add_(
        0, gid, v.to(torch.int64))
    if "count" in want:
        out["count"] = cnt
    if "sum" in want:
        x = torch.where(v, values.to(acc), torch.zeros((), dtype=acc))
        out["sum"] = torch.zeros(G, dtype=acc).index_add_(0, gid, x)
    if "min" in want or "max" in want:
        sortable = _as_unsigned_sortable(normalize_key(values))
        empty = cnt == 0
        for name, red, ident in (
                ("min", "amin", 0x7FFFFFFFFFFFFFFF),
                ("max", "amax", -0x8000000000000000)):
            if name not in want:
                continue
            s = torch.where(v, sortable, torch.full_like(sortable, ident))
            r = torch.full((G,), ident, dtype=torch.int64).scatter_reduce_(
                0, gid, s, red, include_self=True)
            val = denormalize_key(_as_unsigned_sortable(r), values.dtype)
            out[name] = torch.where(empty, torch.zeros_like(val), val)
    return out
