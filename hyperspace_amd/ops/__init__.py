"""Data-plane ops with CPU/HIP dispatch.

Each op routes CUDA tensors to the hand-written HIP/CDNA4 kernels
(csrc/kernels/*.hip, built as hyperspace_amd._hip) and CPU tensors to the
torch reference implementation (cpu_ref.py).  On CUDA the native extension
is REQUIRED — there is no silent PyTorch fallback (KernelUnavailableError).

Op -> reference data-plane mapping:
  murmur3_bucket   K2  hash partitioning (Spark HashPartitioning-compatible,
                       null keys pass the seed through)
  sort_pairs       K3  per-bucket sort (stable LSD radix on device)
  bucket_sort_perm K3  fused (bucket, integer key) sort of the index build
  merge_join       K4  co-bucketed sort-merge join (two-phase per-tile)
  run_merge_perm   K4b segmented two-sorted-run merge (multi-file buckets)
  select_range     K1/filter scan predicate + compaction
  isin_sorted      K7  lineage delete filter
  segmented_minmax K8  data-skipping MinMax sketch
  bloom_build/probe K8 data-skipping BloomFilter sketch
  zorder_key       K10 z-address bit interleave
  group_offsets    K13 group-by: offsets of adjacent equal-key runs
  segmented_reduce K13 group-by: fused per-group sum/min/max/count
  topk_rows        K14 ORDER BY ... LIMIT: radix select of the k smallest keys
  order_key        K14 sql_key, complemented for a descending order
  (extension-only: copy_unaligned/rle_decode/snappy_decompress — the K1
  parquet page decode surface used by sources/parquet_io.py)
"""

from __future__ import annotations

from typing import List, Tuple

import torch

from . import cpu_ref, native
from .cpu_ref import MASK32, SPARK_HASH_SEED  # re-export

__all__ = [
    "murmur3_bucket", "normalize_key", "sql_key", "sort_pairs", "sort_perm",
    "merge_join", "run_merge_perm", "select_range_u64", "isin_sorted", "segmented_minmax",
    "bloom_build", "bloom_probe", "bloom_probe_many", "zorder_key", "gather_rows", "native",
    "group_offsets", "segmented_reduce", "group_tile_size",
    "bucket_sort_perm", "order_key", "topk_rows", "topk_tile_size",
]


def normalize_key(col: torch.Tensor) -> torch.Tensor:
    if col.is_cuda:
        return native.ext().normalize_key(col.contiguous())
    return cpu_ref.normalize_key(col)


def sql_key(col: torch.Tensor) -> torch.Tensor:
    """normalize_key under SQL equality: -0.0 keys as +0.0 and every NaN
    as one key above +inf (same single kernel pass; integers unchanged).
    Filters, join keys and the index build sort compare these."""
    if col.is_cuda:
        return native.ext().normalize_key(col.contiguous(), True)
    return cpu_ref.sql_key(col)


def order_key(col: torch.Tensor, descending: bool = False) -> torch.Tensor:
    """sql_key for an ORDER BY column: ascending u64 order of the result
    is the requested order of the values.  Descending is the bitwise
    complement of sql_key, taken in the same kernel pass."""
    if col.is_cuda:
        return native.ext().normalize_key(col.contiguous(), True,
                                          bool(descending))
    key = cpu_ref.sql_key(col)
    return ~key if descending else key


def gather_rows(values: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    if values.is_cuda:
        return native.ext().gather_rows(values.contiguous(),
                                        idx.contiguous())
    return values[idx]


_INT_KEY_DTYPES = (torch.int64, torch.int32, torch.int16, torch.int8,
                   torch.bool)


def bucket_sort_perm(key: torch.Tensor, bucket_ids: torch.Tensor,
                     num_buckets: int):
    """Fused (bucket, key) sort for one non-null integer key column on
    the device: one stable sort of the composite
    ``(bucket << S) | (normalized key - kmin)``.

    Returns ``(perm, sorted_key, seg)``: the int32 permutation that sorts
    the rows by (bucket, key) keeping source order among equals, the key
    column already in that order, and the num_buckets + 1 segment offsets
    (int64, CPU).  Returns None when the shape is not eligible: a CPU
    tensor, a non-integer key, a key range too wide to sit beside the
    bucket bits in 64 bits, fewer than 2 rows or 2^31 rows and more.
    ``bucket_ids`` must lie in [0, num_buckets)."""
    if (not isinstance(key, torch.Tensor) or not key.is_cuda
            or not bucket_ids.is_cuda or key.dtype not in _INT_KEY_DTYPES
            or not 1 < key.numel() < 1 << 31):
        return None
    res = native.ext().bucket_sort_perm(
        key.contiguous(), bucket_ids.to(torch.int32).contiguous(),
        num_buckets)
    return None if res is None else tuple(res)


def _is_cuda(*tensors: torch.Tensor) -> bool:
    return any(t.is_cuda for t in tensors)


def murmur3_bucket(keys: List[torch.Tensor], num_buckets: int,
                   masks=None) -> torch.Tensor:
    """masks: optional list parallel to keys; entries are bool validity
    tensors or None (no nulls in that key column).  Float keys hash
    their canonical bits: -0.0 as +0.0, every NaN as the quiet NaN."""
    if _is_cuda(*keys):
        if masks is not None and any(m is not None for m in masks):
            mlist = [
                (m.contiguous() if m is not None
                 else torch.empty(0, dtype=torch.bool,
                                  device=keys[0].device))
                for m in masks]
            return native.ext().murmur3_bucket(list(keys), num_buckets,
                                               mlist)
        return native.ext().murmur3_bucket(list(keys), num_buckets)
    return cpu_ref.murmur3_bucket(keys, num_buckets, masks)


def sort_pairs(keys_u64: torch.Tensor, payload: torch.Tensor
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Stable sort (u64-ordered keys stored as int64, int64 payload)."""
    if _is_cuda(keys_u64):
        return native.ext().radix_sort_pairs(keys_u64, payload)
    return cpu_ref.stable_sort_u64(keys_u64, payload)


def sort_perm(keys_u64: torch.Tensor) -> torch.Tensor:
    """Permutation that stably sorts keys_u64 under u64 order."""
    n = keys_u64.numel()
    payload = torch.arange(n, dtype=torch.int64, device=keys_u64.device)
    _, perm = sort_pairs(keys_u64, payload)
    return perm


def run_merge_perm(keys_u64: torch.Tensor, seg: torch.Tensor,
                   split: torch.Tensor) -> torch.Tensor:
    """Segmented two-sorted-run merge permutation (K4b): one launch
    merges every bucket's [A-run | B-run] layout into sorted order."""
    if keys_u64.is_cuda:
        return native.ext().run_merge_perm(keys_u64.contiguous(), seg,
                                           split)
    return cpu_ref.run_merge_perm(keys_u64, seg, split)


def merge_join(lkeys: torch.Tensor, rkeys: torch.Tensor,
               lseg: torch.Tensor, rseg: torch.Tensor,
               mode: str = "inner"
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Segmented sorted merge join.  ``mode`` is one of ``"inner"``,
    ``"left_outer"`` (an unmatched left row yields the pair (i, -1)),
    ``"left_semi"`` and ``"left_anti"`` (left indices only; the second
    tensor is empty).  Output is ascending by left row in every mode."""
    code = cpu_ref.merge_join_mode_code(mode)
    if _is_cuda(lkeys, rkeys):
        if code == 0:
            return native.ext().merge_join(lkeys, rkeys, lseg, rseg)
        return native.ext().merge_join(lkeys, rkeys, lseg, rseg, code)
    return cpu_ref.merge_join(lkeys, rkeys, lseg, rseg, mode)


def select_range_u64(keys_u64: torch.Tensor, lo: int, hi: int,
                     lo_incl: bool = True, hi_incl: bool = True
                     ) -> torch.Tensor:
    if _is_cuda(keys_u64):
        return native.ext().select_range_u64(
            keys_u64, lo, hi, lo_incl, hi_incl)
    return cpu_ref.select_range_u64(keys_u64, lo, hi, lo_incl, hi_incl)


def isin_sorted(values: torch.Tensor, sorted_set: torch.Tensor
                ) -> torch.Tensor:
    if _is_cuda(values):
        return native.ext().isin_sorted(values, sorted_set)
    return cpu_ref.isin_sorted(values, sorted_set)


def segmented_minmax(vals: torch.Tensor, seg_off: torch.Tensor
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    if _is_cuda(vals):
        return native.ext().segmented_minmax(vals, seg_off)
    return cpu_ref.segmented_minmax(vals, seg_off)


def bloom_build(vals: torch.Tensor, m_bits: int, k: int) -> torch.Tensor:
    if _is_cuda(vals):
        return native.ext().bloom_build(vals, m_bits, k)
    return cpu_ref.bloom_build(vals, m_bits, k)


def bloom_probe(vals: torch.Tensor, words: torch.Tensor, m_bits: int, k: int
                ) -> torch.Tensor:
    if _is_cuda(vals):
        return native.ext().bloom_probe(vals, words, m_bits, k)
    return cpu_ref.bloom_probe(vals, words, m_bits, k)


def bloom_probe_many(vals: torch.Tensor, words: torch.Tensor, m_bits: int,
                     k: int) -> torch.Tensor:
    """K9 batched sketch-predicate probe: ``words`` is [n_filters,
    words_per_filter]; returns bool[n_filters] = any value may be in
    that filter (device kernel when the tensors are on GPU)."""
    if _is_cuda(vals):
        return native.ext().bloom_probe_many(vals, words, m_bits, k)
    out = torch.zeros(words.shape[0], dtype=torch.bool)
    for f in range(words.shape[0]):
        out[f] = bool(cpu_ref.bloom_probe(vals, words[f], m_bits, k)
                      .any())
    return out


def zorder_key(cols_u64: List[torch.Tensor], bits_per_col: int
               ) -> torch.Tensor:
    if _is_cuda(*cols_u64):
        return native.ext().zorder_key(list(cols_u64), bits_per_col)
    return cpu_ref.zorder_key(cols_u64, bits_per_col)


def group_tile_size() -> int:
    """Rows per tile of the device group-by kernels (tests aim at it)."""
    return int(native.ext().group_tile_size())


def topk_tile_size() -> int:
    """Rows per tile of the device top-k kernels (tests aim at it)."""
    return int(native.ext().topk_tile_size())


def topk_rows(keys_u64: torch.Tensor, k: int, valid=None,
              keep_ties: bool = False) -> torch.Tensor:
    """int64 row indices, ascending, of the rows holding the ``k`` smallest
    keys (u64 order) among those with ``valid[i]`` true (all rows when
    ``valid`` is None).  With T the k-th smallest such key: every valid row
    below T, then of the rows equal to T all of them (``keep_ties``) or
    the first k - #below in row order, so exactly min(k, n_valid) rows.
    k <= 0 gives no row; the stored key of an invalid row is ignored.
    On the device this is a radix select: no sort, one host read (the
    output length)."""
    k = min(int(k), keys_u64.numel())
    if _is_cuda(keys_u64):
        v = (valid.contiguous() if valid is not None
             else torch.empty(0, dtype=torch.bool, device=keys_u64.device))
        return native.ext().topk_rows(keys_u64.contiguous(), k, v,
                                      bool(keep_ties))
    return cpu_ref.topk_rows(keys_u64, k, valid, keep_ties)


def group_offsets(keys: List[torch.Tensor], masks=None) -> torch.Tensor:
    """Offsets [n_groups + 1] (int64) of the runs of adjacent equal rows.

    ``keys``: one to eight normalize_key()-ed columns.  ``masks``:
    optional list parallel to keys of validity tensors or None.  A row
    starts a group if it is row 0 or any column's (null flag, key) differs
    from the previous row; the stored value of a null row is ignored."""
    if not 1 <= len(keys) <= 8:
        raise ValueError("group_offsets takes one to eight key columns")
    if _is_cuda(*keys):
        dev = keys[0].device
        klist = [k.contiguous() for k in keys]
        if masks is not None and any(m is not None for m in masks):
            mlist = [(m.contiguous() if m is not None
                      else torch.empty(0, dtype=torch.bool, device=dev))
                     for m in masks]
            return native.ext().group_offsets(klist, mlist)
        return native.ext().group_offsets(klist)
    return cpu_ref.group_offsets(keys, masks)


_WANT_BITS = {"sum": 1, "min": 2, "max": 4, "count": 0}


def segmented_reduce(values: torch.Tensor, valid, offsets: torch.Tensor,
                     want=cpu_ref.SEGMENTED_REDUCE_OUTPUTS) -> dict:
    """Fused per-group reduce over ``offsets`` (as group_offsets gives
    them): a dict with the entries of ``want`` among ``sum`` (int64 with
    wrap-around for integers, float64 for floats), ``min`` / ``max`` (the
    input dtype, normalize_key order) and ``count`` (valid rows), all from
    one read of ``values``.  ``valid`` is a validity tensor or None.
    int8/int16/bool values are widened to int32 here."""
    for w in want:
        if w not in _WANT_BITS:
            raise ValueError(f"segmented_reduce: unknown output {w!r}")
    if values.dtype in (torch.int8, torch.int16, torch.bool, torch.uint8):
        values = values.to(torch.int32)
    if values.dtype not in (torch.int32, torch.int64, torch.float32,
                            torch.float64):
        raise ValueError(
            f"segmented_reduce: unsupported dtype {values.dtype}")
    if _is_cuda(values):
        bits = 0
        for w in want:
            bits |= _WANT_BITS[w]
        v = (valid.contiguous() if valid is not None
             else torch.empty(0, dtype=torch.bool, device=values.device))
        s, mn, mx, cnt = native.ext().segmented_reduce(
            values.contiguous(), v, offsets, bits)
        full = {"sum": s, "min": mn, "max": mx, "count": cnt}
        return {w: full[w] for w in want}
    return cpu_ref.segmented_reduce(values, valid, offsets.cpu(), want)
