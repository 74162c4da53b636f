"""Host staging shared by the parquet read paths: the pinned-buffer pool,
the host codec pool and the snappy device/host split knob."""

from __future__ import annotations

import os
import threading as _threading
from typing import Dict, List

import torch

# Pinned host staging buffers are expensive to allocate (~60 ms/GB —
# comparable to the copy itself), so the device read path recycles them
# through a size-classed pool.  Classes are 8 MiB-granular above 8 MiB
# (pow2 wastes up to 2x of the budget on ~40-60 MB parquet files) and
# power-of-two below; total bounded per process (8 ranks share a node's
# host RAM).
_PINNED_POOL: Dict[int, List["torch.Tensor"]] = {}
_PINNED_POOL_BYTES = 0
# Default 32 GiB: a build-then-serve step keeps BOTH the source-staging
# classes (~few large buffers) and the index-read classes (~hundreds of
# bucket files) resident; a 16 GiB cap evicted one set every step and
# re-paid ~190 ms/GB of pinned allocation on the cold query read
# (profiles/cold_read_probe: full path 8.3 GB/s pool-cold vs 36 GB/s
# pool-warm, H2D-bound).  HS_PINNED_POOL_GB overrides.
_PINNED_POOL_MAX = int(
    float(os.environ.get("HS_PINNED_POOL_GB", "32")) * (1 << 30))

_pool_lock = _threading.Lock()


def _pinned_size_class(nbytes: int) -> int:
    if nbytes > (8 << 20):
        gran = 8 << 20
        return (nbytes + gran - 1) // gran * gran
    return 1 << max(12, (nbytes - 1).bit_length())


def _pinned_get(nbytes: int) -> "torch.Tensor":
    global _PINNED_POOL_BYTES
    size = _pinned_size_class(nbytes)
    with _pool_lock:
        # exact class first, then up to 2x oversized (a 48 MB index-file
        # read can reuse a 64 MB source-staging buffer instead of paying
        # a fresh pinned allocation)
        cls = size
        while cls <= 2 * size:
            lst = _PINNED_POOL.get(cls)
            if lst:
                _PINNED_POOL_BYTES -= cls
                return lst.pop()
            cls += (8 << 20) if cls >= (8 << 20) else cls
    return torch.empty(size, dtype=torch.uint8, pin_memory=True)


def _pinned_put(buf: "torch.Tensor") -> None:
    global _PINNED_POOL_BYTES
    size = buf.numel()
    with _pool_lock:
        if _PINNED_POOL_BYTES + size <= _PINNED_POOL_MAX:
            _PINNED_POOL.setdefault(size, []).append(buf)
            _PINNED_POOL_BYTES += size


_CODEC_POOL = None
_codec_tl = _threading.local()
# snappy pages with comp >= ratio*unc (near-incompressible, giant
# literals) decode on device; the rest are copy-dense -> host codec
# pool.  0.93 measured best (see profiles/r2_summary.md); 0 = all
# device, >1 = all host (sweep knob).
_DEV_RATIO = float(os.environ.get("HS_SNAPPY_DEV_RATIO", "0.93"))


def _codec_pool():
    """Shared host-codec thread pool (gzip/zstd/lz4/copy-dense-snappy
    page decompression; the codecs release the GIL)."""
    global _CODEC_POOL
    if _CODEC_POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _CODEC_POOL = ThreadPoolExecutor(
            max_workers=int(os.environ.get("HS_CODEC_WORKERS", "16")),
            thread_name_prefix="hs-codec")
    return _CODEC_POOL


def _tl_decompress(name: str, view, unc: int):
    """Decompress with a THREAD-LOCAL pyarrow codec: a pa.Codec shared
    across threads segfaults (reproduced with zstd at 16 threads), so
    each pool worker keeps its own instance per codec name."""
    c = getattr(_codec_tl, name, None)
    if c is None:
        import pyarrow as _pa
        c = _pa.Codec(name)
        setattr(_codec_tl, name, c)
    return c.decompress(view, unc)
