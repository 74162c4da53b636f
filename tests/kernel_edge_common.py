"""Shared builders and oracles for the kernel-edge tests (CPU and GPU).

Everything here is plain Python / numpy: a snappy raw-block stream
builder with a byte-wise reference decoder, a parquet RLE/bit-packed
hybrid encoder, the hand-built page sets both test modules use, and the
numpy oracles for the ops that ``cpu_ref`` does not cover.  The CPU
module (test_kernel_edge_builders.py) checks these against independent
decoders before the GPU module (test_kernel_edges_gpu.py) trusts them.
"""

import numpy as np
import torch

from hyperspace_amd.ops import cpu_ref

U64 = (1 << 64) - 1


def as_i64(values_u64):
    """Python ints / uint64 array (u64 bit patterns) -> int64 tensor."""
    return torch.from_numpy(
        np.asarray(values_u64, dtype=np.uint64).view(np.int64).copy())


# ---------------------------------------------------------------------------
# Snappy raw-block builder (format_description.txt of google/snappy)
# ---------------------------------------------------------------------------

def varint(n):
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _literal_tag(n, forced_len_bytes=None):
    """Tag (+ length bytes) of an n-byte literal.  ``forced_len_bytes``
    0 = length inline in the tag (n <= 60), 1..4 = that many explicit
    length bytes even when fewer would do (a legal non-minimal form)."""
    assert n >= 1
    if forced_len_bytes is None:
        if n <= 60:
            forced_len_bytes = 0
        else:
            forced_len_bytes = max(1, ((n - 1).bit_length() + 7) // 8)
    if forced_len_bytes == 0:
        assert n <= 60
        return bytes([(n - 1) << 2])
    assert 1 <= forced_len_bytes <= 4
    assert n - 1 < 1 << (8 * forced_len_bytes)
    return bytes([(59 + forced_len_bytes) << 2]) + \
        (n - 1).to_bytes(forced_len_bytes, "little")


def snappy_ops_bytes(ops):
    """Tag stream of an op list, WITHOUT the leading varint and without
    validating offsets (malformed pages are built with this too).
    Ops: ("L", bytes[, forced_len_bytes]), ("C1", off, len),
    ("C2", off, len), ("C4", off, len)."""
    out = bytearray()
    for op in ops:
        kind = op[0]
        if kind == "L":
            data = op[1]
            out += _literal_tag(len(data), op[2] if len(op) > 2 else None)
            out += data
        elif kind == "C1":
            _, off, ln = op
            assert 4 <= ln <= 11 and 0 <= off < 2048
            out += bytes([1 | ((ln - 4) << 2) | ((off >> 8) << 5),
                          off & 0xFF])
        elif kind == "C2":
            _, off, ln = op
            assert 1 <= ln <= 64 and 0 <= off < 1 << 16
            out += bytes([2 | ((ln - 1) << 2)]) + off.to_bytes(2, "little")
        elif kind == "C4":
            _, off, ln = op
            assert 1 <= ln <= 64 and 0 <= off < 1 << 32
            out += bytes([3 | ((ln - 1) << 2)]) + off.to_bytes(4, "little")
        else:
            raise ValueError(kind)
    return bytes(out)


def snappy_reference(ops):
    """Byte-wise decode of a VALID op list: a copy with off < len repeats
    the off-byte pattern, exactly as a serial decoder produces it."""
    out = bytearray()
    for op in ops:
        if op[0] == "L":
            out += op[1]
        else:
            _, off, ln = op
            assert 1 <= off <= len(out), (op, len(out))
            for _ in range(ln):
                out.append(out[-off])
    return bytes(out)


def snappy_stream(ops):
    """(raw-block stream, reference output) of a valid op list."""
    ref = snappy_reference(ops)
    return varint(len(ref)) + snappy_ops_bytes(ops), ref


def _rb(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _mixed_ops(rng, n_ops):
    """A short, copy-dense op list (what a compressed page looks like)."""
    ops = [("L", _rb(rng, int(rng.integers(9, 40))))]
    size = len(ops[0][1])
    for _ in range(n_ops):
        r = int(rng.integers(0, 4))
        if r == 0:
            data = _rb(rng, int(rng.integers(1, 70)))
            ops.append(("L", data))
            size += len(data)
        elif r == 1:
            ln = int(rng.integers(4, 12))
            ops.append(("C1", int(rng.integers(1, min(size, 2047) + 1)), ln))
            size += ln
        else:
            ln = int(rng.integers(1, 65))
            ops.append(("C2" if r == 2 else "C4",
                        int(rng.integers(1, size + 1)), ln))
            size += ln
    return ops


def snappy_valid_pages():
    """Hand-built valid pages: list of dicts with ``name``, ``ops``,
    ``trailing`` (unused bytes after the last op), and the alignment the
    page asks of its source start (``src_mod``: src_off % 8) or of its
    destination start (``dst_mod``: dst_off % 16); None = don't care."""
    rng = np.random.default_rng(1234)
    pages = []

    def page(name, ops, trailing=b"", src_mod=None, dst_mod=None):
        pages.append(dict(name=name, ops=ops, trailing=trailing,
                          src_mod=src_mod, dst_mod=dst_mod))

    # every tag kind, every literal length encoding, the length edges
    ops = [("L", _rb(rng, 1)), ("L", _rb(rng, 60)), ("L", _rb(rng, 61)),
           ("C1", 4, 4), ("C1", 100, 11), ("C2", 122, 64),
           ("L", _rb(rng, 255)), ("L", _rb(rng, 256)),
           ("L", _rb(rng, 257)),
           ("C4", 5, 20),            # 4-byte offset, small and overlapping
           ("C4", 300, 64),
           ("L", _rb(rng, 10), 1), ("L", _rb(rng, 20), 2),
           ("L", _rb(rng, 300), 3), ("L", _rb(rng, 100), 4),
           ("L", _rb(rng, 5003)),
           ("C1", 2047, 7),
           ("L", _rb(rng, 70_001)),  # 3-byte length by necessity
           ("C4", 66_000, 64),       # offset past the 2-byte range
           ("C4", 70_000, 33),
           ("C2", 65_535, 64),
           ("L", _rb(rng, 3))]
    page("all_tags", ops)

    # overlapping copies: a fresh literal before each so the pattern
    # that has to repeat is not already periodic
    ops = []
    for off in (1, 2, 3, 5, 7, 63):
        ops.append(("L", _rb(rng, 67)))
        ops.append(("C2", off, 64))
    ops.append(("L", _rb(rng, 9)))
    for off in (1, 2, 3, 5, 7):
        ops.append(("C1", off, 11))
        ops.append(("C4", off, 64))
    page("overlap", ops)

    page("c1_edges", [("L", _rb(rng, 2100)), ("C1", 2047, 4),
                      ("C1", 2047, 11), ("C1", 1, 4), ("C1", 4, 4),
                      ("C1", 11, 11), ("C1", 256, 5), ("C1", 255, 6)])

    # source start alignment 0..7 (drives the cursor's aligned-down window)
    for r in range(8):
        page(f"src_mod{r}", _mixed_ops(rng, 24), src_mod=r)

    # one long literal at each destination alignment: followed by a short
    # literal (the 16-byte body path has source room) and as the page's
    # last op (no room: byte path)
    for r in range(16):
        page(f"dst_mod{r}_wide",
             [("L", _rb(rng, 256 + 3 * r)), ("L", _rb(rng, 20))],
             dst_mod=r)
    for r in range(16):
        page(f"dst_mod{r}_last", [("L", _rb(rng, 289 - r))], dst_mod=r)

    page("tiny", [("L", _rb(rng, 3))])               # 5 bytes in all
    page("tiny_copy", [("L", b"\x07"), ("C1", 1, 4)])  # 5 bytes in all
    page("empty_output", [])                          # the varint alone
    page("trailing", _mixed_ops(rng, 12), trailing=b"\xff\x00\xfe")
    return pages


def snappy_malformed_pages():
    """(name, stream bytes, dst_len, expected status).  Status codes of
    k_snappy_decomp: 1 varint != dst_len, 2 literal overruns the page,
    3 bad copy offset or op overruns dst_len, 4 stream ends early."""
    lit8 = bytes(range(8))
    good, ref = snappy_stream([("L", lit8), ("C2", 3, 9)])
    return [
        ("wrong_varint", good, len(ref) + 1, 1),
        ("literal_overruns_page",
         varint(100) + _literal_tag(100) + bytes(10), 100, 2),
        ("copy_off_zero",
         varint(20) + snappy_ops_bytes([("L", lit8), ("C2", 0, 4)]), 20, 3),
        ("copy_off_past_out",
         varint(20) + snappy_ops_bytes([("L", lit8), ("C2", 9, 4)]), 20, 3),
        ("op_overruns_dst",
         varint(10) + snappy_ops_bytes([("L", lit8), ("C2", 4, 8)]), 10, 3),
        ("stream_ends_early",
         varint(100) + snappy_ops_bytes([("L", lit8)]), 100, 4),
    ]


def snappy_layout(pages):
    """Lay pages out in one source blob and one destination buffer,
    honouring each page's src_mod / dst_mod by padding in front of it.
    ``pages``: dicts with ``stream`` (bytes incl. trailing), ``dst_len``
    and optional ``src_mod`` / ``dst_mod``.  Returns (blob, src_off,
    src_end, dst_off, dst_total)."""
    blob = bytearray()
    src_off, src_end, dst_off = [], [], []
    dpos = 0
    for p in pages:
        if p.get("src_mod") is not None:
            while len(blob) % 8 != p["src_mod"]:
                blob.append(0xEE)
        if p.get("dst_mod") is not None:
            while dpos % 16 != p["dst_mod"]:
                dpos += 1
        src_off.append(len(blob))
        blob += p["stream"]
        src_end.append(len(blob))
        dst_off.append(dpos)
        dpos += p["dst_len"]
    return bytes(blob), src_off, src_end, dst_off, dpos


# ---------------------------------------------------------------------------
# Parquet RLE / bit-packed hybrid encoder
# ---------------------------------------------------------------------------

def rle_encode(runs, bw):
    """Encode ("rep", value, count) / ("lit", values) runs at bit width
    ``bw`` (no leading bit-width byte).  A literal run is written in
    groups of 8 values; only the LAST run may be short — its final group
    is zero-padded in the stream and the padding is not part of the
    values.  Returns (bytes, values as a uint32 array)."""
    out = bytearray()
    vals = []
    vbytes = (bw + 7) // 8
    for ri, run in enumerate(runs):
        if run[0] == "rep":
            _, v, count = run
            assert 0 <= v < 1 << bw and count >= 1
            out += varint(count << 1)
            out += int(v).to_bytes(vbytes, "little")
            vals += [v] * count
        else:
            lit = [int(v) for v in run[1]]
            assert all(0 <= v < 1 << bw for v in lit)
            assert len(lit) % 8 == 0 or ri == len(runs) - 1
            groups = (len(lit) + 7) // 8
            out += varint((groups << 1) | 1)
            acc = 0
            for i, v in enumerate(lit):
                acc |= v << (i * bw)   # little-endian bit order
            out += acc.to_bytes(groups * bw, "little")
            vals += lit
    return bytes(out), np.array(vals, dtype=np.uint32)


def rle_case(bw, seed=0):
    """The mixed stream of the RLE tests at one bit width: repeat runs
    of 1, 64, 65 and 1000, literal runs of 8 and 72, and a final literal
    run of 13 (last group short).  Values include 0 and 2**bw - 1; at
    bw = 32 that also puts values at or above 2**31 in every run kind."""
    rng = np.random.default_rng(1000 * seed + bw)
    top = (1 << bw) - 1

    def lit(n):
        v = [int(x) for x in rng.integers(0, top + 1, n, dtype=np.uint64)]
        v[0], v[n // 2], v[-1] = top, 0, top
        if bw > 1:
            v[1] = top - 1
        if n > 16:
            v[7], v[8] = top, top   # all-ones across a group boundary
        return v

    runs = [("rep", top, 1), ("lit", lit(8)), ("rep", 0, 64),
            ("rep", top, 65), ("lit", lit(72)),
            ("rep", int(rng.integers(0, top + 1, dtype=np.uint64)) | (
                top ^ (top >> 1)), 1000),  # top bit set
            ("lit", lit(13))]
    return runs


RLE_BIT_WIDTHS = tuple(range(1, 33))


# ---------------------------------------------------------------------------
# numpy oracles where cpu_ref has none
# ---------------------------------------------------------------------------

def exclusive_scan_ref(x):
    """int64 array -> (exclusive prefix sums, total)."""
    x = np.asarray(x, dtype=np.int64)
    inc = np.cumsum(x, dtype=np.int64)
    return inc - x, int(inc[-1]) if x.size else 0


def copy_unaligned_ref(src, src_off, nbytes):
    return np.asarray(src, dtype=np.uint8)[src_off:src_off + nbytes]


def bloom_probe_many_ref(vals, words, m_bits, k):
    """bool[n_filters]: does ANY value probe positive in filter f."""
    return torch.tensor(
        [bool(cpu_ref.bloom_probe(vals, words[f], m_bits, k).any())
         for f in range(words.shape[0])], dtype=torch.bool)


def scan_inputs():
    """(name, int64 array) inputs of the exclusive-scan tests."""
    rng = np.random.default_rng(77)
    cases = []
    for n in (1, 255, 256, 257, 513, 65_537, 524_289):
        x = rng.integers(-1000, 1001, n, dtype=np.int64)
        big = rng.integers(0, n, min(n, 5))
        x[big] = np.where(rng.integers(0, 2, big.size) == 0,
                          2**40, -(2**40))
        cases.append((f"random_{n}", x))
    cases.append(("all_zero_1000", np.zeros(1000, dtype=np.int64)))
    x = rng.integers(1, 1000, 1000, dtype=np.int64)
    x[:256] = 0
    cases.append(("first_256_zero", x))
    return cases


# ---------------------------------------------------------------------------
# Special-value float arrays (normalize_key / murmur3)
# ---------------------------------------------------------------------------

def float_specials(dtype):
    """Strictly ascending special values in numeric order, -0.0 directly
    before +0.0 and NaN last — the order unsigned comparison of
    normalize_key's output must reproduce."""
    if dtype == np.float32:
        fi = np.finfo(np.float32)
        tiny_sub = np.float32(1e-45)            # smallest denormal
        big_sub = np.float32(1.1754942e-38)     # largest denormal
        mid = [np.float32(0.1), np.float32(1) / np.float32(3),
               np.float32(1.0), np.nextafter(np.float32(1), np.float32(2)),
               np.float32(16777216.0)]
    else:
        fi = np.finfo(np.float64)
        tiny_sub = np.float64(5e-324)
        big_sub = np.nextafter(fi.tiny, 0.0)
        mid = [0.1, 1.0 / 3.0, 1.0, np.nextafter(1.0, 2.0), 2.0**53]
    pos = [tiny_sub, big_sub, fi.tiny] + mid + [fi.max, np.inf]
    vals = [-v for v in reversed(pos)] + [-0.0, 0.0] + pos + [np.nan]
    arr = np.array(vals, dtype=dtype)
    body = arr[:-1]
    assert (np.diff(body.astype(np.float64)) >= 0).all()
    assert np.isnan(arr[-1]) and not np.signbit(arr[-1])
    return arr


def bits_of(arr):
    return arr.view(np.uint32 if arr.dtype == np.float32 else np.uint64)


# ---------------------------------------------------------------------------
# Radix-sort key shapes
# ---------------------------------------------------------------------------

RADIX_SHAPES = ("all_equal", "top_byte", "bit63", "extremes", "sorted",
                "reverse", "all_bytes")


def radix_keys(shape, n, seed=0):
    """int64 tensor of u64 key bit patterns of one named shape."""
    rng = np.random.default_rng(seed + 31 * RADIX_SHAPES.index(shape))
    const = np.uint64(0x00A5_5A3C_C3F0_0F77)
    if shape == "all_equal":
        k = np.full(n, 0x92A5_5A3C_C3F0_0F77, dtype=np.uint64)
    elif shape == "top_byte":      # only bits 56..63 vary
        k = (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(56)) \
            | const
    elif shape == "bit63":         # only bit 63 varies
        k = (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63)) \
            | const
    elif shape == "extremes":      # keys from {0, 2**64 - 1}
        k = np.where(rng.integers(0, 2, n) == 0, np.uint64(0),
                     np.uint64(U64))
    else:
        k = rng.integers(0, U64, n, dtype=np.uint64, endpoint=True)
        if shape == "sorted":
            k = np.sort(k)
        elif shape == "reverse":
            k = np.sort(k)[::-1].copy()
    return as_i64(k)


def varying_mask(keys_i64):
    """OR over (key ^ key[0]): the mask the sort plans its passes from."""
    k = keys_i64.numpy().view(np.uint64)
    return int(np.bitwise_or.reduce(k ^ k[0]))


def check_plan_covers(mask, radix, shifts):
    """Every set bit of ``mask`` lies in exactly one digit window, and
    the shifts ascend strictly."""
    bits = {256: 8, 512: 9}[radix]
    assert all(a < b for a, b in zip(shifts, shifts[1:])), shifts
    cover = [0] * 64
    for s in shifts:
        assert 0 <= s < 64
        for b in range(s, min(s + bits, 64)):
            cover[b] += 1
    for b in range(64):
        if (mask >> b) & 1:
            assert cover[b] == 1, (hex(mask), radix, shifts, b)
        else:
            assert cover[b] <= 1, (hex(mask), radix, shifts, b)


# the three key ranges of test_radix_sort_nine_bit_planner
NINE_BIT_RANGES = ((0, 1 << 26), (1 << 8, 1 << 17), (0, 1 << 18))
