"""CPU checks of the kernel-edge builders and oracles.

The GPU module compares the HIP kernels with what kernel_edge_common.py
builds; these tests pin that ground truth to independent implementations
first: pyarrow's snappy codec, the host RLE decoder of native_parquet,
and plain numeric order for normalize_key.
"""

import numpy as np
import pyarrow as pa
import pytest
import torch

from hyperspace_amd.ops import cpu_ref
from hyperspace_amd.sources.native_parquet import _decode_rle_indices

import kernel_edge_common as kc


def test_varint_and_literal_tags():
    assert kc.varint(0) == b"\x00"
    assert kc.varint(127) == b"\x7f"
    assert kc.varint(128) == b"\x80\x01"
    assert kc.varint(70_001) == b"\xf1\xa2\x04"
    # inline, minimal and forced (non-minimal) literal lengths
    assert kc._literal_tag(1) == b"\x00"
    assert kc._literal_tag(60) == bytes([59 << 2])
    assert kc._literal_tag(61) == bytes([60 << 2, 60])
    assert kc._literal_tag(256) == bytes([60 << 2, 255])
    assert kc._literal_tag(257) == bytes([61 << 2, 0, 1])
    assert kc._literal_tag(70_001) == bytes([62 << 2]) + \
        (70_000).to_bytes(3, "little")
    assert kc._literal_tag(10, 4) == bytes([63 << 2, 9, 0, 0, 0])


def test_snappy_reference_repeats_pattern():
    _, ref = kc.snappy_stream([("L", b"abc"), ("C1", 3, 7), ("C2", 1, 3)])
    assert ref == b"abc" + b"abcabca" + b"aaa"


def test_snappy_page_set_reaches_every_op_form():
    """The page set really holds what the GPU tests claim to cover."""
    pages = kc.snappy_valid_pages()
    tags = set()
    lens, overlap_offs = set(), set()
    for p in pages:
        for op in p["ops"]:
            if op[0] == "L":
                tags.add(kc._literal_tag(
                    len(op[1]), op[2] if len(op) > 2 else None)[0] >> 2)
                lens.add(len(op[1]))
            else:
                tags.add(op[0])
                if op[1] < op[2] and op[2] == 64:
                    overlap_offs.add(op[1])
    assert {60, 61, 62, 63, "C1", "C2", "C4"} <= tags
    assert {1, 60, 61, 255, 256, 257} <= lens
    assert {1, 2, 3, 5, 7, 63} <= overlap_offs
    assert any(op[0] == "C4" and op[1] > 65_535
               for p in pages for op in p["ops"])
    assert sorted(p["src_mod"] for p in pages
                  if p["src_mod"] is not None) == list(range(8))
    assert sorted(p["dst_mod"] for p in pages
                  if p["dst_mod"] is not None) == sorted(2 * list(range(16)))


@pytest.mark.parametrize("page", kc.snappy_valid_pages(),
                         ids=lambda p: p["name"])
def test_snappy_streams_decode_under_pyarrow(page):
    stream, ref = kc.snappy_stream(page["ops"])
    if not ref:
        assert stream == b"\x00"   # nothing for a codec to produce
        return
    got = pa.Codec("snappy").decompress(stream, decompressed_size=len(ref))
    assert got.to_pybytes() == ref


def test_snappy_layout_honours_alignment():
    pages = []
    for p in kc.snappy_valid_pages():
        stream, ref = kc.snappy_stream(p["ops"])
        pages.append(dict(p, stream=stream + p["trailing"],
                          dst_len=len(ref)))
    blob, so, se, do, total = kc.snappy_layout(pages)
    for p, a, b, d in zip(pages, so, se, do):
        assert blob[a:b] == p["stream"]
        if p["src_mod"] is not None:
            assert a % 8 == p["src_mod"]
        if p["dst_mod"] is not None:
            assert d % 16 == p["dst_mod"]
    ends = [d + p["dst_len"] for p, d in zip(pages, do)]
    assert all(e <= d for e, d in zip(ends, do[1:])) and ends[-1] == total


def test_snappy_malformed_pages_are_rejected_by_pyarrow():
    codec = pa.Codec("snappy")
    for name, stream, dst_len, status in kc.snappy_malformed_pages():
        if status == 1:
            # a valid stream whose length differs from the page header's:
            # the codec only needs the buffer to be large enough; the
            # kernel insists on the exact length
            got = codec.decompress(stream, decompressed_size=dst_len)
            assert got.to_pybytes()[:dst_len - 1] == \
                bytes(range(8)) + b"\x05\x06\x07" * 3
            continue
        with pytest.raises(Exception):
            codec.decompress(stream, decompressed_size=dst_len)


@pytest.mark.parametrize("bw", [b for b in kc.RLE_BIT_WIDTHS if b <= 31])
def test_rle_streams_decode_on_host(bw):
    runs = kc.rle_case(bw)
    data, vals = kc.rle_encode(runs, bw)
    assert vals.size % 8 != 0                  # last group is short
    assert vals.min() == 0 and vals.max() == (1 << bw) - 1
    got = _decode_rle_indices(data, 0, len(data), vals.size, bw)
    assert np.array_equal(got.view(np.uint32), vals)


def test_rle_case_32_has_high_values():
    data, vals = kc.rle_encode(kc.rle_case(32), 32)
    assert (vals >= 2**31).sum() > 20 and vals.max() == 2**32 - 1
    # 8 values at 32 bits are their little-endian words back to back
    lit = kc.rle_encode([("lit", list(range(2**32 - 8, 2**32)))], 32)[0]
    assert lit == b"\x03" + np.arange(2**32 - 8, 2**32,
                                      dtype=np.uint32).tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_normalize_key_orders_special_floats(dtype):
    vals = kc.float_specials(dtype)
    assert np.unique(kc.bits_of(vals)).size == vals.size
    perm = np.random.default_rng(3).permutation(vals.size)
    shuffled = vals[perm]
    norm = cpu_ref.normalize_key(torch.from_numpy(shuffled))
    order = np.argsort(norm.numpy().view(np.uint64), kind="stable")
    # unsigned order of the keys == numeric order, -0.0 < +0.0, NaN last
    assert np.array_equal(kc.bits_of(shuffled[order]), kc.bits_of(vals))
    assert np.unique(norm.numpy()).size == vals.size


def test_scan_oracle_and_inputs():
    out, total = kc.exclusive_scan_ref(np.array([3, -1, 4], dtype=np.int64))
    assert out.tolist() == [0, 3, 2] and total == 6
    names = [n for n, _ in kc.scan_inputs()]
    assert len(set(names)) == len(names)
    for name, x in kc.scan_inputs():
        if name.startswith("random_") and x.size > 1:
            assert (np.abs(x) == 2**40).any()


def test_radix_shapes_vary_where_they_say():
    for n in (1025, 5000):
        masks = {s: kc.varying_mask(kc.radix_keys(s, n))
                 for s in kc.RADIX_SHAPES}
        assert masks["all_equal"] == 0
        assert masks["top_byte"] == 0xFF << 56
        assert masks["bit63"] == 1 << 63
        assert masks["extremes"] == kc.U64
        for s in ("sorted", "reverse", "all_bytes"):
            assert all((masks[s] >> sh) & 0xFF for sh in range(0, 64, 8))
    k = kc.radix_keys("sorted", 5000).numpy().view(np.uint64)
    assert (np.diff(k.astype(object)) >= 0).all()
    kc.check_plan_covers(0xFF << 56, 256, [56])
    kc.check_plan_covers((1 << 26) - 1, 512, [0, 9, 18])
    with pytest.raises(AssertionError):
        kc.check_plan_covers((1 << 26) - 1, 256, [0, 8, 16])
