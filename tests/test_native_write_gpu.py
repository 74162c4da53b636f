"""Native bucket writer on device batches.

The yardstick throughout is the Python writer on a host copy of the same
batch and the same ``seg`` (write_bucketed with HS_NATIVE_WRITE=0): the
file lists must name the same buckets and every file must be the same,
byte for byte.  Chunks are 4 KiB (HS_WRITE_CHUNK_MB as a fraction), so a
few thousand rows reach every chunk edge, wrap the ring and outnumber the
writer threads.

Run on a GPU box: python -m pytest tests/test_native_write_gpu.py -m gpu -q
"""

import os
import threading

import numpy as np
import pyarrow.parquet as pq
import pytest
import torch

import hyperspace_amd.ops as ops
from hyperspace_amd.execution.columnar import ColumnBatch, StringColumn
from hyperspace_amd.index.covering.index import (sort_by_bucket_and_keys,
                                                 write_bucketed)
from hyperspace_amd.ops import native
from hyperspace_amd.sources import native_parquet as npq
from hyperspace_amd.sources.parquet_io import read_files_batch_device

import native_write_common as nw

pytestmark = pytest.mark.gpu

DTYPES = [torch.int64, torch.int32, torch.float64, torch.float32]


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native.available(), "HIP extension must load on a GPU box"


@pytest.fixture
def small_chunks(monkeypatch):
    monkeypatch.setenv("HS_WRITE_CHUNK_MB", nw.CHUNK_MB)


@pytest.mark.parametrize("threads", [1, 3, 15])
def test_chunk_edges(tmp_path, monkeypatch, small_chunks, threads):
    """int64 and int32 columns in one batch: the element sizes differ
    within one file, and each bucket size puts one of them on an edge."""
    monkeypatch.setenv("HS_WRITE_THREADS", str(threads))
    batch, seg = nw.make_batch(
        nw.CHUNK_EDGE_ROWS,
        {"k": torch.int64, "a": torch.int32, "b": torch.float64,
         "c": torch.float32}, device="cuda")
    spy = nw.Spy(monkeypatch)
    nw.check_against_reference(batch, seg, tmp_path,
                               len(nw.CHUNK_EDGE_ROWS), monkeypatch)
    assert spy.calls == 1


@pytest.mark.parametrize("pattern", sorted(nw.EMPTY_PATTERNS))
def test_empty_buckets(tmp_path, monkeypatch, small_chunks, pattern):
    rows = nw.EMPTY_PATTERNS[pattern]
    batch, seg = nw.make_batch(rows, {"k": torch.int32, "v": torch.float64},
                               seed=3, device="cuda")
    got = nw.check_against_reference(batch, seg, tmp_path, len(rows),
                                     monkeypatch)
    assert len(got) == sum(1 for r in rows if r)


@pytest.mark.parametrize("threads", [1, 3, 15])
@pytest.mark.parametrize("num_buckets", [1, 3, 200])
def test_bucket_counts(tmp_path, monkeypatch, small_chunks, num_buckets,
                       threads):
    """~20 k rows; at 200 buckets there are more files than ring slots
    (64) and than writer threads, and some buckets come out empty."""
    monkeypatch.setenv("HS_WRITE_THREADS", str(threads))
    rng = np.random.default_rng(num_buckets)
    ids = rng.integers(0, num_buckets, 20_000)
    ids[ids % 17 == 5] = 0  # leaves empty buckets at 200
    rows = np.bincount(ids, minlength=num_buckets)
    batch, seg = nw.make_batch(rows, {"k": torch.int64, "v": torch.float32},
                               seed=5, device="cuda")
    spy = nw.Spy(monkeypatch)
    got = nw.check_against_reference(batch, seg, tmp_path, num_buckets,
                                     monkeypatch)
    assert len(got) == int((rows > 0).sum())
    if num_buckets == 200:
        assert 64 < len(got) < 200
    assert spy.calls == (1 if num_buckets > 2 else 0)


@pytest.mark.parametrize("included", DTYPES, ids=str)
@pytest.mark.parametrize("key", DTYPES, ids=str)
def test_dtypes(tmp_path, monkeypatch, small_chunks, key, included):
    batch, seg = nw.make_batch([300, 1, 0, 1500, 77],
                               {"key": key, "inc": included}, seed=9,
                               device="cuda")
    nw.check_against_reference(batch, seg, tmp_path, 5, monkeypatch)


def test_views_with_storage_offset(tmp_path, monkeypatch, small_chunks):
    rows = [513, 0, 1025, 7]
    n = sum(rows)
    rng = np.random.default_rng(11)
    base_k = nw.random_column(n + 5, torch.int64, rng).cuda()
    base_v = nw.random_column(n + 3, torch.float32, rng).cuda()
    base_a = nw.random_column(n + 1, torch.int32, rng).cuda()
    batch = ColumnBatch({"k": base_k[5:], "v": base_v[3:], "a": base_a[1:]})
    assert batch.columns["k"].storage_offset() == 5
    nw.check_against_reference(batch, nw.seg_of(rows), tmp_path, len(rows),
                               monkeypatch)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=str)
def test_float_statistics_fallback(tmp_path, monkeypatch, dtype):
    """-0.0 with +0.0 in both orders, a max of 0.0, NaN of either sign,
    an all-NaN bucket: the footer bytes are those of numpy's min/max."""
    buckets = nw.float_stat_buckets(dtype)
    vals = torch.tensor([v for b in buckets for v in b], dtype=dtype)
    batch = ColumnBatch({"f": vals.cuda(),
                         "i": torch.arange(len(vals), dtype=torch.int64,
                                           device="cuda")})
    seg = nw.seg_of([len(b) for b in buckets])
    spy = nw.Spy(monkeypatch)
    nw.check_against_reference(batch, seg, tmp_path, len(buckets),
                               monkeypatch)
    assert spy.calls == 1


def _ineligible(kind):
    n = 40
    k = torch.arange(n, dtype=torch.int64, device="cuda")
    v = k.to(torch.float64)
    if kind == "string":
        return ColumnBatch({"k": k, "s": StringColumn.from_strings(
            [f"v{i % 7}" for i in range(n)]).to("cuda")})
    if kind == "nullable":
        mask = torch.ones(n, dtype=torch.bool, device="cuda")
        mask[::3] = False
        return ColumnBatch({"k": k, "v": v}, {"v": mask})
    if kind == "all_true_mask":
        return ColumnBatch(
            {"k": k, "v": v},
            {"v": torch.ones(n, dtype=torch.bool, device="cuda")})
    return ColumnBatch({"k": k, "h": k.to(torch.int16)})


@pytest.mark.parametrize("kind", ["string", "nullable", "all_true_mask",
                                  "int16"])
def test_ineligible_shapes_take_the_python_path(tmp_path, monkeypatch, kind):
    spy = nw.Spy(monkeypatch)
    nw.check_against_reference(_ineligible(kind),
                               nw.seg_of([10, 0, 10, 10, 10]), tmp_path, 5,
                               monkeypatch)
    assert spy.calls == 0


def test_switch_off_gives_identical_files(tmp_path, monkeypatch,
                                          small_chunks):
    batch, seg = nw.make_batch([600, 0, 1300, 40, 512],
                               {"k": torch.int64, "v": torch.float64},
                               device="cuda")
    on = str(tmp_path / "on")
    off = str(tmp_path / "off")
    os.makedirs(on)
    os.makedirs(off)
    spy = nw.Spy(monkeypatch)
    got_on = write_bucketed(batch, seg, on, 5)
    assert spy.calls == 1
    monkeypatch.setenv("HS_NATIVE_WRITE", "0")
    got_off = write_bucketed(batch, seg, off, 5)  # device batch, old path
    assert spy.calls == 1
    nw.assert_same_files(got_on, got_off)


def test_layout_cache_and_read_back(tmp_path, monkeypatch, small_chunks):
    rows = [513, 0, 1025, 7, 2000]
    batch, seg = nw.make_batch(
        rows, {"k": torch.int64, "a": torch.int32, "v": torch.float64},
        seed=21, device="cuda")
    out = write_bucketed(batch, seg, str(tmp_path), len(rows))
    host = batch.to("cpu")
    names = list(batch.columns)

    live = [b for b, r in enumerate(rows) if r]
    for b, path in zip(live, out):
        lo, hi = int(seg[b]), int(seg[b + 1])
        got = npq.layout_cache_get(path)
        ref = str(tmp_path / f"ref{b}.parquet")
        npq.write_parquet_native(
            {n: c[lo:hi].numpy() for n, c in host.columns.items()}, ref)
        want = npq.layout_cache_get(ref)
        assert got is not None and want is not None
        assert got[0] == want[0] == hi - lo
        assert len(got[1]) == len(want[1]) == len(names)
        for gl, wl in zip(got[1], want[1]):
            for field in gl.__slots__:
                assert getattr(gl, field) == getattr(wl, field), (b, field)

    def read_and_compare():
        back, counts = read_files_batch_device(out, torch.device("cuda"),
                                               columns=names)
        assert list(counts) == [r for r in rows if r]
        for n in names:
            assert back.columns[n].dtype == batch.columns[n].dtype
            assert torch.equal(back.columns[n], batch.columns[n]), n

    read_and_compare()  # layout from the cache
    for path in out:
        npq._LAYOUT_CACHE.pop(path, None)
    read_and_compare()  # layout from the footer C++ wrote

    for b, path in zip(live, out):
        lo, hi = int(seg[b]), int(seg[b + 1])
        npq._LAYOUT_CACHE.pop(path, None)
        parsed = npq.read_native_layout(path)
        assert parsed is not None
        assert [c.name for c in parsed[1]] == names
        assert all(c.num_values == hi - lo and c.encoding == "plain"
                   for c in parsed[1])
        table = pq.read_table(path)
        md = pq.read_metadata(path).row_group(0)
        for ci, n in enumerate(names):
            want = host.columns[n][lo:hi].numpy()
            assert np.array_equal(table.column(n).to_numpy(), want), (b, n)
            st = md.column(ci).statistics
            assert st.min == want.min() and st.max == want.max(), (b, n)
            assert st.null_count == 0


def test_write_right_after_the_sort(tmp_path, monkeypatch):
    """write_bucketed straight after sort_by_bucket_and_keys, nothing
    synchronised in between: the copies must follow the sort."""
    n, nb = 1 << 21, 16
    g = torch.Generator(device="cuda").manual_seed(1)
    key = torch.randint(0, 1 << 20, (n,), generator=g, device="cuda")
    val = torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    src = ColumnBatch({"key": key, "val": val})
    ids = ops.murmur3_bucket([key], nb)
    torch.cuda.synchronize()
    batch, seg = sort_by_bucket_and_keys(src, ids, ["key"], nb)
    got_dir = str(tmp_path / "got")
    os.makedirs(got_dir)
    spy = nw.Spy(monkeypatch)
    got = write_bucketed(batch, seg, got_dir, nb)
    assert spy.calls == 1
    torch.cuda.synchronize()
    want = nw.write_reference(batch, seg, str(tmp_path / "want"), nb,
                              monkeypatch)
    nw.assert_same_files(got, want)


def test_after_event_of_a_side_stream(tmp_path, monkeypatch):
    """The batch is produced on a side stream; the writer is given the
    event recorded after it and must not read the columns earlier."""
    rows = [200_000, 0, 300_000, 1, 548_575]
    n = sum(rows)
    base = torch.arange(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        k = base.clone()
        for _ in range(20):  # keeps the side stream busy for a while
            k = k * 3 + 1
        v = (k % 1000).to(torch.float64) * 0.5
        ev = torch.cuda.Event()
        ev.record(side)
    batch = ColumnBatch({"k": k, "v": v})
    got_dir = str(tmp_path / "got")
    os.makedirs(got_dir)
    got = write_bucketed(batch, nw.seg_of(rows), got_dir, len(rows),
                         after_event=ev)
    torch.cuda.synchronize()
    hk = torch.arange(n, dtype=torch.int64)
    for _ in range(20):
        hk = hk * 3 + 1
    hv = (hk % 1000).to(torch.float64) * 0.5
    want = nw.write_reference(ColumnBatch({"k": hk, "v": hv}),
                              nw.seg_of(rows), str(tmp_path / "want"),
                              len(rows), monkeypatch)
    nw.assert_same_files(got, want)


def test_error_path(tmp_path, monkeypatch, small_chunks):
    """The output directory's path names a regular file: open fails on
    the host, the call raises, no thread outlives it, and the next call
    works."""
    batch, seg = nw.make_batch([600, 600, 0, 600, 600],
                               {"k": torch.int64, "v": torch.float32},
                               device="cuda")
    not_a_dir = tmp_path / "plain_file"
    not_a_dir.write_bytes(b"x")
    before = threading.active_count()
    with pytest.raises(Exception):
        write_bucketed(batch, seg, str(not_a_dir), 5)
    assert threading.active_count() == before
    spy = nw.Spy(monkeypatch)
    nw.check_against_reference(batch, seg, tmp_path, 5, monkeypatch)
    assert spy.calls == 1
