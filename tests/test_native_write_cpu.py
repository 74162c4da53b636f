"""Native bucket writer on host batches: byte identity with the Python
writer (write_parquet_native through write_bucketed with
HS_NATIVE_WRITE=0) over the chunk-edge and empty-bucket lists.  Host
batches take the same extension entry as device batches and pwrite
straight from the column memory, so this runs without a GPU."""

import os
import threading

import numpy as np
import pytest
import torch

from hyperspace_amd.execution.columnar import ColumnBatch, StringColumn
from hyperspace_amd.index.covering.index import write_bucketed
from hyperspace_amd.ops import native
from hyperspace_amd.sources.native_parquet import (layout_cache_get,
                                                   write_parquet_native)
from hyperspace_amd.sources.parquet_io import bucket_id_of_file

import native_write_common as nw

pytestmark = pytest.mark.skipif(not native.available(),
                                reason="HIP extension not built")


@pytest.fixture
def small_chunks(monkeypatch):
    monkeypatch.setenv("HS_WRITE_CHUNK_MB", nw.CHUNK_MB)


@pytest.mark.parametrize("threads", [1, 3, 15])
def test_chunk_edges(tmp_path, monkeypatch, small_chunks, threads):
    monkeypatch.setenv("HS_WRITE_THREADS", str(threads))
    batch, seg = nw.make_batch(
        nw.CHUNK_EDGE_ROWS,
        {"k": torch.int64, "a": torch.int32, "b": torch.float64,
         "c": torch.float32})
    spy = nw.Spy(monkeypatch)
    nw.check_against_reference(batch, seg, tmp_path,
                               len(nw.CHUNK_EDGE_ROWS), monkeypatch)
    assert spy.calls == 1


def test_matches_write_parquet_native_directly(tmp_path, small_chunks):
    batch, seg = nw.make_batch(nw.CHUNK_EDGE_ROWS,
                               {"k": torch.int64, "a": torch.int32})
    out = write_bucketed(batch, seg, str(tmp_path),
                         len(nw.CHUNK_EDGE_ROWS), task_id=7)
    assert [bucket_id_of_file(p) for p in out] == list(
        range(len(nw.CHUNK_EDGE_ROWS)))
    assert all(os.path.basename(p).startswith("part-00007-") for p in out)
    for b, path in enumerate(out):
        lo, hi = int(seg[b]), int(seg[b + 1])
        got_layout = layout_cache_get(path)
        ref = str(tmp_path / f"ref{b}.parquet")
        write_parquet_native(
            {n: c[lo:hi].numpy() for n, c in batch.columns.items()}, ref)
        with open(path, "rb") as f, open(ref, "rb") as g:
            assert f.read() == g.read(), b
        # the layout cache holds what the Python writer stores
        want_layout = layout_cache_get(ref)
        assert got_layout is not None and want_layout is not None
        assert got_layout[0] == want_layout[0] == hi - lo
        for gl, wl in zip(got_layout[1], want_layout[1]):
            for field in gl.__slots__:
                assert getattr(gl, field) == getattr(wl, field), (b, field)


@pytest.mark.parametrize("pattern", sorted(nw.EMPTY_PATTERNS))
def test_empty_buckets(tmp_path, monkeypatch, small_chunks, pattern):
    rows = nw.EMPTY_PATTERNS[pattern]
    batch, seg = nw.make_batch(rows, {"k": torch.int32, "v": torch.float64},
                               seed=3)
    got = nw.check_against_reference(batch, seg, tmp_path, len(rows),
                                     monkeypatch)
    assert len(got) == sum(1 for r in rows if r)


@pytest.mark.parametrize("num_buckets", [1, 3, 200])
def test_bucket_counts(tmp_path, monkeypatch, small_chunks, num_buckets):
    rng = np.random.default_rng(num_buckets)
    ids = np.sort(rng.integers(0, num_buckets, 20_000))
    rows = np.bincount(ids, minlength=num_buckets)
    batch, seg = nw.make_batch(rows, {"k": torch.int64, "v": torch.float32},
                               seed=5)
    spy = nw.Spy(monkeypatch)
    nw.check_against_reference(batch, seg, tmp_path, num_buckets,
                               monkeypatch)
    # one or two files stay on the Python path
    assert spy.calls == (1 if num_buckets > 2 else 0)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_float_statistics(tmp_path, monkeypatch, dtype):
    buckets = nw.float_stat_buckets(dtype)
    vals = torch.tensor([v for b in buckets for v in b], dtype=dtype)
    batch = ColumnBatch({"f": vals,
                         "i": torch.arange(len(vals), dtype=torch.int64)})
    seg = nw.seg_of([len(b) for b in buckets])
    nw.check_against_reference(batch, seg, tmp_path, len(buckets),
                               monkeypatch)


def test_views_with_storage_offset(tmp_path, monkeypatch, small_chunks):
    rows = [513, 0, 1025, 7]
    n = sum(rows)
    rng = np.random.default_rng(11)
    base_k = nw.random_column(n + 5, torch.int64, rng)
    base_v = nw.random_column(n + 3, torch.float32, rng)
    batch = ColumnBatch({"k": base_k[5:], "v": base_v[3:]})
    assert batch.columns["k"].storage_offset() == 5
    nw.check_against_reference(batch, nw.seg_of(rows), tmp_path, len(rows),
                               monkeypatch)


def _ineligible_batches():
    n = 40
    k = torch.arange(n, dtype=torch.int64)
    yield "string", ColumnBatch(
        {"k": k, "s": StringColumn.from_strings(
            [f"v{i % 7}" for i in range(n)])})
    mask = torch.ones(n, dtype=torch.bool)
    mask[::3] = False
    yield "nullable", ColumnBatch({"k": k, "v": k.to(torch.float64)},
                                  {"v": mask})
    yield "all_true_mask", ColumnBatch(
        {"k": k, "v": k.to(torch.float64)},
        {"v": torch.ones(n, dtype=torch.bool)})
    yield "int16", ColumnBatch({"k": k, "h": k.to(torch.int16)})


@pytest.mark.parametrize("kind", ["string", "nullable", "all_true_mask",
                                  "int16"])
def test_ineligible_shapes_take_the_python_path(tmp_path, monkeypatch, kind):
    batch = dict(_ineligible_batches())[kind]
    spy = nw.Spy(monkeypatch)
    nw.check_against_reference(batch, nw.seg_of([10, 0, 10, 10, 10]),
                               tmp_path, 5, monkeypatch)
    assert spy.calls == 0


def test_switch_off(tmp_path, monkeypatch):
    batch, seg = nw.make_batch([10, 20, 30, 40], {"k": torch.int64})
    spy = nw.Spy(monkeypatch)
    monkeypatch.setenv("HS_NATIVE_WRITE", "0")
    write_bucketed(batch, seg, str(tmp_path), 4)
    assert spy.calls == 0


def test_error_path_joins_every_thread(tmp_path, monkeypatch, small_chunks):
    batch, seg = nw.make_batch([600, 600, 600, 600], {"k": torch.int64})
    not_a_dir = tmp_path / "plain_file"
    not_a_dir.write_bytes(b"x")
    before = threading.active_count()
    with pytest.raises(Exception):
        write_bucketed(batch, seg, str(not_a_dir), 4)
    assert threading.active_count() == before
    nw.check_against_reference(batch, seg, tmp_path, 4, monkeypatch)
