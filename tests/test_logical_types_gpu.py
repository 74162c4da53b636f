"""The device parquet read gives the representation of the logical-type
table, whichever way a file's bytes reach the GPU: native page decode
(copy_unaligned / rle_decode / gather_rows, then the convert step), the
per-file pyarrow unit inside a mixed batch, or the host table path.  All
compared bit for bit with the independent oracle of
logical_types_common; the HIP hash and key kernels then see the same
values and dtypes as the CPU reference.

Run on a GPU box: python -m pytest tests/test_logical_types_gpu.py -m gpu -q
"""

import numpy as np
import pyarrow.parquet as pq
import pytest
import torch

import hyperspace_amd.ops as ops
from hyperspace_amd.exceptions import HyperspaceException
from hyperspace_amd.ops import cpu_ref, native
from hyperspace_amd.sources import parquet_io

import logical_types_common as lt
import test_device_read_native as matrix_mod

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native.available(), "HIP extension must load on a GPU box"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("logical")
    out = lt.write_all_layouts(d)
    out["flba"] = lt.flba_decimal_file(d)
    return out


@pytest.fixture(scope="module")
def refused(tmp_path_factory):
    return lt.write_refused(tmp_path_factory.mktemp("refused"))


def _dev():
    return torch.device("cuda:0")


def _no_bool(table):
    return [c for c in table.column_names if c not in ("b", "n_b")]


def _device_read(paths, columns=None):
    batch, rc = parquet_io.read_files_batch_device(paths, _dev(), columns)
    assert batch.device.type == "cuda"
    return batch, rc


class _Barred:
    """Both pyarrow escapes of the device read raise, as in
    test_device_read_native.check_native."""

    def __enter__(self):
        self.saved = (parquet_io.read_files_batch,
                      parquet_io._pyarrow_file_dict)
        parquet_io.read_files_batch = matrix_mod._raise_host_table
        parquet_io._pyarrow_file_dict = matrix_mod._raise_pyarrow_file

    def __exit__(self, *exc):
        parquet_io.read_files_batch, parquet_io._pyarrow_file_dict = \
            self.saved


@pytest.mark.parametrize("layout", list(lt.LAYOUTS) + ["flba"])
def test_device_read_matches_oracle(files, layout):
    p, table = files[layout]
    # every column: BOOLEAN sends the batch to the host table path
    batch, rc = _device_read([p])
    assert rc == [table.num_rows]
    lt.assert_table(lt.batch_columns(batch), [table], table.column_names)
    # without it: the device read plans the batch itself
    names = _no_bool(table)
    batch, rc = _device_read([p], names)
    lt.assert_table(lt.batch_columns(batch), [table], names)


def test_three_file_mixed_batch(files):
    """[plain, delta, snappy]: the threaded path; the DELTA file has no
    native layout and goes through host_unit into the slices between two
    natively decoded files."""
    order = ["plain", "delta", "snappy_dict"]
    paths = [files[k][0] for k in order]
    tables = [files[k][1] for k in order]
    names = _no_bool(tables[0])
    assert parquet_io._plan_device_read(paths, names) is not None
    calls = []
    real = parquet_io._DeviceRead.host_unit

    def spy(self, i):
        calls.append(i)
        return real(self, i)

    parquet_io._DeviceRead.host_unit = spy
    saved = parquet_io.read_files_batch
    parquet_io.read_files_batch = matrix_mod._raise_host_table
    try:
        batch, rc = _device_read(paths, names)
    finally:
        parquet_io._DeviceRead.host_unit = real
        parquet_io.read_files_batch = saved
    assert calls == [1]
    assert rc == [lt.N] * 3
    lt.assert_table(lt.batch_columns(batch), tables, names)
    # and in another projection order, nullable twins first
    cols = ["n_u32", "n_d", "s", "u32", "i8", "dec32", "d"]
    batch, _ = _device_read(paths, cols)
    lt.assert_table(lt.batch_columns(batch), tables, cols)


@pytest.mark.parametrize("layout", lt.DEVICE_NATIVE)
def test_annotated_columns_decode_natively(files, layout):
    """Every annotated type decodes on the device: narrowing, widening
    and zero-extension happen after the page decode, not in pyarrow."""
    p, table = files[layout]
    names = _no_bool(table)
    with _Barred():
        batch, rc = _device_read([p], names)          # one unit / row group
        lt.assert_table(lt.batch_columns(batch), [table], names)
        q, tq = files["zstd_v2" if layout != "zstd_v2" else "plain"]
        batch, rc = _device_read([p, q, p], names)    # threaded path
    assert rc == [lt.N] * 3
    lt.assert_table(lt.batch_columns(batch), [table, tq, table], names)


@pytest.fixture(scope="module")
def device_batch(files):
    p, table = files["snappy_dict"]
    return _device_read([p], _no_bool(table))[0], table


@pytest.mark.parametrize("twin", ["", "n_"])
@pytest.mark.parametrize("name", lt.INT_LIKE)
def test_device_hash_and_key_match_cpu_on_oracle(device_batch, name, twin):
    batch, table = device_batch
    name = twin + name
    want_vals, valid = lt.oracle(table.column(name))
    ref = torch.from_numpy(want_vals)
    ref_mask = None if valid.all() else [torch.from_numpy(valid)]
    col = batch.tensor(name)
    m = batch.mask(name)
    assert col.is_cuda and col.dtype == ref.dtype
    got = ops.murmur3_bucket([col], lt.NUM_BUCKETS,
                             None if m is None else [m])
    assert got.is_cuda
    assert torch.equal(got.cpu(),
                       cpu_ref.murmur3_bucket([ref], lt.NUM_BUCKETS,
                                              ref_mask))
    key = ops.sql_key(col)
    assert key.is_cuda
    v = torch.from_numpy(valid)
    assert torch.equal(key.cpu()[v], cpu_ref.sql_key(ref)[v])


@pytest.mark.parametrize("kind", sorted(lt.REFUSED))
def test_refused_types_leave_nothing_on_the_device(files, refused, kind):
    p, name = refused[kind]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(HyperspaceException, match=name):
        _device_read([p])
    # also as one file of a threaded batch, behind files that decode
    plain = files["plain"][0]
    with pytest.raises(HyperspaceException, match=name):
        _device_read([p, p, p])
    with pytest.raises(HyperspaceException):
        _device_read([plain, plain, p], None)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before


def test_convert_step_skips_unannotated_columns(tmp_path_factory, files):
    """The convert step runs once per annotated column that needs it and
    never for the un-annotated int64 / int32 / float64 columns of the
    reader matrix."""
    d = tmp_path_factory.mktemp("matrix_spy")
    calls = []
    real = parquet_io.convert_logical

    def spy(col, conv):
        calls.append(conv)
        return real(col, conv)

    parquet_io.convert_logical = spy
    try:
        for with_nulls in (True, False):
            paths = []
            for combo in matrix_mod.COMBOS:
                if combo[3] != with_nulls:
                    continue
                codec, use_dict, dpv, _ = combo
                p = str(d / matrix_mod._name(combo))
                pq.write_table(matrix_mod._table(with_nulls), p,
                               compression=codec, use_dictionary=use_dict,
                               data_page_version=dpv, row_group_size=2500,
                               data_page_size=2048,
                               dictionary_pagesize_limit=4096)
                paths.append(p)
            with _Barred():
                batch, rc = _device_read(paths)
            assert rc == [matrix_mod.N] * 20
            assert batch.tensor("i64").dtype == torch.int64
            assert batch.tensor("i32").dtype == torch.int32
            assert batch.tensor("f64").dtype == torch.float64
        assert calls == []
        # positive control: the annotated file does reach it, once per
        # column whose engine dtype differs from the physical one
        p, table = files["plain"]
        _device_read([p], _no_bool(table))
        assert len(calls) == 2 * len(["i8", "i16", "u32", "dec32"])
    finally:
        parquet_io.convert_logical = real


def test_index_dtypes_round_trip_on_device(tmp_path):
    """An index batch with int8 / int16 columns written by
    write_batch_parquet comes back from the device read, natively, with
    the dtypes and values that went in."""
    from hyperspace_amd.execution.columnar import ColumnBatch
    cols, mask = lt.round_trip_columns()
    for masks in ({}, {"i16": mask, "d": mask}):
        p = str(tmp_path / f"rt{len(masks)}.parquet")
        parquet_io.write_batch_parquet(
            ColumnBatch(dict(cols), dict(masks)), p)
        with _Barred():
            batch, rc = _device_read([p])
        assert rc == [len(mask)]
        lt.assert_round_trip(lt.batch_columns(batch), cols, masks)


def test_end_to_end_cuda(tmp_path, monkeypatch):
    monkeypatch.setenv("HYPERSPACE_SYSTEM_PATH", str(tmp_path / "indexes"))
    session = lt.run_e2e(tmp_path, "cuda")
    assert str(session.device).startswith("cuda")
