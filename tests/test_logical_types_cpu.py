"""Every host read path gives one representation per parquet logical type.

Which path a file takes (native host read, pyarrow fallback) follows from
codec, encoding and footer statistics — things a user never sees — so the
dtype and values of an annotated column (dates, small and unsigned
integers, INT32 decimals, timestamps) must not depend on it.  Each path
is compared with the independent oracle of logical_types_common, bit for
bit, over five layouts of one table; then buckets, refusals, the index's
own dtype round trip and an end-to-end filter/join scenario on the CPU
session.
"""

import datetime

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import hyperspace_amd.ops as ops
from hyperspace_amd.exceptions import HyperspaceException
from hyperspace_amd.execution.columnar import ColumnBatch
from hyperspace_amd.sources import parquet_io
from hyperspace_amd.sources.native_parquet import (read_native_host,
                                                   read_native_layout)
from hyperspace_amd.sources.parquet_io import (_pyarrow_file_dict,
                                               read_files_batch,
                                               write_batch_parquet)

import logical_types_common as lt


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{layout: (path, table)} + "flba"; written once, never modified."""
    d = tmp_path_factory.mktemp("logical")
    out = lt.write_all_layouts(d)
    out["flba"] = lt.flba_decimal_file(d)
    return out


@pytest.fixture(scope="module")
def refused(tmp_path_factory):
    return lt.write_refused(tmp_path_factory.mktemp("refused"))


ALL_FILES = list(lt.LAYOUTS) + ["flba"]


def test_builders_reach_their_shapes(files):
    """The files have the shapes the module promises: three row groups,
    several pages per chunk, the annotations under test, a dictionary
    where one is asked for, and DELTA pages in the delta file."""
    for lay in lt.LAYOUTS:
        p, table = files[lay]
        pf = pq.ParquetFile(p)
        md = pf.metadata
        assert md.num_rows == lt.N and md.num_row_groups == 3
        phys = {pf.schema.column(i).path:
                (pf.schema.column(i).physical_type,
                 pf.schema.column(i).converted_type)
                for i in range(len(pf.schema))}
        assert phys["u32"] == ("INT32", "UINT_32")
        assert phys["u8"] == ("INT32", "UINT_8")
        assert phys["i8"] == ("INT32", "INT_8")
        assert phys["d"] == ("INT32", "DATE")
        assert phys["dec32"] == ("INT32", "DECIMAL")
        assert phys["dec64"] == ("INT64", "DECIMAL")
        encs = set(md.row_group(0).column(
            table.column_names.index("u32")).encodings)
        if lay == "delta":
            assert "DELTA_BINARY_PACKED" in encs
        assert bool(encs & {"RLE_DICTIONARY", "PLAIN_DICTIONARY"}) == \
            (lay in ("snappy_dict", "dict"))
        layout = read_native_layout(p, lt.NATIVE_COLUMNS)
        if lay == "delta":
            assert layout is None
        else:
            assert min(len(c.pages) for c in layout[1]
                       if c.num_values == lt.ROW_GROUP) > 1
    # edge values really are in the table, nulls in the twins
    t = files["plain"][1]
    u32 = set(t.column("u32").to_pylist())
    assert {0, 2**31 - 1, 2**31, 2**32 - 1} <= u32
    days = lt.oracle(t.column("d"))[0]
    assert days.min() < 0 and 0 in days and days.max() > 0
    assert {-128, 127} <= set(t.column("i8").to_pylist())
    assert 65535 in t.column("u16").to_pylist()
    assert lt.oracle(t.column("dec32"))[0].min() < 0
    assert all(t.column("n_" + c).null_count > 0 for c in lt.BASE_COLUMNS)
    assert pq.ParquetFile(files["flba"][0]).schema.column(0) \
        .physical_type == "FIXED_LEN_BYTE_ARRAY"


@pytest.mark.parametrize("layout", ALL_FILES)
def test_pyarrow_path_matches_oracle(files, layout):
    p, table = files[layout]
    cols, masks, n = _pyarrow_file_dict(p, None)
    assert n == table.num_rows
    lt.assert_table(lt.host_columns(cols, masks), [table],
                    table.column_names)


@pytest.mark.parametrize("layout", lt.HOST_NATIVE)
def test_native_host_read_matches_oracle(files, layout):
    p, table = files[layout]
    names = [c for c in table.column_names
             if c not in ("b", "n_b")]
    res = read_native_host(p, names)
    assert res is not None, "layout must decode natively on the host"
    got = lt.host_columns(*res)
    lt.assert_table({n: got[n] for n in names}, [table], names)


@pytest.mark.parametrize("layout", [x for x in ALL_FILES
                                    if x not in lt.HOST_NATIVE])
def test_native_host_read_declines_whole_file(files, layout):
    """A file the host cannot decode natively is declined as a whole
    (None), never half-converted."""
    p, table = files[layout]
    assert read_native_host(p, [c for c in table.column_names
                                if c not in ("b", "n_b")]) is None


@pytest.mark.parametrize("projected", [False, True],
                         ids=["all", "no-bool"])
@pytest.mark.parametrize("layout", ALL_FILES)
def test_read_files_batch_matches_oracle(files, layout, projected):
    p, table = files[layout]
    names = table.column_names
    if projected:  # without BOOLEAN the native path takes what it can
        names = [c for c in names if c not in ("b", "n_b")]
    batch, rc = read_files_batch([p], names if projected else None)
    assert rc == [table.num_rows]
    lt.assert_table(lt.batch_columns(batch), [table], names)


def test_mixed_batch_is_one_representation(files):
    """One batch over a native (PLAIN) and a fallback (DELTA) file: the
    uint32 column used to come back negative in its first half and
    positive in its second, the date column int64."""
    (p1, t1), (p2, t2) = files["plain"], files["delta"]
    names = [c for c in t1.column_names if c not in ("b", "n_b")]
    # the first file does take the native path, the second does not
    assert read_native_host(p1, names) is not None
    assert read_native_host(p2, names) is None
    for paths, tables in (([p1, p2], [t1, t2]), ([p2, p1], [t2, t1])):
        batch, rc = read_files_batch(paths, names)
        assert rc == [lt.N, lt.N]
        lt.assert_table(lt.batch_columns(batch), tables, names)
    u = batch.tensor("u32")
    assert u.dtype == torch.int64 and int(u.min()) == 0 and \
        int(u.max()) == 2**32 - 1
    assert batch.tensor("d").dtype == torch.int32


def _buckets(batch, name):
    m = batch.mask(name)
    return ops.murmur3_bucket([batch.tensor(name)], lt.NUM_BUCKETS,
                              None if m is None else [m])


@pytest.fixture(scope="module")
def layout_batches(files):
    names = [c for c in files["plain"][1].column_names
             if c not in ("b", "n_b")]
    return {lay: read_files_batch([files[lay][0]], names)[0]
            for lay in lt.LAYOUTS}


@pytest.mark.parametrize("twin", ["", "n_"])
@pytest.mark.parametrize("name", lt.INT_LIKE)
def test_buckets_do_not_depend_on_layout(files, layout_batches, name, twin):
    """murmur3 folds int32 with the int hash and int64 with the long
    hash, so a dtype that follows the read path moves rows to other
    buckets.  Every layout must give the bucket of the oracle array."""
    name = twin + name
    want_vals, valid = lt.oracle(files["plain"][1].column(name))
    want = ops.murmur3_bucket(
        [torch.from_numpy(want_vals)], lt.NUM_BUCKETS,
        None if valid.all() else [torch.from_numpy(valid)])
    for lay, batch in layout_batches.items():
        assert torch.equal(_buckets(batch, name), want), (name, lay)


def test_date_hashes_as_int_and_uint32_as_long(files, layout_batches):
    t = files["plain"][1]
    days = [(v - lt.EPOCH).days for v in t.column("d").to_pylist()]
    as_int = ops.murmur3_bucket(
        [torch.tensor(days, dtype=torch.int32)], lt.NUM_BUCKETS)
    as_long = ops.murmur3_bucket(
        [torch.tensor(days, dtype=torch.int64)], lt.NUM_BUCKETS)
    assert not torch.equal(as_int, as_long)  # the two hashes do differ
    vals = t.column("u32").to_pylist()
    u_long = ops.murmur3_bucket(
        [torch.tensor(vals, dtype=torch.int64)], lt.NUM_BUCKETS)
    for lay, batch in layout_batches.items():
        assert torch.equal(_buckets(batch, "d"), as_int), lay
        assert torch.equal(_buckets(batch, "u32"), u_long), lay


@pytest.mark.parametrize("kind", sorted(lt.REFUSED))
def test_refused_types_raise_by_name(refused, kind):
    p, name = refused[kind]
    for read in (lambda: read_files_batch([p]),
                 lambda: read_files_batch([p], [name]),
                 lambda: read_native_host(p),
                 lambda: _pyarrow_file_dict(p, None)):
        with pytest.raises(HyperspaceException, match=name):
            read()


@pytest.mark.parametrize("kind", sorted(lt.REFUSED))
def test_refused_column_not_asked_for_is_not_refused(tmp_path, kind):
    """The refusal is about the columns a read asks for."""
    name, arr = lt.REFUSED[kind]
    p = str(tmp_path / "two.parquet")
    pq.write_table(pa.table({name: arr, "k": pa.array([1, 2, 3])}), p,
                   compression="NONE", use_dictionary=False)
    batch, rc = read_files_batch([p], ["k"])
    assert rc == [3] and batch.tensor("k").tolist() == [1, 2, 3]
    with pytest.raises(HyperspaceException, match=name):
        read_files_batch([p])


def test_from_arrow_refuses_without_a_file():
    for kind, (name, arr) in sorted(lt.REFUSED.items()):
        with pytest.raises(HyperspaceException, match=name):
            ColumnBatch.from_arrow(pa.table({name: arr}))


def test_index_dtypes_round_trip(tmp_path):
    """int8 / int16 index columns are written by pyarrow with an INT
    annotation; every host path must read back what went in."""
    cols, mask = lt.round_trip_columns()
    for masks in ({}, {"i16": mask, "d": mask}):
        batch = ColumnBatch(dict(cols), dict(masks))
        p = str(tmp_path / f"rt{len(masks)}.parquet")
        write_batch_parquet(batch, p)
        native = read_native_host(p)
        assert native is not None
        for got in (lt.host_columns(*native),
                    lt.host_columns(*_pyarrow_file_dict(p, None)[:2]),
                    lt.batch_columns(read_files_batch([p])[0])):
            lt.assert_round_trip(got, cols, masks)


def test_partitioned_date_buckets_like_a_file_column(tmp_path):
    """A date partition column (Delta partitionValues carry ISO dates)
    must land in the bucket the same days get as a file column."""
    from hyperspace_amd.log.entry import Schema, SchemaField
    from hyperspace_amd.sources.parquet_source import (
        _cast_partition_value, partitioned_read_files)

    dates = [datetime.date(1969, 12, 31), datetime.date(1970, 1, 1),
             datetime.date(2020, 2, 29)]
    paths = []
    for i, day in enumerate(dates):
        p = str(tmp_path / f"f{i}.parquet")
        pq.write_table(pa.table({
            "v": pa.array(np.arange(4) + 10 * i),
            "dfile": pa.array([day] * 4, type=pa.date32())}), p)
        paths.append(p)

    class Rel:
        def partition_schema(self):
            return Schema([SchemaField("dpart", "date", False),
                           SchemaField("ipart", "integer", False)])

        def partition_values(self, path):
            i = paths.index(path)
            return {"dpart": _cast_partition_value(dates[i].isoformat(),
                                                   "date"),
                    "ipart": _cast_partition_value(str(i - 1), "integer")}

    batch, rc = partitioned_read_files(
        Rel(), paths, None, torch.device("cpu"),
        lambda p, c, d: read_files_batch(p, c))
    assert rc == [4, 4, 4]
    assert batch.tensor("dpart").dtype == torch.int32
    assert batch.tensor("ipart").dtype == torch.int32
    assert torch.equal(batch.tensor("dpart"), batch.tensor("dfile"))
    assert batch.tensor("dpart")[::4].tolist() == [-1, 0, 18321]
    assert torch.equal(
        ops.murmur3_bucket([batch.tensor("dpart")], lt.NUM_BUCKETS),
        ops.murmur3_bucket([batch.tensor("dfile")], lt.NUM_BUCKETS))


def test_device_plan_converts_only_annotated_columns(files, refused):
    """The device read plan (footers only, no GPU needed): physical
    storage dtypes, a convert entry for exactly the columns whose engine
    dtype differs, none for un-annotated ones, and a refusal before
    anything could be allocated."""
    p, table = files["plain"]
    plan = parquet_io._plan_device_read([p], lt.NATIVE_COLUMNS)
    assert sorted(plan.convs) == sorted(["i8", "i16", "u32", "dec32"])
    assert plan.dtypes["u32"] == np.int32 and plan.dtypes["i8"] == np.int32
    assert plan.convs["u32"].zero_extend and \
        plan.convs["u32"].dtype == np.int64
    plan = parquet_io._plan_device_read(
        [p], ["i32", "i64", "f32", "f64", "s", "d", "ts_us", "dec64"])
    assert plan.convs == {}
    for kind, (rp, name) in sorted(refused.items()):
        with pytest.raises(HyperspaceException, match=name):
            parquet_io._plan_device_read([p, rp], None)


def test_end_to_end_cpu(tmp_path, monkeypatch):
    monkeypatch.setenv("HYPERSPACE_SYSTEM_PATH", str(tmp_path / "indexes"))
    lt.run_e2e(tmp_path, "cpu")
