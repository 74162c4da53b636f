"""The device parquet read must decode the whole reader matrix NATIVELY.

test_reader_matrix accepts "decode exactly or decline", so a change that
quietly sent every file to pyarrow would pass it.  Here the host table
path and the per-file pyarrow read are patched to raise, and the result
must equal pyarrow bit for bit.  The same 40 small files (5 codecs x
dict on/off x page version x nulls; three row groups, several pages per
chunk, mid-chunk dictionary overflow) also pin the page layout on the
CPU.
"""

import itertools
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from hyperspace_amd.execution.columnar import StringColumn
from hyperspace_amd.sources import parquet_io
from hyperspace_amd.sources.native_parquet import read_native_layout

N = 6000
CODECS = ["NONE", "SNAPPY", "ZSTD", "GZIP", "LZ4"]
COMBOS = list(itertools.product(CODECS, [True, False], ["1.0", "2.0"],
                                [True, False]))
# Combos that fall back to pyarrow at the parent of the commit that
# added this test, with the reason: none, all 40 decode natively.
FALLS_BACK = {}
# numeric / string columns whose dictionary overflows mid-chunk at
# dictionary_pagesize_limit=4096 (later pages of the chunk are PLAIN)
OVERFLOW = {"i64", "i32", "f64", "ni", "u"}


def _table(with_nulls):
    rng = np.random.default_rng(9)
    f64 = rng.random(N)
    f64[::97] = -0.0
    f64[5::101] = np.array([0x7FF8000000000123],
                           dtype=np.uint64).view(np.float64)[0]
    cols = {
        "i64": pa.array(rng.integers(-10**12, 10**12, N)),
        "i32": pa.array(rng.integers(-10**6, 10**6, N).astype(np.int32)),
        "f64": pa.array(f64),
        "s": pa.array([f"v{i % 499:03d}" for i in range(N)],
                      type=pa.string()),
        "u": pa.array([f"unique-{(i * 7919) % N:05d}" for i in range(N)],
                      type=pa.string()),
    }
    if with_nulls:
        cols["ni"] = pa.array([None if i % 7 == 0 else int(i)
                               for i in range(N)], type=pa.int64())
        cols["ns"] = pa.array([None if i % 5 == 0 else f"x{i % 311}"
                               for i in range(N)], type=pa.string())
    return pa.table(cols)


def _name(combo):
    codec, use_dict, dpv, with_nulls = combo
    return f"m_{codec}_{use_dict}_{dpv}_{with_nulls}.parquet"


@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    """{combo: (path, pyarrow table read back from it)} — written and
    read once, never modified."""
    d = tmp_path_factory.mktemp("matrix")
    out = {}
    for combo in COMBOS:
        codec, use_dict, dpv, with_nulls = combo
        p = str(d / _name(combo))
        pq.write_table(_table(with_nulls), p, compression=codec,
                       use_dictionary=use_dict, data_page_version=dpv,
                       row_group_size=2500, data_page_size=2048,
                       dictionary_pagesize_limit=4096)
        out[combo] = (p, pq.read_table(p))
    return out


def _ids(combo):
    return "-".join(str(x) for x in combo)


@pytest.mark.parametrize("combo", COMBOS, ids=_ids)
def test_layout_pin(matrix, combo):
    codec, use_dict, _, _ = combo
    p, table = matrix[combo]
    lay = read_native_layout(p)
    assert lay is not None
    chunks = lay[1]
    assert len(chunks) == 3 * table.num_columns  # three row groups
    z = "" if codec == "NONE" else "_z"
    for c in chunks:
        assert all(pg.start < pg.end for pg in c.pages), c.name
        assert sum(pg.num_values for pg in c.pages) == c.num_values
    for name in table.column_names:
        is_str = pa.types.is_string(table.schema.field(name).type)
        plain = "splain" if is_str else "plain"
        if not use_dict:
            want = {plain}
        elif name in OVERFLOW:  # in the 2500-row groups
            want = {"dict", plain}
        else:
            want = {"dict"}
        mine = [c for c in chunks if c.name == name]
        assert {pg.kind for c in mine for pg in c.pages} == \
            {k + z for k in want}, name
        assert max(len(c.pages) for c in mine) > 1, name  # several pages


def _raise_host_table(*a, **k):
    raise AssertionError("device read fell back to the host table path")


def _raise_pyarrow_file(*a, **k):
    raise AssertionError("device read sent a file to pyarrow")


def _assert_exact(batch, tables, names):
    """Every column of ``batch`` equals the concatenated pyarrow tables:
    validity in full, values bit for bit on the valid rows."""
    assert list(batch.columns.keys()) == list(names)
    for name in names:
        col = pa.concat_arrays([c for t in tables
                                for c in t.column(name).chunks])
        valid = col.is_valid().to_numpy(zero_copy_only=False)
        m = batch.mask(name)
        if valid.all():
            assert m is None or bool(m.all()), name
        else:
            assert (m.cpu().numpy() == valid).all(), name
        if pa.types.is_string(col.type):
            s = batch.column(name)
            assert isinstance(s, StringColumn)
            assert list(s.values) == sorted(set(s.values)), name
            got = np.array(s.values, dtype=object)[s.codes.cpu().numpy()]
            ref = np.array(col.to_pylist(), dtype=object)
        else:
            got = batch.tensor(name).cpu().numpy()
            ref = col.fill_null(0).to_numpy(zero_copy_only=False)
            assert got.dtype == ref.dtype, name
            view = f"i{got.dtype.itemsize}"  # NaN payloads, signed zeros
            got, ref = got.view(view), ref.view(view)
        assert (got[valid] == ref[valid]).all(), name


def check_native(paths, tables, columns=None):
    """Device-read ``paths`` with both pyarrow escapes barred and compare
    with ``tables`` exactly."""
    saved = parquet_io.read_files_batch, parquet_io._pyarrow_file_dict
    parquet_io.read_files_batch = _raise_host_table
    parquet_io._pyarrow_file_dict = _raise_pyarrow_file
    try:
        batch, rc = parquet_io.read_files_batch_device(
            paths, torch.device("cuda:0"), columns)
    finally:
        parquet_io.read_files_batch, parquet_io._pyarrow_file_dict = saved
    assert rc == [t.num_rows for t in tables]
    _assert_exact(batch, tables, columns or tables[0].column_names)


@pytest.mark.gpu
@pytest.mark.parametrize("combo", [c for c in COMBOS if c not in FALLS_BACK],
                         ids=_ids)
def test_matrix_decodes_natively(matrix, combo):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    codec, use_dict, dpv, with_nulls = combo
    p, t = matrix[combo]
    # alone: serial path, one decode unit per row group
    check_native([p], [t])
    # three files (threaded path), the middle one under the next codec
    other = (CODECS[(CODECS.index(codec) + 1) % len(CODECS)], use_dict,
             dpv, with_nulls)
    if other in FALLS_BACK:
        other = combo
    q, tq = matrix[other]
    check_native([p, q, p], [t, tq, t])
    # projection in another order than the file's
    cols = ["u", "f64", "ns" if with_nulls else "s", "i32"]
    check_native([p], [t], cols)


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", ["0", "2"])
def test_snappy_device_ratio_extremes(matrix, ratio):
    """HS_SNAPPY_DEV_RATIO=0 sends every snappy page to the device
    kernel and >1 sends every page to the host codec; it is read at
    import, so each value gets a fresh interpreter."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    paths = [matrix[c][0] for c in COMBOS
             if c[0] == "SNAPPY" and c not in FALLS_BACK]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pythonpath = [root] + [p for p in os.environ.get(
        "PYTHONPATH", "").split(os.pathsep) if p]
    env = dict(os.environ, HS_SNAPPY_DEV_RATIO=ratio,
               PYTHONPATH=os.pathsep.join(pythonpath))
    r = subprocess.run(
        [sys.executable, os.path.abspath(__file__), ratio] + paths,
        env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"ok {len(paths)}" in r.stdout


if __name__ == "__main__":
    assert parquet_io._DEV_RATIO == float(sys.argv[1])
    for path in sys.argv[2:]:
        check_native([path], [pq.read_table(path)])
    print("ok", len(sys.argv) - 2)
