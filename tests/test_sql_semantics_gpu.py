"""GPU twin of test_sql_semantics_cpu.py: the same oracle, tables and
matrices with the HIP kernels on the data path (select_range, murmur3
bucketing, the radix sort of the index build, merge_join).  The filter
matrix is split by the way a predicate is run so that each case stays
short."""

import pytest
import torch

import sql_semantics_common as sc
from hyperspace_amd.ops import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native.available(), "HIP extension must load on a GPU box"


@pytest.fixture(scope="module", params=[sc.N_SPECIAL, sc.N_LARGE],
                ids=["bare", "tiled"])
def fenv(request, tmp_path_factory):
    return sc.filter_env(tmp_path_factory.mktemp("sqlsem_f"), "cuda",
                         request.param)


@pytest.fixture(scope="module")
def jenv(tmp_path_factory):
    return sc.join_env(tmp_path_factory.mktemp("sqlsem_j"), "cuda")


@pytest.mark.parametrize("way", sc.WAYS)
@pytest.mark.parametrize("mode", sc.FILTER_MODES)
@pytest.mark.parametrize("col", sc.VALUE_COLS)
def test_filter_matrix(fenv, col, mode, way):
    sc.filter_matrix(fenv, col, mode, (way,))


@pytest.mark.parametrize("mode", sc.FILTER_MODES)
def test_filter_arith_in(fenv, mode):
    sc.filter_arith_in(fenv, mode)


@pytest.mark.parametrize("name", list(sc.ISSUE_TABLE_FILTERS))
def test_issue_table_filter(fenv, name):
    sc.issue_table_filter(fenv, name)


def test_equality_prune_reads_one_bucket(fenv):
    sc.equality_prune_reads_one_bucket(fenv)


@pytest.mark.parametrize("how", sc.JOIN_TYPES)
@pytest.mark.parametrize("physical", ["co_bucketed", "shuffled"])
@pytest.mark.parametrize("keys", list(sc.JOIN_KEYS))
def test_join_matrix(jenv, keys, physical, how):
    sc.join_matrix(jenv, keys, physical, how)


@pytest.mark.parametrize("physical", ["co_bucketed", "shuffled"])
def test_join_int_float_key_is_refused(jenv, physical):
    sc.join_int_float_key_is_refused(jenv, physical)


def test_join_env_buckets_sorted(jenv):
    for keys in ("f64", "f32", "f64_k"):
        sc.assert_buckets_sorted(
            jenv.session, jenv.query(keys, "inner").optimized_plan(),
            sc.JOIN_KEYS[keys][0][0])


@pytest.mark.parametrize("on", list(sc.ISSUE_TABLE_JOINS))
def test_issue_table_joins(tmp_path, on):
    sc.issue_table_joins(tmp_path, "cuda", on)


def test_index_buckets_sorted_by_canonical_key(tmp_path):
    sc.index_buckets_sorted_by_canonical_key(tmp_path, "cuda")


def test_one_answer_on_every_physical_path(fenv, jenv):
    sc.one_answer_on_every_physical_path(fenv, jenv)
