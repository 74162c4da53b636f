"""The host-side units of the parquet read that need no device: the
string dictionary merge and the compressed-segment planner."""

import numpy as np

from hyperspace_amd.sources.device_decode import plan_segments
from hyperspace_amd.sources.native_parquet import (
    ColumnChunkLayout, DictPage, Page, merge_string_dicts,
    string_remap_tables)


def test_merge_identical_sorted_keeps_first():
    a = ["a", "b", "c"]
    merged, remap = merge_string_dicts([a, list(a), list(a)])
    assert merged is a and not remap


def test_merge_identical_unsorted_remaps():
    d = ["b", "a", "c"]
    merged, remap = merge_string_dicts([d, list(d)])
    assert merged == ["a", "b", "c"] and remap
    assert list(string_remap_tables(merged, [d, d])) == [[1, 0, 2]] * 2


def test_merge_disjoint_is_sorted_union():
    merged, remap = merge_string_dicts([["x", "y"], ["a", "z"]])
    assert merged == ["a", "x", "y", "z"] and remap
    assert list(string_remap_tables(merged, [["x", "y"], ["a", "z"]])) == \
        [[1, 2], [0, 3]]


def test_merge_one_empty():
    merged, remap = merge_string_dicts([[], ["a", "b"]])
    assert merged == ["a", "b"] and remap
    # empty dictionary: [0] for its masked zero codes; equal one: as is
    assert list(string_remap_tables(merged, [[], ["a", "b"]])) == \
        [[0], None]
    assert merge_string_dicts([[]]) == ([], False)


def test_merge_empty_list():
    assert merge_string_dicts([]) == ([], False)


def _zchunk(pages, codec="SNAPPY", dict_page=None):
    kind = "dict_z" if dict_page is not None else "plain_z"
    return ColumnChunkLayout("c", np.dtype("int64"), pages,
                             sum(p.num_values for p in pages), kind,
                             dict_page, codec=codec)


def _zpage(start, comp, unc, kind="plain_z", is_compressed=True):
    return Page(kind, start, start + comp, 10, 0, unc, False,
                is_compressed)


def test_plan_snappy_ratio_threshold():
    # 0.93 * 1000 = 930: 929 compressed bytes decode on the host codec,
    # 930 on the device
    c = _zchunk([_zpage(0, 929, 1000), _zpage(929, 930, 1000)])
    plan = plan_segments(c, 0.93)
    assert plan.segs == [(0, 929, 1000), (929, 1859, 1000)]
    assert (plan.dev, plan.host, plan.identity) == ([1], [0], [])
    assert plan.offsets == [0, 1000, 2000]
    assert plan.page_base == [0, 1000]


def test_plan_ratio_extremes():
    c = _zchunk([_zpage(0, 1, 1000), _zpage(1, 1200, 1000)])
    assert plan_segments(c, 0.0).dev == [0, 1]
    assert plan_segments(c, 0.0).host == []
    # a page that GREW under snappy (1200 > 1000) still goes to the host
    # once the ratio is past its growth
    assert plan_segments(c, 1.5).dev == []
    assert plan_segments(c, 1.5).host == [0, 1]


def test_plan_other_codec_is_all_host():
    for codec in ("ZSTD", "GZIP", "LZ4", "BROTLI"):
        c = _zchunk([_zpage(0, 999, 1000), _zpage(999, 10, 1000)], codec)
        plan = plan_segments(c, 0.0)
        assert (plan.dev, plan.host, plan.identity) == ([], [0, 1], [])


def test_plan_v2_uncompressed_page_is_identity():
    c = _zchunk([_zpage(0, 1000, 1000, is_compressed=False),
                 _zpage(1000, 990, 1000)])
    plan = plan_segments(c, 0.93)
    assert (plan.dev, plan.host, plan.identity) == ([1], [], [0])
    c = _zchunk([_zpage(0, 1000, 1000, is_compressed=False)], "ZSTD")
    plan = plan_segments(c, 0.93)
    assert (plan.dev, plan.host, plan.identity) == ([], [], [0])


def test_plan_dict_page_is_segment_zero():
    c = _zchunk([_zpage(300, 50, 400, "dict_z"),
                 _zpage(350, 399, 400, "plain_z")],
                dict_page=DictPage(100, 300, 25, 200, True))
    plan = plan_segments(c, 0.93)
    assert plan.has_dict
    assert plan.segs == [(100, 300, 200), (300, 350, 400), (350, 749, 400)]
    assert plan.offsets == [0, 200, 600, 1000]
    assert plan.page_base == [200, 600]  # shifted past the dictionary
    # dict page 200/200 and the last page 399/400 are incompressible
    assert (plan.dev, plan.host, plan.identity) == ([0, 2], [1], [])
