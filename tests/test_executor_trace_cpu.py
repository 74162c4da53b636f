"""Operator-trace replay on the host: every query of
executor_trace_common must give the recorded operators, counters, rows and
row order, exactly."""

import pytest

import executor_trace_common as tc


@pytest.fixture(scope="module")
def traces():
    return tc.run_traces("cpu")


@pytest.fixture(scope="module")
def golden():
    return tc.load_golden("cpu")


def test_golden_holds_every_query(golden):
    assert sorted(golden) == sorted(tc.QUERY_NAMES)


@pytest.mark.parametrize("name", tc.QUERY_NAMES)
def test_trace_matches_golden(traces, golden, name):
    assert traces[name] == golden[name]
