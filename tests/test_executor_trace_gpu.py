"""Operator-trace replay on the device, against the same recorded traces
as the host run: the values are integers, strings and multiples of 1/4,
so both give the same rows in the same order."""

import pytest
import torch

from hyperspace_amd.ops import native

import executor_trace_common as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def traces():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native.available(), "HIP extension must load on a GPU box"
    return tc.run_traces("cuda")


@pytest.fixture(scope="module")
def golden():
    return tc.load_golden("cuda")


@pytest.mark.parametrize("name", tc.QUERY_NAMES)
def test_trace_matches_golden(traces, golden, name):
    assert traces[name] == golden[name]
