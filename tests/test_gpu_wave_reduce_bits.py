"""The entry points whose wave reductions moved to the shared float64 wave sum and (value, index) pick of csrc/common.h
compute what they computed with their private copies: every case of tests/wave_reduce_cases.py against the SHA-256 of its
results recorded from the earlier code (tests/golden/wave_reduce_before.json).  No tolerance: the DPP steps build the
addition tree of the ascending xor butterfly and a pick's winner does not depend on the order of its comparisons.  A
differing case means an addition order, a tie rule or a launch route changed."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests.wave_reduce_cases import CASES, digest, run


@pytest.fixture(scope="module")
def before(golden_dir):
    from sygnals_amd import ops
    ops.require_gpu()
    with open(os.path.join(golden_dir, "wave_reduce_before.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(before):
    assert sorted(before) == sorted(CASES)


@pytest.mark.parametrize("case", list(CASES))
def test_same_bits(case, before):
    got = digest(run(case))
    print(case, got["sha256"], got["first8"])
    assert got["sha256"] == before[case]["sha256"], (got["first8"], before[case]["first8"])
