"""The strided FFT path computes what it computed before its kernels, launchers and Python compositions were given one
home: every case of tests/fft_strided_cases.py against the SHA-256 of its result recorded from the earlier code
(tests/golden/fft_strided_before.json).  No tolerance: the arithmetic is not meant to change.  A differing case means an
expression, a twiddle path, a tile width or a route changed."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests.fft_strided_cases import CASES, digest, run


@pytest.fixture(scope="module")
def before(golden_dir):
    from sygnals_amd import ops
    ops.require_gpu()
    with open(os.path.join(golden_dir, "fft_strided_before.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(before):
    assert sorted(before) == sorted(CASES)


@pytest.mark.parametrize("case", list(CASES))
def test_same_bits(case, before):
    got = digest(run(case))
    print(case, got["sha256"], got["first8"])
    assert got["sha256"] == before[case]["sha256"], (got["first8"], before[case]["first8"])
