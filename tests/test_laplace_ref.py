"""tests/laplace_ref.py (the float64 restatement that gates syg_laplace_f32) against the reference's own recorded
output, tests/golden/ref_laplace.npz (tests/golden/make_golden_laplace.py), within 1e-12 of the natural scale A."""
import os

import numpy as np
import pytest

from tests import laplace_ref as R

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_laplace.npz"))


@pytest.mark.parametrize("i", range(int(GOLDEN["n"])))
def test_restatement_is_the_reference(i):
    x, s, t, F = GOLDEN[f"x_{i}"], GOLDEN[f"s_{i}"], float(GOLDEN[f"t_step_{i}"]), GOLDEN[f"F_{i}"]
    assert np.array_equal(x, x.astype(np.float32)) and np.all(np.isfinite(F)) and F.dtype == np.complex128
    A = R.scale(x, s, t)
    assert np.all(A > 0)
    assert np.all(np.abs(R.laplace(x, s, t) - F) <= 1e-12 * A)
    assert np.all(np.abs(R.laplace(x, s, t, block=7) - F) <= 1e-12 * A)              # the blocking changes nothing
    assert np.all(np.abs(R.laplace(np.stack([x, 2 * x]), s, t)[1] - 2 * F) <= 2e-12 * A)


def test_fixture_covers_the_domain():
    for i in range(1, int(GOLDEN["n"])):
        x, s, t = GOLDEN[f"x_{i}"], GOLDEN[f"s_{i}"], float(GOLDEN[f"t_step_{i}"])
        g = -s.real * t * (len(x) - 1)
        assert np.isclose(g.max(), 700.0) and s.real.max() * t >= 100.0 and (np.abs(s.imag) * t).max() > np.pi
    assert GOLDEN["F_empty_s"].shape == (0,) and np.array_equal(GOLDEN["F_empty_x"], np.zeros(3, dtype=np.complex128))


def test_scale_bounds_the_sum():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(300)
    s = rng.uniform(-0.02, 0.05, 9) + 1j * rng.uniform(-3, 3, 9)
    assert np.all(np.abs(R.laplace(x, s, 0.7)) <= R.scale(x, s, 0.7) * (1 + 1e-12))
