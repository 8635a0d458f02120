"""The NMF restatement (tests/nmf_ref.py) against scikit-learn's multiplicative-update solver, its divergence against
sklearn's `_beta_divergence`, and the condition under which each iterated GPU case is gated: the float32 restatement
itself lies within a third of the gate of float64."""
import numpy as np
import pytest

from tests import nmf_cases as NC
from tests import nmf_ref as R

SK_SHAPES = [(2, 3, 2), (5, 33, 3), (65, 129, 17), (300, 12, 4)]


def _sk():
    return pytest.importorskip("sklearn.decomposition._nmf")


@pytest.mark.filterwarnings("ignore:When update_H=False")
@pytest.mark.parametrize("n_iter", [1, 10, 50])
@pytest.mark.parametrize("update_C", [False, True])
@pytest.mark.parametrize("loss", R.LOSSES)
def test_restatement_is_sklearn_mu(loss, update_C, n_iter):
    sk = _sk()
    for shape in SK_SHAPES:
        for kind in NC.KINDS:
            V, A0, C0 = (np.array(x, dtype=np.float64) for x in NC.inputs(shape, kind))
            if not update_C:                  # sklearn ignores a given W there and starts from this constant
                A0 = np.full(A0.shape, np.sqrt(V.mean() / shape[2]))
            W, H, n = sk.non_negative_factorization(V, W=A0.copy(), H=C0.copy(), n_components=shape[2], init="custom",
                                                    update_H=update_C, solver="mu", beta_loss=loss, tol=0, max_iter=n_iter)
            assert n == n_iter
            A, C = R.nmf(V, A0, C0, n_iter, loss, True, update_C)
            assert R.rel_peak(A, W) <= 1e-12 and R.rel_peak(C, H) <= 1e-12, (shape, kind)


@pytest.mark.parametrize("loss", R.LOSSES)
def test_divergence_is_sklearn_beta_divergence(loss):
    sk = _sk()
    for shape in SK_SHAPES + [(40, 1025, 8)]:
        for kind in NC.KINDS:
            V, A0, C0 = (np.array(x, dtype=np.float64) for x in NC.inputs(shape, kind))
            for A, C in ((A0, C0), NC.reference(shape, kind, loss, 10)):
                want = sk._beta_divergence(V, A, C, loss)
                assert abs(R.divergence(V, A, C, loss) - want) <= 1e-12 * max(abs(want), 1.0), (shape, kind)


def test_restatement_properties():
    """Zeros stay zeros, a zero frame or bin empties its row or column, a zero denominator takes the eps branch."""
    shape = (17, 65, 5)
    V, A0, C0 = (np.array(x) for x in NC.inputs(shape, "sparse"))
    A0[3, 1] = 0.0
    C0[2, 7] = 0.0
    C0[4, :] = 0.0                                          # a zero row of C: sum_f C = 0 under KL, zero Gram products
    for loss in R.LOSSES:
        A, C = R.nmf(V, A0, C0, 3, loss)
        assert A[3, 1] == 0 and C[2, 7] == 0 and not C[4].any()
        assert not A[17 // 2].any() and not C[:, 65 // 3].any()
        assert np.isfinite(A).all() and np.isfinite(C).all()
    z = np.zeros((4, 3))
    for loss in R.LOSSES:                                   # every denominator zero
        A, C = R.nmf(np.ones((4, 6)), z, np.zeros((3, 6)), 2, loss)
        assert not A.any() and not C.any()


def test_trace_never_rises_in_float64():
    for shape in [(5, 33, 3), (65, 129, 17), (300, 12, 4)]:
        for kind in NC.KINDS:
            for loss in R.LOSSES:
                V, A, C = NC.inputs(shape, kind)
                d = [R.divergence(V, A, C, loss)]
                for _ in range(30):
                    A, C = R.nmf(V, A, C, 1, loss)
                    d.append(R.divergence(V, A, C, loss))
                assert max(np.diff(d)) <= 1e-12 * d[0], (shape, kind, loss)


def test_init_rule():
    V = NC.inputs((5, 33, 3), "squares")[0]
    z = np.random.default_rng(1).standard_normal(3 * 33 + 5 * 3)
    A0, C0 = R.init_factors(V, 3, z)
    s = np.sqrt(V.astype(np.float64).mean() / 3)
    assert A0.dtype == C0.dtype == np.float32 and A0.shape == (5, 3) and C0.shape == (3, 33)
    assert np.allclose(C0, s * np.abs(z[:99]).reshape(3, 33), rtol=1e-6) and np.allclose(A0, s * np.abs(z[99:]).reshape(5, 3), rtol=1e-6)


@pytest.mark.parametrize("shape,kind,loss,n_iter", NC.ITERATED)
def test_condition_of_every_gated_case(shape, kind, loss, n_iter):
    """A case is gated at 1e-5 only where float32 arithmetic itself stays within a third of that."""
    assert NC.floor(shape, kind, loss, n_iter) <= NC.GATE / 3


def test_case_table():
    assert set(NC.ISSUE_SHAPES) <= set(NC.SHAPES) and any(s[1] == 2049 for s in NC.SHAPES)
    assert NC.iters_of(NC.BIG) == (10,) and NC.iters_of((40, 1025, 8)) == (10, 30)
    for T, F, K in NC.SHAPES:
        assert 1 <= F <= 2049 and 1 <= K <= 64 and T >= 1
    V = NC.inputs((65, 129, 17), "sparse")[0]
    assert not V[32].any() and not V[:, 43].any() and 0.2 < (V != 0).mean() < 0.35
