"""Pins tests/lpc_ref.py, the float64 restatement the LPC kernels are held to, and asserts the conditions every input of
tests/test_gpu_lpc.py has to meet for a float64 result to be a reference at all.  CPU only."""
import numpy as np
import pytest
import scipy.linalg
import scipy.optimize
import scipy.signal

from tests import lpc_cases as K
from tests import lpc_ref as R

SIG64 = {kind: K.clip(kind, 2048).astype(np.float64) for kind in K.SIGNALS}


def _burg_states(x, order):
    """The (f, b, k) of every stage, from the restatement's own recurrence."""
    f, b = x[1:].copy(), x[:-1].copy()
    _, k, _ = R.burg(x, order)
    out = []
    for ki in k:
        out.append((f, b, ki))
        f, b = (f + ki * b)[1:], (b + ki * f)[:-1]
    return out


@pytest.mark.parametrize("kind", K.SIGNALS)
def test_burg_k_minimises_the_summed_errors(kind):
    x = SIG64[kind][:400]
    for f, b, ki in _burg_states(x, 8):
        cost = lambda k: np.sum((f + k * b) ** 2 + (b + k * f) ** 2)      # noqa: E731
        res = scipy.optimize.minimize_scalar(cost, bounds=(-1.0, 1.0), method="bounded", options={"xatol": 1e-12})
        assert abs(res.x - ki) <= 1e-6                     # a quadratic's minimum, located to the square root of the tolerance
        assert cost(ki) <= res.fun * (1 + 1e-12) + 1e-300
        assert abs(ki) <= 1.0


@pytest.mark.parametrize("kind", K.SIGNALS)
@pytest.mark.parametrize("order", [1, 16, 64])
def test_burg_forms_agree_and_a_is_the_step_up(kind, order):
    x = SIG64[kind]
    a, k, err = R.burg(x, order)
    a2, k2, err2 = R.burg(x, order, carry_den=True)
    assert np.max(np.abs(a - a2)) <= 1e-8 * np.max(np.abs(a))
    assert np.max(np.abs(k - k2)) <= 1e-8 and abs(err - err2) <= 1e-8 * err
    assert np.all(np.abs(k) <= 1.0) and a[0] == 1.0 and err > 0
    assert np.max(np.abs(a - R.step_up(k))) <= 1e-14 * np.max(np.abs(a))


def test_step_up_by_hand():
    assert np.array_equal(R.step_up([0.5]), [1.0, 0.5])
    assert np.allclose(R.step_up([0.5, -0.25]), [1.0, 0.5 - 0.25 * 0.5, -0.25], rtol=0, atol=1e-16)


LOW_GAIN = ("noise", "ar4", "vowel40")


@pytest.mark.parametrize("kind", LOW_GAIN)
@pytest.mark.parametrize("order", [1, 2, 16, 64])
def test_levinson_is_solve_toeplitz(kind, order):
    xw = SIG64[kind] * scipy.signal.get_window("hann", 2048, fftbins=True)
    a, k, err, r = R.autocorr(xw, order)
    want = scipy.linalg.solve_toeplitz(r[:order], -r[1:])
    assert np.max(np.abs(a[1:] - want)) <= 1e-12 * np.max(np.abs(a))
    assert np.all(np.abs(k) < 1.0) and np.max(np.abs(a - R.step_up(k))) <= 1e-13 * np.max(np.abs(a))
    assert np.isclose(r[0], np.sum(xw * xw), rtol=1e-14) and err > 0
    # the error of the normal equations is the last prediction error power: r[0] prod (1 - k^2)
    assert np.isclose(err * 2048, r[0] * np.prod(1 - k * k), rtol=1e-9)


@pytest.mark.parametrize("n_fft", [64, 2048])
def test_envelope_is_freqz(n_fft):
    a, _, err = R.burg(SIG64["vowel40"], 16)
    w, h = scipy.signal.freqz(1.0, a, worN=n_fft // 2 + 1, include_nyquist=True)
    assert np.allclose(w, 2 * np.pi * np.arange(n_fft // 2 + 1) / n_fft)
    A = R.transfer(a, n_fft)
    assert np.max(np.abs(1.0 / A - h)) <= 1e-10 * np.max(np.abs(h))
    P = R.envelope(a, err, n_fft)
    assert np.allclose(P, err * np.abs(h) ** 2, rtol=1e-10, atol=0)
    assert np.allclose(R.envelope(a, err, n_fft, db=True), 10 * np.log10(np.maximum(P, 1e-10)), rtol=0, atol=1e-12)


def test_zero_and_constant_frames():
    for N, p in ((3, 1), (64, 5), (400, 16)):
        a, k, err = R.burg(np.zeros(N), p)
        assert np.array_equal(a, np.r_[1.0, np.zeros(p)]) and np.array_equal(k, np.zeros(p)) and err == 0.0
        for carry in (False, True):
            a, k, err = R.burg(np.full(N, 0.25), p, carry_den=carry)
            assert np.array_equal(a, np.r_[1.0, -1.0, np.zeros(p - 1)]) and err == 0.0
            assert k[0] == -1.0 and np.array_equal(k[1:], np.zeros(p - 1))
        a, k, err, r = R.autocorr(np.zeros(N), p)
        assert np.array_equal(a, np.r_[1.0, np.zeros(p)]) and np.array_equal(k, np.zeros(p)) and err == 0.0


def test_framing_is_the_cepstrogram_rule():
    from sygnals_amd import ops
    for L, N, hop, center in ((300, 64, 64, True), (500, 65, 160, False), (40, 3, 1, True), (1500, 400, 160, True),
                              (300, 400, 512, True), (5000, 2047, 2047, True), (6000, 2048, 512, True), (1000, 2048, 160, True)):
        T, pad = R.framing(L, N, hop, center)
        assert T == ops.cepstrogram_frames(L, N, hop, center) and pad == (N // 2 if center else 0)
        assert R.frames_of(np.ones(L, np.float32), N, hop, center).shape == (T, N)


def test_librosa_parity():
    librosa = pytest.importorskip("librosa")
    for kind in K.SIGNALS:
        x = SIG64[kind]
        for order in (2, 16):
            a, _, _ = R.burg(x, order, carry_den=True)
            assert np.max(np.abs(a - librosa.lpc(x, order=order))) <= 1e-10 * np.max(np.abs(a))


# ---------------------------------------------------------------- conditions on the inputs of tests/test_gpu_lpc.py
# Every frame and every row that tests/test_gpu_lpc.py compares against a float64 reference at the 1e-5 gates, from the
# same tables (tests/lpc_cases.py) and the same window tables (ops.lpc_window_table): nothing is thinned.
def _window64(window, N):
    from sygnals_amd import ops
    w = ops.lpc_window_table(window, N)
    return None if w is None else w.astype(np.float64)


def _burg_condition(x, order):
    """The two float64 forms of Burg's denominator, as a fraction of max|a|."""
    a, _, _ = R.burg(x, order)
    a2, _, _ = R.burg(x, order, carry_den=True)
    return np.max(np.abs(a - a2)) / np.max(np.abs(a))


def _autocorr_condition(xw, order):
    """Levinson against solve_toeplitz, as a fraction of max|a| (0 for r[0] = 0, where both are [1, 0, ...])."""
    a, _, _, r = R.autocorr(xw, order)
    if r[0] == 0.0:
        return 0.0
    return np.max(np.abs(a[1:] - scipy.linalg.solve_toeplitz(r[:order], -r[1:]))) / np.max(np.abs(a))


def _case_id(c):
    return "N{}-p{}-hop{}-{}-B{}-L{}".format(c[0], c[1], c[2], "c" if c[3] else "nc", c[4], c[5])


@pytest.mark.parametrize("case", K.FRAME_CASES, ids=_case_id)
def test_gpu_frame_inputs_meet_both_conditions(case):
    N, order, hop, center, B, L = case
    Y = K.frame_case_clips(case)
    windows = {name: _window64(name, N) for name in ("hann", "ones")}
    wb = wa = 0.0
    for b in range(B):
        F = R.frames_of(Y[b], N, hop, center)
        assert F.shape[0] == R.framing(L, N, hop, center)[0] >= 1
        for t in range(F.shape[0]):                          # every frame, as the GPU tests compare every frame
            d = _burg_condition(F[t], order)
            assert d <= 1e-8, (case, b, t, d)
            wb = max(wb, d)
            for name, w in windows.items():
                d = _autocorr_condition(F[t] * w, order)
                assert d <= 1e-7, (case, name, b, t, d)
                wa = max(wa, d)
    print(f"{case}: burg den forms {wb:.2e}, levinson vs solve_toeplitz {wa:.2e} of max|a|")


@pytest.mark.parametrize("B,L,order", K.ROW_CASES)
def test_gpu_long_row_inputs_meet_both_conditions(B, L, order):
    Y = K.clips(B, L)
    w = _window64("hann", L)
    for b in range(B):
        x = Y[b].astype(np.float64)
        d = _burg_condition(x, order)
        assert d <= 1e-8, (b, d)
        d = _autocorr_condition(x * w, order)
        assert d <= 1e-7, (b, d)


def test_gpu_end_to_end_inputs_meet_their_conditions():
    x = K.e2e_clip().astype(np.float64)
    assert x.shape == (K.E2E_L,)
    assert _burg_condition(x, K.E2E_ROW_BURG_ORDER) <= 1e-8                     # lpc(y, 12), dsp lpc --order 12
    n, order = K.E2E_ROW_AUTOCORR
    assert _autocorr_condition(x[:n] * _window64("hann", n), order) <= 1e-7      # lpc(y[:1500], 8, method="autocorr")
    N, hop, center, order = K.E2E_FRAMES
    for t, f in enumerate(R.frames_of(K.e2e_clip(), N, hop, center)):            # lpc_batch(y, 12, 400, 160), every frame
        assert _burg_condition(f, order) <= 1e-8, t
