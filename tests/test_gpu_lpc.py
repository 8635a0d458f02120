"""GPU tests of linear prediction (csrc/lpc.hip; ops.lpc_frames, lpc_rows, lpc_envelope and the mirrors in
core/features/cepstral.py) against tests/lpc_ref.py run in float64 on the float32 input.

Gates, per frame or row: |a - a_ref| <= 1e-5 max|a_ref|, |k - k_ref| <= 1e-5, |err - err_ref| <= 1e-5 err_ref.  Burg is
held to the restatement; the autocorrelation method to scipy.linalg.solve_toeplitz on the float64 windowed frame (k to
the restatement's Levinson recursion, which tests/test_lpc_ref.py holds to solve_toeplitz on these inputs).  The inputs
(tests/lpc_cases.py) meet the conditions asserted on the CPU in tests/test_lpc_ref.py: the two float64 forms of Burg's
denominator agree within 1e-8 max|a| and Levinson agrees with solve_toeplitz within 1e-7 max|a| on every one of them.
Pure tones are left out: two noiseless sines make the two float64 forms differ by 1e-4 at order 8, so nothing is a
reference there.  The sine with 1 % noise at order 32 is in the set: a float32 recurrence misses the gate on it by a
factor of 4.

Envelope, fed the device's own float32 a: |sqrt(err / P_dev) - |A_ref|| <= 1e-5 ||a||_1, and the dB form equals
10 log10 of the device's own P, taken in float64, within 1e-5 max(1, |dB|) (the float32 logarithm and the rounding of the
stored value).  Every result is written into an `out=` filled with NaN first.  Each group prints its worst fraction of
the gate; the fractions measured on MI355X are in README.md, "Linear prediction"."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import scipy.linalg

from tests import lpc_cases as K
from tests import lpc_ref as R

GATE = 1e-5


@pytest.fixture(scope="module")
def ops():
    from sygnals_amd import ops
    ops.require_gpu()
    return ops


def _nan(ops, shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=ops.require_gpu())


def _window64(ops, window, N):
    w = ops.lpc_window_table(window, N)
    return None if w is None else w.astype(np.float64)


def _reference(x, order, method):
    """(a, k, err) in float64 of one float64 (windowed) frame."""
    if method == "burg":
        return R.burg(x, order)
    a, k, err, r = R.autocorr(x, order)
    if r[0] != 0.0:
        a = np.r_[1.0, scipy.linalg.solve_toeplitz(r[:order], -r[1:])]
        err = (r[0] + np.dot(a[1:], r[1:])) / x.shape[0]
    return a, k, err


@functools.lru_cache(maxsize=None)
def _frames_ref(case, method, window):
    """(clips, a [B, p + 1, T], k [B, p, T], err [B, T]) in float64: computed once per setting, never written to."""
    from sygnals_amd import ops
    N, order, hop, center, B, L = case
    y = K.frame_case_clips(case)
    w = _window64(ops, window, N)
    T, _ = R.framing(L, N, hop, center)
    a, k, err = np.zeros((B, order + 1, T)), np.zeros((B, order, T)), np.zeros((B, T))
    for b in range(B):
        F = R.frames_of(y[b], N, hop, center, w)
        for t in range(T):
            a[b, :, t], k[b, :, t], err[b, t] = _reference(F[t], order, method)
    for v in (a, k, err):
        v.setflags(write=False)
    return y, a, k, err


def _fractions(a, k, err, a_ref, k_ref, err_ref, axis):
    """The worst errors as fractions of the three gates; the coefficient axis is `axis`."""
    fa = np.max(np.abs(a - a_ref), axis=axis) / (GATE * np.max(np.abs(a_ref), axis=axis))
    fk = np.max(np.abs(k - k_ref)) / GATE
    with np.errstate(invalid="ignore", divide="ignore"):
        fe = np.where(err_ref > 0, np.abs(err - err_ref) / (GATE * err_ref), np.where(err == err_ref, 0.0, np.inf))
    return float(np.max(fa)), float(fk), float(np.max(fe))


def _device_clips(ops, y, strided):
    """The clips on the device; strided: rows 1540 floats apart, starting 7 floats into a buffer of NaN."""
    B, L = y.shape
    if not strided:
        return ops.to_device_f32(y)
    assert L <= 1540
    buf = _nan(ops, (7 + 1540 * B,))
    v = torch.as_strided(buf, (B, L), (1540, 1), 7)
    v.copy_(torch.from_numpy(y))
    return v


def _run_frames(ops, case, method, window, strided=False):
    N, order, hop, center, B, L = case
    y, a_ref, k_ref, err_ref = _frames_ref(case, method, window)
    T = a_ref.shape[2]
    a, k, err = _nan(ops, (B, order + 1, T)), _nan(ops, (B, order, T)), _nan(ops, (B, T))
    got = ops.lpc_frames(_device_clips(ops, y, strided), order, N, hop, center, method, window, True, True, out=a, out_k=k, out_err=err)
    assert got[0] is a and got[1] is k and got[2] is err
    a, k, err = (v.cpu().numpy().astype(np.float64) for v in (a, k, err))
    assert np.isfinite(a).all() and np.isfinite(k).all() and np.isfinite(err).all()
    assert np.all(a[:, 0, :] == 1.0)
    return _fractions(a, k, err, a_ref, k_ref, err_ref, axis=1)


@pytest.mark.parametrize("case", K.FRAME_CASES, ids=lambda c: "N{}-p{}-hop{}-{}-B{}-L{}".format(c[0], c[1], c[2], "c" if c[3] else "nc", c[4], c[5]))
def test_burg_frames(ops, case):
    strided = case[5] <= 1540 and case[4] > 1
    fr = _run_frames(ops, case, "burg", None, strided)
    print(f"burg frames {case}: a {fr[0]:.3g}, k {fr[1]:.3g}, err {fr[2]:.3g} of the gates")
    assert max(fr) <= 1.0, fr


@pytest.mark.parametrize("window", ["hann", "ones"])
@pytest.mark.parametrize("case", K.FRAME_CASES, ids=lambda c: "N{}-p{}-hop{}-{}-B{}-L{}".format(c[0], c[1], c[2], "c" if c[3] else "nc", c[4], c[5]))
def test_autocorr_frames(ops, case, window):
    fr = _run_frames(ops, case, "autocorr", window, case[5] <= 1540 and case[4] > 1)
    print(f"autocorr frames {case} {window}: a {fr[0]:.3g}, k {fr[1]:.3g}, err {fr[2]:.3g} of the gates")
    assert max(fr) <= 1.0, fr


def test_default_windows(ops):
    y = ops.to_device_f32(K.clips(2, 1200))
    assert torch.equal(ops.lpc_frames(y, 8, 400, 160, method="autocorr"), ops.lpc_frames(y, 8, 400, 160, method="autocorr", window="hann"))
    assert torch.equal(ops.lpc_frames(y, 8, 400, 160), ops.lpc_frames(y, 8, 400, 160, method="burg", window=None))
    assert not torch.equal(ops.lpc_frames(y, 8, 400, 160), ops.lpc_frames(y, 8, 400, 160, window="hann"))


@pytest.mark.parametrize("N,order", [(3, 1), (64, 5), (65, 63), (400, 16), (2048, 64)])
def test_zero_and_constant_frames_are_exact(ops, N, order):
    L = 3 * N
    y = np.stack([K.clip("noise", L), np.zeros(L, np.float32), np.full(L, 0.25, np.float32), K.clip("ar4", L)])
    a, k, err = _nan(ops, (4, order + 1, 3)), _nan(ops, (4, order, 3)), _nan(ops, (4, 3))
    ops.lpc_frames(ops.to_device_f32(y), order, N, N, False, "burg", None, True, True, out=a, out_k=k, out_err=err)
    a, k, err = (v.cpu().numpy() for v in (a, k, err))
    for t in range(3):
        assert np.array_equal(a[1, :, t], np.r_[1.0, np.zeros(order)]) and np.array_equal(k[1, :, t], np.zeros(order)) and err[1, t] == 0.0
        assert np.array_equal(a[2, :, t], np.r_[1.0, -1.0, np.zeros(order - 1)]) and err[2, t] == 0.0
        assert np.array_equal(k[2, :, t], np.r_[-1.0, np.zeros(order - 1)])
    ra, rk, rerr = R.burg(np.full(N, 0.25), order)
    assert np.array_equal(a[2, :, 0], ra.astype(np.float32)) and np.array_equal(k[2, :, 0], rk.astype(np.float32)) and rerr == 0.0
    # the zero clip leaves its neighbours alone
    alone = ops.lpc_frames(ops.to_device_f32(y[[0, 3]]), order, N, N, False).cpu().numpy()
    assert np.array_equal(alone, a[[0, 3]])
    # the autocorrelation method: r[0] = 0 gives a = [1, 0, ...], err = 0
    a2, e2 = _nan(ops, (4, order + 1, 3)), _nan(ops, (4, 3))
    ops.lpc_frames(ops.to_device_f32(y), order, N, N, False, "autocorr", "hann", False, True, out=a2, out_err=e2)
    assert np.array_equal(a2[1].cpu().numpy(), np.r_[1.0, np.zeros(order)][:, None].repeat(3, 1)) and torch.all(e2[1] == 0)
    if N >= 64:                                               # whole rows, both forms
        for form in ("frame", "stage"):
            ar, kr, er = ops.lpc_rows(ops.to_device_f32(y[:, :N]), order, "burg", None, form, True, True)
            assert np.array_equal(ar[1].cpu().numpy(), np.r_[1.0, np.zeros(order)]) and float(er[1]) == 0.0
            assert np.array_equal(ar[2].cpu().numpy(), np.r_[1.0, -1.0, np.zeros(order - 1)]) and float(er[2]) == 0.0
            assert np.array_equal(kr[2].cpu().numpy(), np.r_[-1.0, np.zeros(order - 1)])


@functools.lru_cache(maxsize=None)
def _rows_ref(B, L, order, method):
    from sygnals_amd import ops
    y = K.clips(B, L)
    w = _window64(ops, "hann" if method == "autocorr" else None, L)
    got = [_reference(y[b].astype(np.float64) * (1.0 if w is None else w), order, method) for b in range(B)]
    a, k, err = (np.stack([g[i] for g in got]) for i in range(3))
    for v in (a, k, err):
        v.setflags(write=False)
    return y, a, k, err


@pytest.mark.parametrize("method", ["burg", "autocorr"])
@pytest.mark.parametrize("B,L,order", K.ROW_CASES)
def test_long_rows(ops, method, B, L, order):
    y, a_ref, k_ref, err_ref = _rows_ref(B, L, order, method)
    a, k, err = _nan(ops, (B, order + 1)), _nan(ops, (B, order)), _nan(ops, (B,))
    ops.lpc_rows(_device_clips(ops, y, False), order, method, None, None, True, True, out=a, out_k=k, out_err=err)
    a, k, err = (v.cpu().numpy().astype(np.float64) for v in (a, k, err))
    assert np.isfinite(a).all() and np.all(a[:, 0] == 1.0)
    fr = _fractions(a, k, err, a_ref, k_ref, err_ref, axis=1)
    print(f"{method} rows B={B} L={L} p={order}: a {fr[0]:.3g}, k {fr[1]:.3g}, err {fr[2]:.3g} of the gates")
    assert max(fr) <= 1.0, fr


@pytest.mark.parametrize("method", ["burg", "autocorr"])
@pytest.mark.parametrize("L,order", [(2048, 16), (2048, 64), (400, 16)])
def test_the_two_row_forms_agree(ops, method, L, order):
    y = ops.to_device_f32(K.clips(3, L))
    af, kf, ef = ops.lpc_rows(y, order, method, None, "frame", True, True)
    as_, ks, es = ops.lpc_rows(y, order, method, None, "stage", True, True)
    assert torch.equal(ops.lpc_rows(y, order, method), af)               # the rule at L <= 2048 is the frame form
    d = (af.double() - as_.double()).abs().amax(dim=1) / af.double().abs().amax(dim=1)
    print(f"{method} forms at L={L} p={order}: {float(d.max()):.3g} of max|a|")
    assert float(d.max()) <= 1e-6
    assert float((kf.double() - ks.double()).abs().max()) <= 1e-6
    assert float(((ef.double() - es.double()).abs() / ef.double()).max()) <= 1e-6


@pytest.mark.parametrize("order", [1, 64])
@pytest.mark.parametrize("n_fft", [64, 2048, 4096])
def test_envelope(ops, order, n_fft):
    y = ops.to_device_f32(K.clips(6, 2600))
    a, err = ops.lpc_frames(y, order, 1024, 512, True, "burg", None, False, True)
    B, _, T = a.shape
    P, D = _nan(ops, (B, n_fft // 2 + 1, T)), _nan(ops, (B, n_fft // 2 + 1, T))
    assert ops.lpc_envelope(a, err, n_fft, out=P) is P and ops.lpc_envelope(a, err, n_fft, db=True, out=D) is D
    a64, e64 = a.cpu().numpy().astype(np.float64), err.cpu().numpy().astype(np.float64)
    P64, D64 = P.cpu().numpy().astype(np.float64), D.cpu().numpy().astype(np.float64)
    assert np.isfinite(P64).all() and np.isfinite(D64).all()
    worst = 0.0
    for b in range(B):
        for t in range(T):
            A = np.abs(R.transfer(a64[b, :, t], n_fft))
            worst = max(worst, np.max(np.abs(np.sqrt(e64[b, t] / P64[b, :, t]) - A)) / (GATE * np.sum(np.abs(a64[b, :, t]))))
    want = 10.0 * np.log10(np.maximum(P64, 1e-10))
    wdb = np.max(np.abs(D64 - want) / (GATE * np.maximum(1.0, np.abs(want))))
    print(f"envelope p={order} n_fft={n_fft}: |A| {worst:.3g}, dB {wdb:.3g} of the gates")
    assert worst <= 1.0 and wdb <= 1.0


def test_batch_equals_rows_and_calls_repeat(ops):
    for method, window in (("burg", None), ("autocorr", "hann")):
        for N, order, hop in ((400, 16, 160), (2048, 32, 512), (65, 8, 7)):
            y = ops.to_device_f32(K.clips(5, 5000))
            a, k, err = ops.lpc_frames(y, order, N, hop, True, method, window, True, True)
            a2, k2, err2 = ops.lpc_frames(y, order, N, hop, True, method, window, True, True)
            assert torch.equal(a, a2) and torch.equal(k, k2) and torch.equal(err, err2)
            for b in range(5):
                ab, kb, eb = ops.lpc_frames(y[b:b + 1], order, N, hop, True, method, window, True, True)
                assert torch.equal(ab[0], a[b]) and torch.equal(kb[0], k[b]) and torch.equal(eb[0], err[b])
            assert torch.equal(ops.lpc_frames(y, order, N, hop, True, method, window), a)
            assert torch.equal(ops.lpc_frames(y, order, N, hop, True, method, window, return_error=True)[0], a)
        y = ops.to_device_f32(K.clips(3, 30000))
        r1 = ops.lpc_rows(y, 16, method, return_reflection=True, return_error=True)
        r2 = ops.lpc_rows(y, 16, method, return_reflection=True, return_error=True)
        assert all(torch.equal(u, v) for u, v in zip(r1, r2))
        assert torch.equal(ops.lpc_rows(y, 16, method), r1[0])
        for b in range(3):
            assert torch.equal(ops.lpc_rows(y[b:b + 1], 16, method)[0], r1[0][b])


def test_mirrors_and_cli_end_to_end(ops, tmp_path):
    from click.testing import CliRunner
    from scipy.io import wavfile
    from sygnals_amd.cli.main import cli
    from sygnals_amd.core.features import cepstral as CF
    sr, L = K.E2E_SR, K.E2E_L
    pcm = K.e2e_pcm()
    wavfile.write(tmp_path / "a.wav", sr, pcm)
    x32 = K.e2e_clip()
    # the inputs below are the ones tests/test_lpc_ref.py asserts the reference conditions for
    assert (K.E2E_ROW_BURG_ORDER, K.E2E_ROW_AUTOCORR, K.E2E_FRAMES) == (12, (1500, 8), (400, 160, True, 12))
    # lpc(y, order): librosa.lpc's signature, float64 [order + 1]
    a = CF.lpc(x32, 12)
    ref, _, _ = R.burg(x32.astype(np.float64), 12)
    assert a.dtype == np.float64 and a.shape == (13,) and np.max(np.abs(a - ref)) <= GATE * np.max(np.abs(ref))
    a2 = CF.lpc(x32[:1500], order=8, method="autocorr")
    w = _window64(ops, "hann", 1500)
    ref2 = _reference(x32[:1500].astype(np.float64) * w, 8, "autocorr")[0]
    assert np.max(np.abs(a2 - ref2)) <= GATE * np.max(np.abs(ref2))
    assert CF.CEPSTRAL_FEATURES["lpc"] is CF.lpc
    # lpc_batch: NumPy or device clips in, device tensors out
    ab, kb, eb = CF.lpc_batch(x32[None, :], 12, 400, 160, return_reflection=True, return_error=True)
    assert ab.is_cuda and tuple(ab.shape) == (1, 13, R.framing(L, 400, 160, True)[0])
    assert torch.equal(CF.lpc_batch(ops.to_device_f32(x32[None, :]), 12, 400, 160), ab)
    F = R.frames_of(x32, 400, 160, True)
    ref_t = R.burg(F[5], 12)[0]
    assert np.max(np.abs(ab[0, :, 5].cpu().numpy() - ref_t)) <= GATE * np.max(np.abs(ref_t))
    env = CF.lpc_envelope_batch(ab, eb, 512, db=True)
    assert tuple(env.shape) == (1, 257, ab.shape[2]) and torch.isfinite(env).all()
    # dsp lpc
    run = lambda *args: CliRunner().invoke(cli, ["dsp", "lpc", str(tmp_path / "a.wav"), *args])   # noqa: E731
    r = run("-o", str(tmp_path / "w.npz"), "--order", "12", "--envelope", "--n-fft", "512")
    assert r.exit_code == 0, r.output
    z = np.load(tmp_path / "w.npz")
    assert z["a"].shape == (13,) and z["k"].shape == (12,) and z["err"].shape == () and z["envelope"].shape == (257,)
    assert np.max(np.abs(z["a"] - ref)) <= GATE * np.max(np.abs(ref)) and np.allclose(z["frequencies"], np.arange(257) * sr / 512)
    r = run("-o", str(tmp_path / "f.npz"), "--order", "12", "--frames", "--frame-length", "400", "--hop", "160", "--method", "autocorr")
    assert r.exit_code == 0, r.output
    z = np.load(tmp_path / "f.npz")
    assert z["a"].shape == (13, ab.shape[2]) and z["k"].shape == (12, ab.shape[2]) and z["err"].shape == (ab.shape[2],)
    assert "envelope" not in z.files
    r = run("-o", str(tmp_path / "t.csv"), "--order", "4")
    assert r.exit_code == 0, r.output
    import pandas as pd
    tab = pd.read_csv(tmp_path / "t.csv")
    assert list(tab.columns) == ["frame", "index", "a", "k", "err"] and len(tab) == 5 and tab["a"][0] == 1.0
