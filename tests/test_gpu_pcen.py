"""syg_pcen_f32 / ops.pcen and the mirrors of sygnals_amd.core.features.pcen on the device against the float64 restatement
of tests/pcen_ref.py, run in float64 on the same float32 input.

The gate, per row: |y - y64| <= 1e-5 max_t |y64|; a row whose reference is all zero must be exactly zero.  Every device call
writes into a NaN-filled `out`; every test prints its worst fraction of the gate.  Worst figures measured on MI355X: see
README.md, "PCEN"."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from sygnals_amd import ops
from sygnals_amd.core.features import pcen as PN
from tests import pcen_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
WORST = {}


def _note(key, frac):
    WORST[key] = max(WORST.get(key, 0.0), float(frac))
    print(f"{key}: fraction of the gate {float(frac):.3e}, worst so far {WORST[key]:.3e}")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _spec(B, M, T, seed=0):
    """Squared normal noise with a silent row and a silent stretch: float32 [B, M, T]."""
    x = np.random.default_rng(seed).standard_normal((B, M, T)) ** 2
    x[B // 2, M // 2] = 0.0
    x[0, 0, T // 3:T // 2] = 0.0
    return x.astype(np.float32)


def _gate(got, ref, key, what=""):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    peak = np.max(np.abs(ref), axis=-1)
    err = np.max(np.abs(got - ref), axis=-1)
    assert np.all(np.max(np.abs(got), axis=-1)[peak == 0] == 0), f"{what}: a zero row is not exactly zero"
    frac = float(np.max(np.where(peak > 0, err / np.where(peak > 0, peak, 1.0) / TOL, 0.0)))
    _note(key, frac)
    assert frac <= 1.0, f"{what}: {frac:.3e} of the gate"
    return frac


def _run(x, form=None, **kw):
    out = _nan(*x.shape)
    got = ops.pcen(_dev(x), out=out, form=form, **kw)
    assert got is out
    return got.cpu().numpy()


def _forms(T, M, ms):
    """The forms that run at this size: the tiled one always, the resident one while a band fits its LDS."""
    k = ops.pcen_constants()
    fits = ((2 + ms - 1) * (T | 1) + 8) * 4 <= k["lds_max"]
    return ("resident", "tiled") if fits else ("tiled",)


K = None


@pytest.fixture(scope="module", autouse=True)
def constants():
    global K
    K = ops.pcen_constants()
    yield
    print("worst fractions of the 1e-5 gate:", {k: f"{v:.3e}" for k, v in WORST.items()})


def test_frame_counts():
    lim, tile = K["resident_max_t"], K["tile"]
    for T in (1, 2, 63, 64, 65, lim, lim + 1, tile - 1, tile, tile + 1, 2 * tile + 3):
        x = _spec(3, 5, T, seed=T)
        for ms in (1, 3):
            assert ops.pcen_form(T, 5, ms) == ("resident" if T <= lim else "tiled")
            _gate(_run(x, max_size=ms), R.pcen(x, max_size=ms), "sizes", f"T = {T}, max_size = {ms}")


def test_band_counts_and_max_size_both_forms():
    bands = K["bands"]
    for M in (1, 2, bands - 1, bands, bands + 1, 128, 257):
        x = _spec(1 if M > 64 else 3, M, 65, seed=M)
        for ms in sorted({m for m in (1, 2, 3, 5, M) if m <= M}):
            ref = R.pcen(x, max_size=ms)
            for form in _forms(65, M, ms):
                _gate(_run(x, form, max_size=ms), ref, "sizes", f"M = {M}, max_size = {ms}, {form}")


def test_batch_of_33_and_more_rows_than_a_pass_of_the_grid():
    x = _spec(33, 7, 17, seed=1)
    for form in ("resident", "tiled"):
        _gate(_run(x, form, max_size=2), R.pcen(x, max_size=2), "sizes", f"B = 33, {form}")
    B = K["grid_max"] + 1                            # resident: B workgroups; tiled: 5 B / units workgroups
    assert 5 * B > K["grid_max"] * K["units"]
    x = _spec(B, 5, 8, seed=2)
    ref = R.pcen(x)
    for form in ("resident", "tiled"):
        _gate(_run(x, form), ref, "sizes", f"[{B}, 5, 8], {form}")


def test_both_forms_on_the_same_input():
    for T in (65, K["resident_max_t"], 1500):
        x = _spec(2, 6, T, seed=T + 7)
        for ms in (1, 3):
            ref = R.pcen(x, max_size=ms, b=0.056)
            got = {f: _run(x, f, max_size=ms, b=0.056) for f in ("resident", "tiled")}
            for f, g in got.items():
                _gate(g, ref, "forms", f"T = {T}, max_size = {ms}, {f}")


@pytest.mark.parametrize("scale", [1e-6, 1.0, 2.0 ** 31])
def test_parameters_scalars_vectors_and_scales(scale):
    M = 9
    x = _spec(2, M, 200, seed=11)
    vec = dict(gain=np.array([0.98, 0.5, 0.0, 0.8, 1.0, 0.98, 0.98, 0.3, 0.98]),
               bias=np.array([2.0, 0.0, 1.0, 10.0, 0.0, 2.0, 0.0, 0.5, 2.0]),
               power=np.array([0.5, 0.25, 0.0, 1.0, 0.0, 0.5, 0.5, 0.125, 0.5]),
               eps=np.array([1e-6, 1e-3, 1e-6, 1e-9, 1.0, 1e-6, 1e-6, 1e-6, 1e-2]),
               b=np.array([0.05, 1.0, 0.3, 1e-3, 0.5, 0.056, 0.056, 0.9, 0.01]))
    cases = [{}, {"b": 1.0}, {"b": 0.056}, {"power": 0.0}, {"bias": 0.0}, {"bias": 0.0, "power": 1.0}, {"gain": 0.0}, {"sr": 16000, "hop_length": 160},
             vec, {"b": vec["b"]}, {"power": vec["power"], "bias": vec["bias"]}]
    for kw in cases:
        for ms in (1, 3):
            ref = R.pcen(x, max_size=ms, scale=scale, **kw)
            for form in ("resident", "tiled"):
                _gate(_run(x, form, max_size=ms, scale=scale, **kw), ref, f"parameters, scale {scale:g}", f"{sorted(kw)}, {form}")


@pytest.mark.parametrize("b", [1e-3, 1e-4])
def test_slow_smoothers_on_long_noisy_rows(b):
    """64 rows of 20 000 frames with a stretch 1e-4 quieter: where b x + (1 - b) m carried in float32 misses the gate."""
    x = R.noisy_rows(64, 20000, seed=3)[None]
    ref = R.pcen(x, b=b)
    _gate(_run(x, b=b), ref, f"long rows, b = {b:g}", "tiled")
    x3 = x[:, :, :3001]
    for form in ("resident", "tiled"):
        _gate(_run(x3, form, b=b), R.pcen(x3, b=b), f"long rows, b = {b:g}", f"T = 3001, {form}")


def test_strided_rows_in_and_out():
    big = _dev(_spec(3, 64, 70, seed=5))
    buf = _nan(3, 50, 80)
    for form in ("resident", "tiled"):
        for ms in (1, 3):
            S = big[:, :40, :65]
            out = buf[:, 5:45, 3:68]
            assert not S.is_contiguous() and not out.is_contiguous()
            buf.fill_(float("nan"))
            got = ops.pcen(S, max_size=ms, out=out, form=form)
            assert got is out
            _gate(out.cpu().numpy(), R.pcen(S.cpu().numpy(), max_size=ms), "strides", f"{form}, max_size = {ms}")
            rest = buf.clone()
            rest[:, 5:45, 3:68] = float("nan")
            assert torch.isnan(rest).all()           # nothing is written outside `out`
    S = big[::2, 1::3, 2:]                           # every axis but T strided
    _gate(ops.pcen(S).cpu().numpy(), R.pcen(S.cpu().numpy()), "strides", "steps over B and M")


def test_out_is_the_input():
    for T, ms, form in ((65, 1, None), (65, 3, None), (2051, 1, "tiled"), (2051, 2, "tiled"), (300, 1, "resident")):
        x = _spec(2, 6, T, seed=T)
        S = _dev(x)
        got = ops.pcen(S, max_size=ms, out=S, form=form)
        assert got is S
        _gate(S.cpu().numpy(), R.pcen(x, max_size=ms), "in place", f"T = {T}, max_size = {ms}")


@pytest.mark.parametrize("piece", [1, 7, 64, 1000])
def test_pieces_chained_through_zf(piece):
    x = _spec(2, 6, 1500, seed=piece)
    S = _dev(x)
    for ms in (1, 3):
        ref, zf_ref = R.pcen(x, max_size=ms, return_zf=True)
        whole, zf_whole = ops.pcen(S, max_size=ms, return_zf=True)
        assert zf_whole.dtype == torch.float64 and tuple(zf_whole.shape) == (2, 6)
        assert np.max(np.abs(zf_whole.cpu().numpy() - zf_ref) / np.abs(zf_ref)) <= 1e-6
        zi, parts = None, []
        for t0 in range(0, 1500, piece):
            y, zi = ops.pcen(S[..., t0:t0 + piece], max_size=ms, zi=zi, return_zf=True)
            parts.append(y)
        got = torch.cat(parts, dim=-1).cpu().numpy()
        _gate(got, ref, "streaming", f"pieces of {piece}, max_size = {ms}")
        assert np.max(np.abs(zi.cpu().numpy() - zf_ref) / np.abs(zf_ref)) <= 1e-6
        _gate(got, whole.cpu().numpy(), "streaming", f"pieces of {piece} against the whole clip on the device")
    # a host zi in scipy's convention, and the closing state of the resident form
    zi0 = np.random.default_rng(piece).uniform(0.0, 2.0, (2, 6))
    ref, zf_ref = R.pcen(x[..., :100], zi=zi0, return_zf=True)
    for form in ("resident", "tiled"):
        y, zf = ops.pcen(S[..., :100], zi=zi0, return_zf=True, form=form)
        _gate(y.cpu().numpy(), ref, "streaming", f"host zi, {form}")
        assert np.max(np.abs(zf.cpu().numpy() - zf_ref) / np.abs(zf_ref)) <= 1e-6


def test_same_call_twice_and_batch_against_rows_bit_for_bit():
    for T, form in ((65, "resident"), (65, "tiled"), (2051, "tiled"), (300, "resident")):
        x = _spec(3, 70, T, seed=T + 1)
        S = _dev(x)
        for ms in (1, 3):
            a, za = ops.pcen(S, max_size=ms, form=form, return_zf=True)
            b, zb = ops.pcen(S, max_size=ms, form=form, return_zf=True)
            assert torch.equal(a, b) and torch.equal(za, zb)
            for i in range(3):
                r, zr = ops.pcen(S[i:i + 1], max_size=ms, form=form, return_zf=True)
                assert torch.equal(r[0], a[i]) and torch.equal(zr[0], za[i]), (T, form, ms, i)


def test_mirror_takes_librosas_shapes():
    x = _spec(1, 12, 90, seed=4)[0]
    zi = np.random.default_rng(0).uniform(0.1, 1.0, (12, 1))
    ref, zf_ref = R.pcen(x, max_size=3, zi=zi[:, 0], return_zf=True)
    y, zf = PN.pcen(x, max_size=3, zi=zi, return_zf=True)
    assert y.dtype == np.float64 and y.shape == x.shape and zf.shape == (12, 1)
    _gate(y, ref, "mirrors", "pcen [M, T]")
    assert np.allclose(zf[:, 0], zf_ref, rtol=1e-6)
    _gate(PN.pcen(torch.from_numpy(x[3])), R.pcen(x[3:4])[0], "mirrors", "pcen [T] from a tensor")
    _gate(PN.pcen_batch(x[None], b=0.2).cpu().numpy(), R.pcen(x[None], b=0.2), "mirrors", "pcen_batch from an array")


def test_outside_the_contract_gives_nan_and_no_fault():
    x = _spec(1, 4, 65, seed=8)
    x[0, 1, 10] = -1.0
    x[0, 2, 20] = np.nan
    for form in ("resident", "tiled"):
        got = ops.pcen(_dev(x), form=form).cpu().numpy()
        assert np.isfinite(got[0, 0]).all() and np.isfinite(got[0, 3]).all()
        _gate(got[:, ::3], R.pcen(x[:, ::3]), "sizes", f"the rows beside a NaN, {form}")


def test_pcen_mel_batch():
    sr, L = 22050, 22050
    rng = np.random.default_rng(6)
    t = np.arange(L) / sr
    y = (0.3 * np.sin(2 * np.pi * 440 * t) * (t > 0.3) + 0.01 * rng.standard_normal(L)).astype(np.float32)
    ys = np.stack([y, y[::-1].copy()])
    for n_mels, ms in ((128, 1), (40, 3)):
        got = PN.pcen_mel_batch(ys, sr, n_mels=n_mels, max_size=ms)
        assert got.is_cuda and tuple(got.shape) == (2, n_mels, 1 + L // 512)
        mel = ops.stft_front(_dev(ys), sr, 2048, 512, n_mels=n_mels, power=1.0)[0].cpu().numpy()
        _gate(got.cpu().numpy(), R.pcen(mel, sr=sr, hop_length=512, max_size=ms, scale=2.0 ** 31), "mel chain",
              f"{n_mels} bands against the restatement fed the device's mel")
        # end to end against the oracle's mel: the mel block's own float32 error (gated where the mel is tested) comes on
        # top and PCEN's gain divides it by the smoothed level, so this figure is reported, not gated
        want = np.stack([R.pcen(O.melspectrogram(np.abs(O.stft(c, 2048, 512)), sr, 2048, n_mels), sr=sr, hop_length=512,
                                max_size=ms, scale=2.0 ** 31) for c in ys])
        err = np.max(np.abs(got.cpu().numpy() - want), axis=-1) / np.max(np.abs(want), axis=-1)
        print(f"pcen_mel_batch end to end, {n_mels} bands: worst row error {err.max():.3e} of the row's peak")
        assert np.isfinite(err).all()


def test_cli_round_trip(tmp_path):
    import pandas as pd
    import scipy.io.wavfile
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    sr = 22050
    y = (0.2 * np.sin(np.arange(8192) * 0.05)).astype(np.float32)
    wav = tmp_path / "a.wav"
    scipy.io.wavfile.write(wav, sr, y)
    want = PN.pcen_mel_batch(y[None], sr, n_mels=40, max_size=3, gain=0.8)[0].cpu().numpy()
    run = CliRunner().invoke
    opts = ["--n-mels", "40", "--max-size", "3", "--gain", "0.8"]
    r = run(cli, ["features", "pcen", str(wav), "-o", str(tmp_path / "p.npz")] + opts)
    assert r.exit_code == 0, r.output
    z = np.load(tmp_path / "p.npz")
    assert np.array_equal(z["pcen"], want) and np.allclose(z["time"], np.arange(want.shape[1]) * 512 / sr)
    r = run(cli, ["features", "pcen", str(wav), "-o", str(tmp_path / "p.csv")] + opts)
    assert r.exit_code == 0, r.output
    t = pd.read_csv(tmp_path / "p.csv")
    assert list(t.columns) == ["time"] + [f"pcen_{i}" for i in range(40)]
    assert np.allclose(t[[f"pcen_{i}" for i in range(40)]].to_numpy().T, want, rtol=1e-6)
