"""GPU tests of the cepstral analysis (csrc/cepstrum.hip; ops.cepstrogram, real_cepstrum, complex_cepstrum,
inverse_complex_cepstrum, cepstrum_peaks) against tests/cepstrum_ref.py run in float64 on the float32 input.

G1, per frame or row: |c_dev - c_ref| <= 1e-5 K, K = mean over all n bins of ||x w||_1 / max(|X_k|, amin) from the
restatement (a float32 transform errs by a few log2(n) eps of ||x w||_1 in any bin, the logarithm turns an error d of
|X_k| into d / |X_k|, the inverse transform averages these; K >= 1, and the restatement takes K = 1 for a frame of zeros).
G2: the picker on the device's own float32 cepstrogram against the restatement's picker fed the same values: q* and the
voiced flags identical, f0 and strength within 1e-9 relative.  G3: harmonic complexes end to end within half a quefrency
sample.  Every result is written into an `out=` or a buffer filled with NaN first.  Each group prints its worst fraction
of the gate.

The round trip inverse(complex(x)) is held to 1e-5 max|x| K for even n and for the ndelay = 0 rows of odd n.  The pair
(c, ndelay) does not hold the sign of the row's sum (Im fft(c)[0] = 0 for a real c): by the definitions a row of negative
sum comes back as x - 2 mean(x) -- the restatement itself returns that to 1e-12 -- so the row -0.9^n is held, by the
same bound, to that.

Worst fractions measured on MI355X: see README.md, "Cepstral analysis"."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests import cepstrum_cases as CS
from tests import cepstrum_ref as R

GATE = 1e-5
FORMS = (None, "fused", "chain")
ONES = np.ones(2048)
ONES.setflags(write=False)


@pytest.fixture(scope="module")
def ops():
    from sygnals_amd import ops
    ops.require_gpu()
    return ops


def _wkey(window):
    return window if isinstance(window, str) else ("arr", window.shape[0])


@functools.lru_cache(maxsize=None)
def _ref(B, L, n_fft, hop, center, wkey, win_length):
    """(clips [B, L] float32, the float64 cepstrogram with every quefrency [B, n_fft, T], K [B, T]): computed once per
    setting, shared by the forms, never written to."""
    y = CS.clips(B, L)
    window = wkey if isinstance(wkey, str) else np.ones(wkey[1])
    got = [R.cepstrogram(y[b], n_fft, hop, center, window, win_length, n_fft) for b in range(B)]
    c, K = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
    for a in (y, c, K):
        a.setflags(write=False)
    return y, c, K


def _nan(ops, shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=ops.require_gpu())


def _worst(got, want, K):
    """got, want [B, Q, T], K [B, T]: the worst fraction of the gate; asserts G1 on every frame."""
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    err = np.max(np.abs(got.astype(np.float64) - want), axis=1)
    frac = float(np.max(err / (GATE * K)))
    assert np.all(err <= GATE * K), frac
    return frac


def _run(ops, y, c, K, n_fft, hop, center, window, win_length, n_ceps, form, yd=None):
    Q = n_fft // 2 + 1 if n_ceps is None else n_ceps
    out = _nan(ops, (y.shape[0], Q, c.shape[2]))
    yd = ops.to_device_f32(y) if yd is None else yd
    ret = ops.cepstrogram(yd, n_fft, hop, center, window, win_length, n_ceps, form=form, out=out)
    assert ret is out
    return out, _worst(out.cpu().numpy(), c[:, :Q], K)


# ------------------------------------------------------------------ cepstrogram
@pytest.mark.parametrize("form", FORMS)
def test_cepstrogram_lengths_hops_batches(ops, form):
    worst = 0.0
    for L in (1, 2047, 2048, 2049, 6000):
        for hop, B in ((1, 1), (160, 3), (512, 33), (2048, 3)):
            if hop == 1 and L > 2049:
                continue
            for center in (True, False):
                if not center and L < 2048:
                    with pytest.raises(ValueError, match="too short"):
                        ops.cepstrogram(ops.to_device_f32(CS.clips(B, L)), 2048, hop, center, form=form)
                    continue
                y, c, K = _ref(B, L, 2048, hop, center, "hann", None)
                worst = max(worst, _run(ops, y, c, K, 2048, hop, center, "hann", None, None, form)[1])
    print(f"cepstrogram 2048 form={form}: worst {worst:.2e} of the gate")


@pytest.mark.parametrize("form", FORMS)
def test_n_ceps_and_windows(ops, form):
    worst = 0.0
    for window, win_length in (("hann", None), (ONES, None), ("hann", 1024)):
        wkey = _wkey(window)
        y, c, K = _ref(3, 6000, 2048, 512, True, wkey, win_length)
        full = None
        for n_ceps in (2048, None, 1, 13, 400, 1025):
            out, w = _run(ops, y, c, K, 2048, 512, True, window, win_length, n_ceps, form)
            worst = max(worst, w)
            if full is None:
                full = out
            else:                                                    # the first Q rows of the full result, bit for bit
                assert torch.equal(out, full[:, :out.shape[1]].contiguous())
    print(f"cepstrogram n_ceps / windows form={form}: worst {worst:.2e} of the gate")


@pytest.mark.parametrize("n_fft", (256, 1000, 4096))
def test_chain_other_lengths(ops, n_fft):
    worst = 0.0
    for hop, center, B, n_ceps in ((n_fft // 4, True, 3, None), (160, False, 33, 13), (n_fft, True, 1, n_fft), (97, True, 3, 1)):
        y, c, K = _ref(B, 6000, n_fft, hop, center, "hann", None)
        for form in (None, "chain"):
            worst = max(worst, _run(ops, y, c, K, n_fft, hop, center, "hann", None, n_ceps, form)[1])
    y, c, K = _ref(3, 6000, n_fft, n_fft // 2, True, "hann", n_fft // 2)
    worst = max(worst, _run(ops, y, c, K, n_fft, n_fft // 2, True, "hann", n_fft // 2, None, None)[1])
    with pytest.raises(ValueError, match="2048 only"):
        ops.cepstrogram(ops.to_device_f32(y), n_fft, form="fused")
    print(f"cepstrogram n_fft={n_fft} (chain): worst {worst:.2e} of the gate")


def test_more_frames_than_the_grid_holds(ops):
    """40 clips of 16 384 samples at hop 64: 1320 tiles of frames, more than the persistent grid's workgroups."""
    k = ops.cepstrum_constants()
    B, L, hop = 40, 16384, 64
    T = 1 + L // hop
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert B * -(-T // k["tile_frames"]) > 4 * cus
    y, c, K = _ref(B, L, 2048, hop, True, "hann", None)
    worst = 0.0
    for form in ("fused", "chain"):
        worst = max(worst, _run(ops, y, c, K, 2048, hop, True, "hann", None, 64, form)[1])
    print(f"cepstrogram 40 x 16384 at hop 64: worst {worst:.2e} of the gate")


@pytest.mark.parametrize("form", FORMS)
def test_rows_sliced_out_of_a_nan_buffer(ops, form):
    B, L, pitch = 3, 6000, 6100
    y, c, K = _ref(B, L, 2048, 512, True, "hann", None)
    buf = _nan(ops, (B * pitch + 16,))
    rows = buf[7:7 + B * pitch].view(B, pitch)[:, :L]                # a float offset of 7, rows 6100 apart
    rows.copy_(torch.from_numpy(y))
    assert rows.stride(0) == pitch and rows.data_ptr() % 16 != 0
    out, w = _run(ops, y, c, K, 2048, 512, True, "hann", None, None, form, yd=rows)
    assert torch.equal(out, ops.cepstrogram(ops.to_device_f32(y), form=form))
    print(f"cepstrogram strided rows form={form}: worst {w:.2e} of the gate")


@pytest.mark.parametrize("form", FORMS)
def test_impulse_frames_and_zero_clip(ops, form):
    # one impulse a in every frame under the window of ones: c[0] = log a and zeros (K = 1)
    a, L = 2.5, 3 * 2048
    y = np.zeros((1, L), dtype=np.float32)
    y[0, [100, 2048 + 1999, 4096]] = a
    out = _nan(ops, (1, 2048, 3))
    ops.cepstrogram(ops.to_device_f32(y), 2048, 2048, False, ONES, None, 2048, form=form, out=out)
    o = out.cpu().numpy().astype(np.float64)
    assert np.max(np.abs(o[0, 0] - np.log(a))) <= GATE and np.max(np.abs(o[0, 1:])) <= GATE
    # the all-zero clip: log(amin) at q = 0 (to the rounding of a float32 logarithm near 11.5: three ulps), the same bits in
    # every frame, and exact zeros
    for n_fft, f in ((2048, form), (1000, None), (256, "chain")):
        z = torch.zeros((2, 5000), dtype=torch.float32, device=out.device)
        o = ops.cepstrogram(z, n_fft, n_fft // 4, form=f, out=_nan(ops, (2, n_fft // 2 + 1, 1 + 5000 // (n_fft // 4)))).cpu().numpy()
        assert np.all(o[:, 0] == o[0, 0, 0]) and abs(float(o[0, 0, 0]) - np.log(np.float64(np.float32(1e-5)))) <= 3 * 2.0 ** -20
        assert not o[:, 1:].any()
    # a constant clip and the zero clip sit in the batches of the other tests (signals 5 and 4 of tests/cepstrum_cases.py)


@pytest.mark.parametrize("form", FORMS)
def test_same_bits_and_batch_equals_rows(ops, form):
    y = CS.clips(33, 6000)
    yd = ops.to_device_f32(y)
    full = ops.cepstrogram(yd, hop=160, form=form)
    assert torch.equal(full, ops.cepstrogram(yd, hop=160, form=form))
    for b in (0, 5, 32):
        assert torch.equal(full[b:b + 1], ops.cepstrogram(yd[b:b + 1], hop=160, form=form))
    x = ops.to_device_f32(np.stack([CS.complex_row(k, 1000) for k in CS.COMPLEX_ROWS]))
    r = ops.real_cepstrum(x)
    c, nd = ops.complex_cepstrum(x)
    assert torch.equal(r, ops.real_cepstrum(x)) and torch.equal(c, ops.complex_cepstrum(x)[0])
    for b in (0, 3, 6):
        cb, ndb = ops.complex_cepstrum(x[b:b + 1])
        assert torch.equal(r[b:b + 1], ops.real_cepstrum(x[b:b + 1])) and torch.equal(c[b:b + 1], cb) and torch.equal(nd[b:b + 1], ndb)


# ------------------------------------------------------------------ whole rows
def _row_frac(got, want, K):
    assert got.shape == want.shape and np.isfinite(got).all()
    err = np.max(np.abs(got.astype(np.float64) - want), axis=-1)
    assert np.all(err <= GATE * K), float(np.max(err / (GATE * K)))
    return float(np.max(err / (GATE * K)))


@pytest.mark.parametrize("n", (255, 256, 1000, 1024, 4096, 4099, 65536))
def test_real_cepstrum_rows(ops, n):
    x = CS.clips(6, n)
    got = ops.real_cepstrum(ops.to_device_f32(x)).cpu().numpy()
    worst = _row_frac(got, R.real_cepstrum(x), R.row_gate_scale(x))
    for m in (n + n // 2 + 1, n - n // 3):                             # n longer and shorter than the row
        got = ops.real_cepstrum(ops.to_device_f32(x), m).cpu().numpy()
        xs = x[:, :m]
        worst = max(worst, _row_frac(got, R.real_cepstrum(x, m), R.row_gate_scale(xs, m)))
    print(f"real_cepstrum n={n}: worst {worst:.2e} of the gate")


def _complex_case(ops, kinds, n, m=None):
    """Rows of n samples transformed at length m (default n): the gating condition, ndelay, G1 and the round trip."""
    m = n if m is None else m
    x = np.stack([CS.complex_row(k, n) for k in kinds])
    c, nd = ops.complex_cepstrum(ops.to_device_f32(x), None if m == n else m)
    assert c.dtype == torch.float32 and nd.dtype == torch.int32 and tuple(c.shape) == (len(kinds), m) and tuple(nd.shape) == (len(kinds),)
    back = ops.inverse_complex_cepstrum(c, nd).cpu().numpy().astype(np.float64)
    c, nd = c.cpu().numpy(), nd.cpu().numpy()
    worst = worst_rt = 0.0
    for i, kind in enumerate(kinds):
        X = R.spectrum(x[i], m)
        phi_u, ndelay, center = R.unwrapped_phase(X)
        # a condition on the restatement, not a measurement: it holds on every listed row, so none is skipped
        assert R.unwrap_margin(R.phase(X)) > 0.1 and abs(phi_u[center] / np.pi - ndelay) < 0.25, (kind, n, m)
        want, _ = R.complex_cepstrum(x[i], m)
        K = float(R.row_gate_scale(x[i][None, :m], m)[0])
        assert nd[i] == ndelay, (kind, n, m, nd[i], ndelay)
        worst = max(worst, _row_frac(c[i], want, K))
        if m % 2 == 0 or ndelay == 0:
            xs = np.zeros(m)
            xs[:min(n, m)] = x[i, :m]
            target = xs if X[0].real >= 0 else xs - 2 * xs.mean()
            err = float(np.max(np.abs(back[i] - target)))
            bound = GATE * float(np.max(np.abs(xs))) * K
            assert err <= bound, (kind, n, m, err / bound)
            worst_rt = max(worst_rt, err / bound)
    return worst, worst_rt


@pytest.mark.parametrize("n", (255, 256, 1000, 1024, 4096, 4099, 65536))
def test_complex_cepstrum_rows(ops, n):
    w, rt = _complex_case(ops, CS.COMPLEX_ROWS, n)
    for m in (n + n // 2 + 1, n - n // 3):
        w2, rt2 = _complex_case(ops, ("damped", "damped_shift7", "three_taps", "negative"), n, m)
        w, rt = max(w, w2), max(rt, rt2)
    print(f"complex_cepstrum n={n}: worst {w:.2e} of the gate, round trip {rt:.2e} of its bound")


def test_one_row_of_2_to_the_20(ops):
    n = 1 << 20
    x = CS.clip("echo", n)[None, :]
    got = ops.real_cepstrum(ops.to_device_f32(x)).cpu().numpy()
    w = _row_frac(got, R.real_cepstrum(x), R.row_gate_scale(x))
    wc, rt = _complex_case(ops, ("damped_shift_n8",), n)
    wn, rtn = _complex_case(ops, ("negative",), n)
    print(f"one row of 2^20: real {w:.2e}, complex {max(wc, wn):.2e} of the gate, round trip {max(rt, rtn):.2e} of its bound")


def test_dsp_mirrors(ops):
    import sygnals_amd.core.dsp as D
    x = CS.complex_row("damped_shift7", 1000)
    r = D.real_cepstrum(x)
    c, nd = D.complex_cepstrum(x)
    assert r.dtype == np.float64 and c.dtype == np.float64 and isinstance(nd, int) and nd == -7
    K = float(R.row_gate_scale(x[None])[0])
    _row_frac(r, R.real_cepstrum(x), K)
    _row_frac(c, R.complex_cepstrum(x)[0], K)
    back = D.inverse_complex_cepstrum(c, nd)
    assert back.dtype == np.float64 and np.max(np.abs(back - x)) <= GATE * np.max(np.abs(x)) * K
    xd = ops.to_device_f32(x[None])
    assert torch.equal(D.real_cepstrum_batch(xd), ops.real_cepstrum(xd))
    cb, ndb = D.complex_cepstrum_batch(xd)
    assert torch.equal(cb, ops.complex_cepstrum(xd)[0]) and int(ndb[0]) == -7
    assert torch.equal(D.inverse_complex_cepstrum_batch(cb, ndb), ops.inverse_complex_cepstrum(cb, ndb))
    yd = ops.to_device_f32(CS.clips(2, 6000))
    assert torch.equal(D.cepstrogram_batch(yd, hop_length=160, n_ceps=40), ops.cepstrogram(yd, hop=160, n_ceps=40))


# ------------------------------------------------------------------ pitch
SR = 22050


@functools.lru_cache(maxsize=None)
def _harmonic(f0):
    rng = np.random.default_rng(int(10 * f0))
    t = np.arange(SR) / SR
    x = sum(np.sin(2 * np.pi * f0 * h * t) / h for h in range(1, int((SR / 2) // f0) + 1)) + 1e-3 * rng.standard_normal(SR)
    return x.astype(np.float32)


def _same_peaks(ops, ceps, qmin, qmax, threshold=R.THRESHOLD):
    f0, s, q, v = (t.cpu().numpy() for t in ops.cepstrum_peaks(ceps, qmin, qmax, float(SR), threshold))
    assert f0.dtype == np.float64 and s.dtype == np.float32 and q.dtype == np.int32 and v.dtype == np.bool_
    c = ceps.cpu().numpy()
    for b in range(c.shape[0]):
        rf0, rs, rq, rv = R.peaks(c[b], qmin, qmax, float(SR), threshold)
        assert np.array_equal(q[b], rq) and np.array_equal(v[b], rv) and np.array_equal(np.isnan(f0[b]), ~rv)
        assert np.all(np.abs(f0[b][rv] - rf0[rv]) <= 1e-9 * rf0[rv]) and np.all(np.abs(s[b] - rs) <= 1e-9 * np.abs(rs))
    return f0, s, q, v


def test_peaks_g2(ops):
    qmin, qmax = R.quefrency_range(SR, 65.0, 1000.0, 2048)
    y = np.stack([_harmonic(f) for f in (110.0, 220.0, 330.7, 523.3)] + [CS.clip("noise", SR), CS.clip("zero", SR)])
    ceps = ops.cepstrogram(ops.to_device_f32(y), n_ceps=qmax + 1)
    _same_peaks(ops, ceps, qmin, qmax)
    _same_peaks(ops, ceps, qmin, qmax, -np.inf)                       # every frame voiced: every f0 compared
    _same_peaks(ops, ceps, 40, 40)                                   # a range of one quefrency
    # ties on purpose: a plateau, a peak at qmin and at qmax, equal values everywhere, a value under the threshold
    Q, T = 60, 7
    c = np.zeros((2, Q, T), dtype=np.float32)
    c[0, 10:14, 0] = 0.5
    c[0, 5, 1] = c[0, 50, 2] = 0.9
    c[0, 20, 3], c[0, 19, 3], c[0, 21, 3] = 0.8, 0.2, 0.6
    c[0, 20, 4] = 0.12
    c[0, 7, 6] = c[0, 30, 6] = 0.4                                   # two equal peaks: the first
    c[1] = np.random.default_rng(2).standard_normal((Q, T)).astype(np.float32)
    c[1, 30, :] = c[1, 31, :] = 9.0
    f0, s, q, v = _same_peaks(ops, torch.from_numpy(c).to(ceps.device), 5, 50)
    assert list(q[0]) == [10, 5, 50, 20, 20, 5, 7] and list(v[0]) == [True, True, True, True, False, False, True]
    assert np.all(q[1] == 30)


def test_pitch_g3_end_to_end(ops):
    import sygnals_amd.core.audio.features as AF
    truth = (110.0, 220.0, 330.7, 523.3)
    y = np.stack([_harmonic(f) for f in truth] + [CS.clip("noise", SR), CS.clip("zero", SR)])
    times, f0, vf, vp = AF.fundamental_frequency_batch(ops.to_device_f32(y), SR, 65.0, 1000.0, method="cepstrum", hop_length=512)
    f0, vf, vp = f0.cpu().numpy(), vf.cpu().numpy(), vp.cpu().numpy()
    T = 1 + SR // 512
    assert f0.shape == (6, T) and np.array_equal(times, np.arange(T) * 512 / SR) and np.array_equal(vf, vp)
    inner = [t for t in range(T) if 512 * t - 1024 >= 0 and 512 * t + 1024 <= SR]
    worst = 0.0
    for i, f in enumerate(truth):
        assert np.all(vf[i, inner] == 1.0), f
        d = np.abs(SR / f0[i, inner].astype(np.float64) - SR / f)
        assert np.all(d <= 0.5), (f, float(d.max()))
        worst = max(worst, float(d.max()))
    assert not vf[4].any() and not vf[5].any() and np.isnan(f0[4:]).all()
    print(f"cepstral pitch, 110 ... 523.3 Hz: worst {worst:.3f} quefrency samples from the truth")


def test_fundamental_frequency_cepstrum_like_yin(ops):
    import sygnals_amd.core.audio.features as AF
    x = _harmonic(220.0).astype(np.float64)
    got = AF.fundamental_frequency(x, SR, 65.0, 1000.0, method="cepstrum", hop_length=256)
    ref = AF.fundamental_frequency(x, SR, 65.0, 1000.0, method="yin", hop_length=256)
    assert len(got) == len(ref) == 4
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype == np.float64 and a.shape == b.shape
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], got[3])
    v = got[2] > 0.5
    assert v[4:-4].all() and np.all(np.abs(got[1][4:-4] - 220.0) < 2.0) and np.isnan(got[1][~v]).all()
    # another frame length goes through the chain form; a higher threshold silences frames
    t1, f1, v1, _ = AF.fundamental_frequency(x, SR, 100.0, 1000.0, method="cepstrum", hop_length=256, frame_length=1000)
    assert f1.shape == (1 + SR // 256,) and np.nanmedian(np.abs(f1 - 220.0)) < 2.0
    _, _, v2, _ = AF.fundamental_frequency(x, SR, 65.0, 1000.0, method="cepstrum", hop_length=256, threshold=10.0)
    assert not v2.any()


def test_dsp_cepstrum_on_a_wav(ops, tmp_path):
    from click.testing import CliRunner
    from scipy.io import wavfile
    from sygnals_amd.cli.main import cli
    sr, L = 8000, 6000
    rng = np.random.default_rng(4)
    sig = 0.5 * np.sin(2 * np.pi * 440.0 * np.arange(L) / sr) + 0.05 * rng.standard_normal(L)
    pcm = np.round(12000 * sig).astype(np.int16)
    wavfile.write(tmp_path / "a.wav", sr, pcm)
    x32 = (pcm / 32768.0).astype(np.float32)
    run = lambda *a: CliRunner().invoke(cli, ["dsp", "cepstrum", str(tmp_path / "a.wav"), *a])   # noqa: E731
    r = run("-o", str(tmp_path / "c.npz"))
    assert r.exit_code == 0, r.output
    z = np.load(tmp_path / "c.npz")
    assert sorted(z.files) == ["cepstrum", "quefrency"] and np.allclose(z["quefrency"], np.arange(L) / sr, rtol=1e-12)
    w = _row_frac(z["cepstrum"], R.real_cepstrum(x32), float(R.row_gate_scale(x32[None])[0]))
    r = run("-o", str(tmp_path / "f.npz"), "--frames", "--hop", "256", "--n-ceps", "40")
    assert r.exit_code == 0, r.output
    z = np.load(tmp_path / "f.npz")
    want, K = R.cepstrogram(x32, 2048, 256, True, "hann", None, 40)
    assert sorted(z.files) == ["cepstrum", "hop_length", "n_fft", "quefrency"] and z["quefrency"].shape == (40,)
    w = max(w, _worst(z["cepstrum"][None], want[None], K[None]))
    r = run("-o", str(tmp_path / "k.npz"), "--kind", "complex", "--n", "8192")
    assert r.exit_code == 0, r.output
    z = np.load(tmp_path / "k.npz")
    assert sorted(z.files) == ["cepstrum", "ndelay", "quefrency"] and z["cepstrum"].shape == (8192,) and z["ndelay"].shape == ()
    r = run("-o", str(tmp_path / "f.csv"), "--frames", "--n-fft", "1000", "--hop", "500", "--n-ceps", "3")
    assert r.exit_code == 0, r.output
    import pandas as pd
    df = pd.read_csv(tmp_path / "f.csv")
    T = 1 + L // 500
    assert list(df.columns) == ["quefrency", "time", "value"] and len(df) == 3 * T
    want, K = R.cepstrogram(x32, 1000, 500, True, "hann", None, 3)
    w = max(w, _worst(df["value"].to_numpy().reshape(1, 3, T), want[None], K[None]))
    print(f"dsp cepstrum on a WAV: worst {w:.2e} of the gate")
