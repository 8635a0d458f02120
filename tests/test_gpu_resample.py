"""GPU tests of the polyphase resampler (csrc/resample.hip) against scipy.signal.resample_poly run in float64 on the
float32 input.  Gate: |y_dev - y_scipy64| <= 1e-5 max|y_scipy64| per row.  Each group prints its worst ratio.
A one-sample row with padtype='reflect' is never handed to scipy (scipy itself dies on it).

Worst ratios measured on MI355X (fraction of the row's peak, gate 1e-5):
  ratios 2/1 2.3e-7, 1/2 9.5e-6, 3/2 2.6e-7, 2/3 2.9e-7, 1/8 7.4e-7, 160/147 2.6e-7, 147/160 3.0e-7, 160/441 2.7e-6,
  320/441 3.0e-7, 441/160 2.7e-7; 1/32 1.5e-6, 3/64 1.1e-6, 1000/1001 2.7e-7.  The two large ones are rows of TWO samples
  whose single output cancels (1/2: 0.0015 from terms of 1; 160/441: 0.009 from terms of 2): at 1/2 the float32 rounding
  of the table alone, with exact arithmetic after it, gives 7.9e-6 on that row, and 5e-8 at most on rows of Kp - 1
  samples and more.
  pad types at most 3.3e-7 (maximum), cval 2.1e-7, caller taps at most 1.5e-7, the row of 2^25 samples 4.4e-7 (both
  placements, the same bits), resample_batch 3.6e-7, resample 2.3e-7, load_audio 4.1e-7, dsp resample 2.8e-7; unit
  impulses: exact."""
import numpy as np
import pytest
from scipy.signal import resample_poly as sp_resample_poly

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from sygnals_amd import _resample as RS
from tests.gpu_util import assert_parity

GATE = 1e-5
RATIOS = [(2, 1), (1, 2), (3, 2), (2, 3), (1, 8), (160, 147), (147, 160), (160, 441), (320, 441), (441, 160)]
# beyond the issue's list: a tile that reads more input than is staged (the taps read global memory) and a table that
# the rule keeps out of LDS
EXTRA_RATIOS = [(1, 32), (3, 64), (1000, 1001)]
PADS = ("constant", "mean", "minimum", "maximum", "edge", "wrap", "symmetric", "reflect")


@pytest.fixture(scope="module")
def ops():
    from sygnals_amd import ops
    ops.require_gpu()
    return ops


def _rows(B, L, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, L)) + 0.3).astype(np.float32)


def _worst(got, want):
    """Worst per-row ratio of the error to the row's peak; asserts the gate on every row."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    peak = np.max(np.abs(want), axis=1)
    err = np.max(np.abs(got - want), axis=1)
    assert np.all(err <= GATE * peak), float(np.max(err / np.maximum(peak, 1e-300)))
    return float(np.max(err / np.maximum(peak, 1e-300)))


def _forms(ops, up, down, L):
    p = RS.resample_plan(up, down, L)
    return (None, "lds", "global") if ops.resample_table_fits_lds(p.up, p.Kp) else (None, "global")


@pytest.mark.parametrize("up,down", RATIOS + EXTRA_RATIOS)
def test_ratios_lengths_batches_forms(ops, up, down):
    tile = ops.resample_constants()["tile"]
    Kp = RS.resample_plan(up, down, 4097).Kp
    L0 = tile * down // up                                           # about one tile of outputs
    worst = 0.0
    for L in sorted({1, 2, max(Kp - 1, 1), Kp, L0 - 1, L0, L0 + 1, 4097}):
        x = _rows(33, L, 7 * L + up)
        want = sp_resample_poly(x.astype(np.float64), up, down, axis=1)
        xd = ops.to_device_f32(x)
        for form in _forms(ops, up, down, L):
            for B in (1, 3, 33):
                got = ops.resample_poly(xd[:B], up, down, form=form)
                assert got.dtype == torch.float32 and got.shape == (B, -(-L * up // down))
                worst = max(worst, _worst(got.cpu().numpy(), want[:B]))
    print(f"resample {up}/{down}: worst {worst:.2e} of the row's peak")


def test_rule_keeps_a_large_table_out_of_lds(ops):
    p = RS.resample_plan(1000, 1001, 4097)
    assert not ops.resample_table_in_lds(p.up, p.Kp) and not ops.resample_table_fits_lds(p.up, p.Kp)
    with pytest.raises(ValueError, match="form='lds'"):
        ops.resample_poly(ops.to_device_f32(_rows(1, 4097, 0)), 1000, 1001, form="lds")


@pytest.mark.parametrize("up,down,L", [(3, 2, 1500), (160, 441, 3200)])
def test_unit_impulses_give_the_table(ops, up, down, L):
    """An impulse at every position of the first tile's input span and of the last 2 Kp samples: the output is the
    table's own entries at (p, q - m), bit for bit, and zero elsewhere.  Pins n_pre_remove, the phase and q."""
    tile = ops.resample_constants()["tile"]
    p = RS.resample_plan(up, down, L)
    assert p.n_out > tile                                            # more than one tile
    first = tile * down // up + p.Kp + 2
    pos = np.unique(np.concatenate([np.arange(min(first, L)), np.arange(L - 2 * p.Kp, L)]))
    x = np.zeros((pos.size, L), dtype=np.float32)
    x[np.arange(pos.size), pos] = 1.0
    t = (np.arange(p.n_out, dtype=np.int64) + p.n_pre_remove) * down
    ph, q = t % up, t // up
    J = q[None, :] - pos[:, None]
    ok = (J >= 0) & (J < p.Kp)
    want = np.where(ok, p.table[ph[None, :], np.clip(J, 0, p.Kp - 1)], np.float32(0))
    for form in _forms(ops, up, down, L):
        got = ops.resample_poly(ops.to_device_f32(x), up, down, form=form).cpu().numpy()
        assert np.array_equal(got, want), form
    assert np.count_nonzero(want) > 0
    ref = sp_resample_poly(x[::37].astype(np.float64), up, down, axis=1)      # and scipy agrees with the table
    print(f"impulses {up}/{down}: worst {_worst(want[::37], ref):.2e}")


@pytest.mark.parametrize("padtype", PADS)
def test_padtypes(ops, padtype):
    worst = 0.0
    for L in (1, 5, 300):
        if L == 1 and padtype == "reflect":
            with pytest.raises(ValueError, match="at least two samples"):
                ops.resample_poly(ops.to_device_f32(_rows(2, 1, 0)), 160, 147, padtype=padtype)
            continue
        x = _rows(3, L, 11 + L) + np.float32(1.5)
        want = sp_resample_poly(x.astype(np.float64), 160, 147, axis=1, padtype=padtype)
        for form in (None, "global"):
            got = ops.resample_poly(ops.to_device_f32(x), 160, 147, padtype=padtype, form=form)
            worst = max(worst, _worst(got.cpu().numpy(), want))
    print(f"padtype {padtype}: worst {worst:.2e}")


def test_cval(ops):
    worst = 0.0
    for L in (1, 5, 300):
        x = _rows(3, L, 5 + L)
        want = sp_resample_poly(x.astype(np.float64), 160, 147, axis=1, padtype="constant", cval=2.5)
        got = ops.resample_poly(ops.to_device_f32(x), 160, 147, padtype="constant", cval=2.5)
        worst = max(worst, _worst(got.cpu().numpy(), want))
    print(f"cval 2.5: worst {worst:.2e}")


@pytest.mark.parametrize("ntaps", [1, 2, 30, 31])
def test_caller_taps(ops, ntaps):
    h = np.random.default_rng(ntaps).standard_normal(ntaps)
    worst = 0.0
    for up, down in ((3, 4), (5, 3), (2, 7)):
        for L in (1, 9, 1500):
            x = _rows(3, L, ntaps + L)
            want = sp_resample_poly(x.astype(np.float64), up, down, axis=1, window=h)
            for form in (None, "lds", "global"):
                got = ops.resample_poly(ops.to_device_f32(x), up, down, window=h, form=form)
                worst = max(worst, _worst(got.cpu().numpy(), want))
    print(f"caller taps {ntaps}: worst {worst:.2e}")


def test_batch_determinism_and_strides(ops):
    x = ops.to_device_f32(_rows(33, 4097, 1))
    for up, down in ((160, 441), (3, 2), (1, 32)):
        for form in (None, "global"):
            full = ops.resample_poly(x, up, down, form=form)
            assert torch.equal(full, ops.resample_poly(x, up, down, form=form))          # the same call, the same bits
            for b in (0, 16, 32):
                assert torch.equal(full[b:b + 1], ops.resample_poly(x[b:b + 1], up, down, form=form))
    wide = ops.to_device_f32(_rows(5, 6000, 2))
    view = wide[:, 100:4197]                                         # row stride 6000, unit column stride
    assert not view.is_contiguous()
    assert torch.equal(ops.resample_poly(view, 160, 441), ops.resample_poly(view.contiguous(), 160, 441))
    step = wide[:, ::2]                                              # column stride 2
    assert torch.equal(ops.resample_poly(step, 3, 2), ops.resample_poly(step.contiguous(), 3, 2))
    out = torch.zeros((5, 2000), dtype=torch.float32, device="cuda")[:, :1487]
    got = ops.resample_poly(view, 160, 441, out=out)
    assert got is out and torch.equal(out, ops.resample_poly(view, 160, 441))
    with pytest.raises(ValueError, match="out must be"):
        ops.resample_poly(view, 160, 441, out=torch.zeros((5, 1486), device="cuda"))


def test_more_rows_than_a_launch_takes(ops):
    """65537 rows go through in launches of 65535 and 2: the same bits as those rows in two calls, and right against scipy."""
    B, L = 65537, 4
    x = ops.to_device_f32(_rows(B, L, 4))
    got = ops.resample_poly(x, 2, 1)
    assert got.shape == (B, 8)
    assert torch.equal(got[:65535], ops.resample_poly(x[:65535], 2, 1))
    assert torch.equal(got[65535:], ops.resample_poly(x[65535:], 2, 1))
    rows = [0, 65534, 65535, 65536]
    _worst(got[rows].cpu().numpy(), sp_resample_poly(x[rows].cpu().numpy().astype(np.float64), 2, 1, axis=1))


def test_identity_is_a_copy(ops):
    import sygnals_amd.core.dsp as D
    x = ops.to_device_f32(_rows(3, 1000, 3))
    for got in (ops.resample_poly(x, 4, 4), D.resample_batch(x, 48000, 48000), ops.resample_poly(x[:, ::2], 7, 7)):
        want = x if got.shape == x.shape else x[:, ::2]
        assert torch.equal(got, want) and got.data_ptr() != x.data_ptr() and got.is_contiguous()
    assert ops.resample_plan(4, 4, 1000)[1] is None


def test_index_width_one_long_row(ops):
    """One row of 2^25 samples at 160/441, compared in full: t = (n + n_pre_remove) down crosses 2^31 and 2^32 inside it."""
    L = 1 << 25
    p = RS.resample_plan(160, 441, L)
    assert (p.n_out + p.n_pre_remove) * p.down > 1 << 32
    rng = np.random.default_rng(25)
    x = rng.standard_normal(L, dtype=np.float32)
    x[::4099] += 3.0
    want = sp_resample_poly(x.astype(np.float64), 160, 441)
    xd = torch.from_numpy(x).cuda()[None, :]
    for form in (None, "global"):
        got = ops.resample_poly(xd, 160, 441, form=form)[0].cpu().numpy().astype(np.float64)
        assert got.shape == want.shape
        err = np.abs(got - want)
        worst = float(err.max() / np.max(np.abs(want)))
        print(f"2^25 row 160/441 form={form}: worst {worst:.2e}, at n = {int(err.argmax())}")
        assert worst <= GATE
        for n in ((1 << 31) // 441, (1 << 32) // 441):                # around the 32-bit crossings
            assert np.max(err[n - 2000:n + 2000]) <= GATE * np.max(np.abs(want))


def test_resample_batch_and_resample(ops):
    import sygnals_amd.core.dsp as D
    x = _rows(4, 4410, 4)
    want = sp_resample_poly(x.astype(np.float64), 160, 441, axis=1)
    got = D.resample_batch(ops.to_device_f32(x), 44100, 16000)
    assert got.is_cuda and got.shape == (4, 1600)
    w1 = _worst(got.cpu().numpy(), want)
    w2 = _worst(D.resample_poly_batch(ops.to_device_f32(x), 160, 441, padtype="edge").cpu().numpy(),
                sp_resample_poly(x.astype(np.float64), 160, 441, axis=1, padtype="edge"))
    y = D.resample(x[0].astype(np.float64), 44100, 16000)
    assert isinstance(y, np.ndarray) and y.dtype == np.float64 and y.shape == (1600,)
    w3 = _worst(y[None, :], want[:1])
    y = D.resample(list(x[1]), 44100.0, 48000, window="hann", padtype="mean")
    w4 = _worst(y[None, :], sp_resample_poly(x[1:2].astype(np.float64), 160, 147, axis=1, window="hann", padtype="mean"))
    print(f"resample_batch {w1:.2e}, resample_poly_batch {w2:.2e}, resample {w3:.2e} / {w4:.2e}")


def test_load_audio_resamples_on_load(ops, tmp_path):
    from scipy.io import wavfile
    from sygnals_amd.core.audio.io import load_audio
    rng = np.random.default_rng(6)
    pcm = np.round(rng.standard_normal((22050, 2)) * 6000).astype(np.int16)
    wavfile.write(str(tmp_path / "a.wav"), 44100, pcm)
    dec = pcm.astype(np.float64) / 32768.0
    y, sr = load_audio(tmp_path / "a.wav", sr=16000)
    assert sr == 16000 and y.dtype == np.float64 and y.shape == (8000,)
    mono32 = dec.mean(axis=1).astype(np.float32).astype(np.float64)
    w1 = _worst(y[None, :], sp_resample_poly(mono32, 160, 441)[None, :])
    y, sr = load_audio(tmp_path / "a.wav", sr=48000, mono=False, offset=0.1, duration=0.2)
    assert sr == 48000 and y.shape == (2, 9600)
    cut = dec.T[:, 4410:4410 + 8820].astype(np.float32).astype(np.float64)
    w2 = _worst(y, sp_resample_poly(cut, 160, 147, axis=1))
    print(f"load_audio: worst {w1:.2e} / {w2:.2e}")


def test_mfcc_from_files_with_target_sr(ops, tmp_path):
    from scipy.io import wavfile
    from sygnals_amd.pipeline import mfcc_from_files
    rng = np.random.default_rng(8)
    sr, L, paths, clips = 44100, 22050, [], []
    for i in range(5):
        pcm = np.round(np.sin(2 * np.pi * (200.0 + 90 * i) * np.arange(L) / sr) * 9000 + rng.standard_normal(L) * 2000).astype(np.int16)
        wavfile.write(str(tmp_path / f"c{i}.wav"), sr, pcm)
        paths.append(tmp_path / f"c{i}.wav")
        clips.append(pcm.astype(np.float64) / 32768.0)
    got = mfcc_from_files(paths, sr, batch_clips=2, workers=2, target_sr=16000, n_mels=40, n_mfcc=13)
    res = sp_resample_poly(np.stack(clips).astype(np.float32).astype(np.float64), 160, 441, axis=1)
    want = ops.mfcc_batch(ops.to_device_f32(res), 16000, n_mels=40, n_mfcc=13).cpu().numpy()
    assert got.shape == want.shape == (5, 13, 1 + 8000 // 512)
    assert_parity(got, want, 1e-5, "mfcc_from_files(target_sr)")
    plain = mfcc_from_files(paths, sr, batch_clips=2, workers=2, n_mels=40, n_mfcc=13)       # the default is untouched
    assert plain.shape == (5, 13, 1 + L // 512)


def test_cli_dsp_resample(ops, tmp_path):
    from click.testing import CliRunner
    from scipy.io import wavfile
    from sygnals_amd.cli.main import cli
    from sygnals_amd import io as sio
    rng = np.random.default_rng(9)
    pcm = np.round(rng.standard_normal(4410) * 5000).astype(np.int16)
    wavfile.write(str(tmp_path / "in.wav"), 44100, pcm)
    r = CliRunner().invoke(cli, ["dsp", "resample", str(tmp_path / "in.wav"), "-o", str(tmp_path / "out.npz"), "--target-sr", "16000"])
    assert r.exit_code == 0, r.output
    y, _ = sio.signal_from(sio.read_data(tmp_path / "out.npz"))
    x32 = (pcm / 32768.0).astype(np.float32).astype(np.float64)
    w1 = _worst(y[None, :], sp_resample_poly(x32, 160, 441)[None, :])
    r = CliRunner().invoke(cli, ["dsp", "resample", str(tmp_path / "in.wav"), "-o", str(tmp_path / "out.wav"), "--target-sr", "8000",
                                 "--fs", "16000", "--window", "hamming", "--padtype", "edge"])
    assert r.exit_code == 0, r.output
    sr, out = wavfile.read(str(tmp_path / "out.wav"))
    assert sr == 8000 and out.shape == (2205,)
    print(f"dsp resample: worst {w1:.2e}")
