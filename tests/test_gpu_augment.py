"""Augmentation on the device (syg_phase_vocoder_f32, syg_fx_add_noise_f32, ops.time_stretch and the mirrors of
sygnals_amd.core.augment) against the float64 restatement of tests/vocoder_ref.py and the reference's recorded add_noise
(tests/golden/ref_augment.npz).

G1 feeds the restatement the very D the kernel reads and G2 the device's own STFT, so both are well-conditioned and held
to 1e-5 of the peak at every rate; G3 compares end to end and gates only the rates at which the vocoder's products
telescope (0.5 and 1).  Worst figures measured on MI355X (gate 1e-5 of the peak unless stated): G1 1.6e-7 (T' = 11 000,
both forms; rate 1: 1.7e-10), G2 2.4e-7, G3 3.8e-7, G4 5.6e-8 and 2.0e-5 dB of SNR (a clip of one sample at 40 dB)
against 1e-4 dB."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import sygnals_amd.core.audio.effects as E
import sygnals_amd.core.augment as A
from sygnals_amd import ops
from sygnals_amd._lib import lib
from tests import hpss_ref as H
from tests import vocoder_ref as V
from tests.gpu_util import assert_parity, peak_rel

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_augment.npz"))
RATES = (0.25, 0.37, 0.5, 0.8, 1.0, 1.25, 2.0, 3.7)
FORMS = (None, "chain", "chunked")


def parity(a, b, what="", tol=1e-5):
    """assert_parity, with the figure printed first (pytest -s shows the measured errors)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape == b.shape and b.size:
        print(f"parity {what}: {peak_rel(a, b):.2e}")
    assert_parity(a, b, tol=tol, what=what)


def cpu(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------- G1: the kernel from a shared STFT
@functools.lru_cache(maxsize=None)
def synth_D(B, T, seed=0):
    """[B, T, 1025] complex64: magnitudes over eight decades, random phase, and the cases u(z) must get right: an
    all-zero frame, an all-zero bin, one element stored as -0 + 0j, one bin row at 1e-30."""
    rng = np.random.default_rng(1000 * T + 10 * B + seed)
    mag = 10.0 ** rng.uniform(-8.0, 0.0, (B, T, 1025))
    D = (mag * np.exp(2j * np.pi * rng.uniform(0, 1, (B, T, 1025)))).astype(np.complex64)
    D[:, :, 77] = 0
    D[:, :, 500] = (1e-30 * np.exp(2j * np.pi * rng.uniform(0, 1, (B, T)))).astype(np.complex64)
    if T >= 3:
        D[:, T // 2, :] = 0
    D[0, min(1, T - 1), 300] = complex(-0.0, 0.0)
    D[-1, 0, 301] = complex(-0.0, 0.0)                   # in the frame that seeds the phase
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def want_D(B, T, rate, seed=0):
    D = synth_D(B, T, seed)
    return np.stack([V.phase_vocoder(D[b].T.astype(np.complex128), rate).T for b in range(B)])      # [B, T', 1025]


def to_dev(D):
    return torch.from_numpy(np.array(D).view(np.float32).reshape(D.shape + (2,))).cuda()      # a writable copy


def to_host(t):
    a = cpu(t)
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


def check_vocoder(B, T, rate, form, seed=0):
    want = want_D(B, T, rate, seed)
    got = to_host(ops.phase_vocoder(to_dev(synth_D(B, T, seed)), rate, form=form))
    assert got.shape == want.shape == (B, int(np.ceil(T / rate)), 1025)
    worst = 0.0
    for b in range(B):                                   # the gate is each clip's own peak
        pk = np.max(np.abs(want[b]))
        assert np.isfinite(got[b].view(np.float64)).all()
        err = np.max(np.abs(got[b] - want[b])) / pk
        e1024 = np.max(np.abs(got[b][:, 1024] - want[b][:, 1024])) / pk
        worst = max(worst, err)
        # bins far below the clip's peak, on their own: the row at 1e-30 against its own peak (u(z) must not underflow to
        # (1, 0) there), and the all-zero bin, which stays zero
        p500 = np.max(np.abs(want[b][:, 500]))
        e500 = np.max(np.abs(got[b][:, 500] - want[b][:, 500])) / p500 if p500 > 0 else 0.0
        assert e500 <= 1e-5, f"B={B} T={T} rate={rate} form={form} clip {b}: the bin at 1e-30 is off by {e500:.3e} of its peak"
        assert np.all(got[b][:, 77] == 0)
        assert err <= 1e-5 and e1024 <= 1e-5, f"B={B} T={T} rate={rate} form={form} clip {b}: {err:.3e} (bin 1024 {e1024:.3e})"
        if rate == 1.0:
            assert np.max(np.abs(got[b] - synth_D(B, T, seed)[b])) <= 1e-6 * pk
    print(f"G1 B={B} T={T} rate={rate} form={form}: {worst:.2e}")
    return worst


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("T", [1, 2, 3, 65])
def test_g1_small_shapes_every_rate(T, form):
    for rate in RATES + (T + 0.5,):                      # the last: a rate greater than T, one output frame
        check_vocoder(3, T, rate, form)
    check_vocoder(1, T, 0.8, form)


def _frames_for(n_out, rate):
    """T with ceil(T / rate) == n_out, or None."""
    for T in range(max(1, int(n_out * rate) - 2), int(n_out * rate) + 3):
        if len(np.arange(0, T, rate)) == n_out:
            return T
    return None


@pytest.mark.parametrize("form", FORMS)
def test_g1_output_lengths_around_the_chunk(form):
    K = ops.phase_vocoder_chunk()
    seen = 0
    for n_out in (K - 1, K, K + 1, 3 * K + 5, 4 * K, 4 * K + 1):       # 4 K: where the rule takes the chunked form at B = 1
        for rate in (1.0, 1.25, 0.37, 0.8):
            T = _frames_for(n_out, rate)
            if T is not None:
                seen += 1
                for B in (1, 3):
                    check_vocoder(B, T, rate, form)
    assert seen >= 12                                    # rates 1 and 1.25 reach every length


@pytest.mark.parametrize("form", ["chain", "chunked"])
def test_g1_one_long_row(form):
    check_vocoder(1, 8800, 0.8, form, seed=3)            # T' = 11000


@pytest.mark.parametrize("form", ["chain", "chunked"])
def test_g1_forms_agree_and_nothing_is_written_past_the_output(form):
    """The C ABI on a buffer with a canary behind D' (and one in front); the two forms differ by float64 rounding only."""
    B, T, rate = 3, 130, 0.8
    col, alpha = (torch.from_numpy(a).cuda() for a in ops.T.vocoder_steps(T, rate))
    To, f = len(col), ops.VOCODER_FORMS[form]
    D = to_dev(synth_D(B, T))
    n, pad = B * To * 1025 * 2, 4096
    buf = torch.full((n + 2 * pad,), 12345.0, dtype=torch.float32, device="cuda")
    wb = lib().syg_phase_vocoder_work_bytes(B, To, f)
    work = torch.empty((max(wb, 16) // 8,), dtype=torch.float64, device="cuda")
    rc = lib().syg_phase_vocoder_f32(C.c_void_p(D.data_ptr()), B, T, C.c_void_p(col.data_ptr()), C.c_void_p(alpha.data_ptr()),
                                     To, C.c_void_p(buf.data_ptr() + 4 * pad), C.c_void_p(work.data_ptr()), f,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib().syg_last_error()
    h = cpu(buf)
    assert np.all(h[:pad] == 12345.0) and np.all(h[n + pad:] == 12345.0)
    got = h[pad:n + pad].reshape(B, To, 1025, 2)
    other = cpu(ops.phase_vocoder(D, rate, form="chunked" if form == "chain" else "chain"))
    assert np.max(np.abs(got.astype(np.float64) - other)) <= 2.0 ** -22 * np.max(np.abs(other))
    assert np.array_equal(got, cpu(ops.phase_vocoder(D, rate, form=form)))


def test_g1_a_column_outside_the_input_reads_as_zero():
    """A table from elsewhere cannot make the kernel read outside D: columns below 0 and from T on are zero."""
    B, T = 1, 4
    D = synth_D(B, T)
    col = np.array([0, 3, 4, 7, -1, -5, 2], dtype=np.int32)
    alpha = np.array([0.0, 0.5, 0.5, 0.25, 0.5, 0.5, 0.0])
    out = torch.empty((B, len(col), 1025, 2), dtype=torch.float32, device="cuda")
    d, c, a = to_dev(D), torch.from_numpy(col).cuda(), torch.from_numpy(alpha).cuda()
    rc = lib().syg_phase_vocoder_f32(C.c_void_p(d.data_ptr()), B, T, C.c_void_p(c.data_ptr()), C.c_void_p(a.data_ptr()),
                                     len(col), C.c_void_p(out.data_ptr()), None, 0,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib().syg_last_error()
    got = np.abs(to_host(out))[0]                                         # [T', 1025]
    mags = np.abs(D[0].astype(np.complex128))                             # [T, 1025]
    close = lambda x, w: np.allclose(x, w, rtol=1e-6, atol=0)
    assert close(got[0], mags[0]) and close(got[6], mags[2])
    assert close(got[1], 0.5 * mags[3])                                   # column 4 = T is zero
    assert close(got[4], 0.5 * mags[0])                                   # column -1 is zero, column 0 is not
    assert np.all(got[2] == 0) and np.all(got[3] == 0) and np.all(got[5] == 0)


# ---------------------------------------------------------------- G2: the chain against the device's own STFT
@functools.lru_cache(maxsize=None)
def clips(L, seed=0):
    rng = np.random.default_rng(L + seed)
    y = np.stack([V.tones_noise(L, seed=L % 97), 0.3 * rng.standard_normal(L)])
    return y.astype(np.float32)


@pytest.mark.parametrize("L", [1, 511, 512, 2049, 8192, 65536])
def test_g2_chain_from_the_device_stft(L):
    y = torch.from_numpy(clips(L)).cuda()
    D = to_host(ops.stft2048_c2c(y))                     # [B, T, 1025]
    worst = 0.0
    for rate in RATES:
        Lo = V.stretch_length(L, rate)
        if Lo < 1:                                       # L = 1 at rates 2 and 3.7: no sample is left
            with pytest.raises(ValueError):
                ops.time_stretch(y, rate)
            continue
        got = cpu(ops.time_stretch(y, rate))
        assert got.shape == (2, Lo)
        for b in range(2):
            Ds = V.phase_vocoder(D[b].T, rate)
            want = H.istft(Ds, Lo)
            if np.max(np.abs(want)) == 0:
                assert np.all(got[b] == 0)
                continue
            worst = max(worst, peak_rel(got[b], want))
            assert_parity(got[b], want, what=f"G2 L={L} rate={rate} clip {b}")
    print(f"G2 L={L}: {worst:.2e}")


def test_g2_lengths():
    """round(L / rate) is Python's, half to even; it may pass librosa's default length 512 (T' - 1), which istft2048 fills
    from the frames it has (the values are G2's to check)."""
    assert ops.time_stretch(torch.from_numpy(clips(2049)).cuda(), 2.0).shape[1] == 1024      # 1024.5 -> 1024
    assert ops.time_stretch(torch.from_numpy(clips(8192)).cuda(), 3.7).shape[1] == 2214      # T' = 5: 512 * 4 = 2048
    assert ops.time_stretch(torch.from_numpy(clips(511)).cuda(), 0.25).shape[1] == 2044


# ---------------------------------------------------------------- G3: end to end where the problem is well-conditioned
@pytest.mark.parametrize("L", [8192, 65536])
@pytest.mark.parametrize("signal", ["tones_noise", "white"])
def test_g3_end_to_end_at_the_telescoping_rates(signal, L):
    y32 = getattr(V, signal)(L).astype(np.float32)
    for rate in (0.5, 1.0):
        got = cpu(ops.time_stretch(torch.from_numpy(y32[None, :]).cuda(), rate))[0]
        parity(got, V.time_stretch(y32.astype(np.float64), rate), f"G3 {signal} L={L} rate={rate}")


# ---------------------------------------------------------------- G4: add_noise
def _golden_cases():
    for i in range(int(GOLDEN["n_cases"])):
        yield (GOLDEN[f"y_{i}"], float(GOLDEN["snr_db"][i]), int(GOLDEN["seed"][i]), bool(GOLDEN["silent"][i]),
               GOLDEN[f"out_{i}"])


def snr_of(y, out):
    n = np.asarray(out, dtype=np.float64) - y
    return 10.0 * np.log10(np.mean(y ** 2) / np.mean(n ** 2))


def test_g4_add_noise_against_the_recorded_reference():
    for i, (y, snr, seed, silent, want) in enumerate(_golden_cases()):
        got = A.add_noise(y, snr, "gaussian", seed)
        assert got.dtype == np.float64 and got.shape == y.shape
        if silent:
            assert np.array_equal(got, y)
            continue
        parity(got, want, f"G4 golden {i} (L={len(y)}, {snr} dB)")
        parity(got, V.add_noise(y, snr, seed), f"G4 restatement {i}")
        d = abs(snr_of(y, got) - snr)
        print(f"G4 golden {i}: SNR off by {d:.2e} dB")
        assert d <= 1e-4


@pytest.mark.parametrize("L", [1, 7, 4096, "resident", "resident+1", 70001])
def test_g4_rows_with_their_own_snr(L):
    L = ops.fx_add_noise_resident_max() + (L == "resident+1") if isinstance(L, str) else L    # 128 KiB of LDS, and past it
    rng = np.random.default_rng(L)
    B = 5
    y = (0.4 * rng.standard_normal((B, L)) + 0.1).astype(np.float32)
    y[2] = 0.0                                                        # a silent row
    y[3] = np.float32(1e-9)                                           # power 1e-18: silent by the reference's rule
    noise = rng.standard_normal((B, L)).astype(np.float32)
    snr = np.array([-5.0, 10.0, 40.0, 40.0, 23.5])
    yd, nd = torch.from_numpy(y).cuda(), torch.from_numpy(noise).cuda()
    got = cpu(ops.fx_add_noise(yd, nd, snr))
    for b in range(B):
        want = V.add_noise_with(y[b], noise[b], snr[b])
        if b in (2, 3):
            assert np.array_equal(got[b], y[b])                      # bit for bit
            continue
        parity(got[b], want, f"G4 L={L} row {b}")
        d = abs(snr_of(y[b].astype(np.float64), got[b]) - snr[b])
        print(f"G4 L={L} row {b}: SNR off by {d:.2e} dB")
        assert d <= 1e-4
    # one number for the batch, a device tensor of them, and in place
    assert np.array_equal(cpu(ops.fx_add_noise(yd, nd, 10.0))[1], got[1])
    assert np.array_equal(cpu(ops.fx_add_noise(yd, nd, torch.from_numpy(snr).cuda())), got)
    buf = yd.clone()
    assert ops.fx_add_noise(buf, nd, snr, out=buf) is buf and np.array_equal(cpu(buf), got)


def test_g4_zero_noise_rows_and_strided_rows():
    rng = np.random.default_rng(8)
    L = 1000
    wide = torch.from_numpy(rng.standard_normal((3, 2 * L)).astype(np.float32)).cuda()
    y, noise = wide[:, :L], wide[:, L:]                               # row stride 2 L
    got = cpu(ops.fx_add_noise(y, noise, 6.0))
    for b in range(3):
        parity(got[b], V.add_noise_with(cpu(y[b]), cpu(noise[b]), 6.0), f"G4 strided row {b}")
    zero = torch.zeros_like(noise)
    assert np.array_equal(cpu(ops.fx_add_noise(y, zero, 6.0)), cpu(y))


def test_g4_batch_mirror_draws_the_reference_noise():
    rng = np.random.default_rng(4)
    for L in (4096, ops.fx_add_noise_resident_max() + 1):
        y = (0.3 * rng.standard_normal((3, L))).astype(np.float32)
        batch = cpu(A.add_noise_batch(torch.from_numpy(y).cuda(), 10.0, seed=5))
        single = A.add_noise(y[0].astype(np.float64), 10.0, seed=5)
        if L == 4096:
            assert np.array_equal(batch[0].astype(np.float64), single)    # row 0 is the single clip's draw, same launch plan
        else:
            parity(batch[0], single, "G4 row 0 of a long batch", tol=1e-6)  # other slices: the sums round differently
        noise = np.random.default_rng(5).standard_normal((3, L))
        for b in range(3):
            parity(batch[b], V.add_noise_with(y[b], noise[b], 10.0), f"G4 batch row {b}")
        mine = torch.from_numpy(noise[::-1].astype(np.float32).copy()).cuda()
        got = cpu(A.add_noise_batch(torch.from_numpy(y).cuda(), 3.0, noise=mine))
        parity(got[1], V.add_noise_with(y[1], cpu(mine[1]), 3.0), "G4 caller's noise")
    with pytest.warns(UserWarning, match="Pink noise generation is currently a placeholder"):
        pink = A.add_noise(y[0].astype(np.float64), 10.0, "pink", seed=5)
    assert np.array_equal(pink, A.add_noise(y[0].astype(np.float64), 10.0, "white", seed=5))
    with pytest.warns(UserWarning, match="Brown noise generation is currently a placeholder"):
        A.add_noise_batch(torch.from_numpy(y).cuda(), 10.0, "brown", seed=5)


# ---------------------------------------------------------------- G5: mirrors and CLI
def test_g5_mirrors():
    y = V.tones_noise(6000).astype(np.float32).astype(np.float64)
    for fn in (E.time_stretch, A.time_stretch):
        out = fn(y, 0.8)
        assert out.dtype == np.float64 and out.shape == (7500,)
        D = to_host(ops.stft2048_c2c(torch.from_numpy(y.astype(np.float32)[None]).cuda()))[0].T
        parity(out, H.istft(V.phase_vocoder(D, 0.8), 7500), "G5 time_stretch")
    b = E.time_stretch_batch(torch.from_numpy(np.stack([y, -y]).astype(np.float32)).cuda(), 0.8)
    assert b.is_cuda and tuple(b.shape) == (2, 7500) and np.array_equal(cpu(b[0]), E.time_stretch(y, 0.8).astype(np.float32))
    assert E.time_stretch(np.zeros(0), 1.5).shape == (0,) and A.add_noise(np.zeros(0), 3.0).shape == (0,)
    with pytest.raises(ValueError, match="Time stretch rate must be positive."):
        E.time_stretch_batch(b, 0.0)


def test_g5_cli_round_trip(tmp_path):
    from click.testing import CliRunner
    from scipy.io import wavfile
    from sygnals_amd.cli.main import cli
    sr = 8000
    y = np.round(V.tones_noise(6000) * 0.5 * 32767.0) / 32767.0                  # what a 16-bit file holds
    wavfile.write(str(tmp_path / "x.wav"), sr, np.round(y * 32767.0).astype(np.int16))
    np.savez(tmp_path / "x.npz", data=y, sr=np.array(sr))
    run = lambda *a: CliRunner().invoke(cli, ["augment", *map(str, a)])
    r = run("add-noise", tmp_path / "x.npz", "-o", tmp_path / "n.npz", "--snr", 10, "--seed", 3)
    assert r.exit_code == 0, r.output
    stored = np.load(tmp_path / "x.npz")["data"]
    parity(np.load(tmp_path / "n.npz")["data"], V.add_noise(stored.astype(np.float32).astype(np.float64), 10.0, 3), "cli add-noise")
    r = run("add-noise", tmp_path / "x.wav", "-o", tmp_path / "n.wav", "--snr", 20, "--noise-type", "WHITE", "--seed", 1)
    assert r.exit_code == 0, r.output
    sr2, n = wavfile.read(str(tmp_path / "n.wav"))
    assert sr2 == sr and n.shape == (6000,)
    x16 = wavfile.read(str(tmp_path / "x.wav"))[1] / 32768.0
    assert abs(snr_of(x16, n / 32767.0 * 1.0) - 20.0) < 0.5                      # 16-bit rounding and the two scale factors
    r = run("time-stretch", tmp_path / "x.wav", "-o", tmp_path / "s.wav", "--rate", 1.25)
    assert r.exit_code == 0, r.output
    sr3, s = wavfile.read(str(tmp_path / "s.wav"))
    assert sr3 == sr and s.shape == (4800,)
    want = E.time_stretch(x16, 1.25)
    assert np.max(np.abs(s / 32767.0 - want)) <= 1.0 / 32767.0
    r = run("time-stretch", tmp_path / "x.npz", "-o", tmp_path / "s.npz", "--rate", 0.5)
    assert r.exit_code == 0, r.output
    assert np.load(tmp_path / "s.npz")["data"].shape == (12000,)
    assert run("time-stretch", tmp_path / "x.npz", "-o", tmp_path / "z.npz", "--rate", 0).exit_code == 2
