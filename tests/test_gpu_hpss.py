"""HPSS on the device (syg_hpss_masks_f32, syg_istft2048_f32, syg_hnr_rows_f32, harmonic_to_noise_ratio) against the
float64 restatement of tests/hpss_ref.py."""
import warnings

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from sygnals_amd import ops
from tests import hpss_ref as R
from tests.gpu_util import assert_parity

pytestmark = pytest.mark.gpu

F32_TINY = float(np.finfo(np.float32).tiny)


def _noise(L, seed=0, scale=0.3):
    return np.random.default_rng(seed).standard_normal(L) * scale


def _dev_D(y):
    """Device STFT of one clip -> (device D [1, T, 1025, 2], host complex64 [T, 1025])."""
    D = ops.stft2048_c2c(ops.to_device_f32(np.asarray(y)[None, :]))
    h = D[0].cpu().numpy()
    return D, h[..., 0] + 1j * h[..., 1]


def _mag32(Dh):
    """|D| exactly as the kernel computes it: sqrt_rn(re*re + im*im), every step float32 round-to-nearest."""
    re = Dh.real.astype(np.float32)
    im = Dh.imag.astype(np.float32)
    return np.sqrt(re * re + im * im, dtype=np.float32)


# ---------------------------------------------------------------- medians and masks
@pytest.mark.parametrize("win", [(31, 31), (1, 1), (17, 63), (30, 8), (12, 9)])
@pytest.mark.parametrize("T", [1, 2, 15, 16, 94])
def test_medians_exact(win, T):
    L = 512 * (T - 1) + 100
    D, Dh = _dev_D(_noise(L, seed=T))
    _, _, H, P = ops.hpss_masks(D, win, 2.0, 1.0, medians=True)
    S = _mag32(Dh)                                       # [T, 1025]
    Hr = R.median_filter_axis(S, win[0], axis=0)
    Pr = R.median_filter_axis(S, win[1], axis=1)
    assert np.array_equal(H[0].cpu().numpy(), Hr), f"H differs at {np.argwhere(H[0].cpu().numpy() != Hr)[:5]}"
    assert np.array_equal(P[0].cpu().numpy(), Pr), f"P differs at {np.argwhere(P[0].cpu().numpy() != Pr)[:5]}"


@pytest.mark.parametrize("power", [1.0, 2.0, np.inf])
@pytest.mark.parametrize("margin", [(1.0, 1.0), (2.0, 3.0)])
def test_masks_match_softmask(power, margin):
    # 16 000 zeros give 27 all-zero frames: in the middle of the run more than half of every 31-frame time window is
    # zero, so H = P = 0 there and the split_zeros rule decides the mask
    y = np.concatenate([R.sine(22050)[:11025], np.zeros(16000), _noise(8000, 4)])
    D, _ = _dev_D(y)
    Mh, Mp, H, P = ops.hpss_masks(D, 31, power, margin, medians=True)
    H = H[0].cpu().numpy()
    P = P[0].cpu().numpy()
    Mh = Mh[0].cpu().numpy()
    Mp = Mp[0].cpu().numpy()
    split = margin == (1.0, 1.0)
    rh = R.softmask(H, P.astype(np.float64) * margin[0], power, split, tiny=F32_TINY)
    rp = R.softmask(P, H.astype(np.float64) * margin[1], power, split, tiny=F32_TINY)
    assert np.abs(Mh - rh).max() <= 1e-6
    assert np.abs(Mp - rp).max() <= 1e-6
    bad = np.maximum(H, P) < F32_TINY
    assert bad.sum() >= 5 * 1025, "the input must reach the split_zeros rule"
    want = 0.5 if split and np.isfinite(power) else 0.0          # the hard mask never splits
    assert (Mh[bad] == want).all() and (Mp[bad] == want).all()


# ---------------------------------------------------------------- inverse STFT
@pytest.mark.parametrize("L", [1, 511, 512, 1023, 1535, 7679, 7680, 48001])
def test_istft_masked_and_round_trip(L):
    y = _noise(L, seed=L)
    D, Dh = _dev_D(y)
    Mh, Mp = ops.hpss_masks(D)
    yh, yp = ops.istft2048(D, 512, L, mask=(Mh, Mp))
    D64 = Dh.T.astype(np.complex128)
    assert_parity(yh[0].cpu().numpy(), R.istft(Mh[0].cpu().numpy().T.astype(np.float64) * D64, L), what="y_h")
    assert_parity(yp[0].cpu().numpy(), R.istft(Mp[0].cpu().numpy().T.astype(np.float64) * D64, L), what="y_p")
    plain = ops.istft2048(D, 512, L)
    assert_parity(plain[0].cpu().numpy(), R.istft(D64, L), what="istft")
    assert_parity(plain[0].cpu().numpy(), y, what="round trip")
    one = ops.istft2048(D, 512, L, mask=Mh)
    assert torch.equal(one, yh)                          # one component or two: same bits
    s1, s2 = ops.istft2048(D, 512, L, mask=(Mh, Mp), ldy=L + 37)
    assert s1.stride(0) == L + 37 and torch.equal(s1, yh) and torch.equal(s2, yp)


def test_istft_window_one_halves():
    y = _noise(7680, seed=9)
    D, _ = _dev_D(y)
    Mh, Mp = ops.hpss_masks(D, (1, 1))
    assert (Mh == 0.5).all() and (Mp == 0.5).all()
    yh, yp = ops.istft2048(D, 512, len(y), mask=(Mh, Mp))
    assert torch.equal(yh, yp)
    assert torch.equal(yh, 0.5 * ops.istft2048(D, 512, len(y)))
    assert_parity(yh[0].cpu().numpy(), y / 2, what="y/2")


# ---------------------------------------------------------------- end to end from y
def _burst():
    y = _noise(22050, 11, 1e-3)
    t = np.arange(4000) / 22050
    y[9000:13000] += 0.8 * np.sin(2 * np.pi * 660 * t) * np.hanning(4000)
    return y


CASES = {
    "sine": lambda: R.sine(),
    "clicks": lambda: R.clicks(),
    "noise": lambda: _noise(22050, 5),
    "silence": lambda: np.zeros(22050),
    "burst": _burst,
    "synth0": lambda: O.synth_clips(2, 48000, 48000, seed=21)[0].astype(np.float64),
    "synth1": lambda: O.synth_clips(2, 48000, 48000, seed=21)[1].astype(np.float64),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_hpss_end_to_end(name):
    y = CASES[name]()
    yh, yp = ops.hpss(ops.to_device_f32(y[None, :]))
    rh, rp = R.hpss(y)
    pk = max(np.abs(y).max(), 1e-30)
    for dev, ref in ((yh, rh), (yp, rp)):
        err = np.abs(dev[0].cpu().numpy().astype(np.float64) - ref)
        assert err.max() <= 1e-5 * pk, f"{name}: {err.max() / pk:.2e} of the peak"


@pytest.mark.parametrize("name", ["sine", "clicks", "noise", "silence", "burst", "synth0"])
@pytest.mark.parametrize("fl,hop", [(2048, 512), (1024, 256)])
def test_hnr_rows(name, fl, hop):
    from sygnals_amd.core.audio.features import harmonic_to_noise_ratio_batch
    y = CASES[name]()
    dev = harmonic_to_noise_ratio_batch(y[None, :], 22050, fl, hop)[0].cpu().numpy().astype(np.float64)
    rh, rp = R.hpss(y)
    ref, ph, pp = R.hnr_from_components(rh, rp, fl, hop)
    assert dev.shape == ref.shape == (1 + len(y) // hop,)
    near = (np.abs(ph / R.EPSILON - 1) < 0.01) | (np.abs(pp / R.EPSILON - 1) < 0.01)
    cls = lambda v: np.where(np.isnan(v), 0, np.where(v == 80, 1, np.where(v == -80, 2, 3)))  # noqa: E731
    assert np.array_equal(cls(dev)[~near], cls(ref)[~near]), name
    big = max(ph.max(), pp.max())
    sure = (ph > 1e-6 * big) & (pp > 1e-6 * big) & (ph > R.EPSILON) & (pp > R.EPSILON)
    if sure.any():
        assert np.abs(dev[sure] - ref[sure]).max() <= 0.01, name
    if name == "silence":
        assert np.isnan(dev).all()


# ---------------------------------------------------------------- batch, determinism, mirror
def test_batch_rows_equal_single_calls_and_repeat():
    from sygnals_amd.core.audio.features import harmonic_to_noise_ratio_batch
    Y = ops.to_device_f32(O.synth_clips(1024, 48000, 48000, seed=5))
    a = harmonic_to_noise_ratio_batch(Y, 48000)
    b = harmonic_to_noise_ratio_batch(Y, 48000)
    assert a.shape == (1024, 94) and a.dtype == torch.float32 and a.is_cuda
    assert torch.equal(torch.nan_to_num(a, nan=-1234.0), torch.nan_to_num(b, nan=-1234.0))
    c = harmonic_to_noise_ratio_batch(Y[:4].cpu(), 48000)       # a host tensor is moved to the device
    assert c.is_cuda and torch.equal(torch.nan_to_num(c, nan=-1234.0), torch.nan_to_num(a[:4], nan=-1234.0))
    yh, yp = ops.hpss(Y)
    yh2, yp2 = ops.hpss(Y)
    assert torch.equal(yh, yh2) and torch.equal(yp, yp2)
    for r in (0, 511, 1023):
        s = harmonic_to_noise_ratio_batch(Y[r:r + 1], 48000)
        assert torch.equal(torch.nan_to_num(s[0], nan=-1234.0), torch.nan_to_num(a[r], nan=-1234.0))
        sh, sp = ops.hpss(Y[r:r + 1])
        assert torch.equal(sh[0], yh[r]) and torch.equal(sp[0], yp[r])


def test_mirror_contract():
    from sygnals_amd.core.audio.features import harmonic_to_noise_ratio
    y = R.sine()
    with pytest.warns(UserWarning, match="approximation based on HPSS"):
        out = harmonic_to_noise_ratio(y, 22050, frame_length=1024, hop_length=256)
    ref = R.harmonic_to_noise_ratio(y, 1024, 256)
    assert out.dtype == np.float64 and out.shape == ref.shape == (87,)
    assert np.nanmean(out) > 10.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.nanmean(harmonic_to_noise_ratio(R.clicks(), 22050, 1024, 256)) < 5.0
        with pytest.raises(ValueError):
            harmonic_to_noise_ratio(np.zeros((2, 100)), 22050)
        with pytest.raises(TypeError):
            harmonic_to_noise_ratio(y, 22050, pad_mode="reflect")
        bad = harmonic_to_noise_ratio(y, 22050, frame_length=1024, hop_length=256, harmonic_margin=0.5)
        assert bad.shape == (87,) and np.isnan(bad).all()
        empty = harmonic_to_noise_ratio(np.zeros(0), 22050)
        assert empty.shape == (1,) and np.isnan(empty).all()
        p1 = harmonic_to_noise_ratio(y, 22050, power=1.0, n_fft=2048, window="hann", center=True, win_length=2048)
        assert p1.shape == (1 + len(y) // 512,)
        np.testing.assert_allclose(p1, R.harmonic_to_noise_ratio(y, 2048, 512, power=1.0), atol=0.01)
    with pytest.raises(ValueError):
        ops.hpss_masks(ops.stft2048_c2c(ops.to_device_f32(y[None, :])), 31, 2.0, (1.0, 0.9))
