"""The Kaldi front end on the device (csrc/kaldi_front.hip) against tests/kaldi_ref.py.  The cases, their inputs and the
gates are in tests/kaldi_cases.py; tests/test_kaldi_ref.py asserts every gated case's condition on the CPU.

Worst figures measured on MI355X are in README.md beside their gates.  The end-to-end MFCC deviation from the restatement is
measured (printed), not gated: weak-band log errors pass through the DCT."""
import numpy as np
import pytest
import torch

from sygnals_amd import _kaldi as KD
from sygnals_amd import ops
from tests import kaldi_cases as KC
from tests import kaldi_ref as KR

pytestmark = pytest.mark.gpu

CASES = KC.cases()
LOG_EPS_BITS = np.float32(KD.LOG_EPS).view(np.int32)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(ops.require_gpu())


def btc(t, layout):
    """[B, T, C] float32 NumPy of a result in either layout."""
    a = t.cpu().numpy()
    return a.transpose(0, 2, 1) if layout == "ct" else a


def check_gates(who, f_mel, E, use_log=True):
    e_err, l_err, n_dom = KC.gates(f_mel, E, use_log)
    print(f"{who}: energy error / frame peak {e_err:.3e} (gate {KC.ENERGY_TOL:g}), log error on dominant cells {l_err:.3e} "
          f"(gate {KC.LOG_TOL:g}), dominant cells of the poorest frame {n_dom}")
    assert n_dom >= 1
    assert e_err <= KC.ENERGY_TOL
    assert l_err <= KC.LOG_TOL
    return e_err, l_err


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_cases(c):
    x = KC.case_input(c)
    E, e, f_ref = KC.reference(c, x)
    if c["strided"]:
        buf = torch.zeros((c["B"], c["L"] + 37), dtype=torch.float32, device=ops.require_gpu())
        buf[:, :c["L"]] = dev(x)
        y = buf[:, :c["L"]]
        assert not y.is_contiguous()
    else:
        y = dev(x)
    f = btc(ops.kaldi_fbank(y, c["sr"], layout=c["layout"], **c["kw"]), c["layout"])
    assert f.shape == f_ref.shape and np.isfinite(f).all()
    check_gates(c["id"], f[..., KC.mel_columns(c)], E, c["kw"].get("use_log_fbank", True))
    if c["kw"].get("use_energy", False):
        col = -1 if c["kw"].get("htk_compat", False) else 0
        ref = f_ref[..., col]
        err = float(np.max(np.abs(f[..., col] - ref) / np.maximum(1.0, np.abs(ref))))
        print(f"{c['id']}: energy column error {err:.3e} (gate 1e-5 max(1, |ref|))")
        assert err <= 1e-5


def test_past_the_grid_cap():
    """65 537 one-frame clips: more tiles than the capped grid has workgroups, and than a grid dimension has rows."""
    base = KC.signal("noise", 7, 200, 1.0, 8000.0, 11)
    idx = torch.arange(65537, device=ops.require_gpu()) % 7
    y = dev(base)[idx].contiguous()
    f = ops.kaldi_fbank(y, 8000.0)
    assert f.shape == (65537, 23, 1)
    assert torch.equal(f, f[:7][idx])                                    # a batch equals its rows, bit for bit
    c = dict(sr=8000.0, kw={})
    E, _, _ = KC.reference(c, base)
    check_gates("65537 clips", btc(f[:7], "ct"), E)


@pytest.mark.parametrize("M", [23, 80])
def test_each_band_as_the_peak(M):
    """The energy gate is blind to weak bands: a cosine at each band's centre makes that band the frame's peak."""
    sr, L = 16000.0, 560
    fc = KC.band_centres(M, sr)
    n = np.arange(L, dtype=np.float64)
    x = np.cos(2 * np.pi * fc[:, None] * n[None, :] / sr).astype(np.float32)
    f = btc(ops.kaldi_fbank(dev(x), sr, num_mel_bins=M), "ct")
    E = np.stack([KR.mel_energies(r.astype(np.float64), sr, num_mel_bins=M)[0] for r in x])
    check_gates(f"band centres M={M}", f, E)
    m = np.arange(M)
    own = np.abs(f[m, :, m].astype(np.float64) - np.log(np.maximum(E[m, :, m], KD.EPS)))
    assert np.all(E[m, :, m] >= KC.DOMINANT * E.max(axis=-1)[m]) and own.max() <= KC.LOG_TOL
    print(f"band centres M={M}: worst log error of a band in its own turn {own.max():.3e}")


@pytest.mark.parametrize("M", [23, 80])
def test_impulse_frames(M):
    """Rectangular window, no DC removal, no pre-emphasis: an impulse frame has E[m] = sum_k basis[m, k]."""
    x = np.zeros((4, 400), dtype=np.float32)
    for b, p in enumerate((0, 7, 200, 399)):
        x[b, p] = 1.0
    kw = dict(num_mel_bins=M, window_type="rectangular", remove_dc_offset=False, preemphasis_coefficient=0.0)
    f = btc(ops.kaldi_fbank(dev(x), 16000.0, **kw), "ct")
    E = np.broadcast_to(KR.mel_banks(M, 512, 16000.0).sum(axis=1), (4, 1, M))
    check_gates(f"impulse frames M={M}", f, E)


def test_exact_floor():
    for x, kw in ((np.zeros((2, 1000)), {}), (np.full((2, 1000), 0.5), {}), (np.zeros((1, 1200)), dict(snip_edges=False))):
        for layout in KD.LAYOUTS:
            f = ops.kaldi_fbank(dev(x), 16000.0, layout=layout, **kw).cpu().numpy()
            assert f.size and np.all(f.view(np.int32) == LOG_EPS_BITS)
    assert np.float32(KD.LOG_EPS) == np.float32(np.log(np.float64(KD.EPS)))


@pytest.mark.parametrize("mfcc", [False, True])
def test_bits_batch_rows_and_layouts(mfcc):
    fn = ops.kaldi_mfcc if mfcc else ops.kaldi_fbank
    y = dev(KC.signal("noise", 5, 3000, 1.0, 16000.0, 21))
    kw = dict(use_energy=True, snip_edges=False)
    a = fn(y, 16000.0, **kw)
    assert torch.equal(a, fn(y, 16000.0, **kw))                          # the same call twice
    for i in range(5):
        assert torch.equal(a[i:i + 1], fn(y[i:i + 1], 16000.0, **kw))    # a batch equals its rows
    t = fn(y, 16000.0, layout="tc", **kw)
    assert t.shape == (5, a.shape[2], a.shape[1]) and torch.equal(t, a.transpose(1, 2))
    out = torch.empty_like(a)
    assert fn(y, 16000.0, out=out, **kw) is out and torch.equal(out, a)


@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("floor,amp,active", [(0.0, 1.0, False), (1.0, 1.0, False), (1.0, 1e-3, True), (0.0, 1e-3, False)])
def test_energy_column(raw, floor, amp, active):
    x = KC.signal("noise", 2, 1200, amp, 16000.0, 31)
    kw = dict(use_energy=True, raw_energy=raw, energy_floor=floor)
    f = btc(ops.kaldi_fbank(dev(x), 16000.0, **kw), "ct")
    ref = np.stack([KR.fbank(r.astype(np.float64), 16000.0, **kw) for r in x])
    free = np.stack([KR.fbank(r.astype(np.float64), 16000.0, **dict(kw, energy_floor=0.0)) for r in x])
    assert bool(np.all(ref[..., 0] == 0.0) and np.all(free[..., 0] < 0.0)) == active
    err = float(np.max(np.abs(f[..., 0] - ref[..., 0]) / np.maximum(1.0, np.abs(ref[..., 0]))))
    print(f"energy column raw={raw} floor={floor} amp={amp}: error {err:.3e} (gate 1e-5 max(1, |ref|))")
    assert err <= 1e-5
    c = btc(ops.kaldi_mfcc(dev(x), 16000.0, **kw), "ct")
    assert np.array_equal(c[..., 0], f[..., 0])                          # the MFCC's coefficient 0 is the same log-energy


@pytest.mark.parametrize("M,nc,Q,extra", [(23, 13, 22.0, {}), (80, 40, 0.0, {}), (128, 13, 22.0, dict(htk_compat=True)),
                                         (256, 256, 22.0, {}), (23, 13, 22.0, dict(use_energy=True, energy_floor=0.0)),
                                         (40, 20, 10.0, dict(use_energy=True, htk_compat=True, snip_edges=False))])
@pytest.mark.parametrize("layout", KD.LAYOUTS)
def test_mfcc_against_own_fbank(M, nc, Q, extra, layout):
    """The cepstra against the float64 DCT + lifter of the device's own log filterbank from the same launch."""
    x = KC.signal("tone", 3, 16000 // 4, 1.0, 16000.0, 41, freq=1000.0)
    kw = dict(num_mel_bins=M, num_ceps=nc, cepstral_lifter=Q, **extra)
    c, fb = ops.kaldi_mfcc(dev(x), 16000.0, layout=layout, return_fbank=True, **kw)
    c, fb = btc(c, layout), btc(fb, layout)
    assert c.shape[2] == nc and fb.shape[2] == M and c.shape[1] == fb.shape[1] >= 17
    fkw = {k: v for k, v in kw.items() if k in ("num_mel_bins", "snip_edges")}
    assert np.array_equal(fb, btc(ops.kaldi_fbank(dev(x), 16000.0, **fkw), "ct"))        # the filterbank of the fbank call
    own = KR.cepstra(fb.astype(np.float64), nc, Q)
    cols = KD.cep_columns(nc, extra.get("htk_compat", False))
    keep = np.arange(nc) >= int(extra.get("use_energy", False))          # coefficient 0 is the log-energy under use_energy
    scale = np.max(np.abs(own), axis=-1, keepdims=True)
    err = float(np.max(np.abs(c[..., cols[keep]] - own[..., keep]) / scale))
    ref = np.stack([KR.mfcc(r.astype(np.float64), 16000.0, **kw) for r in x])
    e2e = float(np.max(np.abs(c - ref) / np.max(np.abs(ref), axis=-1, keepdims=True)))
    print(f"mfcc M={M} nc={nc} Q={Q} {extra} {layout}: against own fbank {err:.3e} (gate 1e-5 max|c|); "
          f"end to end against the restatement {e2e:.3e} of max|c| (measured, not gated)")
    assert err <= 1e-5 and np.isfinite(c).all()
    if extra.get("use_energy", False):
        e_ref = ref[..., cols[0]]
        assert np.max(np.abs(c[..., cols[0]] - e_ref) / np.maximum(1.0, np.abs(e_ref))) <= 1e-5


@pytest.mark.parametrize("mfcc", [False, True])
def test_subtract_mean(mfcc):
    fn = ops.kaldi_mfcc if mfcc else ops.kaldi_fbank
    y = dev(KC.signal("brown", 3, 16000, 1.0, 16000.0, 51))
    plain = fn(y, 16000.0)
    sub = fn(y, 16000.0, subtract_mean=True)
    assert plain.shape[2] == 98 and torch.equal(sub, ops.cmvn(plain, variance=False))
    means = sub.double().mean(dim=2).abs().max().item()
    print(f"subtract_mean mfcc={mfcc}: worst column mean {means:.3e}, gate {1e-6 * plain.abs().max().item():.3e}")
    assert means <= 1e-6 * plain.abs().max().item()
    assert torch.equal(fn(y, 16000.0, subtract_mean=True, layout="tc"), sub.transpose(1, 2))


def test_dither():
    L = 400 + 97 * 160
    y = torch.zeros((1, L), dtype=torch.float32, device=ops.require_gpu())
    sigma = 0.5
    kw = dict(remove_dc_offset=False, use_energy=True, raw_energy=True, energy_floor=0.0, dither=sigma)
    a = ops.kaldi_fbank(y, 16000.0, seed=7, **kw)
    assert a.shape == (1, 24, 98) and torch.isfinite(a).all()
    assert torch.equal(a, ops.kaldi_fbank(y, 16000.0, seed=7, **kw))
    assert not torch.equal(a, ops.kaldi_fbank(y, 16000.0, seed=8, **kw))
    ratio = float(torch.exp(a[0, 0].double()).mean().item() / (sigma * sigma * 400))
    bound = 6.0 * np.sqrt(2.0 / (400 * 98))
    print(f"dither: mean of sum x^2 / (sigma^2 wl) over 98 frames = {ratio:.5f} (within {bound:.4f} of 1)")
    assert abs(ratio - 1.0) <= bound
    x = dev(KC.signal("noise", 2, 2000, 1.0, 16000.0, 61))
    assert torch.equal(ops.kaldi_fbank(x, 16000.0, dither=0.0, seed=5), ops.kaldi_fbank(x, 16000.0))
    two = torch.zeros((2, L), dtype=torch.float32, device=y.device)
    b = ops.kaldi_fbank(two, 16000.0, seed=7, **kw)
    assert torch.equal(b[0], a[0]) and not torch.equal(b[1], b[0])       # keyed by the clip: rows draw different noise


def test_empty_results():
    y = torch.zeros((2, 399), dtype=torch.float32, device=ops.require_gpu())
    assert ops.kaldi_fbank(y, 16000.0).shape == (2, 23, 0) and ops.kaldi_fbank(y, 16000.0, layout="tc").shape == (2, 0, 23)
    assert ops.kaldi_mfcc(y[:, :79], 16000.0, snip_edges=False).shape == (2, 13, 0)
    c, fb = ops.kaldi_mfcc(y, 16000.0, return_fbank=True, min_duration=1.0)
    assert c.shape == (2, 13, 0) and fb.shape == (2, 23, 0)


def test_mirrors():
    from sygnals_amd.core.features import kaldi as KF
    x = KC.signal("noise", 2, 4000, 1.0, 16000.0, 71)
    f = KF.fbank(x, channel=1, num_mel_bins=40)
    assert f.shape == (23, 40) and f.dtype == np.float32
    assert np.array_equal(f, btc(ops.kaldi_fbank(dev(x[1:2]), 16000.0, num_mel_bins=40), "ct")[0])
    assert np.array_equal(KF.fbank(x[0]), KF.fbank(x, channel=-1))
    c = KF.mfcc(x[0], sample_frequency=16000.0)
    assert c.shape == (23, 13) and np.array_equal(c, KF.mfcc_batch(x[:1]).cpu().numpy()[0])
    assert KF.fbank_batch(dev(x), layout="ct").shape == (2, 23, 23)
