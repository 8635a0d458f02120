"""The Kaldi front end's entries of the C ABI are declared, bound and exported, their constants hold together, and every
refusal fires before device work: at the C ABI, in ops, in the mirrors (core/features/kaldi.py); the plugin registers both
names."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_kaldi_constants", "syg_kaldi_fbank_f32"]


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.fixture()
def p():
    buf = (C.c_float * 65536)()                     # never dereferenced: every call is refused
    return C.cast(buf, C.c_void_p)


def test_symbols_declared_bound_exported(h):
    from sygnals_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(raw, name)
    assert h.syg_abi_version() == 1


def test_constants(h):
    from sygnals_amd import _kaldi as KD, ops
    k = ops.kaldi_constants()
    assert k["tile"] == 16 and (k["n_fft_min"], k["n_fft_max"]) == (KD.N_SERVED[0], KD.N_SERVED[-1]) == (256, 2048)
    assert (k["mel_min"], k["mel_max"]) == (KD.MEL_MIN, KD.MEL_MAX) == (3, 256)
    assert k["lds_worst"] <= k["lds_max"] <= 160 * 1024 and k["wgs_per_cu"] >= 1
    assert h.syg_kaldi_constants(8) == -1 and h.syg_kaldi_constants(-1) == -1


def test_entry_refuses_before_device_work(h, p):
    f, err = h.syg_kaldi_fbank_f32, h.syg_last_error

    def call(y=p, B=2, L=1000, ldy=1000, wl=400, hop=160, n_fft=512, snip=1, T=4, win=p, tw=p, bp=p, M=23, pre=0.97, dc=1, raw=1,
             power=1, log=1, log_eps=-15.9424, floor=1.0, dither=0.0, seed=0, energy=0, htk=0, dct=None, nc=0, out=p, so=(92, 1, 4),
             fb=None, sf=(0, 0, 0)):
        return f(y, B, L, ldy, wl, hop, n_fft, snip, T, win, tw, bp, M, pre, dc, raw, power, log, log_eps, floor, dither, seed, energy,
                 htk, dct, nc, out, *so, fb, *sf, None)
    for kw in ({"y": None}, {"win": None}, {"tw": None}, {"bp": None}, {"out": None}):
        assert call(**kw) == -1 and b"null pointer" in err()
    for bad in (128, 4096, 500, 0):
        assert call(n_fft=bad) == -1 and b"n_fft = %d is not served (served: n_fft 256, 512, 1024 or 2048" % bad in err()
    for bad in (1, 513, -4):
        assert call(wl=bad) == -1 and b"wl = %d is not served at n_fft = 512" % bad in err()
    for bad in (0, -160):
        assert call(hop=bad) == -1 and b"hop = %d is not served" % bad in err()
    for bad in (2, 257, 0):
        assert call(M=bad) == -1 and b"num_mel_bins = %d is not served" % bad in err() and b"3 <= num_mel_bins <= 256" in err()
    for bad in (0, 24, -1):
        assert call(dct=p, nc=bad) == -1 and b"num_ceps = %d is not served at num_mel_bins = 23" % bad in err()
    assert call(fb=p, sf=(92, 1, 4)) == -1 and b"served for the MFCC only" in err()
    assert call(dct=p, nc=13, log=0, so=(52, 1, 4)) == -1 and b"taken from the log filterbank" in err()
    for kw in ({"B": 0}, {"L": 0}, {"ldy": 999}, {"B": 1 << 31}):
        assert call(**kw) == -1 and b"bad B / L / ldy" in err()
    for kw in ({"T": 3}, {"T": 5}, {"T": 0}, {"snip": 0, "T": 4}, {"L": 399, "T": 1}):
        assert call(**kw) == -1 and b"does not match the framing rule" in err()
    for bad in (-0.1, 1.5, float("nan")):
        assert call(pre=bad) == -1 and b"preemphasis_coefficient must be in [0, 1]" in err()
    for bad in (-1.0, float("inf"), float("nan")):
        assert call(dither=bad) == -1 and b"dither must be non-negative and finite" in err()
        assert call(floor=bad) == -1 and b"energy_floor must be non-negative and finite" in err()
    for bad in (0.0, 1.0, float("nan")):
        assert call(log_eps=bad) == -1 and b"log_eps must be the float32 nearest to log(eps)" in err()
    for bad in ((92, 1, 3), (92, 22, 1), (92, 2, 4), (91, 1, 4), (92, 0, 4)):
        assert call(so=bad) == -1 and b"bad output strides" in err()
    assert call(energy=1) == -1 and b"bad output strides" in err()               # C = 24 under use_energy
    assert call(dct=p, nc=13, so=(52, 1, 4), fb=p, sf=(92, 1, 3)) == -1 and b"bad filterbank strides" in err()
    assert call(bp=C.c_void_p(p.value + 4)) == -1 and b"16-byte aligned" in err()


def test_ops_refuse_without_a_device():
    from sygnals_amd import ops
    y = torch.zeros(2, 4000)
    for fn in (ops.kaldi_fbank, ops.kaldi_mfcc):
        who = fn.__name__
        with pytest.raises(ValueError, match=f"{who}: round_to_power_of_two=False is not served \\(served: a frame_length"):
            fn(y, round_to_power_of_two=False)
        with pytest.raises(ValueError, match=f"{who}: vtln_warp = 1.1 is not served"):
            fn(y, vtln_warp=1.1)
        for bad in (2, 257, 0):
            with pytest.raises(ValueError, match=f"{who}: num_mel_bins = {bad} is not served .*3 <= num_mel_bins <= 256"):
                fn(y, num_mel_bins=bad)
        with pytest.raises(ValueError, match=f"{who}: num_mel_bins must be an integer"):
            fn(y, num_mel_bins=23.0)
        for fl, sr in ((5.0, 16000.0), (25.0, 96000.0), (200.0, 16000.0), (0.0, 16000.0)):
            with pytest.raises(ValueError, match=f"{who}: frame_length = .* not served"):
                fn(y, sr, frame_length=fl)
        with pytest.raises(ValueError, match=f"{who}: frame_shift = 0.01 ms at 16000.0 Hz is below one sample"):
            fn(y, frame_shift=0.01)
        with pytest.raises(ValueError, match=f"{who}: window_type = 'hann' is not served"):
            fn(y, window_type="hann")
        with pytest.raises(ValueError, match=f"{who}: need 0 <= low_freq < high_freq <= sr / 2"):
            fn(y, low_freq=5000.0, high_freq=4000.0)
        with pytest.raises(ValueError, match=f"{who}: need 0 <= low_freq < high_freq"):
            fn(y, high_freq=9000.0)
        with pytest.raises(ValueError, match=f"{who}: preemphasis_coefficient must be in \\[0, 1\\]"):
            fn(y, preemphasis_coefficient=1.5)
        with pytest.raises(ValueError, match=f"{who}: dither, energy_floor and min_duration must be non-negative"):
            fn(y, dither=-1.0)
        with pytest.raises(ValueError, match=f"{who}: snip_edges must be True or False"):
            fn(y, snip_edges=1)
        with pytest.raises(ValueError, match=f"{who}: unknown arguments \\['n_mels'\\]"):
            fn(y, n_mels=40)
        with pytest.raises(ValueError, match=f"{who}: sample_frequency must be positive"):
            fn(y, 0.0)
        with pytest.raises(ValueError, match=f"{who}: layout must be 'ct'"):
            fn(y, layout="bt")
        for bad in (-1, 1.5, True, 1 << 64):
            with pytest.raises(ValueError, match=f"{who}: seed must be an integer in \\[0, 2\\^64\\)"):
                fn(y, seed=bad)
        for bad in (y.double(), y[0], y.numpy(), y[None]):
            with pytest.raises(ValueError, match=f"{who}: y must be a float32 tensor \\[B, L\\]"):
                fn(bad)
        with pytest.raises(ValueError, match=f"{who}: empty input"):
            fn(torch.zeros(0, 4000))
        with pytest.raises(ValueError, match=f"{who}: out must be a contiguous float32 tensor"):
            fn(y, out=torch.zeros(2, 5, 5))
    with pytest.raises(ValueError, match="kaldi_fbank: unknown arguments \\['num_ceps'\\]"):
        ops.kaldi_fbank(y, num_ceps=13)
    with pytest.raises(ValueError, match="kaldi_mfcc: unknown arguments \\['use_power'\\]"):
        ops.kaldi_mfcc(y, use_power=False)
    for bad in (0, 24):
        with pytest.raises(ValueError, match=f"kaldi_mfcc: num_ceps = {bad} is not served at num_mel_bins = 23"):
            ops.kaldi_mfcc(y, num_ceps=bad)
    with pytest.raises(ValueError, match="kaldi_mfcc: cepstral_lifter must be non-negative"):
        ops.kaldi_mfcc(y, cepstral_lifter=-1.0)


def test_mirrors_refuse_without_a_device():
    from sygnals_amd.core.features import kaldi as KF
    x = np.zeros(4000)
    for fn in (KF.fbank, KF.mfcc):
        who = fn.__name__
        with pytest.raises(ValueError, match=f"{who}: round_to_power_of_two=False is not served"):
            fn(x, round_to_power_of_two=False)
        with pytest.raises(ValueError, match=f"{who}: vtln_warp = 0.9 is not served"):
            fn(x, vtln_warp=0.9)
        with pytest.raises(ValueError, match=f"{who}: num_mel_bins = 300 is not served"):
            fn(x, num_mel_bins=300)
        with pytest.raises(ValueError, match=f"{who}: waveform must be real, \\[L\\] or \\[channels, L\\]"):
            fn(np.zeros((2, 3, 4)))
        with pytest.raises(ValueError, match=f"{who}: channel = 2 is outside the 2 channels"):
            fn(np.zeros((2, 4000)), channel=2)
        with pytest.raises(ValueError, match=f"{who}: frame_length = 25.0 ms at 4000.0 Hz is 100 samples, padded to 128: not served"):
            fn(x, sample_frequency=4000.0)
    for fn in (KF.fbank_batch, KF.mfcc_batch):
        who = fn.__name__
        with pytest.raises(ValueError, match=f"{who}: y must be real clips \\[B, L\\]"):
            fn(x)
        with pytest.raises(ValueError, match=f"{who}: window_type = 'sine' is not served"):
            fn(x[None], window_type="sine")
        with pytest.raises(ValueError, match=f"{who}: layout must be"):
            fn(x[None], layout="x")
    assert sorted(KF.__all__) == ["fbank", "fbank_batch", "mfcc", "mfcc_batch"]


def test_plugin_registers_both_names():
    from sygnals_amd.core.features import kaldi as KF
    from sygnals_amd.plugins import SygnalsAmdPlugin

    class Reg:
        def __init__(self):
            self.f = {}

        def add_feature(self, name, fn):
            self.f[name] = fn
    r = Reg()
    SygnalsAmdPlugin().register_feature_extractors(r)
    assert r.f["kaldi_fbank"] is KF.kaldi_fbank and r.f["kaldi_mfcc"] is KF.kaldi_mfcc and "mfcc" in r.f
