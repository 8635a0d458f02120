"""GPU checks of the FFT lane layout of the STFT(2048) kernels (lane-indexed exchanges, stft_mel.hip wave_rfft2048).

The transform's lanes own different columns, groups and bins than before the exchanges were made lane-indexed, so
every bin of the complex output is checked against the oracle, including the self-mirrored bins 0, 128, 256, 384 and
512 of lane 0, over odd lengths, hops up to 512 and both `center` settings.  The headline MFCC path (bench.py C2) is
also compared with the output of the library before that change (tests/golden/mfcc_c2_before_addtid.npz, made by that
library on bench.py's seeded clips): the transform's arithmetic is the same, only which lane does which part of it."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import cpu_ref as O
from tests.gpu_util import peak_rel

TOL = 1e-5
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "mfcc_c2_before_addtid.npz")


@pytest.fixture(scope="module")
def ops():
    from sygnals_amd import ops
    ops.require_gpu()
    return ops


@pytest.mark.parametrize("L,hop,center", [(2049, 512, True), (2049, 512, False), (4097, 511, True),
                                          (12345, 333, False), (9999, 1, True), (48001, 480, True),
                                          (20001, 512, False), (3001, 7, False)])
def test_complex_stft_every_bin(ops, L, hop, center):
    rng = np.random.default_rng(L * 7 + hop)
    Y = rng.normal(0, 0.3, (3, L)).astype(np.float32)
    Y[1, ::97] += 2.0                                    # impulse train: energy in every bin, lane 0's included
    X = ops.stft2048_c2c(ops.to_device_f32(Y), hop=hop, center=center).cpu().numpy()
    X = X[..., 0] + 1j * X[..., 1]
    for i in range(Y.shape[0]):
        ref = O.stft(Y[i].astype(np.float64), 2048, hop, center=center).T
        assert X[i].shape == ref.shape and np.isfinite(X[i]).all()
        assert peak_rel(X[i], ref) <= TOL, (L, hop, center, i)
        # the self-mirrored bins of lane 0, each against its own column's peak
        for k in (0, 128, 256, 384, 512, 640, 768, 896, 1024):
            col = ref[:, k]
            assert np.max(np.abs(X[i][:, k] - col)) <= TOL * max(np.max(np.abs(ref)), 1e-30), (L, hop, center, i, k)


def test_mfcc_c2_unchanged_from_before_the_lane_indexed_exchange(ops):
    g = np.load(GOLDEN)
    gold, idx = g["mfcc"], g["clip_index"].astype(np.int64)
    from sygnals_amd.synth import synth_clips
    base = synth_clips(64, 48000, 48000, seed=20250523)           # bench.py's C2 clips (rank 0), tiled to 1024
    y = ops.to_device_f32(np.tile(base, (1024 // 64 + 1, 1))[:1024])
    out = ops.mfcc_batch(y, 48000, 2048, 512, 40, 13, fused=None).cpu().numpy()
    assert out.shape == (1024, 13, 94)
    got = out[idx]
    assert got.shape == gold.shape
    # fp32 rounding: each coefficient within 1e-6 of its clip's peak |coefficient| (measured: 1.1e-7; the transform's
    # lanes now sum in a different order, so coefficients that are themselves near zero are not compared relatively)
    peak = np.max(np.abs(gold), axis=(1, 2), keepdims=True)
    err = np.abs(got.astype(np.float64) - gold)
    assert np.all(err <= 1e-6 * peak), float(np.max(err / peak))
    # the tiled copies of a clip (other workgroups, other positions in their chunk) agree with it bit for bit
    assert np.array_equal(out[np.arange(64)], out[np.arange(64) + 64 * 15])
