"""The free-running form of syg_stft2048_mfcc_tri_f32 whose waves never meet (stft_meet = 0: a clip is handed to its dB + DCT
epilogue, and its LDS matrix back, by counters in LDS) against the barrier-per-clip form (stft_meet = 1), the staged form
(stft_freerun = 0) and the oracle.  Same samples, window, transform, sums in the same order and a maximum: the three forms
are held to the same bits.  A hand-over that went wrong shows as NaN (the bounded waits) or as different bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import cpu_ref as O
from tests.gpu_util import assert_parity

TOL = 1e-5  # fp32 parity tolerance of tests/test_gpu_stft_freerun.py (BASELINE.json north_star)


@pytest.fixture(scope="module")
def ops():
    from sygnals_amd import ops
    ops.require_gpu()
    return ops


def all_forms(ops, y, sr, **kw):
    with ops.override(stft_freerun=1, stft_meet=0):
        new, _ = ops.stft2048_mfcc(y, sr, projection="segments", **kw)
        again, _ = ops.stft2048_mfcc(y, sr, projection="segments", **kw)
    with ops.override(stft_freerun=1, stft_meet=1):
        barrier, _ = ops.stft2048_mfcc(y, sr, projection="segments", **kw)
    with ops.override(stft_freerun=0, stft_meet=0):
        staged, _ = ops.stft2048_mfcc(y, sr, projection="segments", **kw)
    return new, again, barrier, staged


def check_forms(new, again, barrier, staged):
    assert not torch.isnan(new).any(), "a bounded wait of the hand-over ran out (or a NaN was computed)"
    assert torch.isfinite(new).all()
    assert torch.equal(new, barrier), "no-barrier and barrier-per-clip form: the same bits"
    assert torch.equal(new, staged), "no-barrier and staged form: the same bits"
    assert torch.equal(new, again), "repeated launches of the no-barrier form give the same bits"


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# T = 94: six tiles, two idle waves, deferred epilogue | T = 32: no idle wave, epilogue on the first waves, more clips than
# CUs | T = 6: one-tile clips, a hand-over every tile; B = 4 CUs + 1: every workgroup has >= 4 clips (both matrices reused
# twice) and one has one more | T = 17: fifteen idle waves in the second tile | n_mfcc = 20: two rows of output tiles |
# B = 1, 3: fewer clips than workgroups, only the epilogue behind the loop
SHAPES = [(48000, 512, 40, 13, 48000, 8), (16000, 160, 40, 13, 5000, 300), (48000, 512, 40, 13, 3000, None),
          (48000, 512, 40, 13, 8192, 37), (22050, 512, 40, 20, 22050, 37), (48000, 256, 40, 13, 9000, 50),
          (48000, 512, 40, 13, 48000, 1), (48000, 512, 40, 13, 8192, 3)]


@pytest.mark.parametrize("sr,hop,n_mels,n_mfcc,L,B", SHAPES)
def test_nomeet_same_bits_as_barrier_and_staged_and_matches_oracle(ops, sr, hop, n_mels, n_mfcc, L, B):
    if B is None:
        B = 4 * cus() + 1
    assert ops.lib().syg_stft2048_mfcc_tri_freerun(hop, L, L, None) == 1
    Y = O.synth_clips(B, L, sr, seed=5)
    if B > 1:
        Y[B // 2] = 0.0
    y = ops.to_device_f32(Y)
    new, again, barrier, staged = all_forms(ops, y, sr, hop=hop, n_mels=n_mels, n_mfcc=n_mfcc)
    assert new.shape == (B, n_mfcc, 1 + L // hop)
    check_forms(new, again, barrier, staged)
    idx = sorted(set([0, min(1, B - 1), B // 2, B - 1]))
    ref = np.stack([O.mfcc_manager(Y[i].astype(np.float64), sr, 2048, hop, True, "hann", n_mels, n_mfcc) for i in idx])
    assert_parity(new[idx].cpu().numpy(), ref, TOL, "no-barrier form vs oracle")


def test_nomeet_single_frame_without_centering(ops):
    B = 2 * cus() + 3
    Y = O.synth_clips(B, 2048, 16000, seed=8)
    Y[B // 2] = 0.0
    y = ops.to_device_f32(Y)
    new, again, barrier, staged = all_forms(ops, y, 16000, hop=512, center=False, n_mels=40)
    assert new.shape == (B, 13, 1)
    check_forms(new, again, barrier, staged)
    idx = sorted(set([0, 1, B // 2, B - 1]))
    ref = np.stack([O.mfcc_manager(Y[i].astype(np.float64), 16000, 2048, 512, False, "hann", 40, 13) for i in idx])
    assert_parity(new[idx].cpu().numpy(), ref, TOL, "no-barrier form, one frame, center=False")


@pytest.mark.parametrize("L,hop", [(6143, 511), (4001, 128)])
def test_nomeet_changes_nothing_where_the_freerunning_loads_do_not_apply(ops, L, hop):
    """Odd hop / odd length: the predicate says no, the launch runs the kernel it runs today with the option at any value."""
    assert ops.lib().syg_stft2048_mfcc_tri_freerun(hop, L, L, None) == 0
    Y = O.synth_clips(9, L, 16000, seed=8)
    Y[4] = 0.0
    y = ops.to_device_f32(Y)
    new, again, barrier, staged = all_forms(ops, y, 16000, hop=hop, n_mels=40)
    check_forms(new, again, barrier, staged)
    with ops.override(stft_meet=-1):
        default, _ = ops.stft2048_mfcc(y, 16000, projection="segments", hop=hop, n_mels=40)
    assert torch.equal(new, default)
    idx = [0, 1, 4, 8]
    ref = np.stack([O.mfcc_manager(Y[i].astype(np.float64), 16000, 2048, hop, True, "hann", 40, 13) for i in idx])
    assert_parity(new[idx].cpu().numpy(), ref, TOL, f"fallback L={L} hop={hop}")
