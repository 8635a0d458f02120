"""The free-running form of syg_stft2048_mfcc_tri_f32 (stft_freerun = 1: every wave loads its next frame from global memory
under its projection, one workgroup barrier per clip) against the staged form (stft_freerun = 0) and the oracle.  Same
samples, window, transform, sums in the same order and a maximum: the two forms are held to the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import cpu_ref as O
from tests.gpu_util import assert_parity

TOL = 1e-5  # fp32 parity tolerance stated by BASELINE.json north_star


@pytest.fixture(scope="module")
def ops():
    from sygnals_amd import ops
    ops.require_gpu()
    return ops


def both_forms(ops, y, sr, **kw):
    with ops.override(stft_freerun=1):
        new, _ = ops.stft2048_mfcc(y, sr, projection="segments", **kw)
        again, _ = ops.stft2048_mfcc(y, sr, projection="segments", **kw)
    with ops.override(stft_freerun=0):
        staged, _ = ops.stft2048_mfcc(y, sr, projection="segments", **kw)
    return new, again, staged


# T = 94: six tiles, two idle waves, deferred epilogue | T = 32: no idle wave (epilogue on the first waves behind the barrier),
# more clips than CUs (both matrices alternate) | T = 6: one-tile clips, every frame touches the padding, a barrier and a matrix
# swap every tile, every prefetch crosses a clip boundary (B = 2 CUs + 3) | T = 17: fifteen idle waves in the second tile
@pytest.mark.parametrize("sr,hop,n_mels,n_mfcc,L,B", [(48000, 512, 40, 13, 48000, 8), (16000, 160, 40, 13, 5000, 300),
                                                       (48000, 512, 40, 13, 3000, None), (48000, 512, 40, 13, 8192, 37),
                                                       (48000, 256, 32, 13, 9000, 50), (22050, 512, 40, 20, 22050, 37)])
def test_freerun_is_bit_identical_to_staged_and_matches_oracle(ops, sr, hop, n_mels, n_mfcc, L, B):
    if B is None:
        B = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    assert ops.lib().syg_stft2048_mfcc_tri_freerun(hop, L, L, None) == 1
    Y = O.synth_clips(B, L, sr, seed=5)
    Y[B // 2] = 0.0
    y = ops.to_device_f32(Y)
    new, again, staged = both_forms(ops, y, sr, hop=hop, n_mels=n_mels, n_mfcc=n_mfcc)
    assert new.shape == staged.shape == (B, n_mfcc, 1 + L // hop)
    idx = sorted(set([0, 1, B // 2, B - 1]))
    ref = np.stack([O.mfcc_manager(Y[i].astype(np.float64), sr, 2048, hop, True, "hann", n_mels, n_mfcc) for i in idx])
    assert_parity(new[idx].cpu().numpy(), ref, TOL, "free-running form vs oracle")
    assert torch.equal(new, staged), "free-running and staged form: the same bits"
    assert torch.equal(new, again), "repeated launches of the free-running form give the same bits"


def test_freerun_single_frame_without_centering(ops):
    Y = O.synth_clips(9, 2048, 16000, seed=8)
    y = ops.to_device_f32(Y)
    new, again, staged = both_forms(ops, y, 16000, hop=512, center=False, n_mels=40)
    ref = np.stack([O.mfcc_manager(c.astype(np.float64), 16000, 2048, 512, False, "hann", 40, 13) for c in Y])
    assert new.shape == ref.shape == (9, 13, 1)
    assert_parity(new.cpu().numpy(), ref, TOL, "free-running form, one frame, center=False")
    assert torch.equal(new, staged) and torch.equal(new, again)


@pytest.mark.parametrize("L,hop", [(6143, 511), (4001, 128)])
def test_freerun_falls_back_where_its_loads_do_not_apply(ops, L, hop):
    """Odd hop / odd length: the predicate says no, the launch runs the kernel it runs with the form switched off."""
    assert ops.lib().syg_stft2048_mfcc_tri_freerun(hop, L, L, None) == 0
    Y = O.synth_clips(9, L, 16000, seed=8)
    y = ops.to_device_f32(Y)
    new, again, staged = both_forms(ops, y, 16000, hop=hop, n_mels=40)
    ref = np.stack([O.mfcc_manager(c.astype(np.float64), 16000, 2048, hop, True, "hann", 40, 13) for c in Y])
    assert_parity(new.cpu().numpy(), ref, TOL, f"fallback L={L} hop={hop}")
    assert torch.equal(new, staged) and torch.equal(new, again)
