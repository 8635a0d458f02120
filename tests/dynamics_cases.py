"""The cases the dynamics tests share (tests/test_dynamics_ref.py on the CPU, tests/test_gpu_dynamics.py on the device):
parameters, frame counts around the tile and residency edges, and the inputs.  TILE and the residency figures restate
ops.dynamics_constants(); both test files assert that they agree with the library."""
import numpy as np

TILE = 1024
RESIDENT_T = 3072
RESIDENT_T_SLIDING = 2048
DIRECT_WINDOW = 32

DELTA_WO = [(3, 1), (3, 2), (5, 1), (5, 2), (9, 1), (9, 2), (31, 1), (31, 2), (9, 3), (9, 4)]
EDGE_MODES = ["nearest", "mirror", "wrap", "constant"]
CVAL = 2.5
SHAPES_BK = [(1, 1), (3, 13), (33, 40), (1, 13), (3, 40), (33, 1)]

CMVN_T = [1, 2, 3, 64, 65, 94, 600, 601, 1201, TILE - 1, TILE + 1]
STACK = [(n, d) for n in (1, 2, 5) for d in (1, -1, 3, -3, "T+1")]
POST_SHAPES = [(33, 13, 65), (3, 40, 94), (1, 13, TILE + 1)]


def delta_T(width):
    h = width // 2
    Ts = {width, width + 1, 2 * width, 64, 65, 94, 257, TILE - 1, TILE, TILE + 1, TILE + h, 2 * TILE + 3}
    return sorted(t for t in Ts if t >= width)


def mode_T(width):
    h = width // 2
    return sorted({1, 2, h, h + 1, width, 65})


def bk_for(i, T):
    """A (B, K) of SHAPES_BK by case number; the long rows take the small ones."""
    B, K = SHAPES_BK[i % len(SHAPES_BK)]
    if T > 300 and B * K > 39:
        B, K = (3, 13)
    return B, K


def cmvn_windows(T):
    return [None, 1, 2, 3, 31, 300, 600, 601, T, T + 1]


def delta_input(B, K, T, seed):
    """White rows of mixed scale (the gate is per row)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, K, T))
    scale = np.where(np.arange(K) % 3 == 0, 50.0, 1.0)[None, :, None]
    off = np.where(np.arange(K) % 3 == 0, -400.0, 0.0)[None, :, None]
    return (x * scale + off).astype(np.float32)


def cmvn_input(B, K, T, seed):
    """Even rows like MFCC c0 (mean -400, deviation 50), odd rows of unit variance and mean 0.3."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, K, T))
    c0 = (np.arange(K) % 2 == 0)[None, :, None]
    return np.where(c0, -400.0 + 50.0 * x, 0.3 + x).astype(np.float32)


def cmvn_input_ok(x, W=None):
    """Every row has deviation >= 1e-3 |mean| (what keeps E[x^2] - m^2 sound in float64), over the row and, where T allows
    it, needs no more: the generator above has deviation 50 against mean 400.  Rows of T = 1 are exact cases."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[-1] < 2:
        return True
    return bool(np.all(x.std(axis=-1) >= 1e-3 * np.abs(x.mean(axis=-1))))
