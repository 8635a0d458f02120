"""Float64 restatement, vectorised, of the reference's laplace_transform_numerical (sygnals/core/transforms.py:159-199):
the parity contract of syg_laplace_f32.  tests/test_laplace_ref.py pins it to the reference's own recorded output
(tests/golden/ref_laplace.npz)."""
import numpy as np


def _grid(L, s_values, t_step):
    t = np.arange(L) * t_step                                        # the reference's own rounding: n * t_step, then -s * t
    return -np.asarray(s_values, dtype=np.complex128)[:, None] * t[None, :]           # [S, L]


def laplace(x, s_values, t_step=1.0, block=1 << 16):
    """x [L] or [B, L] -> [S] or [B, S] complex128: sum_n x[n] exp(-s n t_step) t_step, in blocks of `block` samples."""
    x = np.asarray(x, dtype=np.float64)
    rows = np.atleast_2d(x)
    s = np.asarray(s_values, dtype=np.complex128)
    out = np.zeros((rows.shape[0], s.size), dtype=np.complex128)
    t = np.arange(rows.shape[1]) * t_step
    for n0 in range(0, rows.shape[1], block):
        E = np.exp(-s[:, None] * t[None, n0:n0 + block])             # [S, block]
        out += rows[:, n0:n0 + block] @ E.T
    out *= t_step
    return out[0] if x.ndim == 1 else out


def scale(x, s_values, t_step=1.0, block=1 << 16):
    """The natural scale of the sum, A = |t_step| sum_n |x[n]| exp(-Re(s) n t_step): the gate is 1e-5 A."""
    sig = np.asarray(s_values, dtype=np.complex128).real.astype(np.complex128)
    return np.abs(laplace(np.abs(np.asarray(x, dtype=np.float64)), sig, t_step, block).real)
