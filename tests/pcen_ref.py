"""Float64 restatement of librosa 0.10's pcen on [..., M, T] arrays (bands, frames): the contract of csrc/pcen.hip.

It is built from the two SciPy calls librosa makes (scipy.ndimage.maximum_filter1d and scipy.signal.lfilter), so those
pieces are pinned to SciPy itself.  gain, bias, power, eps and b may each be a scalar or a vector of one value per band."""
import numpy as np
import scipy.ndimage
import scipy.signal


def b_of(time_constant=0.4, sr=22050, hop_length=512):
    t = time_constant * sr / hop_length
    return (np.sqrt(1 + 4 * t ** 2) - 1) / (2 * t ** 2)


def smoother(ref, b, zi=None):
    """(M, zf) of scipy.signal.lfilter([b], [1, b - 1], ref, zi=zi, axis=-1); zi None: lfilter_zi (= 1 - b), as librosa
    takes it (not scaled by the first frame).  zi, zf: [..., 1]."""
    ref = np.asarray(ref, dtype=np.float64)
    if zi is None:
        zi = np.broadcast_to(scipy.signal.lfilter_zi([b], [1, b - 1]), ref.shape[:-1] + (1,))
    return scipy.signal.lfilter([b], [1, b - 1], ref, zi=np.asarray(zi, dtype=np.float64), axis=-1)


def _pcen_scalar(S, gain, bias, power, eps, b, ref, zi):
    M, zf = smoother(ref, b, zi)
    smooth = np.exp(-gain * (np.log(eps) + np.log1p(M / eps)))
    with np.errstate(divide="ignore"):
        if power == 0:
            out = np.log1p(S * smooth)
        elif bias == 0:
            out = np.exp(power * (np.log(S) + np.log(smooth)))
        else:
            out = (bias ** power) * np.expm1(power * np.log1p(S * smooth / bias))
    return out, zf


def pcen(S, sr=22050, hop_length=512, gain=0.98, bias=2.0, power=0.5, time_constant=0.4, eps=1e-6, b=None, max_size=1,
         scale=1.0, zi=None, return_zf=False):
    """S [..., M, T] -> float64 of the same shape (and zf [..., M]); zi [..., M] or None."""
    S = np.asarray(S, dtype=np.float64) * scale
    if b is None:
        b = b_of(time_constant, sr, hop_length)
    ref = S if max_size == 1 else scipy.ndimage.maximum_filter1d(S, max_size, axis=-2)
    nb = S.shape[-2]
    vec = [np.ndim(v) > 0 for v in (gain, bias, power, eps, b)]
    z = None if zi is None else np.asarray(zi, dtype=np.float64)[..., None]
    if not any(vec):
        out, zf = _pcen_scalar(S, gain, bias, power, eps, b, ref, z)
    else:
        g, bi, p, e, bb = (np.broadcast_to(np.asarray(v, dtype=np.float64), (nb,)) for v in (gain, bias, power, eps, b))
        out, zf = np.empty_like(S), np.empty(S.shape[:-1] + (1,))
        for m in range(nb):
            out[..., m, :], zf[..., m, :] = _pcen_scalar(S[..., m, :], g[m], bi[m], p[m], e[m], bb[m], ref[..., m, :],
                                                        None if z is None else z[..., m, :])
    return (out, zf[..., 0]) if return_zf else out


def reflected_max(S, max_size):
    """The running maximum over bands by hand: window m - max_size // 2 ... + max_size - 1, (d c b a | a b c d | d c b a)."""
    S = np.asarray(S, dtype=np.float64)
    nb = S.shape[-2]
    out = np.empty_like(S)
    for m in range(nb):
        idx = []
        for k in range(m - max_size // 2, m - max_size // 2 + max_size):
            while k < 0 or k >= nb:
                k = -k - 1 if k < 0 else 2 * nb - 1 - k
            idx.append(k)
        out[..., m, :] = S[..., idx, :].max(axis=-2)
    return out


def noisy_rows(rows, T, seed=0, quiet=1e-4):
    """Squared normal noise with a stretch `quiet` times quieter in the middle third: float32 [rows, T]."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, T)) ** 2
    x[:, T // 3:2 * T // 3] *= quiet
    return x.astype(np.float32)
