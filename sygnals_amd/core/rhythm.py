"""Rhythm on the device: librosa 0.10's feature.tempogram (autocorrelation), feature.tempo and beat.beat_track.

The batch calls take clips y [B, L] (through onset_strength_batch) or, with onset_envelope=, envelopes [B, T], and return
device tensors: nothing between the envelope and the beats crosses to the host (the tempo's lag goes to the beat tracker as
a device array).  The single-clip calls take librosa's signatures and return NumPy.  Parity with librosa is unpinned (it is
not a dependency): the float64 restatement of tests/beat_ref.py is the contract.  Two of its rules, said here because a
caller meets them: the trimmed result is b[min v : max v] with the upper end exclusive, as librosa 0.10.0 has it (the last
beat that passes the trim threshold is dropped); an all-zero envelope gives tempo 0.0 and no beats.
"""
from __future__ import annotations

import logging
from typing import Optional

import numpy as np

from .. import _rhythm as RH
from .. import ops
from .audio.features import _as_clips, onset_strength_batch

logger = logging.getLogger(__name__)

__all__ = ["tempogram_batch", "tempo_batch", "beat_track_batch", "tempogram", "tempo", "beat_track"]


def _envelopes(y, sr, onset_envelope, hop_length, who):
    """The envelopes [B, T] of the call as a float32 device tensor: the given ones, or onset_strength_batch of the clips."""
    if onset_envelope is None and y is None:
        raise ValueError(f"{who}: either the audio y or onset_envelope must be given")
    if not (isinstance(hop_length, (int, np.integer)) and hop_length >= 1):
        raise ValueError(f"{who}: hop_length must be a positive integer")
    if not (sr is not None and sr > 0):
        raise ValueError(f"{who}: sr must be positive")
    if onset_envelope is not None:
        env = _as_clips(onset_envelope)
    else:
        env = onset_strength_batch(_as_clips(y), sr, hop_length=hop_length)
    if env.shape[1] < 1:
        raise ValueError(f"{who}: the envelope is empty")
    return env


def tempogram_batch(y=None, sr: float = 22050, onset_envelope=None, hop_length: int = 512, win_length: int = 384,
                    center: bool = True, window="hann", norm=np.inf):
    """The autocorrelation tempogram of every clip -> float32 [B, win_length, n] device tensor (`syg_tempogram_f32`)."""
    who = "tempogram"
    win = RH.check_win_length(win_length, who)
    RH.check_norm(norm, who)
    env = _envelopes(y, sr, onset_envelope, hop_length, who)
    return ops.tempogram(env, win, center, window, norm)


def _tempo(env, sr, hop_length, start_bpm, std_bpm, ac_size, max_tempo, aggregated=True):
    """(k*, bpm) device tensors of envelopes on the device, and the win_length used."""
    win = RH.tempo_win_length(ac_size, sr, hop_length, "tempo")
    bpms, logprior = RH.tempo_prior(win, sr, hop_length, start_bpm, std_bpm, max_tempo)
    if aggregated:
        a = ops.tempogram(env, win, aggregate="only")
    else:
        a = ops.tempogram(env, win)
    kstar, bpm = ops.tempo_pick(a, env, logprior, bpms)
    return kstar, bpm, win


def tempo_batch(y=None, sr: float = 22050, onset_envelope=None, hop_length: int = 512, start_bpm: float = 120.0,
                std_bpm: float = 1.0, ac_size: float = 8.0, max_tempo: Optional[float] = 320.0, aggregate="mean", prior=None):
    """The tempo of every clip in beats per minute -> float64 [B] device tensor, or [B, T] with aggregate=None: one per
    frame (`syg_tempogram_f32`, whose aggregate alone is written, then `syg_tempo_pick_f32`)."""
    who = "tempo"
    if prior is not None:
        raise ValueError(f"{who}: prior= distributions are not served ({RH.SERVED})")
    aggregated = RH.check_aggregate(aggregate, who)
    win = RH.tempo_win_length(ac_size, sr, hop_length, who)
    RH.tempo_prior(win, sr, hop_length, start_bpm, std_bpm, max_tempo)
    env = _envelopes(y, sr, onset_envelope, hop_length, who)
    if not aggregated:
        RH.check_size(env.shape[0], win, env.shape[1], who)
    return _tempo(env, sr, hop_length, start_bpm, std_bpm, ac_size, max_tempo, aggregated)[1]


def beat_track_batch(y=None, sr: float = 22050, onset_envelope=None, hop_length: int = 512, start_bpm: float = 120.0,
                     tightness: float = 100, trim: bool = True, bpm=None, prior=None):
    """Beat tracking of every clip -> (tempo [B] float64, beats [B, T] int32: each clip's beat frames in ascending order, -1
    beyond them; count [B] int32), device tensors.  bpm: None (estimated per clip), a scalar or one value per clip.  The
    chain: tempogram aggregate, tempo pick, local score, DP, beats (`syg_beat_*`), the period handed on as a device array."""
    who = "beat_track"
    if prior is not None:
        raise ValueError(f"{who}: prior= distributions are not served ({RH.SERVED})")
    tight = RH.check_tightness(tightness, who)
    if bpm is None:
        win = RH.tempo_win_length(8.0, sr, hop_length, who)
        RH.tempo_prior(win, sr, hop_length, start_bpm)
    else:
        bpm = bpm.detach().cpu().numpy() if hasattr(bpm, "is_cuda") else bpm
        v = np.asarray(bpm, dtype=np.float64).reshape(-1)           # the rules that need no row count, ahead of device work
        RH.periods_from_bpm(v, len(v), sr, hop_length, who)
    env = _envelopes(y, sr, onset_envelope, hop_length, who)
    B, Tn = env.shape
    if B * Tn > RH.MAX_ELEMS:
        raise ValueError(f"{who}: the result [{B}, {Tn}] has more than 2^31 elements; call it on fewer rows")
    if bpm is None:
        period, tempo_dev, win = _tempo(env, sr, hop_length, start_bpm, 1.0, 8.0, 320.0)
        pmax = max(2, win - 1)
    else:
        p = RH.periods_from_bpm(bpm, B, sr, hop_length, who)
        period = ops.torch.from_numpy(p).to(env.device)
        pmax = int(p.max())
        given = ops.torch.from_numpy(np.broadcast_to(np.asarray(bpm, dtype=np.float64), (B,)).copy()).to(env.device)
        silent = ops.clip_metrics(env)[:, 1] == 0                    # an all-zero envelope: tempo 0.0, as (0, []) says
        tempo_dev = ops.torch.where(silent, ops.torch.zeros_like(given), given)
    ls, lsmax = ops.beat_local_score(env, period)
    cum, back = ops.beat_dp(ls, lsmax, period, tight, period_max=pmax)
    beats, count, _ = ops.beat_track(ls, cum, back, period, trim)
    return tempo_dev, beats, count


# ---------------------------------------------------------------------------------------------------------- single clips
def _one(y, onset_envelope, who):
    if onset_envelope is not None:
        env = np.asarray(onset_envelope)
        if env.ndim != 1:
            raise ValueError(f"{who}: onset_envelope must be a 1D array")
        return None, env[None, :]
    if y is None:
        raise ValueError(f"{who}: either the audio y or onset_envelope must be given")
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError(f"{who}: the audio must be a 1D array")
    return y[None, :], None


def tempogram(y=None, sr: float = 22050, onset_envelope=None, hop_length: int = 512, win_length: int = 384,
              center: bool = True, window="hann", norm=np.inf):
    """librosa.feature.tempogram of one clip -> float32 [win_length, n] NumPy array."""
    yb, eb = _one(y, onset_envelope, "tempogram")
    return tempogram_batch(yb, sr, eb, hop_length, win_length, center, window, norm)[0].cpu().numpy()


def tempo(y=None, sr: float = 22050, onset_envelope=None, hop_length: int = 512, start_bpm: float = 120.0,
          std_bpm: float = 1.0, ac_size: float = 8.0, max_tempo: Optional[float] = 320.0, aggregate=np.mean, prior=None):
    """librosa.feature.tempo of one clip -> float64 array [1], or [T] with aggregate=None."""
    yb, eb = _one(y, onset_envelope, "tempo")
    return tempo_batch(yb, sr, eb, hop_length, start_bpm, std_bpm, ac_size, max_tempo, aggregate, prior)[0].cpu().numpy().reshape(-1)


def beat_track(y=None, sr: float = 22050, onset_envelope=None, hop_length: int = 512, start_bpm: float = 120.0,
               tightness: float = 100, trim: bool = True, bpm=None, prior=None, units: str = "frames"):
    """librosa.beat.beat_track of one clip -> (tempo, beats) with beats in frames, samples or seconds."""
    if units not in ("frames", "samples", "time"):
        raise ValueError(f"beat_track: invalid unit type: {units}")
    if bpm is not None and np.ndim(bpm) != 0:
        raise ValueError("beat_track: a time-varying bpm is not served; give one value")
    yb, eb = _one(y, onset_envelope, "beat_track")
    t, beats, count = beat_track_batch(yb, sr, eb, hop_length, start_bpm, tightness, trim, bpm, prior)
    frames = beats[0, :int(count[0].item())].cpu().numpy().astype(np.int64)
    t = float(t[0].item())
    if units == "frames":
        return t, frames
    samples = frames * int(hop_length)
    if units == "samples":
        return t, samples
    return t, (samples / float(sr)).astype(np.float64)
