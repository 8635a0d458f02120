"""Device-backed mirror of sygnals/core/segmentation.py: segment_fixed_length (:25-117), segment_by_silence (:120-261)
and segment_by_event (:264-347).

segment_fixed_length and segment_by_event are index arithmetic on the host and need no device.  segment_by_silence
takes its per-frame RMS from the device (`syg_frame_stats_f32`; the reference calls librosa.feature.rms) and applies the
reference's run, pad and merge rules to that row on the host (`_segments_from_rms`).  segment_by_onsets joins
detect_onsets to segment_by_event; its (start, end) sample pairs are what format_feature_vectors_per_segment takes.
"""
from __future__ import annotations

import logging
from typing import Any, List, Optional, Tuple

import numpy as np

from .. import ops

logger = logging.getLogger(__name__)

_EPSILON = np.finfo(np.float64).eps
_ROW_RMS = 7


def segment_fixed_length(y, sr: int, segment_length_sec: float, overlap_ratio: float = 0.0, pad: bool = True,
                         min_segment_length_sec: Optional[float] = None) -> List[np.ndarray]:
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("Input signal y must be 1D.")
    if segment_length_sec <= 0:
        raise ValueError("segment_length_sec must be positive.")
    if not 0.0 <= overlap_ratio < 1.0:
        raise ValueError("overlap_ratio must be between 0.0 and < 1.0.")
    seg = int(segment_length_sec * sr)
    if seg == 0:
        logger.warning(f"Segment length in samples is 0 for {segment_length_sec}s and sr={sr}. No segments generated.")
        return []
    hop = max(1, int(seg * (1.0 - overlap_ratio)))
    min_samples = int(min_segment_length_sec * sr) if min_segment_length_sec is not None else 0
    logger.info(f"Segmenting signal (length {len(y)}) into fixed segments: len={segment_length_sec}s ({seg} samples), "
                f"overlap={overlap_ratio * 100:.1f}% ({hop} hop samples), pad={pad}, min_len={min_samples} samples")
    n = len(y)
    out = []
    start = 0
    while start < n:
        piece = y[start:start + seg]
        if min_samples > 0 and len(piece) < min_samples:       # checked on the length before padding
            logger.debug(f"Discarding segment starting at {start} (original length {len(piece)} < min {min_samples}).")
        elif start + seg > n:                                  # the partial tail: zero-filled, or dropped
            if pad:
                out.append(np.pad(piece, (0, seg - len(piece)), mode="constant").astype(np.float64, copy=False))
        else:
            out.append(piece.astype(np.float64, copy=False))
        start += hop
        if not pad and start + seg > n:                        # no full segment starts here or later
            break
    logger.debug(f"Generated {len(out)} fixed-length segments.")
    return out


def _segments_from_rms(rms, total_samples: int, sr: int, hop_length: int, threshold_db: float = -40.0,
                       min_silence_duration_sec: float = 0.1, min_segment_duration_sec: float = 0.2,
                       padding_sec: float = 0.05) -> List[Tuple[int, int]]:
    """The reference's rules after the RMS row (:174-261): threshold relative to the loudest frame, silent runs of at
    least min_silence frames split the signal, the pieces are padded, filtered by length and merged where they overlap."""
    rms = np.asarray(rms, dtype=np.float64)
    if rms.size == 0:
        logger.warning("Could not calculate RMS frames (signal likely too short). Returning no segments.")
        return []
    peak = np.max(rms)
    if peak < _EPSILON:
        logger.warning("Signal maximum RMS is near zero. Assuming entire signal is silent.")
        return []
    silent = rms < peak * (10.0 ** (threshold_db / 20.0))
    min_run = max(1, int(np.ceil(min_silence_duration_sec * sr / hop_length)))
    nf = len(silent)
    # runs of silent frames [a, b) of at least min_run frames
    edges = np.flatnonzero(np.diff(np.concatenate(([0], silent.astype(np.int8), [0]))))
    runs = [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2]) if b - a >= min_run]
    # what lies between them
    pieces = []
    prev = 0
    for a, b in runs:
        if a > prev:
            pieces.append((prev, a))
        prev = b
    if prev < nf:
        pieces.append((prev, nf))
    min_len = int(min_segment_duration_sec * sr)
    padn = int(padding_sec * sr)
    spans = []
    for a, b in pieces:
        s0 = max(0, a * hop_length - padn)
        s1 = min(total_samples, b * hop_length + padn)
        if s1 - s0 >= min_len:                                 # checked after padding
            spans.append((s0, s1))
        else:
            logger.debug(f"Discarding segment ({s0}, {s1}) due to min_segment_duration.")
    if not spans:
        return []
    spans.sort(key=lambda p: p[0])
    merged = []
    cur0, cur1 = spans[0]
    for s0, s1 in spans[1:]:
        if s0 < cur1:
            cur1 = max(cur1, s1)
        else:
            merged.append((cur0, cur1))
            cur0, cur1 = s0, s1
    merged.append((cur0, cur1))
    logger.debug(f"Generated {len(merged)} segments by silence.")
    return merged


def segment_by_silence(y, sr: int, threshold_db: float = -40.0, min_silence_duration_sec: float = 0.1,
                       min_segment_duration_sec: float = 0.2, padding_sec: float = 0.05, frame_length: int = 512,
                       hop_length: Optional[int] = None) -> List[Tuple[int, int]]:
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("Input signal y must be 1D.")
    if threshold_db > 0:
        raise ValueError("threshold_db must be non-positive (e.g., -40.0).")
    if min_silence_duration_sec < 0 or min_segment_duration_sec < 0 or padding_sec < 0:
        raise ValueError("Durations and padding must be non-negative.")
    hop = hop_length if hop_length is not None else frame_length // 4
    if hop <= 0:
        raise ValueError("Hop length must be positive.")
    logger.info(f"Segmenting by silence: threshold={threshold_db}dB, min_silence={min_silence_duration_sec}s, "
                f"min_segment={min_segment_duration_sec}s, padding={padding_sec}s, frame_len={frame_length}")
    ops.require_gpu()
    if y.size == 0:
        return _segments_from_rms(np.empty(0), 0, sr, hop)
    st = ops.frame_stats(ops.to_device_f32(y[None, :]), frame_length, hop, True, mask=1 << _ROW_RMS)
    rms = st[0, _ROW_RMS].cpu().numpy()
    return _segments_from_rms(rms, len(y), sr, hop, threshold_db, min_silence_duration_sec, min_segment_duration_sec,
                              padding_sec)


def detect_activity_batch(y, sr: int, *, frame_length: int = 2048, hop_length: int = 512, threshold: float = 0.02,
                          self_prob=(0.5, 0.6)):
    """A smoothed activity mask of every clip: y [B, L] float32 on the device -> [B, T] int32 of 0 (inactive) / 1 (active).
    librosa's documented Viterbi recipe on the device's own RMS (our definition; nothing here is pinned to librosa):
        r = (rms - threshold) / std(rms);  p = 1 / (1 + exp(-r));
        viterbi_discriminative([1 - p, p], transition_loop(2, self_prob))
    with rms the centred frame RMS of syg_frame_stats_f32, the population standard deviation over the clip's frames and
    r, p in float64.  A clip of constant RMS (std = 0) reads as inactive in every frame, never as NaN.  sr is not used by
    the recipe; it is taken for the signature the segmenters share."""
    import torch
    from .._sequence import transition_loop
    if not isinstance(y, torch.Tensor) or y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError("detect_activity_batch: y must be a float32 tensor [B, L]")
    if frame_length < 1 or hop_length < 1:
        raise ValueError("detect_activity_batch: frame_length and hop_length must be positive")
    if not np.isfinite(threshold):
        raise ValueError("detect_activity_batch: threshold must be finite")
    trans = transition_loop(2, self_prob)
    st = ops.frame_stats(y, frame_length, hop_length, True, mask=1 << _ROW_RMS)
    rms = st[:, _ROW_RMS].to(torch.float64)
    std = rms.std(dim=1, unbiased=False, keepdim=True)
    flat = std == 0
    r = (rms - float(threshold)) / torch.where(flat, torch.ones_like(std), std)
    p = torch.where(flat, torch.zeros_like(r), 1.0 / (1.0 + torch.exp(-r)))
    return ops.viterbi(torch.stack([1.0 - p, p], dim=1), trans, p_state=np.array([0.5, 0.5]))


def segment_by_activity(y, sr: int, frame_length: int = 2048, hop_length: int = 512, threshold: float = 0.02,
                        self_prob=(0.5, 0.6)) -> List[Tuple[int, int]]:
    """(start, end) sample pairs of the active stretches of a 1-D signal, in the shape segment_by_silence returns: the
    runs of 1 in detect_activity_batch's mask, frame a starting at sample a * hop_length."""
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("Input signal y must be 1D.")
    ops.require_gpu()
    if y.size == 0:
        return []
    mask = detect_activity_batch(ops.to_device_f32(y[None, :]), sr, frame_length=frame_length, hop_length=hop_length,
                                 threshold=threshold, self_prob=self_prob)[0].cpu().numpy()
    edges = np.flatnonzero(np.diff(np.concatenate(([0], (mask == 1).astype(np.int8), [0]))))
    return [(int(a) * hop_length, min(len(y), int(b) * hop_length)) for a, b in zip(edges[0::2], edges[1::2])
            if int(a) * hop_length < len(y)]


def segment_by_event(y, sr: int, event_times_sec, segment_duration_sec: Optional[float] = None,
                     pre_event_sec: float = 0.05, post_event_sec: float = 0.2) -> List[Tuple[int, int]]:
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("Input signal y must be 1D.")
    if pre_event_sec < 0 or post_event_sec < 0:
        raise ValueError("pre_event_sec and post_event_sec must be non-negative.")
    if segment_duration_sec is not None and segment_duration_sec <= 0:
        raise ValueError("segment_duration_sec must be positive if specified.")
    if event_times_sec is None or len(event_times_sec) == 0:
        logger.warning("No event times provided for segmentation.")
        return []
    logger.info(f"Segmenting by {len(event_times_sec)} events. "
                f"Method: {'fixed duration' if segment_duration_sec else 'pre/post padding'}.")
    events = (np.asarray(event_times_sec) * sr).astype(int)
    n = len(y)
    if segment_duration_sec:
        dur = int(segment_duration_sec * sr)
        before, after = dur // 2, dur - dur // 2               # centred on the event, `dur` samples long
    else:
        before, after = int(pre_event_sec * sr), int(post_event_sec * sr)
    out = []
    for ev in events:
        s0, s1 = max(0, int(ev) - before), min(n, int(ev) + after)
        if s0 < s1:
            out.append((s0, s1))
        else:
            logger.debug(f"Skipping segment for event at sample {ev} as clipped boundaries are invalid ({s0}, {s1}).")
    logger.debug(f"Generated {len(out)} segments by event.")
    return out


def segment_by_onsets(y, sr: int, hop_length: int = 512, segment_duration_sec: Optional[float] = None,
                      pre_event_sec: float = 0.05, post_event_sec: float = 0.2, **onset_kwargs: Any):
    """Segments around the detected onsets: detect_onsets(units='time') then segment_by_event."""
    from .audio.features import detect_onsets
    times = detect_onsets(y, sr=sr, hop_length=hop_length, units="time", **onset_kwargs)
    return segment_by_event(y, sr, times, segment_duration_sec, pre_event_sec, post_event_sec)


def segment_by_beats(y, sr: int, hop_length: int = 512, segment_duration_sec: Optional[float] = None,
                     pre_event_sec: float = 0.05, post_event_sec: float = 0.2, **beat_kwargs: Any):
    """Segments around the tracked beats: beat_track(units='time') then segment_by_event."""
    from .rhythm import beat_track
    _, times = beat_track(y, sr=sr, hop_length=hop_length, units="time", **beat_kwargs)
    return segment_by_event(y, sr, times, segment_duration_sec, pre_event_sec, post_event_sec)
