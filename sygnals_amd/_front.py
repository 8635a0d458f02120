"""Which kernel serves a request to the STFT front ends (mel power, per-frame statistics, contrast tail means): the one
place that decides it.  Pure host logic -- ops.stft_front launches what front_route returns, tests/test_host_logic.py
pins it -- so neither torch nor the library is imported here."""
from __future__ import annotations

from ._lib import SygnalsHipError


def pow2_takes(n_fft: int, n_mels: int) -> bool:
    """The dense kernel of the other power-of-two frame lengths (stft_mel_pow2.hip): 64 ... 1024, at most 256 bands."""
    return n_fft in (64, 128, 256, 512, 1024) and 1 <= n_mels <= 256


def stats2048_takes(hop: int, L: int, waves: int) -> bool:
    """The C side's conditions of syg_stft2048_stats_f32 (staged tiles need hop <= 512 and 32-bit byte offsets, L < 2^28;
    frame count below 2^24) and the 16-wave kernel."""
    return hop <= 512 and L < (1 << 28) and 1 + L // max(hop, 1) < (1 << 24) and waves == 16


_SEGMENTS = {1024: "stft_mel_w1024_seg", 512: "stft_mel_wseg_small", 256: "stft_mel_wseg_small", 4096: "stft_mel_w4096"}


def front_route(n_fft, hop, L, power, n_mels, rows, caps):
    """(rows wrapper | None, mel wrapper | None): the functions of sygnals_amd.ops that produce the statistics / contrast
    rows and the mel block [B, n_mels, T] of |STFT|^power for clips of L samples.  rows: statistics or contrast are asked
    for; n_mels None: no mel block is.  The rows name is None without rows; the mel name is None when the rows launch
    yields the mel block too (or none is wanted); "generic" is the chain stft_any -> cabs_pow -> mel_dense /
    spectral_stats / contrast_pv, which then serves the whole request.
    caps: what the tables say, decided on the host before anything is launched --
      waves     ops.fused_waves()
      plan2048  the fused 2048 kernel holds the filterbank (ops.fused_mel_ok; of 16 stand-in bands when n_mels is None)
      table     the segment-sum kernel of this frame length (1024, 4096, 512, 256) has a piece table for the filterbank"""
    mel = n_mels is not None
    p12 = power in (1.0, 2.0)
    seg = mel and power == 2.0 and caps["table"]
    if not rows:
        # mel only: 2048 fused -> segment sums -> the dense power-of-two kernel -> generic
        if power == 2.0 and caps["plan2048"]:
            return None, "stft2048_mel"
        if not p12:
            raise SygnalsHipError("mel power must be 1.0 or 2.0 on the device")
        if seg and n_fft in _SEGMENTS:
            return None, _SEGMENTS[n_fft]
        return None, "stft_mel_pow2" if pow2_takes(n_fft, n_mels) else "generic"
    if n_fft == 2048:
        if not mel and stats2048_takes(hop, L, caps["waves"]):
            return "stft2048_stats", None            # transform + row functions, nothing projected
        if power == 2.0 and caps["plan2048"]:
            return "stft2048_mel", None              # (no mel wanted: 16 stand-in bands, discarded)
    elif n_fft == 1024 and (not mel or (p12 and pow2_takes(1024, n_mels))):
        # the mel block from the rows launch where the filterbank has a piece table (power 2), else from the dense kernel
        return "stft_rows_w1024", "stft_mel_pow2" if mel and not seg else None
    elif n_fft == 4096 and (not mel or seg):
        return "stft_rows_w4096", None
    elif n_fft in (512, 256) and (not mel or (p12 and pow2_takes(n_fft, n_mels))):
        # the rows from the segment-sum kernel's transform; the mel block, if wanted, from its own launch
        return "stft_rows_wsmall", ("stft_mel_wseg_small" if seg else "stft_mel_pow2") if mel else None
    return "generic", "generic" if mel else None
