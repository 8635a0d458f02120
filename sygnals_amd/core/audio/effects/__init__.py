"""Device-backed mirror of sygnals/core/audio/effects: delay, tremolo, compression, reverb, time stretch and the
utility effects (gain, spectral noise reduction, HPSS transient shaping, mid / side widening), and the equalizers, which
keep the reference's signatures and deliver what its docstrings promise (equalizer.py: the reference's own stages are
never applied).

Each function takes and returns float64 NumPy like the reference; its `*_batch` form takes a float32 device tensor
[B, L] with one parameter set for the batch and stays on the device.  Not mirrored: apply_chorus / apply_flanger (the
reference's interpolation point lies left of its grid, so both compute apply_delay with
delay_samples = ceil((delay + depth) sr) + 2 and ignore their LFO) and pitch_shift (resampy's tabulated 'kaiser_best' filter: nothing here to pin a restatement against).
"""
from .compression import simple_dynamic_range_compression, simple_dynamic_range_compression_batch
from .delay import apply_delay, apply_delay_batch
from .equalizer import (apply_graphic_eq, apply_graphic_eq_batch, apply_parametric_eq, apply_parametric_eq_batch,
                        design_eq_sos)
from .reverb import apply_reverb, apply_reverb_batch
from .time_stretch import time_stretch, time_stretch_batch
from .tremolo import apply_tremolo, apply_tremolo_batch
from .utility import (adjust_gain, adjust_gain_batch, noise_reduction_spectral, noise_reduction_spectral_batch,
                      stereo_widening_midside, stereo_widening_midside_batch, transient_shaping_hpss,
                      transient_shaping_hpss_batch)

__all__ = [
    "apply_delay", "apply_delay_batch", "apply_tremolo", "apply_tremolo_batch", "simple_dynamic_range_compression",
    "simple_dynamic_range_compression_batch", "apply_reverb", "apply_reverb_batch", "adjust_gain", "adjust_gain_batch",
    "stereo_widening_midside", "stereo_widening_midside_batch", "noise_reduction_spectral",
    "noise_reduction_spectral_batch", "transient_shaping_hpss", "transient_shaping_hpss_batch", "time_stretch",
    "time_stretch_batch", "apply_parametric_eq", "apply_parametric_eq_batch", "apply_graphic_eq", "apply_graphic_eq_batch",
    "design_eq_sos",
]
