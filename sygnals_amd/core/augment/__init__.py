"""Device-backed mirror of sygnals/core/augment: add_noise and time_stretch, and SpecAugment on feature tensors.

Each function takes and returns float64 NumPy like the reference; its `*_batch` form takes a float32 device tensor
[B, L] and stays on the device.  add_noise_device / add_noise_device_batch / generate_noise_batch draw the noise on the
device (this package's own generator, with real pink and brown noise).  spec_augment / spec_augment_batch and the
single-purpose freq_mask_batch / time_mask_batch / time_warp_batch work on [K, T] features, not waveforms, and are this
package's own too (the reference has no counterpart).  Not mirrored: pitch_shift (the reference resamples with resampy's tabulated
'kaiser_best' filter, which this package has nothing to pin a restatement against).
"""
from .effects_based import time_stretch, time_stretch_batch
from .noise import add_noise, add_noise_batch, add_noise_device, add_noise_device_batch, generate_noise_batch
from .spec_augment import freq_mask_batch, spec_augment, spec_augment_batch, time_mask_batch, time_warp_batch

__all__ = ["add_noise", "add_noise_batch", "add_noise_device", "add_noise_device_batch", "generate_noise_batch", "time_stretch",
           "time_stretch_batch", "spec_augment", "spec_augment_batch", "freq_mask_batch", "time_mask_batch", "time_warp_batch"]
