"""ctypes binding of libsygnals_hip.so (the C ABI declared in include/sygnals_hip.h).

The product path has NO CPU fallback: `lib()` raises if the shared library has not been
built, and every op raises if no GPU is present.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SYGNALS_AMD_LIB: development only (timeline builds, A/B of a kernel against an earlier one) -- a library built somewhere else
LIB_PATH = os.environ.get("SYGNALS_AMD_LIB") or os.path.join(_HERE, "lib", "libsygnals_hip.so")

_p = C.c_void_p
_i = C.c_int
_l = C.c_int64
_f = C.c_float
_d = C.c_double
_u = C.c_uint64

# name -> (restype, argtypes); must list every symbol declared in include/sygnals_hip.h
SIGNATURES = {
    "syg_abi_version": (_i, []),
    "syg_build_variant": (_i, []),
    "syg_last_error": (C.c_char_p, []),
    "syg_set_option": (_i, [_i, _i]),
    "syg_get_option": (_i, [_i]),
    "syg_launch_constants": (_l, [_i]),
    "syg_stft2048_mel_f32": (_i, [_p, _l, _l, _l, _i, _i, _l, _p, _p, _p, _p, _i, _p, _f, _f, _f, _i, _p, _p, _p, _p]),
    "syg_stft2048_c2c_f32": (_i, [_p, _l, _l, _l, _i, _i, _l, _p, _p, _p, _p]),
    "syg_stft2048_mfcc_fits": (_i, [_i, _l, _i]),
    "syg_stft2048_mfcc_tri_fits": (_i, [_i, _l, _i]),
    "syg_stft2048_mfcc_tri_freerun": (_i, [_i, _l, _l, _p]),
    "syg_stft2048_mfcc_tri_f32": (_i, [_p, _l, _l, _l, _i, _i, _l, _p, _p, _p, _i, _i, _p, _i, _p, _f, _f, _i, _f, _p, _p]),
    "syg_stft2048_mfcc_f32": (_i, [_p, _l, _l, _l, _i, _i, _l, _p, _p, _p, _p, _i, _p, _i, _p, _f, _f, _i, _f, _p, _p, _p]),
    "syg_stft2048_features_tri_f32": (_i, [_p, _l, _l, _l, _i, _i, _l, _p, _p, _p, _i, _i, _p, _i, _p, _f, _f, _i, _f, _f, _f, _f, _i, _p, _p,
                                           _p, _p, _i, _p]),
    "syg_stft2048_mel_tri_f32": (_i, [_p, _l, _l, _l, _i, _i, _l, _p, _p, _p, _i, _i, _p, _f, _f, _f, _i, _p, _p, _p, _i, _p]),
    "syg_stft2048_stats_f32": (_i, [_p, _l, _l, _l, _i, _i, _l, _p, _p, _f, _f, _f, _i, _p, _p, _p, _p]),
    "syg_stft_mel_w4096_f32": (_i, [_p, _l, _l, _l, _i, _i, _l, _p, _p, _p, _i, _i, _p, _p]),
    "syg_stft_mel_w1024_seg_f32": (_i, [_p, _l, _l, _l, _i, _i, _l, _p, _p, _p, _i, _i, _p, _p]),
    "syg_stft_rows_w1024_f32": (_i, [_p, _l, _l, _l, _i, _i, _l, _p, _p, _p, _i, _i, _p, _f, _f, _f, _i, _p, _p, _p, _p]),
    "syg_stft_mel_wseg_small_f32": (_i, [_p, _l, _l, _l, _i, _i, _i, _l, _p, _p, _p, _i, _i, _p, _p]),
    "syg_stft_rows_wsmall_f32": (_i, [_p, _l, _l, _l, _i, _i, _i, _l, _p, _p, _f, _f, _f, _i, _p, _p, _p, _p]),
    "syg_stft_rows_w4096_f32": (_i, [_p, _l, _l, _l, _i, _i, _l, _p, _p, _p, _i, _i, _p, _f, _f, _f, _i, _p, _p, _p, _p]),
    "syg_cqt_fused_f32": (_i, [_p, _l, _l, _l, _p, _i, _f, _p, _i, _i, _p, _l, _p, _l, _p]),
    "syg_mel_mfcc_f32": (_i, [_p, _l, _i, _l, _p, _i, _p, _f, _f, _i, _f, _p, _p]),
    "syg_fft_pow2_strided_ex_f32": (_i, [_p, _p, _l, _l, _i, _i, _p, _l, _l, _l, _l, _l, _l, _l, _f, _i, _l, _l, _p]),
    "syg_fft_mixed_strided_ex_f32": (_i, [_p, _p, _l, _l, _i, _i, _p, _l, _l, _l, _l, _l, _l, _l, _f, _i, _l, _l, _p]),
    "syg_frame_stats_f32": (_i, [_p, _l, _l, _l, _i, _i, _i, _l, _i, _i, _p, _p]),
    "syg_rms_from_spec_f32": (_i, [_p, _l, _i, _i, _p, _p]),
    "syg_feature_block_f32": (_i, [_p, _l, _i, _l, _p, _i, _f, _f, _p, _f, _p, _i, _f, _f, _p, _p]),
    "syg_logmel_dct_f32": (_i, [_p, _l, _i, _l, _p, _i, _p, _f, _f, _i, _f, _p, _p, _p]),
    "syg_fft_pow2_c2c_f32": (_i, [_p, _p, _l, _i, _i, _p, _p]),
    "syg_fft_pow2_strided_c2c_f32": (_i, [_p, _p, _l, _l, _i, _i, _p, _l, _l, _l, _l, _l, _l, _l, _f, _p]),
    "syg_cmul_c64": (_i, [_p, _p, _p, _l, _l, _i, _p]),
    "syg_pack_real_c64": (_i, [_p, _l, _l, _l, _p, _p, _l, _p]),
    "syg_stft_pow2_c2c_f32": (_i, [_p, _l, _l, _l, _i, _i, _i, _l, _p, _p, _p, _p]),
    "syg_cabs_pow_f32": (_i, [_p, _l, _i, _p, _p]),
    "syg_mel_dense_f32": (_i, [_p, _l, _l, _i, _p, _i, _p, _p]),
    "syg_stft_mel_pow2_f32": (_i, [_p, _l, _l, _l, _i, _i, _i, _l, _p, _p, _p, _i, _i, _i, _p, _p]),
    "syg_stft_mfcc_pow2_fits": (_i, [_i, _i, _l, _i]),
    "syg_stft_mfcc_pow2_f32": (_i, [_p, _l, _l, _l, _i, _i, _i, _l, _p, _p, _p, _i, _i, _p, _i, _p, _f, _f, _i, _f, _p, _p, _p]),
    "syg_spectral_stats_f32": (_i, [_p, _l, _i, _p, _f, _f, _p, _p]),
    "syg_contrast_pv_f32": (_i, [_p, _l, _i, _p, _p, _p]),
    "syg_contrast_db_f32": (_i, [_p, _l, _i, _l, _f, _f, _p, _p]),
    "syg_decimate2_f32": (_i, [_p, _l, _l, _l, _p, _i, _f, _p, _l, _p]),
    "syg_decimate2_chain_f32": (_i, [_p, _l, _l, _l, _p, _i, _f, _i, _p, _p, _p]),
    "syg_cqt_octave_f32": (_i, [_p, _l, _l, _l, _i, _i, _l, _p, _p, _i, _p, _p, _l, _i, _p]),
    "syg_cqt_octave_bf16x3_f32": (_i, [_p, _l, _l, _l, _i, _i, _l, _p, _i, _p, _l, _i, _p]),
    "syg_cqt_octave_gemm_f32": (_i, [_p, _l, _l, _l, _i, _i, _l, _p, _i, _p, _l, _i, _p]),
    "syg_sosfiltfilt_work_bytes": (_l, [_l, _l, _i, _i]),
    "syg_sosfiltfilt_f32": (_i, [_p, _l, _l, _l, _p, _p, _i, _i, _p, _l, _p, _p]),
    "syg_sosfilt_constants": (_l, [_i]),
    "syg_sosfilt_work_bytes": (_l, [_l, _l, _i]),
    "syg_sosfilt_f32": (_i, [_p, _l, _l, _l, _p, _i, _p, _p, _l, _p, _p, _p]),
    "syg_welch_work_bytes": (_l, [_l, _i]),
    "syg_welch_f32": (_i, [_p, _l, _l, _l, _i, _i, _i, _p, _p, _i, _d, _p, _p, _p]),
    "syg_pack_rows_work_bytes": (_l, [_l]),
    "syg_pack_rows_f32": (_i, [_p, _l, _l, _l, _p, _i, _i, _i, _p, _l, _p, _p]),
    "syg_pack_frames_f32": (_i, [_p, _l, _l, _l, _l, _l, _p, _i, _i, _i, _p, _l, _p, _p]),
    "syg_rconv_spectrum_c64": (_i, [_p, _p, _l, _l, _l, _p, _p]),
    "syg_analytic_mask_c64": (_i, [_p, _l, _l, _p]),
    "syg_psd_onesided_f32": (_i, [_p, _l, _l, _d, _p, _p]),
    "syg_col_mean_f32": (_i, [_p, _l, _l, _p, _i, _i, _d, _p, _p]),
    "syg_fft_mixed_plan": (_i, [_l, _p, _i]),
    "syg_fft_mixed_strided_c2c_f32": (_i, [_p, _p, _l, _l, _i, _i, _p, _l, _l, _l, _l, _l, _l, _l, _f, _p]),
    "syg_col_stats_f32": (_i, [_p, _l, _l, _p, _p]),
    "syg_affine_cols_f32": (_i, [_p, _l, _l, _p, _p, _p, _p, _p]),
    "syg_col_quantiles_f32": (_i, [_p, _l, _l, _p, _i, _p, _p]),
    "syg_zoom_f32": (_i, [_p, _i, _i, _i, _i, _i, _p, _p]),
    "syg_pcm_to_f32": (_i, [_p, _i, _l, _l, _i, _l, _p, _l, _p]),
    "syg_pitch_frames_f32": (_i, [_p, _l, _l, _l, _i, _i, _i, _i, _l, _d, _i, _i, _i, _d, _d, _i, _p, _i, _p, _p, _p, _p, _p,
                                  _p, _p, _p]),
    "syg_pyin_work_bytes": (_l, [_l, _l, _i]),
    "syg_pyin_viterbi_f32": (_i, [_p, _p, _p, _p, _l, _l, _i, _i, _i, _p, _i, _p, _d, _p, _l, _p, _p, _p, _p]),
    "syg_hpss_masks_f32": (_i, [_p, _l, _l, _i, _i, _d, _d, _d, _p, _p, _p, _p, _p]),
    "syg_istft2048_f32": (_i, [_p, _l, _l, _i, _i, _l, _p, _p, _p, _p, _p, _p, _l, _p]),
    "syg_hnr_rows_f32": (_i, [_p, _p, _l, _l, _l, _i, _i, _i, _l, _p, _p, _p, _p]),
    "syg_onset_strength_work_bytes": (_l, [_l, _i, _l]),
    "syg_onset_strength_f32": (_i, [_p, _l, _i, _l, _f, _f, _i, _i, _i, _l, _i, _p, _p, _p]),
    "syg_onset_peaks_f32": (_i, [_p, _l, _l, _l, _i, _i, _i, _i, _d, _i, _i, _i, _p, _p, _p, _p]),
    "syg_clip_metrics_f32": (_i, [_p, _l, _l, _l, _p, _p]),
    "syg_dwt_lengths": (_l, [_l, _i, _i, _p]),
    "syg_dwt_fits": (_i, [_l, _i, _i]),
    "syg_dwt_work_bytes": (_l, [_l, _l, _i, _i]),
    "syg_dwt_f32": (_i, [_p, _l, _l, _l, _p, _p, _i, _i, _i, _p, _l, _p, _p]),
    "syg_idwt_length": (_l, [_p, _i, _i]),
    "syg_idwt_work_bytes": (_l, [_l, _p, _i, _i]),
    "syg_idwt_f32": (_i, [_p, _l, _l, _p, _i, _p, _p, _i, _p, _l, _p, _p]),
    "syg_fx_delay_chunk": (_i, []),
    "syg_fx_delay_work_bytes": (_l, [_l, _l, _l]),
    "syg_fx_delay_f32": (_i, [_p, _l, _l, _l, _l, _d, _d, _d, _p, _l, _p, _p]),
    "syg_spectral_gate_f32": (_i, [_p, _l, _l, _p, _l, _d, _p, _p, _p]),
    "syg_fx_mix_f32": (_i, [_p, _l, _l, _p, _l, _l, _l, _l, _d, _d, _p, _l, _p]),
    "syg_fx_tremolo_f32": (_i, [_p, _l, _l, _l, _d, _d, _d, _i, _l, _p, _l, _p]),
    "syg_fx_compress_f32": (_i, [_p, _l, _l, _l, _d, _d, _p, _l, _p]),
    "syg_fx_midside_f32": (_i, [_p, _l, _l, _l, _d, _p, _l, _p]),
    "syg_phase_vocoder_chunk": (_i, []),
    "syg_phase_vocoder_work_bytes": (_l, [_l, _l, _i]),
    "syg_phase_vocoder_f32": (_i, [_p, _l, _l, _p, _p, _l, _p, _p, _i, _p]),
    "syg_fx_add_noise_resident_max": (_l, []),
    "syg_fx_add_noise_work_bytes": (_l, [_l, _l]),
    "syg_fx_add_noise_f32": (_i, [_p, _l, _l, _l, _p, _l, _p, _p, _l, _p, _p]),
    "syg_fx_add_noise_gen_work_bytes": (_l, [_l, _l]),
    "syg_fx_add_noise_gen_f32": (_i, [_p, _l, _l, _l, _u, _l, _p, _p, _l, _p, _p]),
    "syg_laplace_chunk": (_i, []),
    "syg_laplace_tile_rows": (_i, []),
    "syg_laplace_tile_cols": (_i, []),
    "syg_laplace_segment": (_l, []),
    "syg_laplace_steep": (_i, []),
    "syg_laplace_fac_stride": (_i, []),
    "syg_laplace_work_bytes": (_l, [_l, _l, _l, _i]),
    "syg_laplace_f32": (_i, [_p, _l, _l, _l, _p, _p, _p, _p, _l, _l, _l, _l, _l, _d, _p, _p, _i, _p]),
    "syg_resample_tile": (_i, []),
    "syg_resample_table_lds_rule": (_l, []),
    "syg_resample_table_lds_max": (_l, []),
    "syg_resample_table_max": (_l, []),
    "syg_resample_span_max": (_i, []),
    "syg_resample_rate_max": (_i, []),
    "syg_resample_poly_f32": (_i, [_p, _l, _l, _l, _i, _i, _l, _i, _p, _i, _f, _i, _l, _p, _l, _p]),
    "syg_dtw_tile": (_i, []),
    "syg_dtw_tile_max": (_i, []),
    "syg_dtw_resident_max_cols": (_i, []),
    "syg_dtw_run_max": (_i, []),
    "syg_dtw_cost_tile": (_i, []),
    "syg_dtw_form": (_i, [_l, _l, _l, _i]),
    "syg_dtw_work_bytes": (_l, [_l, _l, _l, _i, _i]),
    "syg_dtw_cost_f32": (_i, [_p, _p, _l, _l, _l, _l, _l, _l, _l, _l, _p, _p, _p, _p, _i, _p, _p]),
    "syg_dtw_f32": (_i, [_p, _l, _l, _l, _l, _l, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _l, _p]),
    "syg_cwt_tile": (_i, []),
    "syg_cwt_direct_taps_max": (_i, []),
    "syg_cwt_scales_per_group": (_i, []),
    "syg_cwt_span_max": (_i, []),
    "syg_cwt_taps_lds_max": (_i, []),
    "syg_cwt_work_bytes": (_l, [_l, _l, _l]),
    "syg_cwt_f32": (_i, [_p, _l, _l, _l, _p, _p, _l, _l, _i, _l, _i, _l, _l, _p, _p]),
    "syg_cwt_spectrum_c64": (_i, [_p, _p, _l, _l, _l, _p, _p]),
    "syg_cwt_crop_f32": (_i, [_p, _l, _l, _l, _p, _l, _l, _i, _i, _l, _l, _p, _p]),
    "syg_cepstrum_constants": (_l, [_i]),
    "syg_cepstrogram2048_f32": (_i, [_p, _l, _l, _l, _i, _i, _i, _l, _p, _p, _i, _d, _p, _p]),
    "syg_cepstrum_logmag_c64": (_i, [_p, _l, _l, _l, _d, _p, _p]),
    "syg_cepstrum_gather_f32": (_i, [_p, _l, _l, _l, _l, _d, _p, _p]),
    "syg_cepstrum_unwrap_work_bytes": (_l, [_l, _l]),
    "syg_cepstrum_unwrap_c64": (_i, [_p, _l, _l, _d, _p, _l, _p, _p, _p]),
    "syg_cepstrum_exp_c64": (_i, [_p, _l, _l, _p, _p, _p]),
    "syg_cepstrum_peaks_f32": (_i, [_p, _l, _l, _l, _i, _i, _d, _d, _p, _p, _p, _p, _p]),
    "syg_lpc_constants": (_l, [_i]),
    "syg_lpc_frames_f32": (_i, [_p, _l, _l, _l, _i, _i, _i, _l, _p, _i, _i, _p, _p, _p, _p]),
    "syg_lpc_rows_work_bytes": (_l, [_l, _l, _i, _i]),
    "syg_lpc_rows_f32": (_i, [_p, _l, _l, _l, _p, _i, _i, _p, _l, _p, _p, _p, _p]),
    "syg_lpc_envelope_f32": (_i, [_p, _p, _l, _i, _l, _i, _p, _i, _d, _p, _p]),
    "syg_rng_constants": (_l, [_i]),
    "syg_rng_philox_u32": (_i, [_p, _p, _l, _p, _p]),
    "syg_rng_normal_f32": (_i, [_p, _l, _l, _l, _u, _l, _l, _p]),
    "syg_rng_normal_pairs_c64": (_i, [_p, _l, _l, _u, _l, _p]),
    "syg_rng_power_gain_c64": (_i, [_p, _l, _l, _d, _p]),
    "syg_rng_unpack_pairs_f32": (_i, [_p, _l, _l, _p, _l, _l, _l, _p]),
    "syg_csd_work_bytes": (_l, [_l, _l, _i]),
    "syg_csd_f32": (_i, [_p, _p, _l, _l, _l, _l, _l, _i, _i, _i, _p, _p, _i, _d, _p, _p, _p, _p, _p, _p]),
    "syg_csd_rows_f32": (_i, [_p, _p, _l, _l, _p, _i, _i, _l, _d, _p, _p, _p, _p, _p]),
    "syg_gcc_weight_c64": (_i, [_p, _p, _l, _l, _l, _i, _p, _p]),
    "syg_gcc_crop_f32": (_i, [_p, _l, _l, _l, _p, _p]),
    "syg_peak_pick_f32": (_i, [_p, _l, _l, _l, _l, _d, _p, _p, _p, _p]),
    "syg_dynamics_constants": (_l, [_i]),
    "syg_dynamics_form": (_i, [_l, _l]),
    "syg_dynamics_work_bytes": (_l, [_l, _l, _l]),
    "syg_dynamics_f32": (_i, [_p, _l, _l, _l, _l, _l, _p, _l, _l, _i, _l, _i, _i, _i, _i, _i, _f, _p, _i, _p, _l, _p]),
    "syg_stack_memory_f32": (_i, [_p, _l, _l, _l, _l, _l, _p, _l, _l, _p]),
    "syg_spec_augment_constants": (_l, [_i]),
    "syg_spec_augment_work_bytes": (_l, [_l, _l, _l]),
    "syg_spec_augment_f32": (_i, [_p, _l, _l, _l, _l, _l, _p, _l, _l, _p, _u, _l, _i, _l, _i, _l, _d, _l, _i, _f, _i, _p, _l, _p]),
    "syg_beat_constants": (_l, [_i]),
    "syg_tempogram_tile": (_i, [_i]),
    "syg_tempogram_work_bytes": (_l, [_l, _l, _i, _i]),
    "syg_tempogram_f32": (_i, [_p, _l, _l, _l, _i, _i, _p, _i, _p, _p, _p, _l, _p]),
    "syg_tempo_pick_work_bytes": (_l, [_l]),
    "syg_tempo_pick_f32": (_i, [_p, _p, _l, _i, _l, _p, _l, _l, _p, _p, _p, _p, _p, _p]),
    "syg_beat_local_score_work_bytes": (_l, [_l]),
    "syg_beat_local_score_f32": (_i, [_p, _l, _l, _l, _p, _p, _p, _p, _p]),
    "syg_beat_dp_f32": (_i, [_p, _p, _l, _l, _p, _i, _d, _p, _p, _p, _p]),
    "syg_beat_track_f32": (_i, [_p, _p, _p, _l, _l, _p, _i, _p, _p, _p, _p]),
    "syg_chroma_constants": (_l, [_i]),
    "syg_chroma_fold_rows_f32": (_i, [_p, _l, _l, _i, _i, _i, _p, _i, _i, _f, _i, _p, _p]),
    "syg_chroma_fold_bins_f32": (_i, [_p, _l, _l, _l, _l, _l, _i, _i, _p, _i, _i, _f, _i, _p, _i, _p, _p]),
    "syg_chroma_cens_f32": (_i, [_p, _l, _i, _l, _l, _l, _p, _i, _i, _i, _p, _p]),
    "syg_tuning_hist_work_bytes": (_l, [_l, _l, _i, _i]),
    "syg_tuning_hist_f32": (_i, [_p, _l, _l, _i, _i, _i, _d, _i, _i, _i, _d, _d, _p, _i, _p, _p, _p, _p, _p, _l, _p]),
    "syg_pcen_constants": (_l, [_i]),
    "syg_pcen_form": (_i, [_l, _l, _l]),
    "syg_pcen_work_bytes": (_l, [_l, _l, _l]),
    "syg_pcen_f32": (_i, [_p, _l, _l, _l, _l, _l, _p, _l, _l, _d, _d, _d, _d, _d, _p, _l, _d, _p, _p, _i, _p, _l, _p]),
    "syg_loudness_constants": (_l, [_i]),
    "syg_loudness_segments_work_bytes": (_l, [_l, _l, _l, _i]),
    "syg_loudness_segments_f32": (_i, [_p, _l, _l, _l, _l, _l, _i, _p, _p, _p, _p]),
    "syg_loudness_blocks_f64": (_i, [_p, _l, _l, _l, _i, _p, _p, _l, _p, _l, _p, _p, _p]),
    "syg_loudness_lra_f32": (_i, [_p, _l, _l, _l, _p, _p, _p]),
    "syg_true_peak_f32": (_i, [_p, _l, _l, _l, _l, _l, _i, _l, _i, _p, _p, _p]),
    "syg_loudness_gain_f64": (_i, [_p, _p, _l, _d, _d, _p, _p]),
    "syg_gain_rows_f32": (_i, [_p, _l, _l, _l, _l, _l, _p, _p, _l, _l, _p]),
    "syg_gl_project_work_bytes": (_l, [_l, _l]),
    "syg_gl_project_f32": (_i, [_p, _p, _p, _l, _l, _f, _p, _p, _p, _p]),
    "syg_inv_dense_f32": (_i, [_p, _l, _l, _l, _p, _l, _i, _f, _i, _f, _p, _i, _p]),
    "syg_nmf_constants": (_i, [_i]),
    "syg_nmf_work_bytes": (_l, [_l, _l, _l, _l]),
    "syg_nmf_f32": (_i, [_p, _l, _l, _l, _l, _p, _p, _i, _l, _i, _i, _i, _i, _p, _p]),
    "syg_nmf_divergence_f32": (_i, [_p, _p, _p, _i, _l, _l, _l, _l, _i, _p, _p, _p]),
    "syg_nmf_masks_f32": (_i, [_p, _p, _p, _i, _p, _l, _l, _l, _l, _l, _p, _p]),
    "syg_sim_k_max": (_i, []),
    "syg_sim_knn_work_bytes": (_l, [_l, _l, _l, _i]),
    "syg_sim_knn_f32": (_i, [_p, _p, _l, _l, _l, _l, _l, _l, _l, _l, _p, _p, _l, _l, _i, _p, _p, _p, _p, _p]),
    "syg_sim_dense_f32": (_i, [_p, _p, _p, _l, _l, _l, _l, _i, _i, _i, _p, _p, _p, _p]),
    "syg_nn_filter_f32": (_i, [_p, _l, _l, _l, _l, _l, _p, _p, _l, _p, _p, _i, _p, _p]),
    "syg_repet_masks_f32": (_i, [_p, _p, _l, _d, _d, _d, _p, _p, _p]),
    "syg_viterbi_constants": (_l, [_i]),
    "syg_viterbi_form": (_i, [_l, _l]),
    "syg_viterbi_work_bytes": (_l, [_l, _l, _l]),
    "syg_viterbi_f32": (_i, [_p, _i, _i, _l, _l, _l, _l, _l, _l, _p, _p, _l, _p, _l, _p, _l, _d, _p, _l, _p, _p, _i, _p]),
    "syg_structure_constants": (_l, [_i]),
    "syg_lag_shear_f32": (_i, [_p, _l, _l, _l, _l, _i, _i, _i, _p, _p]),
    "syg_path_enhance_f32": (_i, [_p, _l, _l, _l, _l, _l, _p, _l, _p, _i, _i, _i, _i, _i, _i, _f, _i, _p, _p]),
    "syg_diag_median_f32": (_i, [_p, _l, _l, _l, _l, _i, _i, _i, _i, _f, _p, _p]),
    "syg_agglomerative_work_bytes": (_l, [_l, _l, _l]),
    "syg_agglomerative_f32": (_i, [_p, _l, _l, _l, _l, _l, _p, _p, _p, _l, _l, _l, _p, _p, _p, _l, _p]),
    "syg_segment_sync_f32": (_i, [_p, _l, _l, _l, _l, _l, _p, _l, _l, _i, _p, _p]),
    "syg_kaldi_constants": (_l, [_i]),
    "syg_kaldi_fbank_f32": (_i, [_p, _l, _l, _l, _i, _i, _i, _i, _l, _p, _p, _p, _i, _f, _i, _i, _i, _i, _f, _f, _f, _u, _i, _i, _p, _i, _p,
                                 _l, _l, _l, _p, _l, _l, _l, _p]),
}

_lib = None


class SygnalsHipError(RuntimeError):
    """Raised when the HIP library is missing or a C-ABI call reports an error."""


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SygnalsHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(sygnals_amd has no CPU fallback)")
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)          # AttributeError if the library does not export it
            fn.restype = res
            fn.argtypes = args
        ver = h.syg_abi_version()
        if ver != 1:
            raise SygnalsHipError(f"libsygnals_hip.so ABI version {ver} != 1")
        var = h.syg_build_variant()
        if var != 0 and os.environ.get("SYGNALS_AMD_ALLOW_VARIANT") != str(var):
            raise SygnalsHipError(f"{LIB_PATH} is a development variant (syg_build_variant() = {var}: stamps or ablations, results not for use); "
                                  "rebuild the product library with build_lib.sh")
        _lib = h
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().syg_last_error()
        raise SygnalsHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")
