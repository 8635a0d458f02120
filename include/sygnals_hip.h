/*
 * sygnals_hip.h -- C ABI of libsygnals_hip.so, the MI355X (gfx950) backend for the
 * sygnals windowed-transform / feature-extraction hot path.
 *
 * The reference (araray/sygnals) is pure Python and has no FFI for this path; its
 * boundary is the set of Python functions cited per entry point below (paths are
 * relative to the reference repository).  A binding a maintainer would add is a
 * ctypes stub -- see INTEGRATION.md.  sygnals_amd/_lib.py is that stub for this repo.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in `_host`;
 *   - the caller owns every buffer (inputs, outputs, tables, workspaces); the library
 *     allocates nothing; its only state is a thread-local error string and the process-wide options of
 *     syg_set_option() below (no caches keyed by shape or device: kernel attributes are set at every launch, the
 *     CU count is queried per call).  Nothing is read from the environment;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only
 *     enqueue work on it and never synchronise;
 *   - return value: 0 on success, negative SYG_E_* on error, message via syg_last_error();
 *   - real data is float32, complex data is interleaved float32 (re, im);
 *   - 2-D/3-D arrays are dense row-major with the stated shape unless a leading
 *     dimension (`ld*`, in elements) is given.
 */
#ifndef SYGNALS_HIP_H
#define SYGNALS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SYG_ABI_VERSION 1

#define SYG_OK 0
#define SYG_E_INVALID (-1)   /* bad argument (shape, size, unsupported parameter) */
#define SYG_E_LAUNCH (-2)    /* HIP launch / runtime error */
#define SYG_E_UNSUPPORTED (-3)

int syg_abi_version(void);
/* 0 = product build; non-zero = a development variant (ablation / in-kernel timeline builds, -DSYG_ABL=n) whose
 * results are wrong by design: a binding must refuse to use such a library. */
int syg_build_variant(void);
const char* syg_last_error(void);

/* Process-wide options (atomics; read when a launch is planned).  All but the first select between kernels that the
 * tests hold to the same results and exist for those tests; production code leaves them at their defaults.
 *   SYG_OPT_RESERVED_CUS  n >= 0 (default 0): the persistent syg_stft2048_* kernels leave n CUs out of their grid, for a
 *                         collective (RCCL's send / receive workgroups) running beside them
 *   SYG_OPT_STFT_LOAD     -1 (default: staged tiles) | 0 | 1 | 2: frame load path of the syg_stft2048_* kernels
 *   SYG_OPT_SOS_CLIP      1 (default) | 0: clip-resident form of syg_sosfiltfilt_f32 / the chunked form only
 *   SYG_OPT_CQT_STAGED    -1 (default: where it pays) | 0 (never) | 1 | 2 (also at hop = n_fft / 2): staged form of
 *                         syg_cqt_octave_bf16x3_f32
 *   SYG_OPT_DWT_FORM      1 (default: the clip-resident kernels wherever a row fits) | 0: syg_dwt_f32 / syg_idwt_f32 run
 *                         one launch per level with the approximations through the workspace
 *   SYG_OPT_FX_DELAY_FORM -1 (default: chunked chains where the plain form would leave the device mostly idle) | 0 (one
 *                         lane per residue, always) | 1 (chunked, always): form of syg_fx_delay_f32
 *   SYG_OPT_STFT_FREERUN  -1 (default: the library decides) | 0 (off) | 1 (on where syg_stft2048_mfcc_tri_freerun() holds):
 *                         free-running form of syg_stft2048_mfcc_tri_f32 -- no stage buffer, every wave loads its next frame
 *                         under its projection (how its waves hand a clip over: SYG_OPT_STFT_MEET).  An explicit
 *                         SYG_OPT_STFT_LOAD >= 0 turns the -1 default off
 *   SYG_OPT_STFT_MEET     -1 (default: the library decides) | 0 | 1: how the free-running form hands a finished clip to its
 *                         dB + DCT epilogue, and the clip's LDS matrix back.  1: one workgroup barrier per clip.  0: no barrier
 *                         inside the tile loop -- counters in LDS that only grow; a wait on one is a bounded poll, and a bound
 *                         that runs out turns the clip's output into NaN.  Same bits either way; no effect where the
 *                         free-running form does not run
 * syg_set_option returns SYG_OK or SYG_E_INVALID (unknown key / value out of range); syg_get_option the current value. */
#define SYG_OPT_RESERVED_CUS 0
#define SYG_OPT_STFT_LOAD 1
#define SYG_OPT_SOS_CLIP 2
#define SYG_OPT_CQT_STAGED 3
#define SYG_OPT_DWT_FORM 4
#define SYG_OPT_FX_DELAY_FORM 5
#define SYG_OPT_STFT_FREERUN 6
#define SYG_OPT_STFT_MEET 7
#define SYG_OPT_COUNT 8
int syg_set_option(int key, int value);
int syg_get_option(int key);

/* The launch caps every family shares, -1 for an unknown key.  More rows than SYG_LAUNCH_MAX_GRID_Y are looped over, split
 * into launches or refused, as each entry states; a persistent grid has at most the stated workgroups per CU and its
 * kernel loops over the rest. */
enum {
  SYG_LAUNCH_MAX_GRID_Y = 0,               /* rows of a grid's y dimension */
  SYG_LAUNCH_LPC_FRAMES_WGS_PER_CU = 1,    /* syg_lpc_frames_f32 */
  SYG_LAUNCH_LPC_ENVELOPE_WGS_PER_CU = 2,  /* syg_lpc_envelope_f32 */
  SYG_LAUNCH_PITCH_FRAMES_WGS_PER_CU = 3,  /* syg_pitch_frames_f32 */
  SYG_LAUNCH_NOISE_WGS_PER_CU = 4          /* syg_fx_add_noise_f32, syg_fx_add_noise_gen_f32 */
};
int64_t syg_launch_constants(int which);

/* ---------------------------------------------------------------------------------
 * Fused headline path: framed STFT (n_fft = 2048) -> |X|^2 -> mel filterbank.
 * Replaces, per clip, librosa.stft + np.abs + **2 + librosa.feature.melspectrogram as
 * called at sygnals/core/features/manager.py:184-187, 198, 219-222.
 *
 *   y          [B, L] float32, row stride ldy            (clips)
 *   window     [2048] float32  periodic analysis window (already centre-padded)
 *   twiddle    [2048] complex  W_2048^k = exp(-2*pi*i*k/2048)
 *   wpacked    packed block-sparse mel weights for v_mfma_f32_4x4x1_16b_f32 (sygnals_amd/_tables.py: pack_mel_plan):
 *              [wave][steps / 4][64 lanes][4] A operands (lane l of step i: basis[4 g + (l & 3)][k0 + i] of its slot
 *              l >> 4), then >= 6 groups of zero rows (every wave pre-loads 6 groups unconditionally), then four
 *              int32 tables of 64 entries at float offset table_off: first bin of slot (wave * 4 + s), mel group of the
 *              slot, first slot of group g, slot count of group g (slots of a group are consecutive, ascending bins)
 *   plan_host  HOST int32[5]: {2 (layout), n_waves (8 or 16), steps (multiple of 4), n_groups = ceil(n_mels / 4) <= 64,
 *              table_off}
 *   mel_out    [B, n_mels, T] float32 mel POWER spectrogram
 *   stats_out  optional [B, SYG_NSTAT, T] float32 per-frame spectral statistics
 *              (NULL to skip), rows in SYG_STAT_* order; only the rows selected by stats_mask
 *              (SYG_SM_* bits) are computed and written; replaces the per-frame loop
 *              manager.py:304-316 over frequency_domain.py:24-386
 *   contrast   optional: cplan_host HOST int32[1 + 3*SYG_MAX_BANDS] {n_rows, lo[], hi[], k[]}
 *              and contrast_out [B, 2, n_rows, T] (peak, valley means; NULL to skip);
 *              replaces the band loop of librosa.feature.spectral_contrast reached from
 *              frequency_domain.py:200-207
 *   T          number of frames, = 1 + L/hop (center) or 1 + (L-2048)/hop
 * ------------------------------------------------------------------------------- */
#define SYG_NSTAT 8
#define SYG_STAT_CENTROID 0
#define SYG_STAT_BANDWIDTH 1
#define SYG_STAT_FLATNESS 2
#define SYG_STAT_ROLLOFF_BIN 3
#define SYG_STAT_DOMINANT_BIN 4
#define SYG_STAT_MAG_SUM 5
#define SYG_STAT_POWER_SUM 6
#define SYG_STAT_ROLLOFF_MARGIN 7
#define SYG_MAX_BANDS 16
#define SYG_SM_CENTROID 1   /* also MAG_SUM */
#define SYG_SM_BANDWIDTH 2
#define SYG_SM_FLATNESS 4
#define SYG_SM_ROLLOFF 8    /* also POWER_SUM, ROLLOFF_MARGIN */
#define SYG_SM_DOMINANT 16
#define SYG_SM_NO_MARGIN 32 /* with SYG_SM_ROLLOFF: the ROLLOFF_MARGIN row is not computed (callers that only read the bin) */

int syg_stft2048_mel_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center, int64_t T,
                         const float* window, const float* twiddle, const float* wpacked,
                         const int32_t* plan_host, int n_mels, float* mel_out,
                         float sr, float roll_percent, float bw_p, int stats_mask, float* stats_out,
                         const int32_t* cplan_host, float* contrast_out, void* stream);

/* Same front end, complex STFT output (librosa.stft as called by compute_stft,
 * sygnals/core/dsp.py:167-229).  out [B, T, 1025] complex64, FRAME-major. */
int syg_stft2048_c2c_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center, int64_t T,
                         const float* window, const float* twiddle, float* out, void* stream);

/* ---------------------------------------------------------------------------------
 * Whole MFCC chain in one launch (the headline path): librosa.stft -> |.|^2 -> mel filterbank ->
 * power_to_db(ref=np.max, top_db) -> DCT-II rows (+ lifter), i.e. manager.py:184-187, 198, 219-223 and
 * cepstral.py:106-115.  A workgroup owns whole clips; the clip's [n_mels, T] mel matrix stays in LDS, so
 * only the samples are read from and the MFCCs written to HBM.
 *   y .. n_mels   as syg_stft2048_mel_f32 (the plan must be a 16-wave plan)
 *   dct        [n_mfcc, n_mels] DCT matrix rows;  lifter: optional [n_mfcc] (NULL = none)
 *   amin, top_db (< 0: no clamp), ref_is_max (1: per-clip max, 0: ref_value): as syg_logmel_dct_f32
 *   mel_out    optional [B, n_mels, T] copy of the mel POWER (NULL = not stored)
 *   mfcc_out   [B, n_mfcc, T]
 * Fails (SYG_E_ARG) when n_mels * 16*ceil(T/16) floats do not fit the LDS left beside the transform buffers: ~21 KiB
 * beside the tile stage buffer (e.g. n_mels=40: T <= 128 frames), ~60 KiB in its place -- the launch then loads its frames
 * straight from global memory (n_mels=128: T <= 112); callers otherwise use the two-launch form
 * syg_stft2048_mel_f32 + syg_logmel_dct_f32.
 * ------------------------------------------------------------------------------- */
/* 0: the shape does not fit the one-launch form; 2: it fits beside the stage buffer; 1: in the stage buffer's place */
int syg_stft2048_mfcc_fits(int n_mels, int64_t T, int n_mfcc);
int syg_stft2048_mfcc_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center,
                          int64_t T, const float* window, const float* twiddle, const float* wpacked,
                          const int32_t* plan_host, int n_mels, const float* dct, int n_mfcc,
                          const float* lifter, float amin, float top_db, int ref_is_max, float ref_value,
                          float* mel_out, float* mfcc_out, void* stream);

/* The same chain for TRIANGULAR filterbanks (librosa.filters.mel as manager.py:198 / cepstral.py:106 build it), the mel
 * projection by SEGMENT SUMS: between two band edges the weights of the rising and of the falling band are affine in
 * the bin index, so a run of bins contributes a T0 + b T1 (T0 = sum p, T1 = sum i p) -- each wave projects its own
 * power row, no weight matrix is read and the projection needs no workgroup barrier.
 *   segtab     device, 16-byte aligned: the piece table of sygnals_amd._tables.pack_mel_segments, [2][2][64][4] words
 *              (n_segtab = 1024); filterbanks whose pieces do not fit 128 lane slots have no table -- use the matrix form
 *   other arguments as syg_stft2048_mfcc_f32 (no mel copy: the matrix form stores one)
 * Needs TWO mel matrices in LDS (the dB + DCT of a clip runs beside the next clip's first tile):
 * syg_stft2048_mfcc_tri_fits() says whether a shape fits. */
int syg_stft2048_mfcc_tri_fits(int n_mels, int64_t T, int n_mfcc);
/* 1: the free-running form of syg_stft2048_mfcc_tri_f32 (SYG_OPT_STFT_FREERUN) can load these clips: hop, L and ldy even,
 * y 8-byte aligned, L < 2^28.  Host-side arithmetic only (y is not dereferenced); the launch uses it itself. */
int syg_stft2048_mfcc_tri_freerun(int hop, int64_t L, int64_t ldy, const float* y);
int syg_stft2048_mfcc_tri_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center,
                              int64_t T, const float* window, const float* twiddle, const float* segtab,
                              int n_segtab, int n_mels, const float* dct, int n_mfcc, const float* lifter,
                              float amin, float top_db, int ref_is_max, float ref_value, float* mfcc_out,
                              void* stream);

/* The statistics / contrast rows of syg_stft2048_mel_f32 AND the clip-resident MFCC of syg_stft2048_mfcc_tri_f32 from ONE
 * launch: extract_features(["mfcc", "spectral_centroid", "spectral_rolloff", "spectral_contrast"]) (BASELINE config C4,
 * manager.py:289-371) with only the samples read and the feature rows written -- the mel matrix never reaches HBM.
 * Arguments as in those two entry points (at least one of stats_out / contrast_out).  The MFCC rows of clip b go to
 * mfcc_out + (b * mfcc_rows_per_clip) * T: with mfcc_rows_per_clip > n_mfcc they are the head of a wider per-clip block
 * whose other rows syg_feature_block_f32(mel = NULL, ...) fills.  Shapes that fit: syg_stft2048_mfcc_tri_fits(). */
int syg_stft2048_features_tri_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center, int64_t T,
                                  const float* window, const float* twiddle, const float* segtab, int n_segtab,
                                  int n_mels, const float* dct, int n_mfcc, const float* lifter, float amin,
                                  float top_db, int ref_is_max, float ref_value, float sr, float roll_percent,
                                  float bw_p, int stats_mask, float* stats_out, const int32_t* cplan_host,
                                  float* contrast_out, float* mfcc_out, int mfcc_rows_per_clip, void* stream);

/* The TILE form of the segment-sum projection: samples in, mel POWER out; replaces librosa.stft + np.abs + **2 +
 * librosa.feature.melspectrogram (manager.py:184-187, 198, 219-222) like syg_stft2048_mel_f32, without a weight matrix and
 * without the projection's barriers.  Optional statistics / contrast rows as in syg_stft2048_mel_f32 (manager.py:289-343).
 * Any hop; tiles are shared out evenly over the CUs.
 *   segtab    device, 16-byte aligned.  n_segtab = 2048: sygnals_amd._tables.pack_mel_segments(sr, 2048, n_mels, fmin, fmax,
 *             n_pass=4, row_base=4), [4][2][64][4] 32-bit words -- up to 256 pieces: the reference's default of 128 bands
 *             (sygnals/core/features/manager.py:214; `sygnals features extract -f mfcc`, cli/features_cmd.py:82-90, always
 *             runs it), 64 ... 200 bands at the usual rates.  n_segtab = 1024: the two-pass table of
 *             syg_stft2048_mfcc_tri_f32 (up to 128 pieces, e.g. 40 bands)
 *   waves     16 (one workgroup per CU) or 8 (two per CU)
 *   mel_out   [B, n_mels, T]; stats_out / cplan_host / contrast_out as in syg_stft2048_mel_f32 (NULL to skip) */
int syg_stft2048_mel_tri_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center, int64_t T,
                             const float* window, const float* twiddle, const float* segtab, int n_segtab, int n_mels,
                             float* mel_out, float sr, float roll_percent, float bw_p, int stats_mask, float* stats_out,
                             const int32_t* cplan_host, float* contrast_out, int waves, void* stream);

/* The per-frame statistics / contrast tail means of syg_stft2048_mel_f32 WITHOUT the mel spectrogram: spectral_centroid /
 * bandwidth / flatness / rolloff / contrast (manager.py:289-343 -> frequency_domain.py:25-212) only need |X|.  The kernel of
 * syg_stft2048_features_tri_f32 with nothing projected and no clip epilogue; same stats_mask / stats_out [B, SYG_NSTAT, T] /
 * cplan_host / contrast_out [B, 2, n_rows, T] as syg_stft2048_mel_f32, results bit-identical to it.  hop <= 512. */
int syg_stft2048_stats_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center, int64_t T,
                           const float* window, const float* twiddle, float sr, float roll_percent, float bw_p,
                           int stats_mask, float* stats_out, const int32_t* cplan_host, float* contrast_out,
                           void* stream);

/* frame_length 4096 (librosa.stft + np.abs(.)**2 + melspectrogram, manager.py:184-187, 198, 219-222): samples in, mel power
 * out, one wave per frame (the 4096-point real transform of syg_welch_f32's wave kernel), the mel projection by segment
 * sums as in syg_stft2048_mfcc_tri_f32 with a FOUR-pass piece table (pack_mel_segments(..., n_pass=4): 2048 words).
 *   y [B, L] (row stride ldy), window [4096] device (16-byte aligned), twiddle: W_4096^k for k = 0 .. 4095
 *   mel_out [B, n_mels, T] */
int syg_stft_mel_w4096_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center, int64_t T,
                           const float* window, const float* twiddle, const float* segtab, int n_segtab, int n_mels,
                           float* mel_out, void* stream);

/* frame_length 1024 (the reference's own tests and CLI: tests/test_features_manager.py:183-220, cli/features_cmd.py:35),
 * power 2: samples in, mel power out, free-running waves -- a wave owns two frames per 1024-point complex transform and
 * projects its two power rows by segment sums (no weight matrix, no workgroup barrier per tile).  segtab: the two-row
 * table of sygnals_amd._tables.pack_mel_segments_rows(sr, 1024, n_mels, fmin, fmax) (2048 words, 16-byte aligned).
 * window [1024], twiddle: W_1024^k for k = 0 .. 1023; mel_out [B, n_mels, T].  Other powers and filterbanks without a
 * table: syg_stft_mel_pow2_f32. */
int syg_stft_mel_w1024_seg_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center, int64_t T,
                               const float* window, const float* twiddle, const float* segtab, int n_segtab, int n_mels,
                               float* mel_out, void* stream);

/* syg_stft_mel_w1024_seg_f32 with the per-frame statistics / contrast rows of syg_stft2048_mel_f32 from the same launch
 * (bins 0 .. 512, bin frequency k sr / 1024): extract_features(frame_length=1024, [spectral features ...]) -- the call of
 * the reference's own manager tests (tests/test_features_manager.py:58-62, 167-174; manager.py:289-343 over
 * frequency_domain.py:24-386) -- without a spectrogram in HBM.  stats_out [B, SYG_NSTAT, T] (rows selected by stats_mask)
 * and / or cplan_host + contrast_out [B, 2, n_rows, T]: at least one.  The mel block is optional: segtab == NULL and
 * mel_out == NULL compute the rows alone. */
int syg_stft_rows_w1024_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center, int64_t T,
                            const float* window, const float* twiddle, const float* segtab, int n_segtab, int n_mels,
                            float* mel_out, float sr, float roll_percent, float bw_p, int stats_mask, float* stats_out,
                            const int32_t* cplan_host, float* contrast_out, void* stream);

/* The same for frame_length 512 and 256 (256: the reference's short-signal tests): a wave owns four / eight frames per
 * transform and projects its four / eight power rows.  segtab: pack_mel_segments_rows(sr, n_fft, n_mels, fmin, fmax,
 * rows=4, row_words=296 (512) / 160 (256), n_pass=1, block=16 (512) / 8 (256)) (2048 words); twiddle: W_1024^k for k = 0 .. 1023. */
int syg_stft_mel_wseg_small_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int n_fft, int hop, int center,
                                int64_t T, const float* window, const float* twiddle, const float* segtab,
                                int n_segtab, int n_mels, float* mel_out, void* stream);

/* The per-frame statistics / contrast rows of syg_stft2048_mel_f32 for frame lengths 512 and 256 (bins 0 .. n_fft / 2, bin
 * frequency k sr / n_fft) from the transform of syg_stft_mel_wseg_small_f32, nothing projected: extract_features(
 * frame_length=512 | 256, [spectral features]) -- 256 is the frame length of the reference's short-signal tests
 * (tests/test_features_manager.py:183-220; manager.py:289-343 over frequency_domain.py:24-386) -- without a spectrogram in
 * HBM.  stats_out [B, SYG_NSTAT, T] (rows selected by stats_mask) and / or cplan_host + contrast_out [B, 2, n_rows, T]:
 * at least one.  window [n_fft]; twiddle: W_1024^k, k = 0 .. 1023. */
int syg_stft_rows_wsmall_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int n_fft, int hop, int center, int64_t T,
                             const float* window, const float* twiddle, float sr, float roll_percent, float bw_p,
                             int stats_mask, float* stats_out, const int32_t* cplan_host, float* contrast_out, void* stream);

/* The same rows for frame length 4096 (2049 bins, bin frequency k sr / 4096) from the launch of syg_stft_mel_w4096_f32
 * (one wave per frame): extract_features(frame_length=4096, [spectral features (+ mfcc)]) -- manager.py:289-343 over
 * frequency_domain.py:24-386 -- without a spectrogram in HBM.  stats_out [B, SYG_NSTAT, T] (rows selected by stats_mask)
 * and / or cplan_host + contrast_out [B, 2, n_rows, T]: at least one; with segtab (2048 words, as for
 * syg_stft_mel_w4096_f32) and mel_out [B, n_mels, T] also the mel power block, with segtab NULL nothing is projected.
 * window [4096]; twiddle: W_4096^k, k = 0 .. 4095. */
int syg_stft_rows_w4096_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center, int64_t T,
                            const float* window, const float* twiddle, const float* segtab, int n_segtab, int n_mels,
                            float* mel_out, float sr, float roll_percent, float bw_p, int stats_mask, float* stats_out,
                            const int32_t* cplan_host, float* contrast_out, void* stream);

/* ---------------------------------------------------------------------------------
 * power_to_db + DCT-II (+ lifter): librosa.power_to_db(S_mel, ref=np.max) at
 * manager.py:223 and librosa.feature.mfcc(S=..) at cepstral.py:106-115.
 *   mel        [B, M, T] mel power; converted to dB IN PLACE unless logmel_out given
 *   dct        [K, M] DCT matrix rows (orthonormal DCT-II rows for the default)
 *   lifter     optional [K] multiplicative lifter (NULL = none)
 *   ref_is_max 1: ref = max over the clip's [M, T] (ref=np.max); 0: ref = ref_value;
 *              2: `mel` already holds dB values (mfcc(S=log_mel)): DCT only, mel untouched
 *   top_db     < 0 disables the clamp
 *   mfcc_out   [B, K, T]  (NULL: only the dB conversion)
 * ------------------------------------------------------------------------------- */
int syg_logmel_dct_f32(float* mel, int64_t B, int M, int64_t T, const float* dct, int K,
                       const float* lifter, float amin, float top_db, int ref_is_max, float ref_value,
                       float* logmel_out, float* mfcc_out, void* stream);
/* MFCCs alone (librosa.feature.mfcc(S=power_to_db(S_mel, ref=np.max)), cepstral.py:106-115 behind manager.py:223): as above,
 * but the dB matrix is written nowhere when the clip's matrix fits the LDS; `mel` is scratch for the call. */
int syg_mel_mfcc_f32(float* mel, int64_t B, int M, int64_t T, const float* dct, int K, const float* lifter, float amin,
                     float top_db, int ref_is_max, float ref_value, float* mfcc_out, void* stream);

/* ---------------------------------------------------------------------------------
 * Generic batched power-of-two FFT in LDS (n = 2^k, 2 <= n <= 8192): scipy.fft.fft /
 * ifft as called by compute_fft / compute_ifft, sygnals/core/dsp.py:104, 151.
 *   in/out   [batch, n] complex64 (may alias); inverse != 0 scales by 1/n
 *   twiddle  [n] complex W_n^k = exp(-2*pi*i*k/n)
 * ------------------------------------------------------------------------------- */
int syg_fft_pow2_c2c_f32(const float* in, float* out, int64_t batch, int n, int inverse,
                         const float* twiddle, void* stream);

/* Strided form used to compose transforms longer than 8192 points (four-step) and Bluestein
 * for arbitrary n (scipy.fft.fft(x, n) accepts any n, dsp.py:104).  Element e of transform
 * (o, b) is at in[o*in_os + b*in_bs + e*in_es] (complex elements); if bign > 0 output k of
 * transform b is multiplied by W_bign^(b*k); every output is multiplied by `scale`.  in != out. */
int syg_fft_pow2_strided_c2c_f32(const float* in, float* out, int64_t outer, int64_t batch, int n, int inverse,
                                 const float* twiddle, int64_t in_os, int64_t in_bs, int64_t in_es,
                                 int64_t out_os, int64_t out_bs, int64_t out_es, int64_t bign, float scale,
                                 void* stream);

/* The same for lengths n = 2^a 3^b 5^c 7^d <= 8192 (mixed-radix Stockham: one second of audio at 48 / 44.1 / 16 kHz is
 * such a length, none a power of two); twiddle [n] = W_n^k.  syg_fft_mixed_plan returns the number of passes (0: n has
 * another prime factor -> Bluestein) and, if radices_host is given, their radices.  Longer 7-smooth lengths are
 * composed four-step from two such transforms by the caller, exactly like the power-of-two case. */
int syg_fft_mixed_plan(int64_t n, int32_t* radices_host, int max_passes);
int syg_fft_mixed_strided_c2c_f32(const float* in, float* out, int64_t outer, int64_t batch, int n, int inverse,
                                  const float* twiddle, int64_t in_os, int64_t in_bs, int64_t in_es,
                                  int64_t out_os, int64_t out_bs, int64_t out_es, int64_t bign, float scale,
                                  void* stream);
/* The two strided transforms with FUSED ENDS (the analytic signal / envelope of scipy.signal.hilbert as transforms.py:119-151
 * and dsp.py:565-636 call it, without its three element-wise passes):
 *   flags & 1 (SYG_FFT_REAL_IN)   `in` is a REAL array (same element indexing), imaginary part 0
 *   flags & 2 (SYG_FFT_ABS_OUT)   `out` is a REAL array that receives |result|
 *   flags & 4 (SYG_FFT_PAIR_IN)   `in` is a REAL array read as the complex sequence (x[2 p], x[2 p + 1]), zero from sample
 *                                 in_valid on; in_os is then the row stride in floats (the packed real-input transform of
 *                                 syg_rconv_spectrum_c64's convolutions without a packing pass)
 *   mask_n > 0                    every loaded element is multiplied by the analytic-signal weight of its position p inside
 *                                 the row (the row is a length-mask_n spectrum): 1 at p = 0 and 2 p = mask_n, 2 for
 *                                 2 p < mask_n, 0 above */
int syg_fft_pow2_strided_ex_f32(const float* in, float* out, int64_t outer, int64_t batch, int n, int inverse,
                                const float* twiddle, int64_t in_os, int64_t in_bs, int64_t in_es, int64_t out_os,
                                int64_t out_bs, int64_t out_es, int64_t bign, float scale, int flags, int64_t mask_n,
                                int64_t in_valid, void* stream);
int syg_fft_mixed_strided_ex_f32(const float* in, float* out, int64_t outer, int64_t batch, int n, int inverse,
                                 const float* twiddle, int64_t in_os, int64_t in_bs, int64_t in_es, int64_t out_os,
                                 int64_t out_bs, int64_t out_es, int64_t bign, float scale, int flags, int64_t mask_n,
                                 int64_t in_valid, void* stream);

/* out[i] = a[i] * b[i mod nb] (complex64; conj_b != 0 multiplies by conj(b)); may be in place. */
int syg_cmul_c64(const float* a, const float* b, float* out, int64_t na, int64_t nb, int conj_b, void* stream);

/* Real rows -> zero-padded / truncated complex rows with an optional window (apply_window,
 * dsp.py:641-691, then the implicit pad/truncate of fft(x, n)): out [rows, n] complex64. */
int syg_pack_real_c64(const float* x, int64_t rows, int64_t len, int64_t ldx, const float* window, float* out,
                      int64_t n, void* stream);

/* Generic framed STFT for any power-of-two n_fft in [8, 16384] (slow path of
 * compute_stft and of extract_features for frame lengths other than 2048).
 *   twiddle [n_fft + n_fft/2] complex: W_nfft^k (k < n_fft) followed by W_{nfft/2}^k
 *   out [B, T, 1 + n_fft/2] complex64, frame-major. */
int syg_stft_pow2_c2c_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int n_fft, int hop, int center,
                          int64_t T, const float* window, const float* twiddle, float* out, void* stream);

/* Elementwise helpers on frame-major spectra: out[i] = |X[i]|^power (power 1 or 2). */
int syg_cabs_pow_f32(const float* x_c64, int64_t n, int power, float* out, void* stream);

/* Dense mel projection for the generic path: mel[b, m, t] = sum_f basis[m, f] * P[b, t, f]. */
int syg_mel_dense_f32(const float* P, int64_t B, int64_t T, int F, const float* basis, int M,
                      float* mel_out, void* stream);

/* ---------------------------------------------------------------------------------
 * Fused front end for the OTHER power-of-two frame lengths (n_fft = 64 ... 1024; the reference's own tests and CLI use
 * 1024 and 256: tests/test_features_manager.py:183-220, cli/features_cmd.py:35): librosa.stft -> |.|^power -> mel
 * filterbank in one launch, no spectrogram in HBM (manager.py:184-187, 198, 219-222).
 *   y .. window   as syg_stft_pow2_c2c_f32;  twiddle [n_fft + n_fft/2] complex (W_nfft^k, then W_{nfft/2}^k), for
 *              n_fft = 512 and 256 followed by W_1024^k (1024 entries: four / eight frames share one 1024-point wave
 *              transform)
 *   basis_p    [16*ceil(n_mels/16), Fp] the dense filterbank, zero padded: Fp = (1 + n_fft/2) rounded up to a multiple
 *              of 16; 16-byte aligned
 *   power      1 (magnitude) or 2 (power)
 *   mel_out    [B, n_mels, T]
 * ------------------------------------------------------------------------------- */
int syg_stft_mel_pow2_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int n_fft, int hop, int center,
                          int64_t T, const float* window, const float* twiddle, const float* basis_p, int Fp,
                          int n_mels, int power, float* mel_out, void* stream);

/* The whole MFCC chain for those frame lengths in one launch (a workgroup owns a clip, the clip's mel matrix stays in
 * LDS): ... -> power_to_db(ref=np.max, top_db) -> DCT-II rows (+ lifter) (manager.py:223, cepstral.py:106-115).
 * Arguments as syg_stft_mel_pow2_f32 (power 2) + those of syg_stft2048_mfcc_f32.  syg_stft_mfcc_pow2_fits() says
 * whether the clip's mel matrix fits the LDS; when not, use syg_stft_mel_pow2_f32 + syg_logmel_dct_f32. */
int syg_stft_mfcc_pow2_fits(int n_fft, int n_mels, int64_t T, int n_mfcc);
int syg_stft_mfcc_pow2_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int n_fft, int hop, int center,
                           int64_t T, const float* window, const float* twiddle, const float* basis_p, int Fp,
                           int n_mels, const float* dct, int n_mfcc, const float* lifter, float amin, float top_db,
                           int ref_is_max, float ref_value, float* mel_out, float* mfcc_out, void* stream);

/* Per-frame spectral statistics of frame-major magnitude spectra mag [N, F] with bin
 * frequencies freqs [F] (frequency_domain.py:24-386).  stats_out [SYG_NSTAT, N]. */
int syg_spectral_stats_f32(const float* mag, int64_t N, int F, const float* freqs, float roll_percent,
                           float bw_p, float* stats_out, void* stream);

/* Spectral-contrast peak/valley means of frame-major magnitude spectra mag [N, F]:
 * for each band row r: mean of the k[r] smallest / largest values of bins lo[r]..hi[r]-1.
 *   out [2, n_rows, N] (peak then valley). */
int syg_contrast_pv_f32(const float* mag, int64_t N, int F, const int32_t* cplan_host, float* out, void* stream);

/* contrast[b, r, t] = power_to_db(peak) - power_to_db(valley) (ref 1, amin, top_db clamp per
 * [R, T] matrix), the last step of librosa.feature.spectral_contrast (frequency_domain.py:200-207).
 *   pv [B, 2, R, T] (peak, valley) -> out [B, R, T]; top_db < 0 disables the clamp;
 *   amin <= 0 selects librosa's linear=True: out = peak - valley. */
int syg_contrast_db_f32(const float* pv, int64_t B, int R, int64_t T, float amin, float top_db, float* out,
                        void* stream);

/* ---------------------------------------------------------------------------------
 * Zero-phase SOS filtering: scipy.signal.sosfiltfilt(sos, x) (padtype='odd') as called by
 * apply_sos_filter, sygnals/core/filters.py:85-115.
 *   x, y        [B, L] float32 (row strides ldx, ldy); y may alias x
 *   sos_host    HOST float64 [n_sections, 6]
 *   zi_host     HOST float64 [n_sections, 2]  sosfilt_zi(sos)
 *   padlen      edge extension length (3*ntaps rule), must be < L
 *   work        device workspace of syg_sosfiltfilt_work_bytes(B, L, padlen, n_sections) bytes; that is 0 for
 *               clips the clip-resident form takes (L + 2 padlen <= 65536, <= 4 sections): work may then be NULL
 * ------------------------------------------------------------------------------- */
int64_t syg_sosfiltfilt_work_bytes(int64_t B, int64_t L, int padlen, int n_sections);
int syg_sosfiltfilt_f32(const float* x, int64_t B, int64_t L, int64_t ldx, const double* sos_host,
                        const double* zi_host, int n_sections, int padlen, float* y, int64_t ldy,
                        void* work, void* stream);

/* ---------------------------------------------------------------------------------
 * Causal SOS filtering with state in and out: y, zf = scipy.signal.sosfilt(sos, x, zi=zi) per row.  Direct form II
 * transposed; recurrences and states float64, signals float32.
 *   x, y        [B, L] float32 (row strides ldx, ldy), L >= 1, any B; y may alias x
 *   sos_host    HOST float64 [n_sections, 6], 1 <= n_sections <= 32 (more than 8 run as consecutive groups of 8, each
 *               group filtering y in place)
 *   zi          DEVICE float64 [B, n_sections, 2], scipy's (z0, z1) per section, or NULL = zero state
 *   zf          DEVICE float64 [B, n_sections, 2]: the state behind sample L - 1, i.e. the next block's zi; or NULL.
 *               zf must not alias zi
 *   work        device workspace of syg_sosfilt_work_bytes(B, L, n_sections) bytes (-1: not served)
 *               = 2 * min(B, 65535) * (n + ceil(n / ahead)) * 2 * min(n_sections, 8) * 8 with n = ceil(L / chunk); rows of
 *               at most one chunk do not touch it (work may then be NULL)
 * The chunk in which the float64 recurrence is cut and rejoined is a function of the sample index alone, so a result
 * does not depend on a row's address or on the batch it is part of.
 * syg_sosfilt_constants(k): 0 samples per chunk, 1 samples per tile, 2 chunks per wave, 3 chunk states the scan keeps
 * in flight (ahead), 4 sections per group, 5 sections per call, 6 chunks of a row above which the scan over the chunks
 * runs in segments (three short launches instead of one long one); -1 for another k.
 * ------------------------------------------------------------------------------- */
int64_t syg_sosfilt_constants(int which);
int64_t syg_sosfilt_work_bytes(int64_t B, int64_t L, int n_sections);
int syg_sosfilt_f32(const float* x, int64_t B, int64_t L, int64_t ldx, const double* sos_host, int n_sections,
                    const double* zi, float* y, int64_t ldy, double* zf, void* work, void* stream);

/* ---------------------------------------------------------------------------------
 * Welch PSD: scipy.signal.welch(..., return_onesided=True) as called by
 * compute_psd_welch, sygnals/core/dsp.py:545-555.  nfft power of two in [8, 16384],
 * nperseg <= nfft.  twiddle as for syg_stft_pow2_c2c_f32 ([nfft + nfft/2] complex).
 *   x        [B, L] float32
 *   window   [nperseg] float32
 *   detrend  0 none, 1 constant (per-segment mean removal), 2 linear (per-segment least-squares line,
 *            scipy.signal.detrend type='linear')
 *   scale    density: 1/(fs*sum(w^2)); spectrum: 1/sum(w)^2   (computed by the caller)
 *   psd_out  [B, 1 + nfft/2] float32 ; partial sums in work (syg_welch_work_bytes)
 * ------------------------------------------------------------------------------- */
int64_t syg_welch_work_bytes(int64_t B, int nfft);
int syg_welch_f32(const float* x, int64_t B, int64_t L, int64_t ldx, int nperseg, int step, int nfft,
                  const float* window, const float* twiddle, int detrend, double scale, float* psd_out,
                  void* work, void* stream);

/* ---------------------------------------------------------------------------------
 * BASELINE config C4's per-clip feature block in one launch behind syg_stft2048_mel_f32 (mel + centroid + rolloff +
 * contrast tail means): block_out [B, K + 2 + R, T] float32 with rows
 *   0 .. K-1      MFCC = DCT rows x power_to_db(mel, ref = max of the clip, amin, top_db)   (manager.py:219-223,
 *                 cepstral.py:106-115; the dB matrix stays in LDS: M * T * 4 bytes <= 150 KiB)
 *   K, K + 1      spectral centroid (Hz), spectral rolloff (Hz = bin x binhz)              (manager.py:304-316)
 *   K + 2 ..      spectral contrast dB rows from contrast_pv [B, 2, R, T] (peak, valley)    (frequency_domain.py:200-207)
 * -- the columns extract_features(["mfcc", "spectral_centroid", "spectral_rolloff", "spectral_contrast"]) returns, in
 * order: the [B/W, 22, 94] block a rank contributes to config C4's gather.  stats: [B, SYG_NSTAT, T].
 * mel == NULL (dct may then be NULL too): rows 0 .. K-1 are left as they are -- syg_stft2048_features_tri_f32 has
 * written the MFCCs there -- and only the statistics / contrast rows are filled.
 * ------------------------------------------------------------------------------- */
int syg_feature_block_f32(const float* mel, int64_t B, int M, int64_t T, const float* dct, int K, float amin,
                          float top_db, const float* stats, float binhz, const float* contrast_pv, int R,
                          float c_amin, float c_top_db, float* block_out, void* stream);

/* ---------------------------------------------------------------------------------
 * Time-domain frame features, one value per frame:
 *   rows 0..6: mean |x|, population std, skewness (scipy.stats.skew bias=False), excess kurtosis
 *              (scipy.stats.kurtosis fisher, bias=False), max |x|, crest factor, Shannon entropy of
 *              np.histogram(frame, num_bins) -- sygnals/core/features/time_domain.py:23-227 applied per frame
 *              of the zero-padded signal by manager.py:264-286
 *   row 7:     RMS energy  -- core/audio/features.py:73-131 (librosa.feature.rms, zero padding)
 *   row 8:     zero-crossing rate -- core/audio/features.py:26-71 (librosa.feature.zero_crossing_rate,
 *              edge padding, threshold 1e-10)
 *   y [B, L] float32 (row stride ldy); T as syg_stft2048_mel_f32's framing rule with n_fft = frame_length;
 *   mask: bit r selects row r (unselected rows are left untouched);  out [B, SYG_NFSTAT, T] float32.
 * syg_rms_from_spec_f32: librosa.feature.rms(S=...) for rows of magnitudes S [rows, F] -> out [rows].
 * ------------------------------------------------------------------------------- */
#define SYG_NFSTAT 9
int syg_frame_stats_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int frame_length, int hop,
                        int center, int64_t T, int num_bins, int mask, float* out, void* stream);
int syg_rms_from_spec_f32(const float* S, int64_t rows, int F, int frame_length, float* out, void* stream);

/* ---------------------------------------------------------------------------------
 * Pitch: librosa 0.10 yin / pyin as called by fundamental_frequency, sygnals/core/audio/features.py:135-220 (jitter
 * :319 and shimmer :412 call it when no f0 / voiced_flag is given).  Parity is unpinned (librosa is not a dependency):
 * the float64 restatement of tests/pitch_ref.py is the contract; the host constants come from sygnals_amd/_pitch.py.
 * syg_pitch_frames_f32: one wave per frame, frame_length = 2048 only (SYG_E_UNSUPPORTED otherwise), any
 *   1 <= win_length < 2048, any hop; center pads frame_length / 2 zeros on each side.  Lags min_period .. max_period
 *   (n_lag = max_period - min_period + 1), 1 <= min_period < max_period <= frame_length - win_length - 1.
 *   twiddle      [2048] complex W_2048^k
 *   mode 0 (yin) f0_out [B, T]: sr / (min_period + idx + parabolic shift), idx = first trough under trough_threshold,
 *                else the first global minimum
 *   mode 1 (pyin) per frame a candidate list of stride K >= ceil(n_lag / 2) + 1: cand_bin int32 / cand_prob float32
 *                [B, T, K], cand_count [B, T] (bins distinct and < n_bins, in lag order), voiced_prob [B, T];
 *                ptab: float64 table of sygnals_amd/_pitch.py (thresholds, beta probabilities, no-trough masses,
 *                Boltzmann factors); fmin / n_bins define the 10-cent pitch grid
 *   cmndf_out    [B, T, n_lag] float32 or NULL: the cumulative mean normalised difference the decisions are taken on
 * syg_pyin_viterbi_f32: one workgroup per clip over the 2 n_bins pYIN states.  Consumes candidate lists as above
 *   (bins must be distinct within a frame) and voiced_prob; ltab: [2, n_rows, 2 half_width + 1] float64
 *   log(p T + tiny) of the stay (p = 0.99) and switch blocks, rows as _pitch.transition_tables(); lconst_host: HOST
 *   float64 {log(tiny), log p_init voiced, log p_init unvoiced}.  Writes f0_out (NaN where unvoiced), voiced_out
 *   (0 / 1) and state_out (may be NULL) [B, T]; backpointers in work (syg_pyin_work_bytes(B, T, n_bins) bytes).
 * ------------------------------------------------------------------------------- */
int syg_pitch_frames_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int frame_length, int win_length, int hop,
                         int center, int64_t T, double sr, int min_period, int max_period, int mode,
                         double trough_threshold, double fmin, int n_bins, const double* ptab, int K,
                         const float* twiddle, float* f0_out, int* cand_bin, float* cand_prob, int* cand_count,
                         float* voiced_prob, float* cmndf_out, void* stream);
int64_t syg_pyin_work_bytes(int64_t B, int64_t T, int n_bins);
int syg_pyin_viterbi_f32(const int* cand_bin, const float* cand_prob, const int* cand_count, const float* voiced_prob,
                         int64_t B, int64_t T, int K, int n_bins, int half_width, const double* ltab, int n_rows,
                         const double* lconst_host, double fmin, void* work, int64_t work_bytes, float* f0_out,
                         uint8_t* voiced_out, int* state_out, void* stream);

/* ---------------------------------------------------------------------------------
 * HPSS: librosa 0.10 effects.hpss (kernel_size 31, margins, power) as called by harmonic_to_noise_ratio,
 * sygnals/core/audio/features.py:225-316, after the complex STFT of syg_stft2048_c2c_f32 (D [B, T, 1025] complex,
 * frame-major).  Parity is unpinned (librosa is not a dependency): the float64 restatement of tests/hpss_ref.py is the
 * contract.
 * syg_hpss_masks_f32: S = |D| computed as __fsqrt_rn(__fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im))) with IEEE
 *   round-to-nearest at every step, no FMA (a host test rebuilds it bit for bit).  H = median over time (window win_harm) per bin, P = median over bins (window win_perc)
 *   per frame, scipy.ndimage.median_filter semantics: window [i - k/2, i - k/2 + k - 1], element of rank k/2 (the upper
 *   median for even k), indices folded by half-sample symmetric reflection as often as needed.  1 <= win <= 63 each.
 *   mask_harm = softmask(H, P margin_harm), mask_perc = softmask(P, H margin_perc) [B, T, 1025] float32 (util.softmask:
 *   Z = max(X, X_ref), Z < FLT_MIN -> 0.5 when both margins are 1, else 0; power = +inf -> X > X_ref).
 *   power > 0 (finite or +inf), margins >= 1.  harm_out / perc_out [B, T, 1025] or NULL: the medians H / P.
 * syg_istft2048_f32: librosa.istft(D masked, n_fft 2048, hop 512, center, length) -> y [B, length] (row stride ldy).
 *   window: [2048] float64, a periodic window (w[s] = w[2048 - s]: only w[0 .. 1024] is read; hann for every
 *   reference call path), twiddle: [2048] complex W_2048^k.  Frames
 *   min(T, ceil((length + 2048) / 512)); each is window * irfft (Im of bins 0 and 1024 ignored), overlap-added in frame
 *   order, the first 1024 samples trimmed, divided by the float64 window sum-square (rounded once) where it exceeds
 *   FLT_MIN.  mask_a / mask_b [B, T, 1025] float32 multiply D on load (mask_a NULL: the plain istft into y_a); a second
 *   component (mask_b, y_b) runs in the same launch, its waves beside the first's so that the reads of D meet in
 *   cache.  No atomics: the result is bit-identical from run to run.  hop != 512 or center != 1: SYG_E_UNSUPPORTED.
 * syg_hnr_rows_f32: frames of frame_length at hop (center pads frame_length / 2 zeros on each side; T frames, the
 *   framing rule of librosa.feature.rms) of y_harm / y_perc [B, L] (row stride ldy).  Frame powers P = rms^2, rms =
 *   sqrt(mean x^2) in float64; hnr_out [B, T] = 10 log10(P_h / P_p) where both exceed 1e-10, +80 / -80 where only
 *   P_h / P_p does, NaN otherwise.  rms_harm_out / rms_perc_out [B, T] or NULL.
 * ------------------------------------------------------------------------------- */
int syg_hpss_masks_f32(const float* D, int64_t B, int64_t T, int win_harm, int win_perc, double power,
                       double margin_harm, double margin_perc, float* mask_harm, float* mask_perc, float* harm_out,
                       float* perc_out, void* stream);
int syg_istft2048_f32(const float* D, int64_t B, int64_t T, int hop, int center, int64_t length, const double* window,
                      const float* twiddle, const float* mask_a, float* y_a, const float* mask_b, float* y_b,
                      int64_t ldy, void* stream);
int syg_hnr_rows_f32(const float* y_harm, const float* y_perc, int64_t B, int64_t L, int64_t ldy, int frame_length,
                     int hop, int center, int64_t T, float* hnr_out, float* rms_harm_out, float* rms_perc_out,
                     void* stream);

/* ---------------------------------------------------------------------------------
 * Audio effects: sygnals/core/audio/effects/ (delay.py, tremolo.py, compression.py, reverb.py, utility.py).  Rows are
 * [B, L] float32 with a row stride (ld*, in elements); `out` may alias `x` in every entry of this block.  No atomics: the
 * results are bit-identical from run to run.  The float64 restatement of tests/effects_ref.py is the contract (the two
 * spectral effects rest on librosa, which is not a dependency; the others are pinned to the reference's own output).
 * syg_fx_delay_f32: apply_delay (delay.py:15-111) with D = delay_samples >= 1: w[n] = x[n] + feedback w[n - D],
 *   out[n] = dry x[n] + wet w[n - D], w = 0 at negative indices; D >= L is legal (out = dry x).  0 <= feedback < 1 (also
 *   after rounding to float32).  The output expression is __fadd_rn(__fmul_rn(dry, x), __fmul_rn(wet, w)), no FMA: at
 *   feedback = 0 the result is exactly dry x[n] + wet x[n - D] in float32.  One lane per residue n mod D walks its chain;
 *   where that would leave the device mostly idle (B min(D, L) under 256 lanes per CU) and a chain has at least
 *   4 syg_fx_delay_chunk() steps, the chains are cut into chunks of syg_fx_delay_chunk() steps whose carries are scanned by
 *   the same recurrence with feedback^chunk; that form needs `work`, syg_fx_delay_work_bytes(B, L, D) bytes (0 otherwise:
 *   work may be NULL; -1 for a bad shape).  apply_chorus (chorus.py:24-156) computes this with
 *   D = ceil((delay + depth) sr) + 2: its interpolation point lies left of its grid, so its LFO has no effect.
 * syg_spectral_gate_f32: the gain of noise_reduction_spectral (utility.py:59-131) on the STFTs of syg_stft2048_c2c_f32:
 *   D [B, T, 1025] complex of the clip, Dn [B, Tn, 1025] complex of its first noise_samples samples.
 *   noise [B, 1025] float32 (always written) = mean over the Tn frames of re^2 + im^2, summed in float64;
 *   gain [B, T, 1025] float32 = sqrt(max(0, 1 - (amount noise) / P)), P = __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im))
 *   of D; 0 where P == 0, never NaN.  gain D is the reference's sqrt(max(0, |D|^2 - amount noise)) exp(i angle D):
 *   pass it to syg_istft2048_f32 as mask_a.  amount >= 0, finite.
 * syg_fx_mix_f32: out[r, n] = a x[r, n] + b y[r, n], n < L; x reads as 0 from Lx on and y from Ly on; y may be NULL
 *   (out = a x: adjust_gain, utility.py:22-55).  The dry / wet mix of apply_reverb over the longer wet signal, and
 *   transient_shaping_hpss's harmonic + scale percussive.
 * syg_fx_tremolo_f32: apply_tremolo (tremolo.py:55-111): out = x ((1 - depth) + depth lfo(n0 + n)), the LFO in float64
 *   on the device, phase = ((2 pi) rate) ((n0 + n) / sr) in that order; SYG_LFO_SINE (sin + 1) / 2, SYG_LFO_TRIANGLE
 *   (scipy.signal.sawtooth(phase, 0.5) + 1) / 2, SYG_LFO_SQUARE 1 where sin(phase) > 0, else 0.  The product is formed in
 *   float64 and rounded once.  rate > 0, 0 <= depth <= 1, sr > 0, n0 >= 0 (the index of the row's first sample).
 * syg_fx_compress_f32: simple_dynamic_range_compression (compression.py:14-64): where |x| > threshold,
 *   x (threshold + (|x| - threshold) / ratio) / |x| (float64, rounded once), elsewhere x bit for bit.  ratio >= 1.
 * syg_fx_midside_f32: stereo_widening_midside (utility.py:188-253) on x [B, 2, L] (row 2 b + c at (2 b + c) ldx):
 *   mid = (l + r) / 2, side = width (l - r) / 2, out = (mid + side, mid - side).  width >= 0.
 * ------------------------------------------------------------------------------- */
#define SYG_LFO_SINE 0
#define SYG_LFO_TRIANGLE 1
#define SYG_LFO_SQUARE 2
int syg_fx_delay_chunk(void);
int64_t syg_fx_delay_work_bytes(int64_t B, int64_t L, int64_t delay_samples);
int syg_fx_delay_f32(const float* x, int64_t B, int64_t L, int64_t ldx, int64_t delay_samples, double feedback, double dry,
                     double wet, float* out, int64_t ldo, void* work, void* stream);
int syg_spectral_gate_f32(const float* D, int64_t B, int64_t T, const float* Dn, int64_t Tn, double amount, float* gain,
                          float* noise, void* stream);
int syg_fx_mix_f32(const float* x, int64_t Lx, int64_t ldx, const float* y, int64_t Ly, int64_t ldy, int64_t B, int64_t L,
                   double a, double b, float* out, int64_t ldo, void* stream);
int syg_fx_tremolo_f32(const float* x, int64_t B, int64_t L, int64_t ldx, double sr, double rate, double depth, int shape,
                       int64_t n0, float* out, int64_t ldo, void* stream);
int syg_fx_compress_f32(const float* x, int64_t B, int64_t L, int64_t ldx, double threshold, double ratio, float* out,
                        int64_t ldo, void* stream);
int syg_fx_midside_f32(const float* x, int64_t B, int64_t L, int64_t ldx, double width, float* out, int64_t ldo,
                       void* stream);

/* ---------------------------------------------------------------------------------
 * Onset detection: librosa 0.10 onset.onset_strength / util.peak_pick / onset.onset_detect as called by detect_onsets,
 * sygnals/core/audio/features.py:555-619, after any mel front end (mel POWER [B, M, T], T contiguous), and the clip
 * totals of get_basic_audio_metrics (:508-551).  Parity is unpinned (librosa is not a dependency): the float64
 * restatement of tests/onset_ref.py is the contract.
 * syg_onset_strength_f32: S = power_to_db(mel, ref 1.0, amin, top_db relative to the clip's own maximum; top_db < 0:
 *   no clip), never written out.  d[t] = mean_m max(0, S[m, t + lag] - R[m, t]), t < T - lag, R = S (max_size 1) or
 *   the maximum of S over mel rows [m - max_size / 2, m - max_size / 2 + max_size - 1] (scipy.ndimage.maximum_filter1d).
 *   env [B, T_out]: `pad` zeros, then d, cut or zero-filled to T_out <= pad + T; detrend != 0 then applies
 *   lfilter([1, -1], [1, -0.99]) along each row.  The mel mean is a fixed-order sum: bit-identical from run to run.
 *   Clips of more than 2048 frames are split over workgroups and need `work`, syg_onset_strength_work_bytes(B, M, T)
 *   bytes (0 for shorter clips: work may be NULL).  lag >= 1, lag < T, max_size >= 1, amin > 0.
 * syg_onset_peaks_f32: env [B, T] (row stride ld, shared by energy).  normalize != 0: x = (env - min) / (max - min +
 *   FLT_MIN) per clip.  Frame n is a candidate when x[n] is the maximum of x[max(0, n - pre_max) : min(T, n + post_max)],
 *   x[n] >= mean(x[max(0, n - pre_avg) : min(T, n + post_avg)]) + delta (a direct float64 sum over the window) and
 *   x[n] != 0; candidates are kept left to right, each only if n > last + wait.  backtrack != 0 moves each onset to the
 *   nearest i at or before it with e[i] <= e[i - 1] and e[i] < e[i + 1] (frame 0 always qualifies), e = energy or, when
 *   NULL, env.  An all-zero or non-finite clip has no onsets.  frames [B, T] int32: the kept frames in ascending order,
 *   -1 beyond them; count [B] int32.  No atomics.  Windows and wait >= 0, post_max >= 1, post_avg >= 1, delta finite
 *   and >= 0.  The cost is T (pre_max + post_max + pre_avg + post_avg) loads per clip.
 * syg_clip_metrics_f32: y [B, L] (row stride ldy) -> out [B, 2] float32: sum of y^2 (float64 partial sums, fixed-order
 *   tree, rounded once) and max |y|.
 * ------------------------------------------------------------------------------- */
int64_t syg_onset_strength_work_bytes(int64_t B, int M, int64_t T);
int syg_onset_strength_f32(const float* mel, int64_t B, int M, int64_t T, float amin, float top_db, int lag,
                           int max_size, int pad, int64_t T_out, int detrend, float* env, void* work, void* stream);
int syg_onset_peaks_f32(const float* env, int64_t B, int64_t T, int64_t ld, int pre_max, int post_max, int pre_avg,
                        int post_avg, double delta, int wait, int normalize, int backtrack, const float* energy,
                        int32_t* frames, int32_t* count, void* stream);
int syg_clip_metrics_f32(const float* y, int64_t B, int64_t L, int64_t ldy, float* out, void* stream);

/* ---------------------------------------------------------------------------------
 * Constant-Q transform building blocks: librosa.cqt as called by compute_cqt,
 * sygnals/core/dsp.py:276-284 (recursive per-octave algorithm; the host composes the octaves).
 *   syg_decimate2_f32   y[b, n] = scale * sum_j taps[j] * x[b, 2n + (ntaps-1)/2 - j], n < ceil(L/2)
 *                       (zero outside the signal) -- the decimation between octaves
 *   syg_cqt_octave_f32  rectangular-window centred STFT frame (n_fft = 2^k, 8 ... 1024; hop) of y [B, L],
 *                       times the frequency-domain basis [n_filt, n_fft/2+1] complex64 ->
 *                       out[b * out_bstride + (row0 + f) * T + t] complex64; hull_host (host int32
 *                       [2 * n_filt], may be NULL = dense): first non-zero bin and run length of every
 *                       basis row (librosa sparsifies the basis; only the run is multiplied); twiddle as for
 *                       syg_stft_pow2_c2c_f32 ([n_fft + n_fft/2] complex)
 * ------------------------------------------------------------------------------- */
int syg_decimate2_f32(const float* x, int64_t B, int64_t L, int64_t ldx, const float* taps, int ntaps, float scale,
                      float* y, int64_t ldy, void* stream);
 /* syg_decimate2_chain_f32: `levels` (1..4) successive decimations in one pass; y / ldy are HOST arrays of `levels`
 *   device pointers / row strides, level s of length ceil(L / 2^(s+1)); an entry of y may be NULL when that level is
 *   not wanted (41 taps only; the last level is always written).  Bit-identical to `levels` calls of
 *   syg_decimate2_f32: with the CQT's 41-tap filter a workgroup carries its tile through all levels in LDS, so every
 *   level is written once and only x is read (the recursive octave walk of librosa.cqt, core/dsp.py:276-284, needs
 *   every level).  */
int syg_decimate2_chain_f32(const float* x, int64_t B, int64_t L, int64_t ldx, const float* taps, int ntaps, float scale,
                            int levels, float* const* y, const int64_t* ldy, void* stream);
 /* syg_cqt_octave_gemm_f32: the same octave as ONE framed matrix product on the matrix cores (n_fft 128 / 256 / 512):
 *   out[f, t] = sum_n y[t hop - n_fft/2 + n] * g_f[n],  g_f[n] = sum_k basis[f, k] exp(-2 pi i k n / n_fft)
 *   (the frequency-domain rows taken to the time domain by the caller, in float64 -- the same linear map).
 *   gpacked float32 [row tile][n_fft/16][4][64]: A operands of v_mfma_f32_16x16x4_f32, row r = 2 f + (0: re, 1: im):
 *   entry (mt, s, u, lane) = G[16 s + 4 (lane >> 4) + u][16 mt + (lane & 15)] (0 past 2 n_filt rows).  */
int syg_cqt_octave_gemm_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int n_fft, int hop, int64_t T,
                            const float* gpacked, int n_filt, float* out, int64_t out_bstride, int row0, void* stream);
 /* syg_cqt_octave_bf16x3_f32: the same product with both operands split into three bfloat16 terms and the six products
 *   above 2^-24 accumulated in fp32 on v_mfma_f32_16x16x32_bf16 (fp32-equivalent: error <= 3 x 2^-24 |a b| per product,
 *   parity tests at 1e-5 like the fp32 form; 3/8 of its matrix-pipe time).  n_fft 128 / 256, n_filt <= 16.
 *   gsplit: bfloat16 [3 terms hi, mid, lo][row tile][n_fft/32][64 lanes][8]: entry (p, mt, s, lane, j) = term p of
 *   float32(G[32 s + 8 (lane >> 4) + j][16 mt + (lane & 15)]); 16-byte aligned.  */
int syg_cqt_octave_bf16x3_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int n_fft, int hop, int64_t T,
                              const void* gsplit, int n_filt, float* out, int64_t out_bstride, int row0, void* stream);

/* The whole transform of compute_cqt (sygnals/core/dsp.py:231-289) in ONE launch for its usual shape -- hop_length 512, one
 * early decimation, n_oct <= 7 octaves of n_filt <= 16 filters at frame length 256 and hop 256 >> o that share one operand
 * table (below): the stream is read once, every decimation level
 * lives in LDS only (syg_decimate2_chain_f32 + n_oct x syg_cqt_octave_bf16x3_f32 write and re-read them through HBM), the
 * same values to the rounding of the float32 sums (the decimator's symmetric taps are paired, the products' k range is
 * summed in four parts).  taps: the 41-tap half-band decimator (zero at the even offsets from its centre, symmetric);
 * scale: sqrt(2); row0_host[n_oct]: first output row of octave o; out [B, n_bins, T] complex (float pairs),
 * out_bstride in complex elements, T <= the smallest centred frame count over the octaves (1 + L_o / hop_o).
 * gsplit: the layout of syg_cqt_octave_bf16x3_f32's table at n_fft 256 with ALWAYS two row tiles, whatever n_filt is --
 * bfloat16 [3 terms][2 row tiles][8 steps][64 lanes][8] = 24576 16-bit words (48 KiB), 16-byte aligned; rows past 2 n_filt
 * (the whole second tile when n_filt <= 8) are zero (sygnals_amd.ops.cqt_fused_table).  The level-by-level entry above
 * reads ONE row tile when n_filt <= 8: the two tables differ there. */
int syg_cqt_fused_f32(const float* y, int64_t B, int64_t L, int64_t ldy, const float* taps, int ntaps, float scale,
                      const void* gsplit, int n_filt, int n_oct, const int32_t* row0_host, int64_t T, float* out,
                      int64_t out_bstride, void* stream);
int syg_cqt_octave_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int n_fft, int hop, int64_t T,
                       const float* twiddle, const float* basis, int n_filt, const int32_t* hull_host,
                       float* out, int64_t out_bstride, int row0, void* stream);

/* ---------------------------------------------------------------------------------
 * FFT-backed 1-D operations; the host composes them with the power-of-two complex FFT above.
 *   syg_pack_rows_f32       (row stride ldx may be smaller than len: overlapping rows = frames of one signal)
 *                           out[r, i] = (x[r, j] - mean_r) * window[i] for i < min(len, n), 0 up to n;
 *                           j = reverse ? len-1-i : i; detrend 0 none, 1 mean_r, 2 least-squares line (float64 sums, need `work` of
 *                           syg_pack_rows_work_bytes(rows) bytes); cplx != 0 writes complex rows (value, 0).
 *                           A real row of n floats is at the same time the packed row z[m] = x[2m] + i x[2m+1]
 *                           of n/2 complex elements consumed by syg_rconv_spectrum_c64.
 *   syg_rconv_spectrum_c64  za [rows, H], zb [rows_b (1 or rows), H] (any H >= 2): length-H complex FFTs of two packed real
 *                           rows of 2H samples -> out [rows, H] (may alias za): the packed transform of their
 *                           circular convolution; its inverse length-H FFT, read as 2H floats, is the real
 *                           result.  scipy.signal.fftconvolve / correlate as called at sygnals/core/dsp.py:333,
 *                           :388 (correlation = convolution with the reversed second input).
 *   syg_analytic_mask_c64   in place X[r, k] *= h[k], h = scipy.signal.hilbert's mask (1, 2.., [1], 0..)
 *                           -- sygnals/core/transforms.py:146, sygnals/core/dsp.py:609
 *   syg_psd_onesided_f32    out[r, k] = scale * |X[r, k]|^2 * (1 for DC and the even-n Nyquist bin, else 2),
 *                           k <= n/2, from the full spectrum X [rows, n] -- scipy.signal.periodogram as called
 *                           at sygnals/core/dsp.py:484-492
 *   syg_col_mean_f32        acc[k] (float64 [F], caller-owned) = (first ? 0 : acc[k]) + sum_r in[r, k]; on the `last`
 *                           call out[k] = acc[k] / divisor: the average of per-segment periodograms for Welch with
 *                           a segment length that is not a power of two (segments = overlapping rows, row stride
 *                           ldx = nperseg - noverlap, through syg_pack_rows_f32 -> FFT -> syg_psd_onesided_f32)
 * ------------------------------------------------------------------------------- */
int64_t syg_pack_rows_work_bytes(int64_t rows);
int syg_pack_rows_f32(const float* x, int64_t rows, int64_t len, int64_t ldx, const float* window, int detrend,
                      int reverse, int cplx, float* out, int64_t n, void* work, void* stream);
/* syg_pack_rows_f32 for the frames of several clips at once: row r starts at
 * x + (r / rows_per_group) * group_stride + (r % rows_per_group) * ldx  (rows_per_group = 0: x + r * ldx). */
int syg_pack_frames_f32(const float* x, int64_t rows, int64_t len, int64_t ldx, int64_t rows_per_group,
                        int64_t group_stride, const float* window, int detrend, int reverse, int cplx, float* out,
                        int64_t n, void* work, void* stream);
int syg_rconv_spectrum_c64(const float* za, const float* zb, int64_t rows, int64_t rows_b, int64_t H, float* out,
                           void* stream);
int syg_analytic_mask_c64(float* X, int64_t rows, int64_t n, void* stream);
int syg_psd_onesided_f32(const float* X, int64_t rows, int64_t n, double scale, float* out, void* stream);
int syg_col_mean_f32(const float* in, int64_t rows, int64_t F, double* acc, int first, int last, double divisor,
                     float* out, void* stream);

/* ---------------------------------------------------------------------------------
 * Batched audio ingest: integer PCM frames as stored in a WAV file -> float32 mono clips, after the
 * host-to-device copy (half the PCIe bytes of float32 for 16-bit audio).  Replaces librosa.load's conversion
 * reached through sygnals/core/audio/io.py:84-90 (scale 2^-(bits-1), mono = mean over channels) and the mix-down of
 * sygnals/cli/features_cmd.py:66-68.
 *   pcm   [rows, frames, channels] interleaved; int16 (bits 16), int32 (bits 32; 24-bit files left-justified),
 *         uint8 (bits 8, offset 128); row stride ld in ELEMENTS
 *   out   [rows, frames] float32, row stride ldo:  out[r, i] = mean_c pcm[r, i, c] / 2^(bits-1)
 * ------------------------------------------------------------------------------- */
int syg_pcm_to_f32(const void* pcm, int bits, int64_t rows, int64_t frames, int channels, int64_t ld, float* out,
                   int64_t ldo, void* stream);

/* ---------------------------------------------------------------------------------
 * Feature formatting for ML on the device.  x is a [n, F] float32 matrix (frames x features);
 * statistics are float64 and NaN-aware like scikit-learn's fit (NaNs ignored; all-NaN column -> NaN).
 *   syg_col_stats_f32      out [5, F] float64: count, mean, population variance, min, max per column -- the fit
 *                          of StandardScaler / MinMaxScaler, sygnals/core/ml_utils/scaling.py:108-118
 *   syg_affine_cols_f32    out[r, c] = (x[r, c] - sub[c]) * mul[c] + add[c] (float64 arithmetic): every scaler's
 *                          transform, scaling.py:118, 133
 *   syg_col_quantiles_f32  out [nq, F] float64 = np.nanpercentile(x, 100 q, axis=0) (linear interpolation), q in
 *                          [0, 1]; n <= 32768 -- RobustScaler's centre and scale, scaling.py:114
 *   syg_zoom_f32           scipy.ndimage.zoom(img [H, W], order 0 | 1, mode='nearest') to [H2, W2] --
 *                          format_features_as_image, sygnals/core/ml_utils/formatters.py:296-316
 * ------------------------------------------------------------------------------- */
int syg_col_stats_f32(const float* x, int64_t n, int64_t F, double* out, void* stream);
int syg_affine_cols_f32(const float* x, int64_t n, int64_t F, const double* sub, const double* mul, const double* add,
                        float* out, void* stream);
int syg_col_quantiles_f32(const float* x, int64_t n, int64_t F, const double* q, int nq, double* out, void* stream);
int syg_zoom_f32(const float* img, int H, int W, int H2, int W2, int order, float* out, void* stream);

/* ---------------------------------------------------------------------------------
 * Discrete wavelet transform: pywt.wavedec / pywt.waverec (PyWavelets 1.x) as called at sygnals/core/transforms.py:74
 * and :110, for orthogonal filter banks of F = 2 ... 20 taps (F even; sygnals_amd/_wavelets.py computes the Daubechies
 * family) and the signal extension modes below.  One level of a length-N input gives (N + F - 1) / 2 coefficients:
 *     cA[o] = sum_j dec_lo[j] ext(x)[2 o + 1 - j],  cD[o] likewise with dec_hi;
 * one synthesis level of K pairs gives 2 K - F + 2 samples,
 *     y[n] = sum_k a[k] rec_lo[n + F - 2 - 2 k] + d[k] rec_hi[n + F - 2 - 2 k].
 * All arithmetic is float32, every sum a chain of fused multiply-adds in a fixed order.
 *
 *   syg_dwt_lengths      lens_host [levels + 1] (HOST) <- the wavedec order [cA_n, cD_n, ..., cD_1]; returns their sum
 *                        (the packed row length), -1 on error
 *   syg_dwt_fits         1: the clip-resident form (one workgroup a clip, all levels in one launch, the running
 *                        approximation in LDS) takes rows of L samples; 0: the streaming form (one level a pass until
 *                        the rest fits).  The rule: the first two approximations fit 160 KiB of LDS
 *   syg_dwt_work_bytes   workspace of the streaming form (0 when the row is resident or levels = 1), -1 on error
 *   syg_dwt_f32          x [B, L] (row stride ldx), dec_lo / dec_hi [F] float32 DEVICE arrays -> out [B, total] (row
 *                        stride ldout): one packed row a clip, [cA_n | cD_n | ... | cD_1] with the lengths of
 *                        syg_dwt_lengths
 *   syg_idwt_length      output length that follows from lens_host (HOST, [levels + 1], the same order): at each level
 *                        the approximation must be as long as the detail or one longer (its last sample is dropped, as
 *                        pywt.waverec does), and a level needs at least F / 2 pairs; -1 on inconsistent lens
 *   syg_idwt_work_bytes  workspace of syg_idwt_f32 for these lens (0 when every level is resident), -1 on error
 *   syg_idwt_f32         coeffs [B, sum(lens)] (row stride ldc) in the packed layout, rec_lo / rec_hi [F] float32 DEVICE
 *                        arrays -> y [B, syg_idwt_length] (row stride ldy)
 * ------------------------------------------------------------------------------- */
#define SYG_DWT_ZERO 0
#define SYG_DWT_CONSTANT 1
#define SYG_DWT_SYMMETRIC 2
#define SYG_DWT_REFLECT 3
#define SYG_DWT_PERIODIC 4
int64_t syg_dwt_lengths(int64_t L, int F, int levels, int64_t* lens_host);
int syg_dwt_fits(int64_t L, int F, int levels);
int64_t syg_dwt_work_bytes(int64_t B, int64_t L, int F, int levels);
int syg_dwt_f32(const float* x, int64_t B, int64_t L, int64_t ldx, const float* dec_lo, const float* dec_hi, int F,
                int mode, int levels, float* out, int64_t ldout, void* work, void* stream);
int64_t syg_idwt_length(const int64_t* lens_host, int levels, int F);
int64_t syg_idwt_work_bytes(int64_t B, const int64_t* lens_host, int levels, int F);
int syg_idwt_f32(const float* coeffs, int64_t B, int64_t ldc, const int64_t* lens_host, int levels, const float* rec_lo,
                 const float* rec_hi, int F, float* y, int64_t ldy, void* work, void* stream);

/* ---------------------------------------------------------------------------------
 * Augmentation: the phase vocoder of librosa.effects.time_stretch (sygnals/core/audio/effects/time_stretch.py:15-48,
 * sygnals/core/augment/effects_based.py:60-99) and add_noise (sygnals/core/augment/noise.py:19-101).
 *
 * syg_phase_vocoder_f32: librosa 0.10 core.phase_vocoder between syg_stft2048_c2c_f32 and syg_istft2048_f32.
 *   D [B, T, 1025, 2] frame-major -> out [B, T_out, 1025, 2].  col [T_out] int32 and alpha [T_out] float64 are DEVICE
 *   arrays, the step table of step = np.arange(0, T, rate): col[t] = int(step_t), alpha[t] = step_t mod 1
 *   (sygnals_amd/_tables.vocoder_steps).  Per (clip, bin), in the order t = 0 .. T_out - 1:
 *       out[t] = ((1 - alpha[t]) |D[col[t]]| + alpha[t] |D[col[t] + 1]|) p,   then p <- p u(D[col[t] + 1]) conj(u(D[col[t]])),
 *   p = u(D[0]) at t = 0, u(z) = z / |z| formed in float64 (no magnitude of float32 parts under- or overflows) and
 *   u(0) = (copysign(1, re), 0), which is exp(i np.angle(z)) for a bin stored as -0 + 0j as well; p is float64.  That is
 *   librosa's phase accumulator modulo 2 pi without atan2 / sincos.  A column outside [0, T) reads as zero (librosa pads
 *   two), so no table makes the kernel read outside D.
 *   form: -1 the rule | 0 the chain form (one lane per (clip, bin) walks every step) | 1 the chunked form (steps cut into
 *   chunks of syg_phase_vocoder_chunk(), the chunks' products scanned into chunk-start phasors; it reads D twice).  The
 *   rule takes the chunked form where the chain form has fewer than eight waves a CU (17 B < 8 CUs) and T_out >= 4
 *   chunks.  The chunked form needs `work`, syg_phase_vocoder_work_bytes(B, T_out, form) bytes, 16-byte aligned (0
 *   otherwise: `work` may be NULL).  The two forms agree to the rounding of the float64 products.
 *
 * syg_fx_add_noise_f32: y [B, L], noise [B, L] (row strides ldy, ldn), snr_db [B] float64 DEVICE array -> out [B, L] (may
 *   alias y).  Per row Ps = mean(y^2), Pn = mean(noise^2) in float64, sums in a fixed order; Ps or Pn below the float64
 *   epsilon: the row is copied bit for bit; otherwise out = y + noise sqrt((Ps / 10^(snr_db / 10)) / Pn), formed in
 *   float64 and rounded once.  L <= syg_fx_add_noise_resident_max(): one launch, a workgroup keeps its row in LDS between
 *   the sums and the mix.  Longer rows: two launches (slice sums, then the mix) and `work` of
 *   syg_fx_add_noise_work_bytes(B, L) bytes, 16-byte aligned.
 *
 * syg_fx_add_noise_gen_f32: the same mix on noise that is never stored: noise[b, n] is the standard normal
 *   (seed, row first_row + b, sample n) of syg_rng_normal_f32 (below), generated in registers.  Rows first_row ..
 *   first_row + B - 1 must lie in [0, 2^31).  L <= syg_fx_add_noise_resident_max(): one launch, y alone is kept in LDS
 *   (8 bytes a sample, every normal drawn once).  Longer rows: a power pass and a mix pass that both generate (12 bytes
 *   a sample), the power pass in as many slices as fill the device; between them one wave a row adds the slices in a
 *   fixed order (runs of consecutive slices, the runs in order) and leaves the row's scale factor; `work` of
 *   syg_fx_add_noise_gen_work_bytes(B, L) bytes, 16-byte aligned.  The result is within one float32 ulp of
 *   syg_fx_add_noise_f32 on the stored noise (the sums are taken in another order).
 * ------------------------------------------------------------------------------- */
int syg_phase_vocoder_chunk(void);
int64_t syg_phase_vocoder_work_bytes(int64_t B, int64_t T_out, int form);
int syg_phase_vocoder_f32(const float* D, int64_t B, int64_t T, const int32_t* col, const double* alpha, int64_t T_out,
                          float* out, void* work, int form, void* stream);
int64_t syg_fx_add_noise_resident_max(void);
int64_t syg_fx_add_noise_work_bytes(int64_t B, int64_t L);
int syg_fx_add_noise_f32(const float* y, int64_t B, int64_t L, int64_t ldy, const float* noise, int64_t ldn,
                         const double* snr_db, float* out, int64_t ldo, void* work, void* stream);
int64_t syg_fx_add_noise_gen_work_bytes(int64_t B, int64_t L);
int syg_fx_add_noise_gen_f32(const float* y, int64_t B, int64_t L, int64_t ldy, uint64_t seed, int64_t first_row,
                             const double* snr_db, float* out, int64_t ldo, void* work, void* stream);

/* ---------------------------------------------------------------------------------
 * Numerical Laplace transform (sygnals/core/transforms.py:159-199), an arbitrary-point z-transform:
 *     out[b, i] = t_step sum_{n < L} x[b, n] exp(-s_i n t_step),   x [B, L] float32 (row stride ldx) -> out [B, S, 2] float64.
 * Gate: |out - float64 formula| <= 1e-5 |t_step| sum_n |x[b, n]| exp(-Re(s_i) n t_step).  Same call, same bits (no atomics).
 *
 * The s-values reach the library as DEVICE tables built on the host in float64 (sygnals_amd/_laplace.plan builds them;
 * the kernels trust them, so these are preconditions).  With C = syg_laplace_chunk(), a = Re(s) t_step, a column is
 *   forward   if a >= 0: z = exp(-s t_step), anchor = 1;
 *   reversed  if a <  0: z = exp(+s t_step), anchor = exp(-s (L - 1) t_step)  (the transform of the reversed row);
 *   steep     if |a| (C - 1) > 40, in either direction; steep columns need |a| syg_laplace_steep() >= 746, which that
 *             threshold implies: the kernel reads only the first (reversed: last) syg_laplace_steep() samples for them.
 * Every |z| <= 1, and -a (L - 1) <= 700 keeps every anchor finite (the reference's own exp overflows beyond that).
 * Columns are ordered [forward, padded to a multiple of syg_laplace_tile_cols() | reversed, padded likewise | steep
 * forward | steep reversed]: S_fwd and S_rev are the PADDED counts, S16 = S_fwd + S_rev, Sc = S16 + S_steep_fwd +
 * S_steep_rev.
 *   table  [C, 2, S16] float32: table[i][0 / 1][c] = Re / Im of z_c^i (forward) or z_c^(C - 1 - i) (reversed), each
 *          formed in float64 and rounded once; zero in padding columns.  May be NULL when S16 = 0.
 *   fac    [Sc, syg_laplace_fac_stride()] float64: (re, im) of Z^r for r = 0 .. 15 | Z^16 | Z^(segment / C) | z, with
 *          Z = z^C; every power formed by one exp, not by repeated products.  Zero in padding columns.
 *   anchor [Sc, 2] float64, as above (it alone depends on L).
 *   col    [Sc] int32: the index in [0, S) that column writes, -1 for padding (any value outside [0, S) writes nothing,
 *          so no table makes the kernel write outside `out`; an index no column names is left unwritten).
 * Launch forms: -1 the rule | 0 whole-row (one wave per (clip, column tile) walks the row) | 1 segmented (the row is cut
 * into segments of syg_laplace_segment() samples whose float64 sums go to `work`; a second launch adds them in a fixed
 * order).  The rule takes the segmented form for rows longer than one segment where the whole-row form has fewer than
 * eight waves a CU (B S16 / 16 < 8 CUs).  It needs `work`, syg_laplace_work_bytes(B, L, S16, form) bytes (0 otherwise:
 * `work` may be NULL); `out` and `work` are 16-byte aligned.  A tile is syg_laplace_tile_rows() chunks of one clip: a
 * clip with fewer chunks pads the tile with zero chunks.
 * ------------------------------------------------------------------------------- */
int syg_laplace_chunk(void);
int syg_laplace_tile_rows(void);
int syg_laplace_tile_cols(void);
int64_t syg_laplace_segment(void);
int syg_laplace_steep(void);
int syg_laplace_fac_stride(void);
int64_t syg_laplace_work_bytes(int64_t B, int64_t L, int64_t S16, int form);
int syg_laplace_f32(const float* x, int64_t B, int64_t L, int64_t ldx, const float* table, const double* fac,
                    const double* anchor, const int32_t* col, int64_t S_fwd, int64_t S_rev, int64_t S_steep_fwd,
                    int64_t S_steep_rev, int64_t S, double t_step, double* out, void* work, int form, void* stream);

/* ---------------------------------------------------------------------------------
 * Polyphase resampling, scipy.signal.resample_poly in index form (the plan is host work: sygnals_amd/_resample.py):
 *     t = (n + n_pre_remove) down,  p = t mod up,  q = t div up,
 *     y[b, n] = sum_{j < Kp} table[p][j] x~[b, q - j],     n < n_out = ceil(L up / down),
 * x [B, L] float32 (row stride ldx) -> y [B, n_out] float32 (row stride ldy); x~ is x inside [0, L) and the pad rule
 * outside.  Gate: |y - scipy.signal.resample_poly in float64| <= 1e-5 of the row's peak.  float32 accumulation in a
 * fixed order, no atomics: the same call gives the same bits and a batch equals its rows.
 *   up, down  reduced by their gcd by the caller, each in [1, syg_resample_rate_max()]
 *   table     DEVICE [up, Kp] float32, dense: table[p][j] = hp[p + j up] of the padded, up-scaled filter hp, zero past
 *             its end (a precondition: the kernel reads up Kp floats)
 *   pad       0 constant (cval) | 1 edge | 2 wrap | 3 symmetric | 4 reflect (L >= 2); scipy's mean / minimum / maximum
 *             are the constant rule with 0 on the row minus its statistic and are formed by the caller
 *   form      -1 the rule | 0 table in LDS | 1 table read from global memory.  The rule: LDS where up Kp 4 bytes <=
 *             syg_resample_table_lds_rule(), global memory beyond (measured the faster place for a large table).  Form 0
 *             serves up (Kp | 1) 4 bytes <= syg_resample_table_lds_max() (rows are stored with an odd stride) and is
 *             an error beyond.  A table of more than syg_resample_table_max() bytes is refused.
 * A block takes tiles of syg_resample_tile() consecutive outputs of one row and stages their input span in LDS; where
 * a full tile reads more than syg_resample_span_max() input samples (strong decimation) the taps read global memory.
 * B <= 65535 a call.
 * ------------------------------------------------------------------------------- */
int syg_resample_tile(void);
int64_t syg_resample_table_lds_rule(void);
int64_t syg_resample_table_lds_max(void);
int64_t syg_resample_table_max(void);
int syg_resample_span_max(void);
int syg_resample_rate_max(void);
int syg_resample_poly_f32(const float* x, int64_t B, int64_t L, int64_t ldx, int up, int down, int64_t n_pre_remove, int Kp,
                          const float* table, int pad, float cval, int form, int64_t n_out, float* y, int64_t ldy,
                          void* stream);

/* ---------------------------------------------------------------------------------
 * Dynamic time warping, librosa.sequence.dtw with its default step set [[1,1],[0,1],[1,0]] (the float64 restatement
 * that is the contract: tests/dtw_ref.py).  Three stages, each usable alone:
 *
 * syg_dtw_cost_f32: C[b, n, m] = metric(X[b, :, n], Y[b, :, m]).
 *   X [B, K, N], Y [B, K, M] float32, row strides ldx >= N, ldy >= M, batch strides bsx, bsy >= 0 in elements (0: every
 *   pair shares that sequence) -> C [B, N, M] float32, dense.  metric: 0 euclidean | 1 sqeuclidean | 2 cityblock |
 *   3 cosine.  The first three are sums over k, in ascending order, of f(x_k - y_k), never the norm-and-dot form: a
 *   frame against itself costs exactly 0.  cosine is 1 - x.y / (|x| |y|); a zero-norm frame gives NaN as SciPy's
 *   cdist does, and what the recurrence does with a NaN is unspecified.  Gate: |C - C in float64| <= 1e-5 max C.
 *   A block takes a tile of syg_dtw_cost_tile() frames of X by as many of Y and stages them in LDS.
 *
 * syg_dtw_f32: the accumulated cost, the step codes, the end value and the warping path of every pair of C
 *   [B, N, M] float32 (row stride ldc >= M, batch stride bsc >= 0 elements).
 *     D[n, m] = min_k ( D[n - s0_k, m - s1_k] + (w_mul_k C[n, m] + w_add_k) ),  D[0, 0] = C[0, 0], under subseq
 *     D[0, :] = C[0, :]; a later step replaces an earlier one only if strictly smaller (the diagonal wins ties).
 *   The accumulators are float64 and every operation is rounded on its own (t = w_mul C; t = t + w_add; t = D + t):
 *   D depends on nothing but C and, with the default weights, equals a float64 NumPy evaluation bit for bit.
 *   weights_mul_host, weights_add_host: HOST [3] float64, finite, or NULL for 1 and 0.
 *   Outputs, all DEVICE; the optional ones are skipped when NULL:
 *     D        optional [B, N, M] float64
 *     steps    optional [B, N, M] uint8, the index of the step taken into each cell, one byte a cell (lanes and
 *              tiles that border each other never share a byte, so no store is a read-modify-write)
 *     cost     [B] float64: D[N - 1, M - 1], under subseq the least value of the last row
 *     end_col  [B] int32: M - 1, under subseq the first arg-min column of the last row (np.argmin's tie rule)
 *     path     optional [B, N + M - 1, 2] int32, from the end cell to (0, 0) (to row 0 under subseq) as librosa
 *              returns it, (-1, -1) past path_len; path_len [B] int32 goes with it; both need `steps`.  The walk runs
 *              on the device.
 *   With neither D nor steps nothing of size N M is written: the distance-only path.
 *   form  -1 the rule | 0 pair-resident | 1 tiled (syg_dtw_form() tells which one the rule takes).
 *     Pair-resident: one wave owns a pair, a lane a run of up to syg_dtw_run_max() columns; serves
 *     M <= syg_dtw_resident_max_cols() and needs no workspace.  Tiled: tiles of `tile` x `tile` cells (0: the product
 *     tile syg_dtw_tile(); at most syg_dtw_tile_max()), one launch per block anti-diagonal, no waiting between
 *     workgroups inside a launch; needs `work`, syg_dtw_work_bytes(B, N, M, form, tile) bytes (8-byte aligned).  The
 *     rule: pair-resident wherever M fits it, tiled beyond.
 *
 * Ragged batches (both entries): x_len, y_len DEVICE [B] int32 or NULL, with their HOST copies x_len_host, y_len_host
 * (both or neither; the library checks the host copy, the kernels read the device one and hold it inside [1, N] /
 * [1, M]).  Pair b is the top left x_len[b] x y_len[b] corner of its matrix; nothing outside it is read by syg_dtw_f32
 * or written by it, and syg_dtw_cost_f32 writes zeros there.
 * No atomics: the same call gives the same bits and a batch equals its pairs.  B <= 65535 a call.
 * ------------------------------------------------------------------------------- */
int syg_dtw_tile(void);
int syg_dtw_tile_max(void);
int syg_dtw_resident_max_cols(void);
int syg_dtw_run_max(void);
int syg_dtw_cost_tile(void);
int syg_dtw_form(int64_t B, int64_t N, int64_t M, int form);
int64_t syg_dtw_work_bytes(int64_t B, int64_t N, int64_t M, int form, int tile);
int syg_dtw_cost_f32(const float* X, const float* Y, int64_t B, int64_t K, int64_t N, int64_t M, int64_t ldx, int64_t ldy,
                     int64_t bsx, int64_t bsy, const int32_t* x_len, const int32_t* y_len, const int32_t* x_len_host,
                     const int32_t* y_len_host, int metric, float* C, void* stream);
int syg_dtw_f32(const float* C, int64_t B, int64_t N, int64_t M, int64_t ldc, int64_t bsc, const int32_t* x_len,
                const int32_t* y_len, const int32_t* x_len_host, const int32_t* y_len_host, const double* weights_mul_host,
                const double* weights_add_host, int subseq, int form, int tile, double* D, uint8_t* steps, double* cost,
                int32_t* end_col, int32_t* path, int32_t* path_len, void* work, int64_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Continuous wavelet transform, pywt.cwt as a bank of FIR filters (the float64 restatement that is the contract:
 * tests/cwt_ref.py; the plan is host work: sygnals_amd/_cwt.py):
 *     W[b, s, t] = sum_{j < taps_s} h_s[j] x~[b, t + shift_s - j],     t = c stride,  c < n_out = ceil(L / stride),
 * x [B, L] float32 (row stride ldx), x~ = x inside [0, L) and 0 outside.  h_s = -sqrt(s) d(k_s): pywt.cwt's
 * diff(convolve(x, k_s)) with the difference taken on the filter, in float64, by the plan; shift_s = floor(d_s) + 1 is
 * pywt.cwt's crop.  Gate: |W - W in float64| <= 1e-5 A_s per clip and scale, A_s = ||h_s||_1 max|x|.
 *   table   DEVICE float32: the taps of every filter; a complex wavelet's filter is a re plane of `taps` floats followed
 *           by its im plane
 *   meta    DEVICE [S][4] int32: {offset of the filter in table, taps, shift, index of the scale in y}.  A precondition:
 *           the kernel reads table[offset .. offset + taps) (twice that for cplx); an entry whose index is outside
 *           [0, S_out) or whose taps < 1 is skipped
 *   cplx    0 real wavelet | 1 complex wavelet
 *   output  0 coef: y [B, S_out, n_out] float32 ([B, S_out, n_out, 2], re and im interleaved, for cplx)
 *           1 magnitude |W|, 2 power |W|^2: y [B, S_out, n_out] float32
 *   y       dense; only the rows that meta names are written
 * syg_cwt_f32 is the direct form: a block takes syg_cwt_tile() output columns of one clip and up to
 * syg_cwt_scales_per_group() consecutive entries of meta, stages their input span in LDS (`reach`: the widest span of a
 * group at one column, max shift - min (shift - taps + 1) + 1; it sizes the staged words only) and reuses it for each of
 * them; a span of more than syg_cwt_span_max() samples is read from global memory instead.  float32 accumulation, taps
 * ascending, no atomics: the same call gives the same bits, a batch equals its rows, a strided call equals the columns
 * it keeps.  Filters of at most syg_cwt_direct_taps_max() taps are the ones the caller's rule sends here.  At stride 1 a
 * block also stages the taps of the scale at hand, in at most syg_cwt_taps_lds_max() words (both planes of a complex
 * filter, each padded by six); a longer filter reads its taps from global memory.
 * The spectral form is three steps around the strided transforms of length M >= L + taps - 1:
 *   syg_cwt_spectrum_c64  Z[b, r, :] = X[b, :] H[r, :] (complex64, [B, M] by [R, M] -> [B, R, M]), one launch
 *   the inverse transform of every row of Z
 *   syg_cwt_crop_f32      row r of Z [B, R, M] read at m = shift + c stride -> y in the requested form.
 *                         rmeta DEVICE [R][4] int32: {shift_a, index_a, shift_b, index_b}.  Real wavelet: the real part
 *                         is scale a, the imaginary part scale b (index_b = -1: none).  cplx: {shift, index, 0, -1}.
 * syg_cwt_work_bytes(B, R, M): the bytes the spectral form holds for B clips (padded rows, their transform, the
 * products, the inverse's result and the four-step temporary), -1 on bad arguments.  B <= 65535 a call.
 * ------------------------------------------------------------------------------- */
int syg_cwt_tile(void);
int syg_cwt_direct_taps_max(void);
int syg_cwt_scales_per_group(void);
int syg_cwt_span_max(void);
int syg_cwt_taps_lds_max(void);
int64_t syg_cwt_work_bytes(int64_t B, int64_t R, int64_t M);
int syg_cwt_f32(const float* x, int64_t B, int64_t L, int64_t ldx, const float* table, const int32_t* meta, int64_t S,
                int64_t S_out, int cplx, int64_t reach, int output, int64_t stride, int64_t n_out, float* y, void* stream);
int syg_cwt_spectrum_c64(const float* X, const float* H, int64_t B, int64_t R, int64_t M, float* Z, void* stream);
int syg_cwt_crop_f32(const float* Z, int64_t B, int64_t R, int64_t M, const int32_t* rmeta, int64_t L, int64_t S_out, int cplx,
                     int output, int64_t stride, int64_t n_out, float* y, void* stream);

/* ---------------------------------------------------------------------------------
 * Cepstral analysis (the float64 restatement that is the contract: tests/cepstrum_ref.py).
 *     real cepstrum      c = ifft(log(max(|X|, amin))).real,  X = fft(x, n)
 *     complex cepstrum   c = ifft(log(max(|X|, amin)) + i phi_u).real, phi_u the unwrapped phase with its linear term
 *                        pi ndelay k / center taken out (center = (n + 1) / 2, ndelay = rint(phi_u[center] / pi))
 * amin must be finite and >= 0 everywhere (at 0 a zero bin gives -inf and the result is unspecified).
 * Gate: |c - c in float64| <= 1e-5 K per frame or row, K = mean_k ||x w||_1 / max(|X_k|, amin).
 *
 * syg_cepstrogram2048_f32: the fused kernel, frames of 2048 samples only (another frame_length: SYG_E_UNSUPPORTED).
 *   y [B, L] float32 (row stride ldy), framed, zero-padded and counted as syg_stft2048_c2c_f32 does (T by its rule);
 *   window [2048] float32 (the padded analysis window), twiddle [2048][2] = exp(-2 pi i k / 2048);
 *   out [B, n_ceps, T] float32, quefrencies 0 .. n_ceps - 1, 1 <= n_ceps <= 2048.  One wave per frame, a workgroup of
 *   syg_cepstrum_constants(SYG_CEPS_WAVES) waves per tile of SYG_CEPS_TILE_FRAMES consecutive frames, staged in LDS and
 *   stored with the frame index fastest.  float32 in one fixed order, no atomics: the same call gives the same bits, a
 *   batch equals its rows, n_ceps = Q equals the first Q rows of the full result.
 * The chain form, for every length (the transforms between the steps are the caller's: the strided FFT entries):
 *   syg_cepstrum_logmag_c64  X [rows, in_bins][2] complex64, in_bins = n (a whole spectrum) or n / 2 + 1 (a one-sided one,
 *                            extended evenly) -> Z [rows, n][2] = (log(max(|X|, amin)) - log(amin), 0); for amin = 0
 *                            nothing is subtracted.  In place (Z == X) only for in_bins == n.
 *   syg_cepstrum_gather_f32  Z [rows, n][2], the inverse transform of the above -> out[(b n_ceps + q) T + t] = Re Z[b T + t, q]
 *                            (+ log(amin) at q = 0; pass amin = 0 to add nothing), q < n_ceps; T = 1: out [rows, n_ceps].
 *                            rows is a multiple of T (whole clips) or less than T (a run of one clip's frames, `out`
 *                            pointing at its first frame).
 * Complex cepstrum of rows:
 *   syg_cepstrum_unwrap_c64  X [B, n][2] -> Z [B, n][2] = (log(max(|X|, amin)) - log(amin), phi_u) and ndelay [B] int32.
 *                            phi = atan2f, except bin 0: 0 for Re X[0] >= 0, else +pi.  np.unwrap's rule as integer wrap
 *                            counts, their prefix sum exact, phi_u formed in float64 and stored as float32.  work:
 *                            syg_cepstrum_unwrap_work_bytes(B, n) bytes, 4-byte aligned (-1 on bad arguments).  Blocks of
 *                            SYG_CEPS_SCAN bins, block sums and a second pass; no workgroup waits on another.  n >= 2.
 *   syg_cepstrum_exp_c64     Xh [B, n][2] -> Z = exp(Re Xh) (cos, sin)(Im Xh + pi ndelay[b] k / center): the middle of the
 *                            inverse complex cepstrum (exact for even n; for odd n only at ndelay = 0).
 * syg_cepstrum_peaks_f32: over ceps [B, Q, T] float32, per frame q* = the first maximum of c[qmin .. qmax]
 *   (1 <= qmin <= qmax < Q), the parabolic shift d = (c[q*-1] - c[q*+1]) / (2 (c[q*-1] - 2 c[q*] + c[q*+1])) where
 *   qmin < q* < qmax and the denominator is negative (else 0), in float64 from the float32 values;
 *   f0 [B, T] float64 = sr / (q* + d), NaN where strength < threshold; strength [B, T] float32 = c[q*]; qstar [B, T] int32;
 *   voiced [B, T] uint8.
 * syg_cepstrum_constants(key): the figures above (SYG_CEPS_*), -1 for an unknown key.
 * ------------------------------------------------------------------------------- */
enum {
  SYG_CEPS_FRAME = 0,        /* frame length of the fused kernel */
  SYG_CEPS_TILE_FRAMES = 1,  /* consecutive frames a workgroup stages and stores together */
  SYG_CEPS_WAVES = 2,        /* waves of a workgroup */
  SYG_CEPS_SCAN = 3,         /* bins a block of the unwrap scans */
  SYG_CEPS_LDS_FIXED = 4,    /* bytes of LDS a workgroup of the fused kernel holds beside its stage */
  SYG_CEPS_LDS_MAX = 5       /* bytes of LDS at n_ceps = 2048 */
};
int64_t syg_cepstrum_constants(int key);
int syg_cepstrogram2048_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int frame_length, int hop, int center, int64_t T,
                            const float* window, const float* twiddle, int n_ceps, double amin, float* out, void* stream);
int syg_cepstrum_logmag_c64(const float* X, int64_t rows, int64_t in_bins, int64_t n, double amin, float* Z, void* stream);
int syg_cepstrum_gather_f32(const float* Z, int64_t rows, int64_t n, int64_t n_ceps, int64_t T, double amin, float* out,
                            void* stream);
int64_t syg_cepstrum_unwrap_work_bytes(int64_t B, int64_t n);
int syg_cepstrum_unwrap_c64(const float* X, int64_t B, int64_t n, double amin, void* work, int64_t work_bytes, float* Z,
                            int32_t* ndelay, void* stream);
int syg_cepstrum_exp_c64(const float* Xh, int64_t B, int64_t n, const int32_t* ndelay, float* Z, void* stream);
int syg_cepstrum_peaks_f32(const float* ceps, int64_t B, int64_t Q, int64_t T, int qmin, int qmax, double sr, double threshold,
                           double* f0, float* strength, int32_t* qstar, uint8_t* voiced, void* stream);

/* ---------------------------------------------------------------------------------
 * Linear prediction (the float64 restatement that is the contract: tests/lpc_ref.py).  order p, 1 <= p <= min(64, N - 2).
 *     SYG_LPC_BURG      librosa.lpc's recurrence on f = x[1:], b = x[:-1]: k_i = -2 sum f b / (sum (f^2 + b^2) + DBL_MIN),
 *                       a <- a + k_i reversed(a), err = sum (f^2 + b^2) / (2 (N - 1 - p)) over the last f and b
 *     SYG_LPC_AUTOCORR  r[l] = sum_n xw[n] xw[n + l] (biased, not normalised), Levinson-Durbin in float64,
 *                       err = (r[0] + sum_j a[j] r[j]) / N;  r[0] = 0 gives a = [1, 0, ...], err = 0
 * Samples are float32, promoted to float64 and multiplied by the float32 window table where one is given (NULL: none);
 * everything after that is float64.  Gates: |a - a_ref| <= 1e-5 max|a_ref|, |k - k_ref| <= 1e-5, |err - err_ref| <= 1e-5 err_ref.
 * One fixed summation order, no atomics: the same call gives the same bits and a batch equals its rows.
 *
 * syg_lpc_frames_f32: y [B, L] float32 (row stride ldy), frames of frame_length N in [p + 2, 2048] (longer:
 *   SYG_E_UNSUPPORTED), any hop >= 1; centred frames start at t hop - N / 2, samples outside the clip are 0; T by
 *   frames_expected for N a power of two >= 8 and by the padded rule otherwise (ops.cepstrogram_frames).  window [N] or NULL.
 *   a [B, p + 1, T] (a[0] = 1), k [B, p, T] or NULL (reflection coefficients), err [B, T] or NULL; the frame index is fastest.
 *   One wave per frame, sample n in lane n % 64 and register n / 64 (ceil(N / 64) registers); a workgroup of SYG_LPC_WAVES waves takes
 *   SYG_LPC_TILE_FRAMES consecutive frames and reads their span once into LDS where it is at most SYG_LPC_SPAN_MAX floats.
 * syg_lpc_rows_f32: whole rows y [B, L] of any length L in [p + 2, 2^26] -> a [B, p + 1], k [B, p] or NULL, err [B] or NULL.
 *   window [L] or NULL.  Burg: p + 1 launches over a float64 workspace f, b [B, L] (each applies k_{i-1} to chunks of
 *   SYG_LPC_STAGE_CHUNK samples and leaves the partial sums of k_i, which the next launch adds in a fixed order), then a
 *   one-wave step-up.  Autocorr: partial lag sums over chunks of SYG_LPC_ACORR_CHUNK samples, then a one-wave Levinson.
 *   work: syg_lpc_rows_work_bytes(B, L, order, method) bytes, 8-byte aligned (-1 on bad arguments).
 * syg_lpc_envelope_f32: a [B, p + 1, T], err [B, T] -> out [B, n_fft / 2 + 1, T] = P[k] = err / |A(e^{-2 pi i k / n_fft})|^2,
 *   A(z) = sum_j a[j] z^-j by Horner's rule in float64; phasor [n_fft / 2 + 1][2] float64 = (cos, -sin)(2 pi k / n_fft);
 *   db = 1: 10 log10(max(P, amin)).  n_fft even.
 * syg_lpc_constants(key): the figures above (SYG_LPC_*), -1 for an unknown key.
 * ------------------------------------------------------------------------------- */
enum { SYG_LPC_BURG = 0, SYG_LPC_AUTOCORR = 1 };
enum {
  SYG_LPC_MAX_FRAME = 0,     /* longest frame of the frame kernel */
  SYG_LPC_MAX_ORDER = 1,     /* highest order */
  SYG_LPC_WAVES = 2,         /* waves of a workgroup of the frame kernel */
  SYG_LPC_TILE_FRAMES = 3,   /* consecutive frames a workgroup takes and stores together */
  SYG_LPC_SPAN_MAX = 4,      /* floats of a tile's span that are read once into LDS */
  SYG_LPC_STAGE_CHUNK = 5,   /* samples a workgroup of a Burg stage over whole rows owns */
  SYG_LPC_ACORR_CHUNK = 6    /* samples a workgroup of the row autocorrelation owns */
};
int64_t syg_lpc_constants(int key);
int syg_lpc_frames_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int frame_length, int hop, int center, int64_t T,
                       const float* window, int order, int method, float* a, float* k, float* err, void* stream);
int64_t syg_lpc_rows_work_bytes(int64_t B, int64_t L, int order, int method);
int syg_lpc_rows_f32(const float* y, int64_t B, int64_t L, int64_t ldy, const float* window, int order, int method, void* work,
                     int64_t work_bytes, float* a, float* k, float* err, void* stream);
int syg_lpc_envelope_f32(const float* a, const float* err, int64_t B, int order, int64_t T, int n_fft, const double* phasor, int db,
                         double amin, float* out, void* stream);

/* ---------------------------------------------------------------------------------
 * Noise generation (the float64 restatement that is the contract: tests/rng_ref.py; the host-side twin in integer
 * NumPy: sygnals_amd/_rng.py).
 *
 * The generator is Philox4x32-10 (Salmon et al. 2011, the Random123 constants): multipliers 0xD2511F53 / 0xCD9E8D57, key
 * increments 0x9E3779B9 / 0xBB67AE85, ten rounds, the key bumped between rounds, per round
 *     (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)).
 * Stream layout: key = (seed & 0xffffffff, seed >> 32); counter = (q & 0xffffffff, q >> 32, row, stream), q = n / 4,
 * 0 <= row < 2^31; stream SYG_RNG_STREAM_NOISE: noise samples, SYG_RNG_STREAM_ROW: per-row draws (taken on the host).
 * The words w0 .. w3 of one call give samples 4q .. 4q + 3: with u(w) = (2 (w >> 9) + 1) 2^-24 (exact in float32,
 * strictly inside (0, 1)), z[4q] = r cos(t), z[4q + 1] = r sin(t), r = sqrt(-2 ln u(w0)), t = 2 pi u(w1); z[4q + 2] and
 * z[4q + 3] likewise from (w2, w3).  |z| <= 5.77.  float32 with the accurate logf / sqrtf and sincospif(2 u).
 * A sample depends on (seed, stream, row, n) alone: not on the launch shape, not on where the row lies in a batch; no
 * atomics; the same call gives the same bits.  Gate: |z - z in float64| <= 1e-5 max(1, max |z|) per row.
 *
 * syg_rng_philox_u32: counter [n][4], key [n][2] uint32 DEVICE arrays -> out [n][4] raw words (counter / out 16-byte
 *   aligned, key 8-byte aligned).
 * syg_rng_normal_f32: out [B, L] (row stride ldo) = samples offset .. offset + L - 1 of rows first_row .. first_row + B - 1.
 *   Rejected before any device work: a null pointer, B < 1, L < 1, ldo < L, first_row < 0 or first_row + B > 2^31,
 *   offset outside [0, 2^62).
 * Power-law ("coloured") noise, noise[r] = irfft(rfft(w_r) g, M)[:L] (Timmer & Koenig 1995): M the smallest power of two
 *   >= max(L, 2), w_r the M white samples of (seed, row r), g[0] = 0 and g[k] = k^(-alpha / 2); alpha = 1 pink, 2 brown;
 *   at alpha = 0 nothing diverges and g = 1 everywhere (the white row unchanged).  g is real and symmetric, so rows
 *   r and r ^ 1 (ABSOLUTE row indices) share one complex transform, which is the caller's (the strided FFT entries):
 *   syg_rng_normal_pairs_c64  Z [P, M][2] = w_a + i w_b for rows a = first_row + 2p, b = a + 1; first_row even.
 *   syg_rng_power_gain_c64    X [rows, M][2] *= g[min(k, M - k)] in place; M a power of two in [2, 2^26], alpha in [0, 2].
 *   syg_rng_unpack_pairs_f32  out [B, L] (row stride ldo): row b is the real (R even) or imaginary (R odd) part of
 *                             Z[(R >> 1) - (first_row >> 1)][0 .. L - 1], R = first_row + b; Z [.., M][2].
 * syg_rng_constants(key): the figures above (SYG_RNG_*), -1 for an unknown key.
 * ------------------------------------------------------------------------------- */
enum {
  SYG_RNG_ROUNDS = 0,        /* Philox rounds */
  SYG_RNG_STREAM_NOISE = 1,  /* counter word 3 of noise samples */
  SYG_RNG_STREAM_ROW = 2,    /* counter word 3 of per-row draws */
  SYG_RNG_ROW_LIMIT = 3,     /* rows lie in [0, this) */
  SYG_RNG_COLORED_MAX = 4    /* longest coloured row (the longest transform) */
};
int64_t syg_rng_constants(int key);
int syg_rng_philox_u32(const uint32_t* counter, const uint32_t* key, int64_t n, uint32_t* out, void* stream);
int syg_rng_normal_f32(float* out, int64_t B, int64_t L, int64_t ldo, uint64_t seed, int64_t first_row, int64_t offset,
                       void* stream);
int syg_rng_normal_pairs_c64(float* Z, int64_t P, int64_t M, uint64_t seed, int64_t first_row, void* stream);
int syg_rng_power_gain_c64(float* X, int64_t rows, int64_t M, double alpha, void* stream);
int syg_rng_unpack_pairs_f32(const float* Z, int64_t M, int64_t first_row, float* out, int64_t B, int64_t L, int64_t ldo,
                             void* stream);

/* ---------------------------------------------------------------------------------
 * Cross-spectral analysis of two real signals (cross_spectrum.hip): scipy.signal.csd / welch / coherence with
 * return_onesided=True, average='mean'.  Segment s starts at s * step, nseg = (L - (nperseg - step)) / step; detrend,
 * window, zero padding to nfft, scale and the one-sided factor as syg_welch_f32, each signal detrended on its own.
 *   Pxy = mean_s conj(X_s) Y_s,  Pxx = mean_s |X_s|^2,  Pyy = mean_s |Y_s|^2,  Cxy = |Pxy|^2 / (Pxx Pyy)
 * Cxy is formed in float64 from the raw float64 sums (scale and one-sided factor cancel); 0 / 0 gives NaN.
 * Outputs: pxy_out [B, F][2], pxx_out, pyy_out, coh_out [B, F] float32, F = nfft / 2 + 1; any may be NULL, not all.
 *
 * syg_csd_f32, the fused form: nfft a power of two in [8, 8192], nperseg <= nfft, 1 <= step <= nperseg, B <= 65535.
 *   x [B, L] (row stride ldx), y [By, L] (row stride ldy), By = B or 1: one reference row read by every x row.
 *   twiddle [nfft] complex, W_nfft^k (as syg_fft_pow2_c2c_f32).  One complex transform per segment carries both signals.
 *   A row's segments are split over workgroups by the segment count alone (runs of max(16, ceil(nseg / 2048))
 *   consecutive segments), so a batch equals its rows bit for bit; no atomics: the same call gives the same bits.
 *   work: syg_csd_work_bytes(B, nseg, nfft) bytes (-1 for B, nseg < 1 or nfft < 2): the float32 partial sums
 *   [B, workgroups, 4, F], then the float64 slice sums [B, slices, 4, F] (16 slices from 64 workgroups, else 1).
 * syg_csd_rows_f32, every other length: X, Y [rows, n][2] are the full complex spectra of `rows` consecutive segments
 *   of ONE row pair (the caller packs and transforms them); acc [4, F] float64 is the caller's and carries the raw sums
 *   from call to call: `first` starts them, `last` writes the outputs with scale / nseg.  Segment order, float64.
 *
 * Generalised cross-correlation:
 * syg_gcc_weight_c64  out[r, k] = W X[r, k] conj(Y[ry, k]), k < n, over plain complex spectra [rows, n][2] (Y: rows_y = 1
 *                     or rows); phat 0: W = 1; 1: W = 1 / |X conj(Y)|, 0 on a bin that is exactly 0.  out may be X.
 * syg_gcc_crop_f32    out[r, j] = Re c[r, (j - max_lag) mod n], j in [0, 2 max_lag]; 2 max_lag + 1 <= n.
 * syg_peak_pick_f32   per row of r [B, W] (row stride ldr), one wave: i* = the first maximum; lag = lag0 + i*; where i* is
 *                     interior and den = r[i*-1] - 2 r[i*] + r[i*+1] < 0, delta = (r[i*-1] - r[i*+1]) / (2 den) and
 *                     peak = r[i*] - (r[i*-1] - r[i*+1]) delta / 4, else delta = 0 and peak = r[i*] (float64);
 *                     delay = (lag + delta) / fs.  A row of NaN gives NaN, lag 0.
 * Every argument check is made before any device work.
 * ------------------------------------------------------------------------------- */
int64_t syg_csd_work_bytes(int64_t B, int64_t nseg, int nfft);
int syg_csd_f32(const float* x, const float* y, int64_t B, int64_t By, int64_t L, int64_t ldx, int64_t ldy, int nperseg,
                int step, int nfft, const float* window, const float* twiddle, int detrend, double scale, float* pxy_out,
                float* pxx_out, float* pyy_out, float* coh_out, void* work, void* stream);
int syg_csd_rows_f32(const float* X, const float* Y, int64_t rows, int64_t n, double* acc, int first, int last,
                     int64_t nseg, double scale, float* pxy_out, float* pxx_out, float* pyy_out, float* coh_out,
                     void* stream);
int syg_gcc_weight_c64(const float* X, const float* Y, int64_t rows, int64_t rows_y, int64_t n, int phat, float* out,
                       void* stream);
int syg_gcc_crop_f32(const float* c, int64_t rows, int64_t n, int64_t max_lag, float* out, void* stream);
int syg_peak_pick_f32(const float* r, int64_t B, int64_t W, int64_t ldr, int64_t lag0, double fs, double* delay_out,
                      int64_t* lag_out, double* peak_out, void* stream);

/* ---------------------------------------------------------------------------------
 * Feature dynamics along T of x [B, K, T] float32 (dynamics.hip): unit stride along T, strides sxb / sxk (in floats,
 * non-negative) over B and K.  Everything is per row (b, k).  The float64 restatement: tests/dynamics_ref.py.
 *
 * syg_dynamics_f32 writes `statics + n_delta` blocks of K rows, out[b, blk K + k, t] (strides sob / sok, sok >= T):
 *   statics  s = x, or with cmvn = 1  s = (x - m) / sqrt(max(v, 1e-20))  (variance = 0: s = x - m), rounded once to
 *            float32.  window = 0 (or >= T): m, v the mean and the population variance of the row, float64 sums over
 *            chunks of SYG_DYN_TILE frames combined in index order.  1 <= window < T: Kaldi's centred sliding window,
 *            s = t - W / 2, e = s + W, shifted back into [0, T); windows up to SYG_DYN_DIRECT_WINDOW are summed
 *            explicitly (W = 1 is exact), longer ones come from float64 prefix sums of x and x^2.
 *   deltas   block d (1-based) = scipy.signal.savgol_filter(s, width, deriv = d0 + d - 1 .., mode), taken from the
 *            ROUNDED statics: interior frames h <= t < T - h (h = width / 2) are sum_j w[j] s[t - h + j], float32 fmaf,
 *            j ascending; under mode 0 (interp) the first / last h frames are sum_j e[j] s[j] / s[T - width + j] with
 *            a table row per frame; modes 1 nearest, 2 mirror, 3 wrap, 4 constant (cval) map t - h + j into the row.
 *            tab: per delta block width^2 floats: w [width] (savgol_coeffs reversed), the left edge rows [h][width],
 *            the right edge rows [h][width] (sygnals_amd/_dynamics.py builds them in float64 and rounds once).
 *            statics = 0, n_delta = 1 is the plain delta of any order (the order is the table's).
 *   form     0: the rule (syg_dynamics_form: 0 resident, 1 tiled), 1 resident, 2 tiled.  Resident: a wave holds a whole
 *            row in LDS, up to SYG_DYN_UNITS rows a workgroup, one launch.  Tiled: SYG_DYN_TILE frames a wave with a halo
 *            of width (+ window) frames; global statistics come from launches ahead of it that write float64 chunk
 *            sums and their in-order totals to work (syg_dynamics_work_bytes(B, K, T) bytes).  The deltas and the global CMVN are bit-identical in both
 *            forms; the sliding CMVN may differ by 2 float32 ulp.  No atomics; a batch equals its rows bit for bit.
 *   Rejected before any device work: null pointers, an empty input, bad strides, a result above 2^31 elements, width
 *   even or outside [3, 255], an unknown mode, interp with T < width, an out that overlaps x (cmvn alone may write
 *   onto x itself; not with a sliding window in the tiled form), a sliding window above SYG_DYN_WINDOW_MAX in the tiled
 *   form, wrap with CMVN over more than one tile, a missing workspace.
 * syg_stack_memory_f32: out [B, n_steps K, T] contiguous, out[b, i K + k, t] = x[b, k, t - i delay], 0 outside [0, T);
 *   n_steps >= 1, delay != 0 (either sign).  A pure gather.
 * ------------------------------------------------------------------------------- */
enum {
  SYG_DYN_TILE = 0,                /* frames of a tile and of a chunk of the global sums */
  SYG_DYN_RESIDENT_T = 1,          /* the rule: longest resident row */
  SYG_DYN_RESIDENT_T_SLIDING = 2,  /* the rule: longest resident row under a sliding window */
  SYG_DYN_WINDOW_MAX = 3,          /* longest sliding window (below T) of the tiled form */
  SYG_DYN_DIRECT_WINDOW = 4,       /* sliding windows up to this are summed explicitly */
  SYG_DYN_WIDTH_MAX = 5,
  SYG_DYN_ORDER_MAX = 6,
  SYG_DYN_UNITS = 7,               /* rows (waves) of a workgroup, at most */
  SYG_DYN_MAX_OUT = 8,             /* elements of a result, at most */
  SYG_DYN_LDS_MAX = 9              /* LDS bytes of a one-row workgroup: what a forced resident row may take */
};
int64_t syg_dynamics_constants(int key);
int syg_dynamics_form(int64_t T, int64_t window);
int64_t syg_dynamics_work_bytes(int64_t B, int64_t K, int64_t T);
int syg_dynamics_f32(const float* x, int64_t B, int64_t K, int64_t T, int64_t sxb, int64_t sxk, float* out, int64_t sob,
                     int64_t sok, int cmvn, int64_t window, int variance, int statics, int n_delta, int width, int mode,
                     float cval, const float* tab, int form, void* work, int64_t work_bytes, void* stream);
int syg_stack_memory_f32(const float* x, int64_t B, int64_t K, int64_t T, int64_t sxb, int64_t sxk, float* out,
                         int64_t n_steps, int64_t delay, void* stream);

/* -------------------------------------------------------------------------------
 * SpecAugment of x [B, K, T] float32 (spec_augment.hip): a time warp, then the union of frequency and time masks, drawn
 * per clip.  Rows as in syg_dynamics_f32 (unit stride along T, strides in floats over B and K).  The package's own
 * definition; the integer / float64 restatement: tests/specaug_ref.py, the host twin: sygnals_amd/_specaug.py.
 *
 * Clip b has T_b = lengths[b] valid frames (device int64 [B], each in [1, T]; NULL: T) and generator row
 * r = first_row + b.  Frames t >= T_b are copied and nothing is drawn from them.  Item q is one Philox call at counter
 * (q, 0, r, SYG_SPEC_STREAM) with key `seed`; words w0, w1 are used; draw(w, n) = (uint64(w) n) >> 32.
 *   warp (q = 0), only if time_warp = W > 0 and T_b > 2 W:  c = W + draw(w0, T_b - 2 W), w' = c - W + 1 + draw(w1, 2 W);
 *     frames [0, c) are resized to w' frames and [c, T_b) to T_b - w', each as torch's linear interpolate with
 *     align_corners = False: s = max(0, ((2u + 1) n_in - n_out) / (2 n_out)) by integer quotient and remainder,
 *     i0 = min(floor(s), n_in - 1), i1 = min(i0 + 1, n_in - 1), value a + (s - floor(s)) (b - a) in float32.
 *   frequency mask i (q = 1 + i):  f = draw(w0, freq_width + 1), f0 = draw(w1, K - f + 1): rows [f0, f0 + f).
 *   time mask j (q = 17 + j):  We = min(time_width, floor(time_ratio T_b)) (float64), t = draw(w0, We + 1),
 *     t0 = draw(w1, T_b - t + 1): frames [t0, t0 + t).
 * A masked cell (t < T_b) holds mask_value bit for bit, or with mean = 1 the mean of x[b, :, :T_b] before the warp:
 * float64 sums over chunks of SYG_SPEC_TILE cells (cell j: row j / T_b, frame j % T_b) added in index order, rounded once.
 * form (mean only): 0 the rule (resident up to SYG_SPEC_RESIDENT_MAX cells a clip), 1 resident (one launch, a workgroup a
 * clip), 2 tiled (two small launches ahead, `work` of syg_spec_augment_work_bytes(B, K, T) bytes); same bits.
 * out = x itself (same strides) with time_warp = 0 writes the masked cells only (mean: the tiled sums, `work` needed).
 * No atomics: the same call gives the same bits, and a batch equals its clips called with first_row + b.
 * Rejected before any device work: null x / out, an empty input, more than 2^31 elements, bad strides, counts outside
 * 0 .. 16, freq_width outside [0, K], a negative time_width or time_warp, time_ratio outside (0, 1], a non-finite
 * mask_value, rows beyond 2^31, an out that overlaps x otherwise, a missing workspace.
 * ------------------------------------------------------------------------------- */
enum {
  SYG_SPEC_STREAM = 0,        /* counter word 3 of the draws */
  SYG_SPEC_MAX_MASKS = 1,     /* masks of one kind, at most */
  SYG_SPEC_TILE = 2,          /* cells of a workgroup's tile and of a chunk of the mean's sums */
  SYG_SPEC_RESIDENT_MAX = 3,  /* the rule: cells of a clip up to which the mean is taken in the one launch */
  SYG_SPEC_MAX_ELEMS = 4      /* elements of a call, at most */
};
int64_t syg_spec_augment_constants(int key);
int64_t syg_spec_augment_work_bytes(int64_t B, int64_t K, int64_t T);
int syg_spec_augment_f32(const float* x, int64_t B, int64_t K, int64_t T, int64_t sxb, int64_t sxk, float* out, int64_t sob,
                         int64_t sok, const int64_t* lengths, uint64_t seed, int64_t first_row, int freq_masks,
                         int64_t freq_width, int time_masks, int64_t time_width, double time_ratio, int64_t time_warp, int mean,
                         float mask_value, int form, void* work, int64_t work_bytes, void* stream);

/* -------------------------------------------------------------------------------
 * Rhythm after the onset envelope (beat.hip): librosa 0.10 feature.tempogram (autocorrelation), feature.tempo and
 * beat.beat_track.  Parity is unpinned (librosa is not a dependency): the float64 restatement of tests/beat_ref.py is the
 * contract.  env [B, T] float32, row stride ld >= T, unit stride along T.  No atomics: the same call gives the same bits
 * and a batch equals its rows.  Every entry checks its arguments before any device work.
 *
 * syg_tempogram_f32: center != 0: the envelope is padded by p = win_length / 2 linear ramps to zero on both sides
 *   (np.pad(..., "linear_ramp"), formed on the fly) and n = T; else n = T - win_length + 1 >= 1.  With f_t[j] =
 *   window[j] xp[t + j] (window: device float32 [win_length]), r_t[k] = sum_j f_t[j] f_t[j + k]: float32 products summed
 *   64 at a time, the sums added in float64, in a fixed order.  norm 1 (inf): the column is divided by max_k |r_t[k]|
 *   unless that is below FLT_MIN; norm 0: as it is.  tg [B, win_length, n] float32, frames fastest, or NULL.
 *   agg [B, win_length] float64 or NULL: the mean of tg over frames, summed in frame order (a partial row per
 *   SYG_BEAT_SLICE_TILES tiles of syg_tempogram_tile(win_length) frames, the rows added in order); needs `work`,
 *   syg_tempogram_work_bytes(B, T, win_length, center) bytes.  win_length 2 .. SYG_BEAT_WIN_MAX; the result at most
 *   SYG_BEAT_MAX_ELEMS elements.  Cost: win_length^2 / 2 multiply-adds a frame, of which the kernel issues twice as many.
 * syg_tempo_pick_f32: the first argmax over k of log1p(1e6 a[k]) + logprior[k] (float64; a NaN score wins, as in
 *   numpy), a = the aggregate [B, win_length] (then n = 1) or each column of tg [B, win_length, n]: exactly one of the
 *   two is given.  logprior, bpms: device float64 [win_length], made on the host.  kstar [B, n] int32, tempo [B, n]
 *   float64 = bpms[kstar].  A row whose envelope env is all zeros gives 0 and 0.0.  work: syg_tempo_pick_work_bytes(B).
 * syg_beat_local_score_f32: e = env / std(env, ddof 1) (float64 sums; e = env when T < 2 or the deviation is not a
 *   positive finite number); ls[i] = sum_q exp(-0.5 (32 q / P)^2) e[i - q], |q| <= min(P, ceil(7 P / 32)) (the taps
 *   beyond are below 2.3e-11), zeros outside the row, float64, stored as float32; P = period[b], device int32 [B].
 *   lsmax [B] float32 = max_i ls[i].  A period outside 2 .. SYG_BEAT_PERIOD_MAX: ls = 0.
 *   work: syg_beat_local_score_work_bytes(B).
 * syg_beat_dp_f32: offsets o_j = -2 P + j up to -round_half_even(P / 2); tx[j] = -tightness (d d), d = logtab[-o_j - 1]
 *   - logtab[P - 1], logtab: device float64 [SYG_BEAT_LOG_TABLE], log of 1 .. SYG_BEAT_LOG_TABLE made on the host.
 *   cum[i] = ls[i] + max_j (tx[j] + (cum[i + o_j] if i + o_j >= 0 else 0)), the first j among equals; back[i] = -1 while
 *   no beat has been admitted and ls[i] < 0.01 lsmax, else i + o_j (which may be below -1 in the first 2 P frames: any
 *   negative link ends a walk).  Float64 additions and comparisons only.  cum [B, T] float64, back [B, T] int32.
 *   period_max: a bound on every period[b] known to the host, 2 .. SYG_BEAT_PERIOD_MAX; it chooses the kernel (one wave a
 *   clip up to SYG_BEAT_DP_WAVE_PERIOD, four beyond) and the LDS ring.  A period outside 2 .. period_max: cum = 0,
 *   back = -1.  Serial in T: about J = 1.5 P additions over the wave and one reduction a frame.
 * syg_beat_track_f32: the local maxima of cum (interior: cum[i] > cum[i - 1] and cum[i] >= cum[i + 1]; frame 0 never;
 *   frame T - 1: cum[T - 1] > cum[T - 2]); their exact median (numpy's: the mean of the two middle values of an even
 *   count); the last beat = the largest i with 2 cum[i] lm[i] > median; the walk along `back`; the trim: sm[i] =
 *   (0.5 ls[b[i - 1]] + ls[b[i]]) + 0.5 ls[b[i + 1]], th = 0.5 sqrt(sum sm^2 / count) in index order (trim = 0: th = 0),
 *   v = {i : sm[i] > th}, result b[min v : max v] with the upper end EXCLUSIVE.  beats [B, T] int32 ascending, -1 beyond
 *   them; count [B] int32; last [B] int32 (the last beat before the trim, -1: none) or NULL.
 * ------------------------------------------------------------------------------- */
enum {
  SYG_BEAT_WIN_MAX = 0,         /* largest win_length */
  SYG_BEAT_PERIOD_MAX = 1,      /* largest beat period in frames */
  SYG_BEAT_LOG_TABLE = 2,       /* entries of logtab */
  SYG_BEAT_SLICE_TILES = 3,     /* tiles of frames a tempogram workgroup takes: one partial row of the aggregate */
  SYG_BEAT_DP_WAVE_PERIOD = 4,  /* period_max up to which the DP runs one wave a clip */
  SYG_BEAT_MAX_ELEMS = 5        /* elements of a result, at most */
};
int64_t syg_beat_constants(int key);
int syg_tempogram_tile(int win_length);
int64_t syg_tempogram_work_bytes(int64_t B, int64_t T, int win_length, int center);
int syg_tempogram_f32(const float* env, int64_t B, int64_t T, int64_t ld, int win_length, int center, const float* window,
                      int norm, float* tg, double* agg, void* work, int64_t work_bytes, void* stream);
int64_t syg_tempo_pick_work_bytes(int64_t B);
int syg_tempo_pick_f32(const double* a, const float* tg, int64_t B, int win_length, int64_t n, const float* env, int64_t T,
                       int64_t ld, const double* logprior, const double* bpms, int32_t* kstar, double* tempo, void* work,
                       void* stream);
int64_t syg_beat_local_score_work_bytes(int64_t B);
int syg_beat_local_score_f32(const float* env, int64_t B, int64_t T, int64_t ld, const int32_t* period, float* ls,
                             float* lsmax, void* work, void* stream);
int syg_beat_dp_f32(const float* ls, const float* lsmax, int64_t B, int64_t T, const int32_t* period, int period_max,
                    double tightness, const double* logtab, double* cum, int32_t* back, void* stream);
int syg_beat_track_f32(const float* ls, const double* cum, const int32_t* back, int64_t B, int64_t T, const int32_t* period,
                       int trim, int32_t* beats, int32_t* count, int32_t* last, void* stream);

/* -------------------------------------------------------------------------------
 * Tonal features (chroma.hip): librosa 0.10 feature.chroma_stft / chroma_cqt / chroma_cens / tonnetz and estimate_tuning
 * after the transforms.  Parity is unpinned (librosa is not a dependency): the float64 restatement of
 * tests/chroma_ref.py is the contract; the host tables are made by sygnals_amd/_chroma.py.  No floating-point atomics:
 * the same call gives the same bits and a batch equals its rows.  Every entry checks its arguments before any device work.
 *
 * norm: 0 none, 1 inf (max |x|), 2 L1, 3 L2, per frame over the n_chroma rows, the length in float64; a frame whose
 * length is below FLT_MIN is left as it is (librosa.util.normalize).  has_threshold != 0: sums below `threshold` (<)
 * become 0 before the norm.  complex != 0: x is interleaved (re, im) and |z|^power (1 or 2) is taken on load,
 * fmaf(re, re, im * im) as syg_cabs_pow_f32 forms it (x aligned to 8 bytes); complex = 0: x is used as it is.  1 <= n_chroma <= SYG_CHROMA_NC_MAX.
 *
 * syg_chroma_fold_rows_f32: x [B, T, F(, 2)] contiguous (frame-major, as the STFT entries leave it), tab [n_chroma, F]
 *   -> out [B, n_chroma, T] contiguous.  A wave a frame, the lanes along the bins, float32 sums k = lane, lane + 64, ...
 *   then a butterfly; the table is staged in LDS where it fits SYG_CHROMA_TABLE_LDS_MAX bytes beside the tile's sums.
 * syg_chroma_fold_bins_f32: x [B, K, T(, 2)], unit stride along T, strides sxb / sxk in floats (even for complex input);
 *   wt [K, n_chroma] (the weights of one bin side by side) -> out [B, n_chroma, T].  A lane a frame, k ascending.
 *   P > 0: after the norm the frame is L1-normalised and out [B, P, T] = phi [P, n_chroma] times it (tonnetz: P = 6),
 *   P <= SYG_CHROMA_P_MAX.  At most 65535 clips a call.
 * syg_chroma_cens_f32: x [B, n_chroma, T] (strides in floats) -> out [B, n_chroma, T] contiguous: the L1 norm per frame,
 *   q = 0.25 (count of steps 0.4 / 0.2 / 0.1 / 0.05 below the value), out[c, t] = sum_j win[j] q[c, t - left + j] (zeros
 *   beyond the row, j ascending; win [n_win] <= SYG_CHROMA_CENS_WIN_MAX taps as scipy.ndimage.convolve applies them),
 *   then the norm `norm` (librosa: 3, L2).  n_win = 1, win = {1}: no smoothing.  SYG_CHROMA_CENS_TILE frames a workgroup, any T.
 * syg_tuning_hist_f32: x = S [B, T, F(, 2)], F = 1 + n_fft / 2.  The peaks of librosa.piptrack: with ref = threshold
 *   max_k S and x = S where S > ref, else 0, bin k in [k_lo, k_hi) is a peak where x[k] > x[k - 1] and x[k] >= x[k + 1]
 *   (edges repeated); a = S[k + 1] + S[k - 1] - 2 S[k], b = (S[k + 1] - S[k - 1]) / 2, shift = -b / a where |b| < |a| (0 at
 *   the last bin), pitch = (k + shift) sr / n_fft, mag = S[k] + 0.5 b shift, all float64 from the float32 S.
 *   counts != NULL: per clip th = the exact median of mag (the mean of the two middle values of an even count; radix
 *   selection over the bit patterns), r = frac(bins_per_octave log2(pitch / 27.5)) moved into [-0.5, 0.5), and
 *   counts [B, n_bins] int32 = the peaks with mag >= th by edges[i] <= r < edges[i + 1] (edges: device float64
 *   [n_bins + 1]); n_peaks [B] int32 = all peaks of the clip.  Needs `work` of syg_tuning_hist_work_bytes(B, T, k_lo, k_hi)
 *   bytes, 8-byte aligned.  pitch_out / mag_out (both or neither) [B, T, F] float32: piptrack's dense pair.
 * ------------------------------------------------------------------------------- */
enum {
  SYG_CHROMA_NC_MAX = 0,         /* largest n_chroma */
  SYG_CHROMA_ROW_TILE = 1,       /* frames of a wave's tile of syg_chroma_fold_rows_f32 */
  SYG_CHROMA_TABLE_LDS_MAX = 2,  /* LDS bytes up to which syg_chroma_fold_rows_f32 stages its table */
  SYG_CHROMA_P_MAX = 3,          /* rows of the output transform, at most */
  SYG_CHROMA_CENS_TILE = 4,      /* frames of a CENS workgroup */
  SYG_CHROMA_CENS_WIN_MAX = 5,   /* taps of the CENS window, at most */
  SYG_CHROMA_HIST_BINS_MAX = 6,  /* bins of the tuning histogram, at most */
  SYG_CHROMA_MAX_ELEMS = 7       /* elements of an input, at most */
};
int64_t syg_chroma_constants(int key);
int syg_chroma_fold_rows_f32(const float* x, int64_t B, int64_t T, int F, int complex_in, int power, const float* tab, int n_chroma,
                             int has_threshold, float threshold, int norm, float* out, void* stream);
int syg_chroma_fold_bins_f32(const float* x, int64_t B, int64_t K, int64_t T, int64_t sxb, int64_t sxk, int complex_in, int power,
                             const float* wt, int n_chroma, int has_threshold, float threshold, int norm, const float* phi, int P,
                             float* out, void* stream);
int syg_chroma_cens_f32(const float* x, int64_t B, int n_chroma, int64_t T, int64_t sxb, int64_t sxk, const float* win, int n_win,
                        int left, int norm, float* out, void* stream);
int64_t syg_tuning_hist_work_bytes(int64_t B, int64_t T, int k_lo, int k_hi);
int syg_tuning_hist_f32(const float* x, int64_t B, int64_t T, int F, int complex_in, int power, double sr, int n_fft, int k_lo,
                        int k_hi, double threshold, double bins_per_octave, const double* edges, int n_bins, int32_t* counts,
                        int32_t* n_peaks, float* pitch_out, float* mag_out, void* work, int64_t work_bytes, void* stream);

/* -------------------------------------------------------------------------------
 * Per-channel energy normalisation (pcen.hip): librosa 0.10's pcen of x [B, M, T] float32 >= 0, unit stride along T,
 * strides sxb / sxk (in floats, non-negative) over B and M; out strided the same way (sok >= T).  The float64
 * restatement tests/pcen_ref.py is the contract.  Per row (b, m), with S = scale x:
 *   ref    = S, or for max_size > 1 scipy.ndimage.maximum_filter1d(S, max_size, axis = bands) (mode reflect, origin 0:
 *            bands m - max_size / 2 ... m - max_size / 2 + max_size - 1)
 *   y      = scipy.signal.lfilter([b], [1, b - 1], ref, zi = z):  y[0] = b ref[0] + z,  y[t] = y[t-1] + b (ref[t] - y[t-1]),
 *            closing state (1 - b) y[T-1]; the state is float64.  zi [B, M] float64 (NULL: 1 - b, lfilter_zi's value,
 *            not scaled by the first frame); zf [B, M] float64 (NULL: not wanted).
 *   smooth = exp(-gain log(eps + y))
 *   out    = log1p(S smooth) where power = 0; exp(power (log S + log smooth)) where bias = 0 (0 at S = 0); otherwise
 *            bias^power expm1(power log1p(S smooth / bias)); float32.
 * Parameters: the scalars gain, bias, power >= 0, eps > 0, 0 < b <= 1, or with tab != NULL a device table [M]
 * [SYG_PCEN_TABLE_WORDS] of float64 per band: b, (1 - b)^SYG_PCEN_TILE, eps, gain, power, bias, bias^power, the case
 * (0 general, 1 power = 0, 2 bias = 0); the scalars are then ignored and the table's values are its maker's to check
 * (sygnals_amd/_pcen.py).
 * form 0: the rule (syg_pcen_form: 0 resident, 1 tiled; -1 for arguments it does not serve), 1 resident, 2 tiled.
 *   Resident: a workgroup holds up to SYG_PCEN_BANDS bands of a clip and the max_size - 1 halo bands in LDS (at most
 *   SYG_PCEN_LDS_MAX bytes: fewer bands where rows are long), a lane a row; the rule takes it for T <= SYG_PCEN_RESIDENT_T
 *   while a band fits.  Tiled: a wave takes SYG_PCEN_TILE frames of a row; with more than one tile a row a first launch
 *   writes every tile's closing state from rest to work (syg_pcen_work_bytes(B, M, T) bytes, 0 for one tile) and the
 *   second folds them in index order in float64.  No atomics: a call repeats its bits, a batch equals its rows.
 * Rejected before any device work: null x / out, an empty axis, bad strides, a result above 2^31 elements, a scalar
 * outside its range, max_size outside [1, M], a scale that is not positive and finite, an unknown form, an out that
 * overlaps x (out = x itself is served with max_size = 1), a resident row that does not fit, a missing workspace.
 * ------------------------------------------------------------------------------- */
enum {
  SYG_PCEN_TILE = 0,         /* frames of a tile of the tiled form */
  SYG_PCEN_BANDS = 1,        /* bands of a resident workgroup, at most */
  SYG_PCEN_RESIDENT_T = 2,   /* the rule: longest resident row */
  SYG_PCEN_LDS_MAX = 3,      /* LDS bytes of a workgroup, at most: two workgroups a CU */
  SYG_PCEN_GRID_MAX = 4,     /* workgroups of a launch, at most */
  SYG_PCEN_UNITS = 5,        /* tiles (waves) of a workgroup of the tiled form */
  SYG_PCEN_MAX_OUT = 6,      /* elements of a result, at most */
  SYG_PCEN_TABLE_WORDS = 7   /* float64 words of a band in tab */
};
int64_t syg_pcen_constants(int key);
int syg_pcen_form(int64_t T, int64_t M, int64_t max_size);
int64_t syg_pcen_work_bytes(int64_t B, int64_t M, int64_t T);
int syg_pcen_f32(const float* x, int64_t B, int64_t M, int64_t T, int64_t sxb, int64_t sxk, float* out, int64_t sob,
                 int64_t sok, double gain, double bias, double power, double eps, double b, const double* tab,
                 int64_t max_size, double scale, const double* zi, double* zf, int form, void* work, int64_t work_bytes,
                 void* stream);

/* -------------------------------------------------------------------------------
 * Loudness metering (loudness.hip): ITU-R BS.1770 / EBU R128 on clips x [B, C, L] float32, unit stride along L, strides
 * sb / sc (in floats, non-negative, rows not overlapping) over B and C; mono rows are C = 1.  The float64 restatement
 * tests/loudness_ref.py is the contract; the K-weighting design is sygnals_amd/_loudness.py's.  fs is an integer rate in
 * [SYG_LOUDNESS_FS_MIN, SYG_LOUDNESS_FS_MAX].  Segment j is samples [s_j, s_j+1), s_j = j fs div 10; a row has
 * n_seg = 10 L div fs whole segments, n_m = max(0, n_seg - 3) momentary blocks (segments j ... j + 3) and
 * n_s = max(0, n_seg - 29) short-term blocks (segments j ... j + 29).
 *   syg_loudness_segments_f32   seg [B, C, n_seg] float64 = sum y^2 per segment, y = x through the cascade sos_host
 *       ([2, 6] float64 on the HOST, scipy's b0 b1 b2 a0 a1 a2 per section) from rest, in float64; y is never written.
 *       work: syg_loudness_segments_work_bytes(B, C, L, fs) bytes on the device, 8-byte aligned (0 bytes where
 *       n_seg = 0: nothing is launched, seg and work may be NULL).  Chunks of SYG_LOUDNESS_CHUNK samples, the scan of
 *       syg_sosfilt_f32; a chunk holds at most one segment boundary and writes two partial sums, added per segment
 *       with the chunks ascending.
 *   syg_loudness_blocks_f64     from seg and the channel weights [C] float64 (on the DEVICE), block power
 *       z_j = sum_c w_c (sum of the block's segments) / (s_j+K - s_j), loudness l_j = -0.691 + 10 log10 z_j:
 *       M [B, n_m] and S [B, n_s] float32 (row strides ldm / lds; -inf where z_j = 0), integ [B] float64 (blocks above
 *       -70, then above the power-mean of those less 10 LU; -inf where none is left), lra_thr [B] float64
 *       = max(-70, power-mean of the short-term values above -70, less 20 LU), +inf where none is above -70.  Any of
 *       the four may be NULL.  One workgroup per clip, float64 sums in a fixed order.
 *   syg_loudness_lra_f32        s_sorted [B, n_s] float32 ASCENDING (row stride lds) and thr [B] -> lra [B] float32
 *       (EBU Tech 3342): of the n values above thr, v[floor((n - 1) 0.95 + 1/2)] - v[floor((n - 1) 0.10 + 1/2)], the
 *       ranks in integers; 0 where n < 2.
 *   syg_true_peak_f32           peak [B] float32 = max over channels and samples of |scipy.signal.resample_poly(x, up, 1)|
 *       (padtype constant) without the oversampled signal: table [up, Kp] float32, n_pre_remove and Kp are the plan of
 *       syg_resample_poly_f32 at down = 1, and every value is that entry's, fma for fma.  up in [1, SYG_LOUDNESS_TP_UP_MAX]
 *       (up = 1: the sample peak, table may be NULL), Kp <= SYG_LOUDNESS_TP_KP_MAX.  The maximum is an integer maximum on
 *       the bit pattern of |y| (a NaN comes out on top), peak is cleared on the stream first.
 *   syg_loudness_gain_f64       gain [B] float64 = 10^((target_lufs - integ) / 20); with peak != NULL (linear true peak
 *       [B] float32) lowered to 10^(limit_dbtp / 20) / peak where gain peak is above that; 1 where integ is not finite.
 *   syg_gain_rows_f32           y[b, c, n] = float32(float64(x[b, c, n]) gain[b]), y strided yb / yc; y may be x.
 * No floating-point atomics anywhere: a call repeats its bits, and a batch equals its rows bit for bit wherever they lie.
 * Rejected before any device work: null pointers, B / C / L < 1, overlapping rows, fs outside the served rates, a zero
 * a0, up or Kp outside their bounds, a non-finite target or limit.
 * ------------------------------------------------------------------------------- */
enum {
  SYG_LOUDNESS_CHUNK = 0,       /* samples of a chunk of the segment-power passes */
  SYG_LOUDNESS_FS_MIN = 1,      /* lowest rate served: a chunk holds at most one segment boundary */
  SYG_LOUDNESS_FS_MAX = 2,      /* highest rate served */
  SYG_LOUDNESS_MOMENTARY = 3,   /* segments of a momentary block */
  SYG_LOUDNESS_SHORT_TERM = 4,  /* segments of a short-term block */
  SYG_LOUDNESS_TP_TILE = 5,     /* input samples a true-peak workgroup stages at a time */
  SYG_LOUDNESS_TP_UP_MAX = 6,   /* largest oversampling factor */
  SYG_LOUDNESS_TP_KP_MAX = 7    /* taps per phase, at most */
};
int64_t syg_loudness_constants(int key);
int64_t syg_loudness_segments_work_bytes(int64_t B, int64_t C, int64_t L, int fs);
int syg_loudness_segments_f32(const float* x, int64_t B, int64_t C, int64_t L, int64_t sb, int64_t sc, int fs,
                              const double* sos_host, double* seg, void* work, void* stream);
int syg_loudness_blocks_f64(const double* seg, int64_t B, int64_t C, int64_t n_seg, int fs, const double* weights, float* M,
                            int64_t ldm, float* S, int64_t lds, double* integ, double* lra_thr, void* stream);
int syg_loudness_lra_f32(const float* s_sorted, int64_t B, int64_t n_s, int64_t lds, const double* thr, float* lra,
                         void* stream);
int syg_true_peak_f32(const float* x, int64_t B, int64_t C, int64_t L, int64_t sb, int64_t sc, int up, int64_t n_pre_remove,
                      int Kp, const float* table, float* peak, void* stream);
int syg_loudness_gain_f64(const double* integ, const float* peak, int64_t B, double target_lufs, double limit_dbtp,
                          double* gain, void* stream);
int syg_gain_rows_f32(const float* x, int64_t B, int64_t C, int64_t L, int64_t sb, int64_t sc, const double* gain, float* y,
                      int64_t yb, int64_t yc, void* stream);

/* -------------------------------------------------------------------------------
 * Features back to audio (csrc/griffinlim.hip): the projection step of Griffin-Lim as librosa 0.10 `griffinlim` runs it
 * (the loop's other steps are syg_istft2048_f32 and syg_stft2048_c2c_f32), and the dense inversions of the mel and MFCC
 * maps.  tests/inverse_ref.py is the contract.
 * Geometry is the inverse STFT's: n_fft 2048, hann, hop 512, centred; spectra are frame-major [B, T, 1025, 2] float32,
 * magnitudes S [B, T, 1025] float32, all contiguous.
 *   syg_gl_project_f32      D = S A / (|A| + FLT_MIN), A = R - alpha P per bin (P NULL: A = R); alpha is
 *       momentum / (1 + momentum) rounded to float32 by the caller, in [0, 0.5).  The modulus is formed on A scaled by a
 *       power of two: a component of 1e-25 or 1e30 neither underflows nor overflows, |D| <= S (1 + 1e-6), A = 0 gives
 *       D = 0.  D may be R.  sums (may be NULL) [B, 2] float64: per clip sum (|R| - S)^2 and sum S^2 in float64, added in
 *       a fixed order that depends on T alone (no atomics: a call repeats its bits and a batch equals its rows); it needs
 *       work, syg_gl_project_work_bytes(B, T) bytes on the device, 8-byte aligned.
 *   syg_inv_dense_f32       out[b, t, f] = post(sum_m W[f, m] pre(X[b, m, t])): X mel-major [B, M, T], W [F, M] row-major,
 *       out frame-major [B, T, F], or [B, F, T] with out_mel_major = 1; float32 sums with m ascending.  pre 0: identity;
 *       1: db_to_power, pre_ref 10^(x / 10) (-inf dB is 0).  post 0: identity; 1: max(., 0)^(1 / post_arg), post_arg the
 *       power; 2: db_to_power, post_arg 10^(. / 10), post_arg the reference.  M <= 4096, F <= 65536.
 * Rejected before any device work: null pointers, B / T / M / F < 1, alpha outside [0, 0.5), sums without work, a
 * non-positive or non-finite pre_ref or post_arg.
 * ------------------------------------------------------------------------------- */
int64_t syg_gl_project_work_bytes(int64_t B, int64_t T);
int syg_gl_project_f32(const float* R, const float* P, const float* S, int64_t B, int64_t T, float alpha, float* D,
                       double* sums, void* work, void* stream);
int syg_inv_dense_f32(const float* X, int64_t B, int64_t M, int64_t T, const float* W, int64_t F, int pre, float pre_ref,
                      int post, float post_arg, float* out, int out_mel_major, void* stream);

/* -------------------------------------------------------------------------------
 * Non-negative matrix factorisation by multiplicative updates (csrc/nmf.hip): scikit-learn's solver="mu" at tol = 0,
 * which is what librosa.decompose.decompose runs when handed NMF(solver="mu").  tests/nmf_ref.py is the contract.
 * Frame-major and contiguous: V [B, T, F] float32, non-negative and finite; activations A [B, T, K] (sklearn's W);
 * components C [B, K, F] (sklearn's H), or one dictionary [1, K, F] for every clip with c_shared = 1.  eps is FLT_EPSILON.
 * Served: F in [1, 2049], K in [1, 64], T >= 1, B >= 1 (B T F <= 2^40, T <= 2^30).
 *   syg_nmf_f32             n_iter iterations in place on A and C, each the A-step, then the C-step with the new A:
 *       Frobenius  A <- A (V C^T) / (A (C C^T)),  C <- C (A^T V) / ((A^T A) C);
 *       KL         A <- A ((V / AC) C^T) / sum_f C,  C <- C (A^T (V / AC)) / sum_t A, AC raised to eps where below it;
 *       a denominator equal to 0 becomes eps; under KL an entry of the new C below 2^-52 (float64's epsilon) becomes 0, as
 *       sklearn has it.  update_A = 0 or update_C = 0 leaves that factor untouched (update_C = 0
 *       is librosa's fit=False).  Only V, A, C and K K + K floats of scratch a clip pass through memory.  No stopping
 *       rule, no regularisation.  form: how the contractions over F and T run -- SYG_NMF_FORM_FMA, plain fp32 FMA;
 *       SYG_NMF_FORM_MFMA, v_mfma_f32_16x16x4_f32 (exact fp32, another summation order); SYG_NMF_FORM_AUTO, the faster of
 *       the two as measured: MFMA from K = syg_nmf_constants(8) up.  work: syg_nmf_work_bytes(B, T, F, K) bytes on the device, 8-byte aligned.
 *   syg_nmf_divergence_f32  out [B] float64: sklearn's _beta_divergence of each clip, AC and the sum formed in float64
 *       from the float32 factors.  Frobenius: sum (V - AC)^2 / 2.  KL: sum over V > eps of V log(V / max(AC, eps)) - V,
 *       plus sum AC.  Sums are added in an order that depends on (T, F) alone.  work as above.
 *   syg_nmf_masks_f32       out [B, n_groups, T, F, 2] = D [B, T, F, 2] times the soft mask of each group,
 *       (sum_k G[g, k] A[t, k] C[k, f]) / max(sum_k A[t, k] C[k, f], eps), G [n_groups, K] row-major, n_groups <= 64.
 *   syg_nmf_constants(i)    0: largest K, 1: largest F, 2: largest n_groups, 3 / 4: frames of an A-step tile and bins of
 *       its chunk, 5 / 6: bins of a C-step tile and frames of its chunk, 7: chunk of the per-clip sums, 8: the smallest K that SYG_NMF_FORM_AUTO gives to the MFMA form; -1 past them.
 * Rejected before any device work: null pointers, sizes outside the served ranges, an unknown loss (Itakura-Saito and
 * other beta are not served), a negative n_iter, update_C with c_shared.
 * ------------------------------------------------------------------------------- */
#define SYG_NMF_FROBENIUS 0
#define SYG_NMF_KL 1
#define SYG_NMF_FORM_AUTO (-1)
#define SYG_NMF_FORM_FMA 0
#define SYG_NMF_FORM_MFMA 1
int syg_nmf_constants(int which);
int64_t syg_nmf_work_bytes(int64_t B, int64_t T, int64_t F, int64_t K);
int syg_nmf_f32(const float* V, int64_t B, int64_t T, int64_t F, int64_t K, float* A, float* C, int c_shared, int64_t n_iter,
                int loss, int update_A, int update_C, int form, void* work, void* stream);
int syg_nmf_divergence_f32(const float* V, const float* A, const float* C, int c_shared, int64_t B, int64_t T, int64_t F,
                           int64_t K, int loss, double* out, void* work, void* stream);
int syg_nmf_masks_f32(const float* D, const float* A, const float* C, int c_shared, const float* G, int64_t B, int64_t T,
                      int64_t F, int64_t K, int64_t n_groups, float* out, void* stream);

/* -------------------------------------------------------------------------------
 * Self-similarity (csrc/similarity.hip): the k nearest frames of every frame, the dense recurrence matrix of those lists,
 * librosa.decompose.nn_filter over them and the soft masks of REPET-SIM.  tests/similarity_ref.py is the contract.
 * Frame-major float32: X [B, T, D] the query frames (row stride ldx >= D, batch stride bsx), Y [B, T', D] the frames
 * searched (ldy, bsy; bsy = 0 shares one Y), or Y = NULL for self-similarity, where the candidates of row i are the j with
 * |i - j| >= width.  x_len / y_len [B] int32 on the device, or NULL: frames past a length are neither queries nor candidates.
 *   syg_sim_knn_f32   row i keeps its min(k, candidates) nearest candidates, ordered by distance, then by index: idx
 *       [B, T, k] int32 (-1 past the count), dist [B, T, k] (+inf past it), count [B, T] int32.  metric:
 *       SYG_SIM_SQEUCLIDEAN sum (x - y)^2, SYG_SIM_EUCLIDEAN its root, SYG_SIM_COSINE 1 - x.y / max(|x| |y|, FLT_MIN).
 *       The selection runs on v_mfma_f32_16x16x4_f32 dot products and the squared norms; the kept distances are formed
 *       again from the frames themselves and the list put in their order.  Equal frames give bit-equal distances.  Nothing
 *       of size T T' passes through memory.  work: syg_sim_knn_work_bytes(B, T, T', Y != NULL) bytes on the device (the
 *       squared norms), 8-byte aligned.  k <= syg_sim_k_max() = 256.
 *   syg_sim_dense_f32 out [B, T, T'] from the lists: SYG_SIM_CONNECTIVITY 1, SYG_SIM_DISTANCE the distance,
 *       SYG_SIM_AFFINITY exp(-distance / bandwidth[b]) (bandwidth [B] float64 on the device); 0 elsewhere.  sym keeps
 *       (i, j) only if i is in j's list too; self sets the diagonal to 1 (0 under SYG_SIM_DISTANCE).  rowmax [B, T], or
 *       NULL: the largest kept distance of each row, -1 where none is kept; out may be NULL where rowmax is wanted alone.
 *   syg_nn_filter_f32 out [B, T, F] (contiguous): out[b, i] aggregates S[b, j] (row stride lds, batch stride bss) over row
 *       i's list.  SYG_NN_MEAN; SYG_NN_AVERAGE sum w S / sum w with w = weights [B, T, k], or exp(-weights / bandwidth[b])
 *       where bandwidth is given (the weights are then distances); SYG_NN_MEDIAN numpy's median, an input value bit for
 *       bit at odd counts.  A frame with an empty list (or a zero sum of weights) keeps S[b, i].
 *   syg_repet_masks_f32  with Sf = min(S, R), R the filtered magnitudes: mask_b = softmask(Sf, margin_b (S - Sf), power),
 *       mask_f = softmask(S - Sf, margin_f Sf, power), librosa.util.softmask without split_zeros; n cells.
 * Rejected before any device work: null pointers, sizes outside the served ranges, k outside [1, 256], width < 1, a width
 * other than 1 with Y, an unknown metric (cityblock has no contraction form), mode or aggregate, a row stride below the
 * row's length, sym or self on a matrix that is not square, non-positive margins or power.
 * ------------------------------------------------------------------------------- */
#define SYG_SIM_EUCLIDEAN 0
#define SYG_SIM_SQEUCLIDEAN 1
#define SYG_SIM_COSINE 2
#define SYG_SIM_CONNECTIVITY 0
#define SYG_SIM_DISTANCE 1
#define SYG_SIM_AFFINITY 2
#define SYG_NN_MEAN 0
#define SYG_NN_AVERAGE 1
#define SYG_NN_MEDIAN 2
int syg_sim_k_max(void);
int64_t syg_sim_knn_work_bytes(int64_t B, int64_t T, int64_t Ty, int has_y);
int syg_sim_knn_f32(const float* X, const float* Y, int64_t B, int64_t T, int64_t Ty, int64_t D, int64_t ldx, int64_t ldy,
                    int64_t bsx, int64_t bsy, const int* x_len, const int* y_len, int64_t k, int64_t width, int metric, int* idx,
                    float* dist, int* count, void* work, void* stream);
int syg_sim_dense_f32(const int* idx, const float* dist, const int* count, int64_t B, int64_t T, int64_t Ty, int64_t k, int mode,
                      int sym, int self, const double* bandwidth, float* out, float* rowmax, void* stream);
int syg_nn_filter_f32(const float* S, int64_t B, int64_t T, int64_t F, int64_t lds, int64_t bss, const int* idx, const int* count,
                      int64_t k, const float* weights, const double* bandwidth, int aggregate, float* out, void* stream);
int syg_repet_masks_f32(const float* S, const float* Sf, int64_t n, double margin_b, double margin_f, double power, float* mask_f,
                        float* mask_b, void* stream);

/* -------------------------------------------------------------------------------
 * Viterbi decoding (csrc/sequence.hip): the most likely state path of a hidden Markov chain, the recurrence of
 * librosa.sequence.viterbi, viterbi_discriminative and viterbi_binary.  tests/sequence_ref.py is the contract.
 *   emission   [B, S, T] float32 (SYG_VITERBI_F32) or float64 (SYG_VITERBI_F64) on the device, addressed as
 *              emission[b stride_b + j stride_s + t stride_t] (element strides, none negative): [B, S, T] and [B, T, S]
 *              blocks are both read in whole lines.  log_domain: the values are log-probabilities and are used as given;
 *              otherwise lp = log(emission + eps), taken in float64.
 *   lengths    [B] int32 on the device, each in 1 .. T, or NULL (every sequence has T frames): states past a length
 *              are -1.  (The kernels clamp a length into 1 .. T; the caller checks it.)
 *   log_trans  float64 [S, S] (row = source state), batch stride trans_bs = 0 (shared) or S S; log_init float64 [S],
 *              init_bs = 0 or S; log_marginal float64 [S] (marginal_bs = 0 or S), or NULL: lp[t, j] -= log_marginal[j],
 *              the discriminative form.  These logs are made on the host.
 *   value[0, j] = lp[0, j] + log_init[j];  ptr[t, j] = the FIRST i that maximises value[t-1, i] + log_trans[i, j];
 *   value[t, j] = lp[t, j] + (value[t-1, ptr] + log_trans[ptr, j]);  states[len-1] = the first argmax of value[len-1],
 *   states[t] = ptr[t+1, states[t+1]];  logp = value[len-1, states[len-1]].  Scores, additions and comparisons are
 *   float64 in this order and there are no atomics: the same call gives the same bits, a batch equals its rows.
 *   states [B, T] int32, logp [B] float64.  work: syg_viterbi_work_bytes(B, S, T) bytes on the device, 8-byte aligned
 *   (the back pointers: one byte each up to 256 states, two beyond).
 *   form: SYG_VITERBI_AUTO takes syg_viterbi_form(B, S); SYG_VITERBI_WIDE one workgroup a sequence and one thread a
 *   state (any S); SYG_VITERBI_NARROW one lane a sequence, S <= SYG_VITERBI_S_NARROW.  Both forms give the same bits.
 * Rejected before any device work: null pointers, an unknown dtype or form, S outside 1 .. SYG_VITERBI_S_MAX, B or T
 * below 1, more than 2^40 back pointers, a workspace that is too small, a negative stride, a batch stride of a table that
 * is neither 0 nor the table's size, an eps that is negative or not finite, the narrow form above its S.
 * ------------------------------------------------------------------------------- */
#define SYG_VITERBI_F32 0
#define SYG_VITERBI_F64 1
#define SYG_VITERBI_AUTO 0
#define SYG_VITERBI_WIDE 1
#define SYG_VITERBI_NARROW 2
enum {
  SYG_VITERBI_S_MAX = 0,     /* largest S */
  SYG_VITERBI_S_LDS = 1,     /* largest S whose log_trans lives in LDS (beyond it is read from global memory) */
  SYG_VITERBI_S_NARROW = 2,  /* largest S of the narrow form */
  SYG_VITERBI_TILE = 3       /* frames of an emission tile staged through LDS */
};
int64_t syg_viterbi_constants(int key);
int syg_viterbi_form(int64_t B, int64_t S);
int64_t syg_viterbi_work_bytes(int64_t B, int64_t S, int64_t T);
int syg_viterbi_f32(const void* emission, int dtype, int log_domain, int64_t stride_b, int64_t stride_s, int64_t stride_t,
                    int64_t B, int64_t S, int64_t T, const int* lengths, const double* log_trans, int64_t trans_bs,
                    const double* log_init, int64_t init_bs, const double* log_marginal, int64_t marginal_bs, double eps,
                    void* work, int64_t work_bytes, int* states, double* logp, int form, void* stream);

/* -------------------------------------------------------------------------------
 * Structure analysis (csrc/structure.hip): what librosa.segment does with a recurrence matrix and the feature sequence
 * behind it.  tests/structure_ref.py is the contract.  Matrices are float32 [B, rows, cols] on the device with a row stride
 * (ld*) and a batch stride (bs*, 0 shares one matrix); outputs are contiguous.
 *   syg_lag_shear_f32   recurrence_to_lag (inverse = 0) and lag_to_recurrence (inverse = 1) of square matrices [t, t].
 *       n = 2 t (pad = 1) or t.  axis 1 (librosa's -1): lag [n, t], lag[l, i] = R~[(l + i) mod n, i], R~ being R with zero
 *       rows appended; rec[r, i] = lag[(r - i) mod n, i], r < t.  axis 0: the transpose of all of it, lag [t, n].  A read
 *       and a write an element.
 *   syg_path_enhance_f32   out[b, r, c] = max over filters f of sum over the taps e in [fstart[f], fstart[f + 1]) of
 *       w_e R~[b, r + dr_e, c + dc_e], clipped at 0 with clip = 1.  R [B, T, T'] may be rectangular; R~ extends it by the
 *       boundary rule `mode` (scipy.ndimage's: SYG_BOUNDARY_*; cval fills under SYG_BOUNDARY_CONSTANT), folded as often
 *       as the offsets need.  taps: int32 [n_taps, 4] on the device, (dr, dc, the weight's float32 bits, 0); fstart int32
 *       [n_filters + 1] on the device.  dr_min .. dc_max: the extent of the offsets; each spans at most
 *       SYG_STRUCT_PATH_SPAN_MAX.  (The kernel clamps a tap's offsets into that extent and fstart into [0, n_taps].)  The
 *       taps of a filter are summed in list order into four float32 partial sums (tap e into sum e mod 4, counted from
 *       the filter's first tap) combined as (s0 + s1) + (s2 + s3): the same call gives the same bits, a batch equals its rows.
 *   syg_diag_median_f32   timelag_filter(median_filter, size = (1, w)) of square R [B, t, t] without the lag matrix:
 *       out[r, i] = median over j < w of R~[(r - i + c_j) mod n, c_j], c_j = m(i + j - w / 2), m the boundary rule along
 *       time (cval where the constant fills), R~ zero in rows t .. n - 1, n = 2 t (pad = 1) or t.  axis 0: the transpose.
 *       w odd, 1 .. SYG_STRUCT_MEDIAN_W_MAX; the result is an input value bit for bit (-0 orders below +0).
 *   syg_agglomerative_f32   Ward clustering of chains of frames.  X [B, T, D] frame-major (frame stride ldx, batch stride
 *       bsx).  Span s covers length[s] frames from frame offset[s] of the flattened [B T] frame index and stays inside its
 *       clip; spans must not overlap.  Start from singletons, merge the neighbouring pair with the least
 *       n_a n_b / (n_a + n_b) |S_a / n_a - S_b / n_b|^2 (float64; the leftmost on ties) until k[s] segments remain.  bounds
 *       [n_spans, k_max] int32: the segment starts relative to the span, ascending, -1 past k[s]; count [n_spans].  offset,
 *       length, k: int32 [n_spans] on the device (the kernel clamps them into the clip, max_len and k_max).  max_len: the
 *       longest span, at most SYG_STRUCT_AGG_T_MAX.  work: syg_agglomerative_work_bytes(B, T, D) bytes on the device
 *       (the float64 segment sums), 8-byte aligned.
 *   syg_segment_sync_f32   out [B, n_seg, D]: SYG_SYNC_MEAN (summed in float64, ascending), SYG_SYNC_MAX or SYG_SYNC_MIN of
 *       the frames [edges[j], edges[j + 1]) of X [B, T, D]; edges int32 [n_seg + 1] on the device, batch stride edge_bs = 0
 *       (shared) or n_seg + 1.  An empty segment gives 0.  The median is not served.
 * Rejected before any device work: null pointers, sizes outside the served ranges, flags other than 0 or 1, an unknown
 * boundary rule or aggregate, an even w or one above the cap, offsets that span more than the cap, a span or k_max above
 * its cap, a stride below the row's length, a workspace that is too small.
 * ------------------------------------------------------------------------------- */
#define SYG_BOUNDARY_REFLECT 0
#define SYG_BOUNDARY_MIRROR 1
#define SYG_BOUNDARY_NEAREST 2
#define SYG_BOUNDARY_WRAP 3
#define SYG_BOUNDARY_CONSTANT 4
#define SYG_SYNC_MEAN 0
#define SYG_SYNC_MAX 1
#define SYG_SYNC_MIN 2
enum {
  SYG_STRUCT_AGG_T_MAX = 0,       /* frames of the longest span syg_agglomerative_f32 serves */
  SYG_STRUCT_MEDIAN_W_MAX = 1,    /* widest window of syg_diag_median_f32 */
  SYG_STRUCT_PATH_TILE_ROWS = 2,  /* outputs of a path_enhance tile */
  SYG_STRUCT_PATH_TILE_COLS = 3,
  SYG_STRUCT_PATH_SPAN_MAX = 4,   /* widest extent (max - min) of the tap offsets along an axis */
  SYG_STRUCT_SHEAR_T_MAX = 5      /* largest t of syg_lag_shear_f32 and syg_diag_median_f32 */
};
int64_t syg_structure_constants(int key);
int syg_lag_shear_f32(const float* in, int64_t B, int64_t t, int64_t ldi, int64_t bsi, int inverse, int axis, int pad, float* out,
                      void* stream);
int syg_path_enhance_f32(const float* R, int64_t B, int64_t T, int64_t Tc, int64_t ldr, int64_t bsr, const int* taps, int64_t n_taps,
                         const int* fstart, int n_filters, int dr_min, int dr_max, int dc_min, int dc_max, int mode, float cval,
                         int clip, float* out, void* stream);
int syg_diag_median_f32(const float* R, int64_t B, int64_t t, int64_t ldr, int64_t bsr, int w, int axis, int pad, int mode, float cval,
                        float* out, void* stream);
int64_t syg_agglomerative_work_bytes(int64_t B, int64_t T, int64_t D);
int syg_agglomerative_f32(const float* X, int64_t B, int64_t T, int64_t D, int64_t ldx, int64_t bsx, const int* offset,
                          const int* length, const int* k, int64_t n_spans, int64_t max_len, int64_t k_max, int* bounds, int* count,
                          void* work, int64_t work_bytes, void* stream);
int syg_segment_sync_f32(const float* X, int64_t B, int64_t T, int64_t D, int64_t ldx, int64_t bsx, const int* edges, int64_t n_seg,
                         int64_t edge_bs, int aggregate, float* out, void* stream);

/* -------------------------------------------------------------------------------
 * Kaldi-compatible front end (csrc/kaldi_front.hip): torchaudio.compliance.kaldi.fbank / mfcc on y [B, L] float32 clips
 * (row stride ldy), samples in, features out, one launch.  tests/kaldi_ref.py is the contract; the host tables are made
 * in sygnals_amd/_kaldi.py (float64, rounded to float32 once).
 *   Frames of wl samples, zero-padded on the right to n_fft for the transform.  snip_edges = 1: T = 1 + (L - wl) / hop
 *   (0 if L < wl), frame t starts at t hop.  snip_edges = 0: T = (L + hop / 2) / hop, frame t starts at
 *   t hop + hop / 2 - wl / 2, an index s outside [0, L) reflected (s <- -s - 1 or 2 L - 1 - s until inside).  Per frame:
 *   dither N(0, 1) (Philox, keyed by seed, clip, frame, sample), the frame mean removed (remove_dc; float64 sum, rounded
 *   once), pre-emphasis x[i] -= preemph x[i - 1] with x[-1] := x[0], the window.  The log-energy log(max(sum x^2, eps)) is
 *   taken before the pre-emphasis (raw_energy = 1) or behind the window, and floored at log(energy_floor) if that is > 0.
 *   |rfft|^2 (use_power = 1) or |rfft| of the bins [0, n_fft / 2) goes onto the filterbank; use_log = 1 writes
 *   E > eps ? logf(E) : log_eps, with eps = 1.1920929e-07 and log_eps the float32 nearest to log(eps).
 * Tables, float32 on the device:
 *   window   [wl]
 *   twiddle  [n_fft + n_fft / 2][2]: W_n_fft^k, k < n_fft, then W_(n_fft/2)^k, k < n_fft / 2 (cos, sin of -2 pi k / n)
 *   basis_p  [16 ceil(n_mels / 16), n_fft / 2], rows past n_mels zero, 16-byte aligned (the Nyquist bin carries no weight)
 *   dct      [num_ceps, n_mels]: the orthonormal DCT-II rows times the lifter, or null for the filterbank output
 * Output out[b sob + t sot + c soc], one of sot and soc being 1: [B, C, T] and [B, T, C] are both one launch.
 *   dct null: C = n_mels + use_energy; the energy column is first, or last under htk_compat.
 *   dct set:  C = num_ceps; use_energy replaces coefficient 0 by the log-energy, htk_compat moves coefficient 0 to the end;
 *             fb (or null) receives the log filterbank [B, T, n_mels] through its own strides.
 * Served: n_fft 256, 512, 1024 or 2048, 2 <= wl <= n_fft, hop >= 1, 3 <= n_mels <= 256, 1 <= num_ceps <= n_mels,
 * 0 <= preemph <= 1, dither >= 0, energy_floor >= 0.  Everything else is rejected before any device work, as are null
 * pointers, a T that does not follow the framing rule and strides below the row's length.  No atomics: a call repeats its
 * bits and a batch equals its rows.  A workgroup takes SYG_KALDI_TILE frames of a clip; the grid is capped at
 * SYG_KALDI_WGS_PER_CU workgroups a CU and loops over the rest.
 * ------------------------------------------------------------------------------- */
enum {
  SYG_KALDI_TILE = 0,         /* frames of a workgroup's tile */
  SYG_KALDI_N_MIN = 1,        /* smallest and */
  SYG_KALDI_N_MAX = 2,        /* largest padded frame length (powers of two between them) */
  SYG_KALDI_MEL_MIN = 3,
  SYG_KALDI_MEL_MAX = 4,
  SYG_KALDI_LDS_MAX = 5,      /* LDS bytes of a workgroup, at most */
  SYG_KALDI_WGS_PER_CU = 6,   /* workgroups a CU of the capped grid */
  SYG_KALDI_LDS_WORST = 7     /* LDS bytes of the largest served shape */
};
int64_t syg_kaldi_constants(int key);
int syg_kaldi_fbank_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int wl, int hop, int n_fft, int snip_edges, int64_t T,
                        const float* window, const float* twiddle, const float* basis_p, int n_mels, float preemph,
                        int remove_dc, int raw_energy, int use_power, int use_log, float log_eps, float energy_floor,
                        float dither, uint64_t seed, int use_energy, int htk_compat, const float* dct, int num_ceps, float* out,
                        int64_t sob, int64_t sot, int64_t soc, float* fb, int64_t sfb, int64_t sft, int64_t sfc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYGNALS_HIP_H */
