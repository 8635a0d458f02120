// Host side of the fused STFT front ends (stft_mel.hip, stft_mel_pow2.hip, stft_mel_w1024_seg.hip, stft_mel_w4096.hip,
// stft_mel_wseg_small.hip) on top of host.h: the argument checks their entry points share and the contrast plan, row
// and MFCC arguments an entry point hands to its kernel, and the launch tail of the free-running front ends.  No device
// code.  `who` names the entry point in the message; every check returns SYG_OK or sets the last error and returns the
// code to pass on.
#pragma once
#include "host.h"
#include <string.h>

namespace syg {

// y [B, L] (row stride ldy), window, twiddle and the frame count T of manager.py:149-157's framing rule
inline int check_clips(const char* who, const float* y, int64_t B, int64_t L, int64_t ldy, int n_fft, int hop, int center,
                       int64_t T, const float* window, const float* twiddle) {
  SYG_REQUIRE(y && window && twiddle, "%s: null pointer argument", who);
  SYG_REQUIRE(B >= 1 && L >= 1 && ldy >= L, "%s: need B >= 1, L >= 1, ldy >= L (B=%lld L=%lld ldy=%lld)", who, (long long)B,
              (long long)L, (long long)ldy);
  SYG_REQUIRE(hop >= 1, "%s: hop must be >= 1 (got %d)", who, hop);
  return check_framing(who, T, frames_expected(L, n_fft, hop, center));
}

// frames-per-clip limit of the entry points with statistics / contrast rows (below it a clip's [SYG_NSTAT, T] float
// block stays under 2^32 bytes)
inline int check_row_frames(const char* who, int64_t T) {
  SYG_REQUIRE(T < ((int64_t)1 << 27), "%s: too many frames per clip (T=%lld, at most 2^27 - 1)", who, (long long)T);
  return SYG_OK;
}

// parameters of the statistics rows (looked at only when stats_out is given)
inline int check_stats_args(const char* who, float sr, float roll_percent, float bw_p, int stats_mask) {
  SYG_REQUIRE(sr > 0.f && roll_percent >= 0.f && roll_percent <= 1.f && bw_p > 0.f && (stats_mask & 31) != 0 && stats_mask > 0 &&
                  stats_mask < 64, "%s: invalid statistics parameters", who);
  return SYG_OK;
}

// cplan_host (HOST int32 [1 + 3 SYG_MAX_BANDS] {n_rows, lo[], hi[], k[]}; bands inside bins 0 .. n_bins - 1) -> the
// n_rows / ascending / lo / hi / k fields of `plan` (ContrastPlan of stft_mel.hip, RowArgs of row_features.h), which the
// caller has zeroed and which stay zero without contrast_out
template <class Plan>
int parse_contrast_plan(const char* who, int n_bins, const float* contrast_out, const int32_t* cplan_host, Plan& plan) {
  if (!contrast_out) return SYG_OK;
  SYG_REQUIRE(cplan_host, "%s: contrast_out given without cplan_host", who);
  plan.n_rows = cplan_host[0];
  SYG_REQUIRE(plan.n_rows >= 1 && plan.n_rows <= SYG_MAX_BANDS, "%s: contrast rows must be in [1, %d]", who, SYG_MAX_BANDS);
  for (int r = 0; r < plan.n_rows; ++r) {
    plan.lo[r] = cplan_host[1 + r];
    plan.hi[r] = cplan_host[1 + SYG_MAX_BANDS + r];
    plan.k[r] = cplan_host[1 + 2 * SYG_MAX_BANDS + r];
    SYG_REQUIRE(plan.lo[r] >= 0 && plan.hi[r] <= n_bins && plan.lo[r] < plan.hi[r] && plan.k[r] >= 1 &&
                    plan.k[r] <= plan.hi[r] - plan.lo[r],
                "%s: contrast band %d invalid (lo=%d hi=%d k=%d)", who, r, plan.lo[r], plan.hi[r], plan.k[r]);
  }
  plan.ascending = 1;
  for (int r = 1; r < plan.n_rows; ++r)
    if (plan.lo[r] < plan.hi[r - 1] - 1 || plan.hi[r] < plan.hi[r - 1]) plan.ascending = 0;   // (a band may include the bin below it)
  return SYG_OK;
}

// The statistics / contrast arguments of a rows entry point of frame length n_fft, checked, as the kernel's RowArgs
template <class Rows>
int fill_row_args(const char* who, int n_fft, int64_t T, float sr, float roll_percent, float bw_p, int stats_mask,
                  float* stats_out, const int32_t* cplan_host, float* contrast_out, Rows& rw) {
  memset(&rw, 0, sizeof(rw));
  int rc = check_row_frames(who, T);
  if (!rc && stats_out) rc = check_stats_args(who, sr, roll_percent, bw_p, stats_mask);
  if (!rc) rc = parse_contrast_plan(who, n_fft / 2 + 1, contrast_out, cplan_host, rw);
  rw.binhz = sr / (float)n_fft; rw.roll_percent = roll_percent; rw.bw_p = bw_p; rw.smask = stats_mask;
  rw.stats_out = stats_out; rw.contrast_out = contrast_out;
  return rc;
}

// The dB + DCT arguments of an MFCC entry point, checked, as the members the kernels' argument structs share (MfccArgs of
// stft_mel.hip, Pow2Mfcc of stft_mel_pow2.hip; what else a struct holds -- padded frame count, row stride -- is the caller's).
//   count_rule      the entry point's wording of the n_mfcc rule: a format that is given (who, n_mfcc, n_mels)
//   rows_per_clip   rows between two clips of `out` (n_mfcc where the entry point has no such argument)
//   frame_limit     T must stay below it (0: the entry point has no limit of its own)
template <class Mfcc>
int fill_mfcc_args(const char* who, const char* count_rule, int n_mels, const float* dct, int n_mfcc, int rows_per_clip,
                   const float* lifter, float amin, float top_db, int ref_is_max, float ref_value, float* out, int64_t T,
                   int64_t frame_limit, Mfcc& mf) {
  SYG_REQUIRE(n_mfcc >= 1 && n_mfcc <= n_mels && rows_per_clip >= n_mfcc, count_rule, who, n_mfcc, n_mels);
  SYG_REQUIRE(amin >= 1.17549435e-38f, "%s: amin must be strictly positive (a normal float)", who);
  SYG_REQUIRE(ref_is_max == 0 || ref_is_max == 1, "%s: ref_is_max must be 0 or 1", who);
  SYG_REQUIRE(frame_limit == 0 || T < frame_limit, "%s: clip too long", who);
  mf.dct = dct; mf.lifter = lifter; mf.out = out; mf.n_mfcc = n_mfcc; mf.ref_is_max = ref_is_max;
  mf.ref_value = ref_value; mf.amin = amin; mf.top_db = top_db;
  return SYG_OK;
}

// piece table of the segment-sum projection (sygnals_amd._tables.pack_mel_segments / pack_mel_segments_rows) on the device
inline int check_segtab(const char* who, const float* segtab, int n_segtab, int expect_words, int n_mels, int max_mels) {
  SYG_REQUIRE(n_segtab == expect_words, "%s: the piece table has %d words, this library reads %d "
              "(sygnals_amd._tables.pack_mel_segments / pack_mel_segments_rows)", who, n_segtab, expect_words);
  SYG_REQUIRE(((uintptr_t)segtab) % 16 == 0, "%s: the piece table must be 16-byte aligned", who);
  SYG_REQUIRE(n_mels >= 1 && n_mels <= max_mels, "%s: n_mels must be in [1, %d] (got %d)", who, max_mels, n_mels);
  return SYG_OK;
}

// The launch of a free-running front end (frame lengths 1024 / 512 / 256 / 4096): `kern` -- the caller's choice between
// its <ROWS> instantiations -- on `threads` threads per workgroup with lds_bytes of dynamic LDS, on at most wgs_per_cu
// workgroups per CU (what is resident times the rounds the kernel's loop is good for).  The kernel takes args..., then
// the rows argument by value: *rows, or all zero (no rows) for a null pointer.
template <class Rows, class Kern, class... Args>
int launch_front(const char* who, Kern kern, int64_t wgs, int wgs_per_cu, int threads, size_t lds_bytes, hipStream_t st,
                 const Rows* rows, Args... args) {
  Rows rw;
  memset(&rw, 0, sizeof(rw));
  if (rows) rw = *rows;
  if (const int rc = reserve_dynamic_lds(who, (const void*)kern, lds_bytes)) return rc;
  hipLaunchKernelGGL(kern, dim3(capped_grid(wgs, wgs_per_cu)), dim3(threads), lds_bytes, st, args..., rw);
  SYG_CHECK_LAUNCH(who);
  return SYG_OK;
}

}  // namespace syg
