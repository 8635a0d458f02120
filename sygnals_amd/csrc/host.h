// Host side of every entry point: the two device queries in front of a launch, the launch caps, the frame-count rules and
// the small integer helpers.  No device code.  `who` names the entry point in the message; a check returns SYG_OK or sets the
// last error and returns the code to pass on.  (What only the fused STFT front ends share is in stft_host.h.)
#pragma once
#include "common.h"

namespace syg {

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline bool is_pow2(int n) { return n >= 2 && (n & (n - 1)) == 0; }

// CU count of the CURRENT device, asked at every call (an attribute query, no device properties round trip): no
// process-wide cache that a second device or a second thread could read stale.  256 if the query fails: no error is
// reported here, the launch that follows a failed query fails too and SYG_CHECK_LAUNCH reports that.
inline int device_cu_count() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      cus <= 0)
    cus = 256;
  return cus;
}

constexpr int64_t MAX_GRID_Y = 65535;  // rows of a grid's y dimension: an entry loops or splits past it, or refuses more
// y dimension of a grid over `rows` rows
inline unsigned grid_rows(int64_t rows) { return (unsigned)(rows < MAX_GRID_Y ? rows : MAX_GRID_Y); }
// Rows of the piece [b0, b0 + per) of a batch of B rows that is launched `per` rows at a time
inline int64_t piece_rows(int64_t b0, int64_t B, int64_t per) { return B - b0 < per ? B - b0 : per; }
// Persistent grid: a workgroup for each of `want` pieces of work, at most wgs_per_cu a CU; the kernel loops over the rest
inline unsigned capped_grid(int64_t want, int wgs_per_cu) {
  const int64_t cap = (int64_t)device_cu_count() * wgs_per_cu;
  return (unsigned)(want < cap ? want : cap);
}

// workgroups a CU of the persistent grids (a figure that an LDS budget decides stays with its kernel)
constexpr int LPC_FRAMES_WGS_PER_CU = 8;       // lpc_frames_kernel
constexpr int LPC_ENVELOPE_WGS_PER_CU = 32;    // lpc_envelope_kernel
constexpr int PITCH_FRAMES_WGS_PER_CU = 16;    // pitch_frames_kernel
constexpr int ISTFT_WGS_PER_CU = 64;           // istft2048_kernel
constexpr int CEPS_POINTWISE_WGS_PER_CU = 32;  // the pointwise cepstrum kernels
constexpr int NOISE_WGS_PER_CU = 8;            // noise_resident_kernel, noise_gen_resident_kernel, noise_gen_scale_kernel

// Dynamic LDS of a launch.  Up to 64 KiB needs no attribute (and no runtime call).  Above it the attribute is set at
// every launch: it belongs to the (function, device) pair, and a per-process "already set" flag would leave a second
// device without it.
inline int reserve_dynamic_lds(const char* who, const void* kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return SYG_OK;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) return SYG_OK;
  set_error("%s: cannot reserve %zu B LDS: %s", who, bytes, hipGetErrorString(e));
  return SYG_E_LAUNCH;
}

// Frames of a clip of L samples.  Centred, frame t is centred on sample t * hop: manager.py:149-157's rule, which every
// entry point but one follows.
inline int64_t frames_expected(int64_t L, int frame, int hop, int center) {
  return center ? 1 + L / hop : (L >= frame ? 1 + (L - frame) / hop : 0);
}

// librosa.feature.rms's rule (syg_hnr_rows_f32): the frames that fit the signal padded by frame / 2 on both sides.  One
// less than frames_expected for an odd frame length when hop divides L; the same otherwise.
inline int64_t frames_padded(int64_t L, int frame, int hop, int center) {
  return center ? 1 + (L + 2 * (frame / 2) - frame) / hop : (L >= frame ? 1 + (L - frame) / hop : 0);
}

// T against the count of the entry point's rule (frames_expected or frames_padded)
inline int check_framing(const char* who, int64_t T, int64_t Texp) {
  SYG_REQUIRE(T >= 1 && T == Texp, "%s: T=%lld does not match the framing rule (%lld)", who, (long long)T, (long long)Texp);
  return SYG_OK;
}

}  // namespace syg
