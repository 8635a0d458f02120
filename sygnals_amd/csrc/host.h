// Host side of every entry point: the two device queries in front of a launch, the frame-count rules and the small
// integer helpers.  No device code.  `who` names the entry point in the message; a check returns SYG_OK or sets the
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
