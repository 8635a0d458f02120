// Fused STFT(4096) -> |X|^2 -> mel for frame_length 4096: librosa.stft + np.abs(.)**2 + melspectrogram as the feature
// manager calls them (sygnals/core/features/manager.py:184-187, 198, 219-222) at `frame_length=4096`, one WAVE per frame.
//
// The transform is wave_fft.h's 4096-point real-input power spectrum (shared with welch_wave.hip): two 1024-point wave
// FFTs of the even and odd elements of z[m] = x[2m] + i x[2m+1], the radix-2 combine and the real-input split on mirror
// pairs, all in registers.  The 2049 powers go to the wave's own LDS row (the exchange scratch of the transforms aliases
// it) and the same wave projects the row onto the mel bands by segment sums (mel_segments.h, four passes of 64 lanes;
// table: sygnals_amd._tables.pack_mel_segments(..., n_pass=4)): no weight matrix, no spectrogram in HBM, no workgroup
// barrier behind the table set-up -- the waves of a workgroup only share constant tables.  The band values leave from the
// lanes that hold them (4-byte stores; the 16 waves of a CU work on consecutive frames, so the stores of a band meet in L2).
// ROWS (syg_stft_rows_w4096_f32): the same launch also hands the finished row to the per-frame row functions of
// row_features.h (spectral statistics, contrast tail means: 2049 bins, two 16-bin blocks per lane), behind the projection
// (which is skipped without a piece table); the results leave from the lanes that hold them.
#include "wave_fft.h"
#include "stft_host.h"

namespace syg {
namespace {
#include "mel_segments.h"
#include "row_features.h"

constexpr int W4_WAVES = 4;                         // waves per workgroup (186-245 registers: two waves per SIMD)
constexpr int W4_N = 4096, W4_BINS = 2049;
constexpr int W4_ROW = 2200;                        // row_pos(2048) = 2176, + the 17-word window of the last piece, 8-aligned
constexpr int W4_SEG_WORDS = 4 * 2 * 64 * 4;        // piece table, four passes

struct W4Lds {                                       // dynamic LDS in words, read by the kernel and its launcher
  static constexpr int O_ROW = 0;
  static constexpr int O_TW2 = O_ROW + W4_WAVES * W4_ROW;
  static constexpr int O_TW1 = O_TW2 + wfft::TW2_COMPLEX * 2;
  static constexpr int O_T2048 = O_TW1 + wfft::TW1_COMPLEX * 2;
  static constexpr int O_T4096 = O_T2048 + wfft::RFFT4096_TW * 2;
  static constexpr int O_SEG = O_T4096 + wfft::RFFT4096_TW * 2;
  static constexpr int O_CPL = O_SEG + W4_SEG_WORDS;       // ROWS: the contrast plan (lo / hi / k per band)
  static constexpr int TOTAL = O_CPL + 3 * SYG_MAX_BANDS;
  static_assert(W4_ROW >= 2 * wfft::SC_COMPLEX && W4_ROW % 4 == 0 && O_SEG % 4 == 0, "scratch inside the row, aligned tables");
};

__device__ __forceinline__ int w4_pos(int k) { return k + (k >> 4); }      // == _tables.row_pos

template <bool ROWS>
__global__ __launch_bounds__(W4_WAVES * 64) void stft_mel_w4096_kernel(
    const float* __restrict__ y, int64_t L, int64_t ldy, int hop, int pad, int64_t T, int64_t n_frames,
    const float* __restrict__ win, const float2* __restrict__ tw4096, const float4* __restrict__ segtab, int n_mels,
    float* __restrict__ mel_out, int aligned, RowArgs rw) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* prow = lds + W4Lds::O_ROW + w * W4_ROW;
  float2* sc = reinterpret_cast<float2*>(prow);
  float2* tw2l = reinterpret_cast<float2*>(lds + W4Lds::O_TW2);
  float2* tw1l = reinterpret_cast<float2*>(lds + W4Lds::O_TW1);
  float2* t2048 = reinterpret_cast<float2*>(lds + W4Lds::O_T2048);
  float2* t4096 = reinterpret_cast<float2*>(lds + W4Lds::O_T4096);
  float4* segl = reinterpret_cast<float4*>(lds + W4Lds::O_SEG);
  int* cpl = reinterpret_cast<int*>(lds + W4Lds::O_CPL);
  wfft::Lane lc;
  wfft::init_lane(lc, lane);
  wfft::init_tables(tw2l, tw1l, tw4096, 4096, tid, W4_WAVES * 64);
  wfft::init_rfft4096_tables(t2048, t4096, tw4096, tid, W4_WAVES * 64);
  if (ROWS) stage_contrast_plan(cpl, rw, tid);
  const bool project = !ROWS || segtab != nullptr;
  const bool scan8 = tri_stage_table<4>(segl, segtab, project, tid, W4_WAVES * 64);

  // consecutive frames go to consecutive waves (of this and of the neighbouring workgroups): overlapping samples meet in L2
  for (int64_t f = (int64_t)blockIdx.x * W4_WAVES + w; f < n_frames; f += (int64_t)gridDim.x * W4_WAVES) {
    const int64_t b = f / T, t = f - b * T;
    const float* yb = y + b * ldy;
    const int64_t s0 = t * (int64_t)hop - pad;
    int lf = lane;
    asm volatile("" : "+v"(lf));                    // (per-lane addresses are recomputed per frame, not hoisted)
    float2 ve[16], vo[16];
    {
      const float4* w4 = reinterpret_cast<const float4*>(win);
      if (aligned && s0 >= 0 && s0 + W4_N <= L) {
        const float4* sp = reinterpret_cast<const float4*>(yb + s0);
#pragma unroll
        for (int a = 0; a < 16; ++a) {
          const float4 r = sp[64 * a + lf], ww = w4[64 * a + lf];
          ve[a] = make_float2(r.x * ww.x, r.y * ww.y);
          vo[a] = make_float2(r.z * ww.z, r.w * ww.w);
        }
      } else {
        // frames over the clip's ends (the zero padding of center=True) and unaligned shapes: element loads
#pragma unroll
        for (int a = 0; a < 16; ++a) {
          const int64_t s = s0 + 4 * (64 * a + lf);
          const float4 ww = w4[64 * a + lf];
          float r[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) r[i] = (s + i >= 0 && s + i < L) ? yb[s + i] : 0.f;
          ve[a] = make_float2(r[0] * ww.x, r[1] * ww.y);
          vo[a] = make_float2(r[2] * ww.z, r[3] * ww.w);
        }
      }
    }
    float2 ek[2][4], em[2][4], ok[2][4], om[2][4], e512, o512;
    wfft::cfft1024(ve, lc, sc, tw1l, tw2l, lane, ek, em, e512);
    wfft::cfft1024(vo, lc, sc, tw1l, tw2l, lane, ok, om, o512);
    wave_lds_sync();                                // the scratch is dead: the row may be written
    wfft::rfft4096_pow(ek, em, e512, ok, om, o512, t2048, t4096, lf, [&](int slot, int bin, float p) {
      // (bin 1024 once: its repeat at k = 0 is dropped; bins 512 / 1536 from lane 0)
      const bool skip = slot >= 32 ? lf != 0 : (slot & 3) == 3 && bin == 1024;
      if (!skip) prow[w4_pos(bin)] = p;
    });
    wave_lds_sync();
    // ---- the row holds 4 |X|^2: project it (this wave alone), take the factor back at the store (exact)
    if (project) {
      float* mo = mel_out + (b * n_mels) * T + t;
      tri_project<4>(prow, segl, lf, scan8, [&](int band, float v) { mo[(int64_t)band * T] = 0.25f * v; });
    }
    if (ROWS) {
      // statistics / contrast of the row (4 |X|^2: PS = 1), one out-of-line call; the values come back in lanes 0 .. 15
      wave_lds_sync();                              // (the projection has read the row: a wide contrast band may park in it)
      lds_row pr = (lds_row)prow;
      const float3 fr = row_results<W4_BINS, 1, true>(pr, lf, rw, (lds_iptr)cpl);
      int lq = lane;
      asm volatile("" : "+v"(lq));
      store_row_results(rw, b, t, T, lq, fr.x, fr.y, fr.z);
    }
    wave_lds_sync();                                // the row is read: the next frame's transforms may use the scratch
  }
}

int w4096_launch(const char* who, const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center, int64_t T,
                 const float* window, const float* twiddle, const float* segtab, int n_segtab, int n_mels, float* mel_out,
                 const RowArgs* rows, hipStream_t st) {
  int rc = check_clips(who, y, B, L, ldy, W4_N, hop, center, T, window, twiddle);
  if (rc) return rc;
  if (segtab) {
    SYG_REQUIRE(mel_out, "%s: a piece table without mel_out", who);
    if ((rc = check_segtab(who, segtab, n_segtab, W4_SEG_WORDS, n_mels, 255))) return rc;
  }
  SYG_REQUIRE(((uintptr_t)window) % 16 == 0, "%s: the window must be 16-byte aligned", who);
  SYG_REQUIRE(B * T < ((int64_t)1 << 40), "%s: too many frames", who);
  const int pad = center ? W4_N / 2 : 0;
  const int aligned = (hop % 4 == 0) && (ldy % 4 == 0) && (((uintptr_t)y) % 16 == 0);
  const int64_t n_frames = B * T;
  // two workgroups per CU resident; a few rounds each
  return launch_front(who, rows ? stft_mel_w4096_kernel<true> : stft_mel_w4096_kernel<false>,
                      (n_frames + W4_WAVES - 1) / W4_WAVES, 2 * 4, W4_WAVES * 64, W4Lds::TOTAL * sizeof(float), st, rows, y, L,
                      ldy, hop, pad, T, n_frames, window, (const float2*)twiddle, (const float4*)segtab, n_mels, mel_out, aligned);
}

}  // namespace
}  // namespace syg

using namespace syg;

// y [B, L] (row stride ldy) -> mel_out [B, n_mels, T], power 2, for triangular filterbanks with a four-pass piece table
// (segtab: sygnals_amd._tables.pack_mel_segments(..., n_pass=4), 2048 words on the device, 16-byte aligned).  window [4096];
// twiddle: W_4096^k, k = 0 .. 4095.
extern "C" int syg_stft_mel_w4096_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center, int64_t T,
                                      const float* window, const float* twiddle, const float* segtab, int n_segtab,
                                      int n_mels, float* mel_out, void* stream) {
  SYG_REQUIRE(segtab && mel_out, "stft_mel_w4096: null pointer argument");
  return w4096_launch("stft_mel_w4096", y, B, L, ldy, hop, center, T, window, twiddle, segtab, n_segtab, n_mels, mel_out, nullptr,
                      (hipStream_t)stream);
}

// The per-frame statistics / contrast rows of syg_stft2048_mel_f32 for frame length 4096 (bins 0 .. 2048, bin frequency
// k sr / 4096) from the same launch: stats_out [B, SYG_NSTAT, T] (rows selected by stats_mask) and / or cplan_host +
// contrast_out [B, 2, n_rows, T] -- at least one; with segtab (and mel_out) also the mel power block, else nothing is projected.
extern "C" int syg_stft_rows_w4096_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center, int64_t T,
                                       const float* window, const float* twiddle, const float* segtab, int n_segtab, int n_mels,
                                       float* mel_out, float sr, float roll_percent, float bw_p, int stats_mask,
                                       float* stats_out, const int32_t* cplan_host, float* contrast_out, void* stream) {
  SYG_REQUIRE(stats_out || contrast_out, "stft_rows_w4096: no statistics requested");
  RowArgs rw;
  const int rc = fill_row_args("stft_rows_w4096", W4_N, T, sr, roll_percent, bw_p, stats_mask, stats_out, cplan_host, contrast_out, rw);
  if (rc) return rc;
  return w4096_launch("stft_rows_w4096", y, B, L, ldy, hop, center, T, window, twiddle, segtab, n_segtab, n_mels, mel_out, &rw,
                      (hipStream_t)stream);
}
