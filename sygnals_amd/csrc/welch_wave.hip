// Welch partial periodograms for nperseg = nfft = 4096 (BASELINE config C5: one-hour streams, 50 % overlap), one
// WAVE per segment: scipy.signal.welch as called by compute_psd_welch (sygnals/core/dsp.py:495-560).
//
// The transform is wave_fft.h's 4096-point real-input power spectrum (two 1024-point wave FFTs, the radix-2 combine and
// the real-input split on mirror pairs, all in registers; lane l loads x[4 (64 a + l) .. + 3] as one 16-byte word).
// |X|^2 is accumulated per bin in registers over the segments of a wave (segment g, g + n_waves, ...); the per-wave sums
// go to the work buffer and are combined in float64, fixed order, by welch_final_kernel (fft_generic.hip).
// No workgroup barrier inside the segment loop: the waves of a workgroup only share the constant tables.
#include "wave_fft.h"

namespace syg {
namespace {

constexpr int WW = 4;                    // waves per workgroup
constexpr int NSEG = 4096;
constexpr int MBIN = 2048;               // one-sided bins 0 .. 2048

struct WelchLds {
  float2 sc[WW][wfft::SC_COMPLEX];
  float2 tw2l[wfft::TW2_COMPLEX];
  float2 tw1l[wfft::TW1_COMPLEX];
  float2 t2048[wfft::RFFT4096_TW];       // W_2048^k, W_4096^k of the lanes' bins (wfft::init_rfft4096_tables)
  float2 t4096[wfft::RFFT4096_TW];
  float win[NSEG];
};

template <int DETREND>
__global__ __launch_bounds__(WW * 64) void welch_wave_kernel(const float* __restrict__ x, int64_t ldx, int step,
                                                             int64_t nseg, const float* __restrict__ win,
                                                             const float2* __restrict__ tw4096, int nblk,
                                                             float* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) WelchLds L;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  wfft::Lane lc;
  wfft::init_lane(lc, lane);
  wfft::init_tables(L.tw2l, L.tw1l, tw4096, 4096, tid, WW * 64);
  for (int i = tid; i < NSEG; i += WW * 64) L.win[i] = win[i];
  wfft::init_rfft4096_tables(L.t2048, L.t4096, tw4096, tid, WW * 64);
  __syncthreads();

  const int64_t b = blockIdx.y;
  const float* xr = x + b * ldx;
  const int g = blockIdx.x * WW + w;                    // this wave's slot among the nblk partial sums of the stream
  float acc[34];                                        // 4 |X|^2 summed over the segments, by slot of wfft::rfft4096_pow
#pragma unroll
  for (int i = 0; i < 34; ++i) acc[i] = 0.f;

  for (int64_t sg = g; sg < nseg; sg += nblk) {
    const float4* sp = reinterpret_cast<const float4*>(xr + sg * (int64_t)step);
    float4 raw[16];
#pragma unroll
    for (int a = 0; a < 16; ++a) raw[a] = sp[64 * a + lane];
    // detrend 1: subtract the mean; 2: subtract the least-squares line, written around the segment centre so that
    // slope and mean decouple (scipy.signal.detrend type='linear'): x - mean - slope (i - (n - 1) / 2)
    float mean = 0.f, slope = 0.f;
    constexpr float JC = 0.5f * (float)(NSEG - 1);
    if (DETREND) {
      float s = 0.f, sj = 0.f;
#pragma unroll
      for (int a = 0; a < 16; ++a) {
        s += (raw[a].x + raw[a].y) + (raw[a].z + raw[a].w);
        if (DETREND == 2) {
          const float i0 = (float)(4 * (64 * a + lane)) - JC;
          sj += (i0 * raw[a].x + (i0 + 1.f) * raw[a].y) + ((i0 + 2.f) * raw[a].z + (i0 + 3.f) * raw[a].w);
        }
      }
      mean = wave_sum(s) * (1.f / (float)NSEG);
      if (DETREND == 2) {
        const double nn = (double)NSEG;
        slope = (float)((double)wave_sum(sj) / (nn * (nn * nn - 1.0) / 12.0));
      }
    }
    float2 ve[16], vo[16];
    {
      const float4* w4 = reinterpret_cast<const float4*>(L.win);
#pragma unroll
      for (int a = 0; a < 16; ++a) {
        const float4 ww = w4[64 * a + lane];
        float4 r = raw[a];
        if (DETREND == 1) { r.x -= mean; r.y -= mean; r.z -= mean; r.w -= mean; }
        if (DETREND == 2) {
          const float i0 = (float)(4 * (64 * a + lane)) - JC;
          r.x -= mean + slope * i0; r.y -= mean + slope * (i0 + 1.f);
          r.z -= mean + slope * (i0 + 2.f); r.w -= mean + slope * (i0 + 3.f);
        }
        ve[a] = make_float2(r.x * ww.x, r.y * ww.y);
        vo[a] = make_float2(r.z * ww.z, r.w * ww.w);
      }
    }
    float2 ek[2][4], em[2][4], ok[2][4], om[2][4], e512, o512;
    wfft::cfft1024(ve, lc, L.sc[w], L.tw1l, L.tw2l, lane, ek, em, e512);
    wfft::cfft1024(vo, lc, L.sc[w], L.tw1l, L.tw2l, lane, ok, om, o512);
    // (the factor 1/4 is applied once, by the combine kernel)
    wfft::rfft4096_pow(ek, em, e512, ok, om, o512, L.t2048, L.t4096, lane, [&](int slot, int, float p) { acc[slot] += p; });
  }
  float* po = partial + ((int64_t)b * nblk + g) * (int64_t)(MBIN + 1);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int q = 4 * j + d;
      const int k = wfft::bin_of(lane, j, d);
      po[k] = acc[4 * q + 0];
      po[MBIN - k] = acc[4 * q + 1];
      po[1024 - k] = acc[4 * q + 2];
      if (k != 0) po[1024 + k] = acc[4 * q + 3];      // (k = 0: bin 1024 once)
    }
  if (lane == 0) { po[512] = acc[32]; po[1536] = acc[33]; }
}

}  // namespace

// Partial sums of nblk waves per stream into work [B, nblk, 2049]; the values carry a factor 4 (see wfft::split_pow).
// Preconditions (checked by the caller): nperseg = nfft = 4096, 16-byte aligned segments, nblk % 4 == 0, nblk <= nseg
// rounded up to a multiple of 4 (idle waves write zeros).
int welch_wave_launch(const float* x, int64_t B, int64_t ldx, int step, int64_t nseg, const float* window,
                      const float* twiddle, int detrend, int nblk, float* work, hipStream_t st) {
  const dim3 grid((unsigned)(nblk / WW), (unsigned)B), block(WW * 64);
  if (detrend == 0)
    hipLaunchKernelGGL(welch_wave_kernel<0>, grid, block, 0, st, x, ldx, step, nseg, window, (const float2*)twiddle, nblk, work);
  else if (detrend == 1)
    hipLaunchKernelGGL(welch_wave_kernel<1>, grid, block, 0, st, x, ldx, step, nseg, window, (const float2*)twiddle, nblk, work);
  else
    hipLaunchKernelGGL(welch_wave_kernel<2>, grid, block, 0, st, x, ldx, step, nseg, window, (const float2*)twiddle, nblk, work);
  SYG_CHECK_LAUNCH("welch_wave");
  return SYG_OK;
}

}  // namespace syg
