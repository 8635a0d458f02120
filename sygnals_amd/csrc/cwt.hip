// Continuous wavelet transform as a bank of S FIR filters over one shared input (the float64 restatement that is the
// contract lives in tests/cwt_ref.py; the plan comes from sygnals_amd/_cwt.py):
//     W[b, s, t] = sum_{j < taps_s} h_s[j] x~[b, t + shift_s - j],      t = c stride,  c < n_out = ceil(L / stride),
// x~ = x inside [0, L) and 0 outside.  h_s = -sqrt(s) d(k_s) is the differenced, integrated, reversed wavelet of scale s:
// pywt.cwt's diff(convolve(x, k_s)) with the cancellation of the diff done in float64 on the host, so the device runs a
// plain FIR bank.  shift_s = floor(d_s) + 1 is the crop of pywt.cwt in this index form.  A complex wavelet has a re and
// an im plane of taps and two sums.
//
// Direct kernel (syg_cwt_f32), for the short filters.  The grid is (column tiles, scale groups, clips).  A block takes
// CW_TILE consecutive output columns of one clip and a group of up to CW_SPG entries of `meta`; it stages the input span
// of the group's widest reach once in LDS, zeros outside the row, and reuses it for every scale of the group.  At
// stride 1 (cw_scale_vec) a lane owns four consecutive outputs and the block stages the scale's taps as well: a step
// of four taps is one 16-byte read of x and one 16-byte broadcast read of taps for sixteen fmas.  At another stride
// (cw_scale) lane e owns the outputs e + k CW_THREADS, k < CW_PER, and the wave-uniform tap comes from global memory.
// Every output is one chain of fmaf with j ascending in both: no atomics, the same bits on every call, for every batch
// size and for every stride (a strided call computes only the columns it keeps, by the same chain).  A block whose span
// does not fit the staged words (a long filter forced here, or a large stride) reads x from global memory instead: same
// arithmetic, same order.
//
// Spectral path, for the long filters: the transforms are the strided FFT's (sygnals_amd/ops.py runs them); this file
// adds its two ends.  syg_cwt_spectrum_c64 forms Z[b, r, :] = X[b, :] H[r, :] for every filter row in one launch (X is
// read once for all rows).  After the inverse transform, syg_cwt_crop_f32 reads row r at m = shift + c stride and writes
// the requested form.  A filter row of a real wavelet carries two scales, h_a + i h_b: x is real, so the real part of
// the inverse is scale a and the imaginary part scale b.
//
// Output forms (both paths): 0 coef (float32; re, im interleaved for a complex wavelet), 1 magnitude |W|, 2 power |W|^2.
#include "host.h"

namespace syg {
namespace {

constexpr int CW_TILE = 1024;                          // output columns per tile
constexpr int CW_THREADS = 256;
constexpr int CW_PER = CW_TILE / CW_THREADS;           // outputs a lane owns
constexpr int CW_SPG = 8;                              // entries of meta a block serves from one staged span
constexpr int CW_SPAN_MAX = 16384;                     // input samples a block stages at most (64 KiB)
constexpr int CW_TAPS_LDS_MAX = 2 * (8192 + 8);        // words of staged taps at most (64 KiB: both planes of 8192 taps)
constexpr int CW_DIRECT_TAPS_MAX = 1024;               // the rule: filters up to this many taps run direct
enum { CW_OUT_COEF = 0, CW_OUT_MAG, CW_OUT_POWER, CW_OUT_COUNT };

struct CwArgs {
  const float* x; int64_t L, ldx;
  const float* tab; const int32_t* meta; int S, S_out;
  int64_t stride, n_out; float* y; int output, xs_words, hs_words;
};

template <bool CPLX>
__device__ __forceinline__ void cw_store(float* __restrict__ y, int64_t at, float re, float im, int output) {
  if (output == CW_OUT_COEF) {
    if (CPLX) reinterpret_cast<float2*>(y)[at] = make_float2(re, im);
    else y[at] = re;
  } else if (output == CW_OUT_MAG) {
    y[at] = CPLX ? sqrtf(fmaf(re, re, im * im)) : fabsf(re);
  } else {
    y[at] = CPLX ? fmaf(re, re, im * im) : re * re;
  }
}

// one entry of meta over the block's tile.  STAGE: x comes from the staged span xs (local index), else from the row
// through the zero rule (ts0: the time of local index 0)
template <bool CPLX, bool STAGE>
__device__ __forceinline__ void cw_scale(const CwArgs& A, const float* xs, const float* __restrict__ xr, int64_t ts0, int base,
                                         const float* __restrict__ hr, int taps, float* __restrict__ yrow, int64_t c0, int cnt) {
  const int tid = threadIdx.x;
  const float* __restrict__ hi = hr + taps;            // the im plane
  int64_t at[CW_PER];                                  // local index of tap 0's sample
  bool ok[CW_PER];
#pragma unroll
  for (int k = 0; k < CW_PER; ++k) {
    const int o = tid + k * CW_THREADS;
    ok[k] = o < cnt;
    at[k] = (int64_t)(ok[k] ? o : 0) * A.stride + base;   // an output past the end repeats the first and is not stored
  }
  float re[CW_PER], im[CW_PER];
#pragma unroll
  for (int k = 0; k < CW_PER; ++k) re[k] = im[k] = 0.f;
  auto tap = [&](int j) {
    const float hr_j = hr[j], hi_j = CPLX ? hi[j] : 0.f;
#pragma unroll
    for (int k = 0; k < CW_PER; ++k) {
      float v;
      if (STAGE) {
        v = xs[(int)at[k] - j];
      } else {
        const int64_t t = ts0 + at[k] - j;
        v = (t >= 0 && t < A.L) ? xr[t] : 0.f;
      }
      re[k] = fmaf(hr_j, v, re[k]);
      if (CPLX) im[k] = fmaf(hi_j, v, im[k]);
    }
  };
  int j = 0;
  for (; j + 4 <= taps; j += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) tap(j + u);
  }
  for (; j < taps; ++j) tap(j);
#pragma unroll
  for (int k = 0; k < CW_PER; ++k)
    if (ok[k]) cw_store<CPLX>(yrow, c0 + tid + k * CW_THREADS, re[k], im[k], A.output);
}

// The staged form at stride 1.  Lane e owns the FOUR CONSECUTIVE outputs 4 e ... 4 e + 3 and walks the taps four at a
// time: the sixteen products of a step read the seven samples x[a - 3 ... a + 3], a = base + 4 e - 4 q, which are two
// aligned 16-byte words of the span, and the upper one is the lower one of the step before.  So a step costs a lane one
// 16-byte read of x and one 16-byte broadcast read of the taps (hs, staged by the block) for sixteen fmas (thirty-two
// for a complex wavelet, with a second tap read).  To make `a` a multiple of four the filter is shifted by delta < 4
// zero taps in front (and padded with zeros to a multiple of four behind): a zero tap adds 0 to a chain, so every output
// is still the chain of fmaf with j ascending that cw_scale runs.  xs4 is the span from four words before local index 0.
template <bool CPLX>
__device__ __forceinline__ void cw_scale_vec(const CwArgs& A, const float4* xs4, float* hs, int base, const float* __restrict__ hr,
                                             int taps, float* __restrict__ yrow, int64_t c0, int cnt) {
  const int tid = threadIdx.x;
  const int delta = (4 - (base & 3)) & 3;
  const int t4 = (taps + delta + 3) & ~3;              // taps of the shifted, padded filter
  float* hsi = hs + t4;                                // the im plane
  __syncthreads();                                     // the scale before has read its taps
  for (int j = tid; j < t4; j += CW_THREADS) {
    const int src = j - delta;
    const bool in = src >= 0 && src < taps;
    hs[j] = in ? hr[src] : 0.f;
    if (CPLX) hsi[j] = in ? hr[taps + src] : 0.f;
  }
  __syncthreads();
  if (4 * tid >= cnt) return;                          // (no barrier below)
  const float4* h4 = reinterpret_cast<const float4*>(hs);
  const float4* g4 = reinterpret_cast<const float4*>(hsi);
  int w = (base + delta) / 4 + tid + 1;                // word of x[a ... a + 3] in xs4 (one word of front pad)
  float re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
  float4 hi = xs4[w];
  for (int q = 0; q < t4 / 4; ++q, --w) {
    const float4 lo = xs4[w - 1];
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};      // x[a - 4 ... a + 3]
    const float4 hq = h4[q];
    const float hr4[4] = {hq.x, hq.y, hq.z, hq.w};
    float hi4[4] = {0.f, 0.f, 0.f, 0.f};
    if (CPLX) { const float4 gq = g4[q]; hi4[0] = gq.x; hi4[1] = gq.y; hi4[2] = gq.z; hi4[3] = gq.w; }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        re[k] = fmaf(hr4[u], v[4 + k - u], re[k]);
        if (CPLX) im[k] = fmaf(hi4[u], v[4 + k - u], im[k]);
      }
    }
    hi = lo;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (4 * tid + k < cnt) cw_store<CPLX>(yrow, c0 + 4 * tid + k, re[k], im[k], A.output);
}

template <bool CPLX>
__global__ __launch_bounds__(CW_THREADS) void cwt_direct_kernel(CwArgs A) {
  extern __shared__ __align__(16) float cw_smem[];
  float* xs = cw_smem + 4;                             // [xs_words]: four words of pad in front of local index 0 ...
  float* hs = cw_smem + A.xs_words;                    // [hs_words]: the taps of the scale at hand (the stride-1 form)
  const int tid = threadIdx.x;
  const int s0 = blockIdx.y * CW_SPG, s1 = min(A.S, s0 + CW_SPG);
  const int64_t b = blockIdx.z;
  const float* __restrict__ xr = A.x + b * A.ldx;
  const int64_t c0 = (int64_t)blockIdx.x * CW_TILE;
  const int cnt = (int)(A.n_out - c0 < CW_TILE ? A.n_out - c0 : CW_TILE);
  // the group's reach: local index 0 is the earliest sample any of its filters reads for the tile's first column
  int lo_rel = 0x7fffffff, hi_rel = -0x7fffffff;
  for (int s = s0; s < s1; ++s) {
    const int taps = A.meta[4 * s + 1], shift = A.meta[4 * s + 2];
    lo_rel = min(lo_rel, shift - (taps - 1));
    hi_rel = max(hi_rel, shift);
  }
  const int64_t ts0 = c0 * A.stride + lo_rel;
  const int64_t span = (int64_t)(cnt - 1) * A.stride + (int64_t)(hi_rel - lo_rel) + 1;
  const bool stage = span + 12 <= (int64_t)A.xs_words; // block-uniform (... and eight behind the span: cw_scale_vec)
  if (stage) {
    for (int i = tid - 4; i < (int)span + 8; i += CW_THREADS) {
      const int64_t t = ts0 + i;
      xs[i] = (t >= 0 && t < A.L) ? xr[t] : 0.f;
    }
  }
  __syncthreads();
  for (int s = s0; s < s1; ++s) {
    const int taps = A.meta[4 * s + 1], shift = A.meta[4 * s + 2], oi = A.meta[4 * s + 3];
    if (taps < 1 || oi < 0 || oi >= A.S_out) continue; // (a table the plan did not make: nothing is read or written)
    const float* __restrict__ hr = A.tab + A.meta[4 * s];
    float* __restrict__ yrow = A.y + (b * A.S_out + oi) * A.n_out * (CPLX && A.output == CW_OUT_COEF ? 2 : 1);
    // (block-uniform: the barriers inside cw_scale_vec are reached by every thread)
    if (stage && A.stride == 1 && (CPLX ? 2 : 1) * (taps + 6) <= A.hs_words)
      cw_scale_vec<CPLX>(A, reinterpret_cast<const float4*>(cw_smem), hs, shift - lo_rel, hr, taps, yrow, c0, cnt);
    else if (stage) cw_scale<CPLX, true>(A, xs, xr, ts0, shift - lo_rel, hr, taps, yrow, c0, cnt);
    else cw_scale<CPLX, false>(A, xs, xr, ts0, shift - lo_rel, hr, taps, yrow, c0, cnt);
  }
}

// Z[b, r, m] = X[b, m] H[r, m]: a thread takes one bin of one clip through every filter row
__global__ __launch_bounds__(256) void cwt_spectrum_kernel(const float2* __restrict__ X, const float2* __restrict__ H, int64_t R,
                                                           int64_t M, float2* __restrict__ Z) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (m >= M) return;
  const float2 x = X[b * M + m];
  for (int64_t r = 0; r < R; ++r) Z[(b * R + r) * M + m] = cmul(x, H[r * M + m]);
}

struct CropArgs {
  const float2* Z; int64_t R, M; const int32_t* rmeta; int cplx, output;
  int64_t stride, n_out; int S_out; float* y;
};

__global__ __launch_bounds__(256) void cwt_crop_kernel(CropArgs A) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, b = blockIdx.z;
  if (c >= A.n_out) return;
  const float2* __restrict__ z = A.Z + (b * A.R + r) * A.M;
  const int32_t* q = A.rmeta + 4 * r;
  auto at = [&](int shift) {
    const int64_t m = (int64_t)shift + c * A.stride;
    return (m >= 0 && m < A.M) ? z[m] : make_float2(0.f, 0.f);
  };
  if (A.cplx) {
    const int oi = q[1];
    if (oi < 0 || oi >= A.S_out) return;
    const float2 v = at(q[0]);
    cw_store<true>(A.y + (b * A.S_out + oi) * A.n_out * (A.output == CW_OUT_COEF ? 2 : 1), c, v.x, v.y, A.output);
  } else {
    const int oa = q[1], ob = q[3];
    if (oa >= 0 && oa < A.S_out) cw_store<false>(A.y + (b * A.S_out + oa) * A.n_out, c, at(q[0]).x, 0.f, A.output);
    if (ob >= 0 && ob < A.S_out) cw_store<false>(A.y + (b * A.S_out + ob) * A.n_out, c, at(q[2]).y, 0.f, A.output);
  }
}

int cw_check_out(const char* who, int64_t B, int64_t L, int64_t S_out, int cplx, int output, int64_t stride, int64_t n_out) {
  SYG_REQUIRE(B >= 1 && B <= MAX_GRID_Y && L >= 1 && L < ((int64_t)1 << 40), "%s: bad B / L (B in [1, 65535], L in [1, 2^40))", who);
  SYG_REQUIRE(S_out >= 1 && S_out <= MAX_GRID_Y, "%s: bad S (the scales of y, in [1, 65535])", who);
  SYG_REQUIRE(cplx == 0 || cplx == 1, "%s: cplx must be 0 (real wavelet) or 1 (re and im planes)", who);
  SYG_REQUIRE(output >= 0 && output < CW_OUT_COUNT, "%s: unknown output code %d (0 coef, 1 magnitude, 2 power)", who, output);
  SYG_REQUIRE(stride >= 1 && stride < ((int64_t)1 << 40), "%s: stride must be at least 1", who);
  SYG_REQUIRE(n_out == ceil_div(L, stride), "%s: n_out=%lld is not ceil(L / stride) = %lld", who, (long long)n_out,
              (long long)ceil_div(L, stride));
  return SYG_OK;
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int syg_cwt_tile(void) { return CW_TILE; }
extern "C" int syg_cwt_direct_taps_max(void) { return CW_DIRECT_TAPS_MAX; }
extern "C" int syg_cwt_scales_per_group(void) { return CW_SPG; }
extern "C" int syg_cwt_span_max(void) { return CW_SPAN_MAX; }
extern "C" int syg_cwt_taps_lds_max(void) { return CW_TAPS_LDS_MAX; }

extern "C" int64_t syg_cwt_work_bytes(int64_t B, int64_t R, int64_t M) {
  if (B < 1 || R < 1 || M < 2 || B > MAX_GRID_Y || R > MAX_GRID_Y || M > ((int64_t)1 << 27)) {
    set_error("cwt_work_bytes: bad B / R / M (B, R in [1, 65535], M in [2, 2^27])");
    return -1;
  }
  // the padded real rows and their transform, then the products, the inverse's result and the four-step temporary
  return 4 * B * M + 8 * B * M + 3 * 8 * B * R * M;
}

extern "C" int syg_cwt_f32(const float* x, int64_t B, int64_t L, int64_t ldx, const float* table, const int32_t* meta, int64_t S,
                           int64_t S_out, int cplx, int64_t reach, int output, int64_t stride, int64_t n_out, float* y, void* stream) {
  SYG_REQUIRE(x && table && meta && y, "cwt: null pointer argument (x / table / meta / y)");
  if (const int rc = cw_check_out("cwt", B, L, S_out, cplx, output, stride, n_out)) return rc;
  SYG_REQUIRE(S >= 1 && S <= S_out, "cwt: bad S (the entries of meta, in [1, the scales of y])");
  SYG_REQUIRE(ldx >= L, "cwt: ldx=%lld is less than L=%lld", (long long)ldx, (long long)L);
  SYG_REQUIRE(reach >= 1 && reach < ((int64_t)1 << 31), "cwt: reach must be in [1, 2^31)");
  const int64_t gx = ceil_div(n_out, CW_TILE);
  SYG_REQUIRE(gx < 0x7fffffff, "cwt: too many tiles");
  // the words a full tile of the widest group stages; a block whose span is longer reads global memory
  // (twelve words of pad around the span, rounded to 16 bytes: the stride-1 form reads it in 16-byte words)
  const int64_t want = ((int64_t)(CW_TILE - 1) * stride + reach + 12 + 3) & ~(int64_t)3;
  const int xs_words = (int)(want < CW_SPAN_MAX + 12 ? want : CW_SPAN_MAX + 12);
  // the stride-1 form stages one filter at a time, shifted and padded (at most taps + 6 words a plane); a filter is at
  // most `reach` taps long.  Filters too long for the words left to them run the scalar form.
  const int64_t hs_want = stride == 1 ? (cplx ? 2 : 1) * ((reach + 6 + 3) & ~(int64_t)3) : 0;
  const int hs_words = (int)(hs_want < CW_TAPS_LDS_MAX ? hs_want : CW_TAPS_LDS_MAX);
  CwArgs A{x, L, ldx, table, meta, (int)S, (int)S_out, stride, n_out, y, output, xs_words, hs_words};
  const size_t lds = sizeof(float) * ((size_t)xs_words + (size_t)hs_words);
  void (*k)(CwArgs) = cplx ? cwt_direct_kernel<true> : cwt_direct_kernel<false>;
  if (const int rc = reserve_dynamic_lds("cwt", (const void*)k, lds)) return rc;
  const dim3 grid((unsigned)gx, (unsigned)ceil_div(S, CW_SPG), (unsigned)B);
  hipLaunchKernelGGL(k, grid, dim3(CW_THREADS), lds, (hipStream_t)stream, A);
  SYG_CHECK_LAUNCH("cwt");
  return SYG_OK;
}

extern "C" int syg_cwt_spectrum_c64(const float* X, const float* H, int64_t B, int64_t R, int64_t M, float* Z, void* stream) {
  SYG_REQUIRE(X && H && Z, "cwt_spectrum: null pointer argument (X / H / Z)");
  SYG_REQUIRE(B >= 1 && B <= MAX_GRID_Y && R >= 1 && R <= MAX_GRID_Y && M >= 2 && M <= ((int64_t)1 << 27),
              "cwt_spectrum: bad B / R / M (B, R in [1, 65535], M in [2, 2^27])");
  SYG_REQUIRE(Z != X && Z != H, "cwt_spectrum: in-place operation is not supported");
  hipLaunchKernelGGL(cwt_spectrum_kernel, dim3((unsigned)ceil_div(M, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                     (const float2*)X, (const float2*)H, R, M, (float2*)Z);
  SYG_CHECK_LAUNCH("cwt_spectrum");
  return SYG_OK;
}

extern "C" int syg_cwt_crop_f32(const float* Z, int64_t B, int64_t R, int64_t M, const int32_t* rmeta, int64_t L, int64_t S_out,
                                int cplx, int output, int64_t stride, int64_t n_out, float* y, void* stream) {
  SYG_REQUIRE(Z && rmeta && y, "cwt_crop: null pointer argument (Z / rmeta / y)");
  if (const int rc = cw_check_out("cwt_crop", B, L, S_out, cplx, output, stride, n_out)) return rc;
  SYG_REQUIRE(R >= 1 && R <= S_out && M >= L && M <= ((int64_t)1 << 27), "cwt_crop: bad R / M (R in [1, S], M in [L, 2^27])");
  const int64_t gx = ceil_div(n_out, 256);
  SYG_REQUIRE(gx < 0x7fffffff, "cwt_crop: too many tiles");
  CropArgs A{(const float2*)Z, R, M, rmeta, cplx, output, stride, n_out, (int)S_out, y};
  hipLaunchKernelGGL(cwt_crop_kernel, dim3((unsigned)gx, (unsigned)R, (unsigned)B), dim3(256), 0, (hipStream_t)stream, A);
  SYG_CHECK_LAUNCH("cwt_crop");
  return SYG_OK;
}
