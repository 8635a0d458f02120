// The strided transform that large FFTs are composed from (four-step, on the host side), once for every in-LDS engine:
// the row kernel, the column-tiled kernel, the fused ends of their loads and stores, and the launcher behind
// syg_fft_{pow2,mixed}_strided_ex_f32.  An ENGINE is a small functor passed to the kernel by value:
//   eng(x, y, n, tw, tid, nt)   the n-point transform of x in LDS by the nt threads tid = 0 .. nt - 1 (ping-pong buffer y,
//                               twiddles tw = W_n^k); returns the buffer that holds the result, natural order
//   Engine::POW2                n is a power of two: index splits by shift and mask, float four-step twiddle
//   eng.plan(n)                 host: prepares the engine for length n; false when it cannot take n
// Pow2Fft (block_fft: fft_generic.hip) and MixedFft (block_fft_mixed and its radices: fft_mixed.hip).  The engine is the
// LAST kernel argument: an empty one then leaves every other argument where it would be without it.
#pragma once
#include "host.h"

namespace syg {
namespace {

// Fused ends (the `flags` of syg_fft_*_strided_ex_f32): a REAL input array (imaginary part 0: no packing pass),
// the analytic-signal weights of scipy.signal.hilbert applied to the loaded element (its index inside the row is its
// frequency bin: 1 at 0 and n / 2, 2 below n / 2, 0 above: no masking pass), magnitudes as the output (no |.| pass).
constexpr int SYG_FFT_REAL_IN = 1, SYG_FFT_ABS_OUT = 2, SYG_FFT_PAIR_IN = 4;
// element at position pos of the row that starts at element offset ibase.  PAIR_IN: `in` is a real array whose row (in_valid
// samples, zero beyond) is read as the complex sequence (x[2 p], x[2 p + 1]) -- the packed form of a real-input transform of
// twice the length (rfft_conv) without its packing pass; ibase is then the row's offset in FLOATS.
__device__ __forceinline__ float2 fft_load(const float2* __restrict__ in, int64_t ibase, int64_t pos, int flags, int64_t mask_n,
                                           int64_t in_valid) {
  float2 v;
  if (flags & SYG_FFT_PAIR_IN) {
    const float* r = reinterpret_cast<const float*>(in) + ibase;
    v = make_float2(2 * pos < in_valid ? r[2 * pos] : 0.f, 2 * pos + 1 < in_valid ? r[2 * pos + 1] : 0.f);
  } else if (flags & SYG_FFT_REAL_IN) {
    v = make_float2(reinterpret_cast<const float*>(in)[ibase + pos], 0.f);
  } else {
    v = in[ibase + pos];
  }
  if (mask_n > 0) {
    const float h = (pos == 0 || 2 * pos == mask_n) ? 1.f : (2 * pos < mask_n ? 2.f : 0.f);
    v.x *= h; v.y *= h;
  }
  return v;
}
__device__ __forceinline__ void fft_store(float2* __restrict__ out, int64_t idx, float2 v, int flags) {
  if (flags & SYG_FFT_ABS_OUT) reinterpret_cast<float*>(out)[idx] = sqrtf(fmaf(v.x, v.x, v.y * v.y));
  else out[idx] = v;
}

// W_bign^e, e < bign.  The float path needs e / bign exact in float: bign a power of two up to 2^24 -- the column kernel
// of the power-of-two engine only (MAY_FLOAT); every other caller takes the double path.
template <bool MAY_FLOAT>
__device__ __forceinline__ float2 four_step_twiddle(int64_t e, int64_t bign) {
  if (MAY_FLOAT && bign <= (1 << 24)) {
    float sn, cs;
    sincospif(-2.0f * ((float)e / (float)bign), &sn, &cs);
    return make_float2(cs, sn);
  }
  double sn, cs;
  sincospi(-2.0 * (double)e / (double)bign, &sn, &cs);
  return make_float2((float)cs, (float)sn);
}

// element e of transform (o, b) at in[o*in_os + b*in_bs + e*in_es]; output k of transform b times W_bign^(b k) when
// bign > 0 (the four-step twiddle), times scale; inverse via conj(FFT(conj(x)))
template <class Engine>
__global__ void fft_strided_kernel(const float2* __restrict__ in, float2* __restrict__ out, int n, int inverse,
                                   const float2* __restrict__ tw, int64_t in_os, int64_t in_bs, int64_t in_es,
                                   int64_t out_os, int64_t out_bs, int64_t out_es, int64_t bign, float scale, int flags,
                                   int64_t mask_n, int64_t in_valid, Engine eng) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float2* x = reinterpret_cast<float2*>(lds);
  float2* y = x + n;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t b = blockIdx.x, o = blockIdx.y;
  const int64_t ibase = o * in_os, irow = b * in_bs, obase = o * out_os + b * out_bs;
  for (int i = tid; i < n; i += nt) {
    float2 v = fft_load(in, ibase, irow + (int64_t)i * in_es, flags, mask_n, in_valid);
    if (inverse) v.y = -v.y;
    x[i] = v;
  }
  __syncthreads();
  float2* r = eng(x, y, n, tw, tid, nt);
  for (int k = tid; k < n; k += nt) {
    float2 v = r[k];
    if (bign > 0) {
      const int64_t e = (b * (int64_t)k) % bign;
      v = cmul(v, four_step_twiddle<false>(e, bign));
    }
    v.x *= scale; v.y *= scale;
    if (inverse) v.y = -v.y;
    fft_store(out, obase + (int64_t)k * out_es, v, flags);
  }
}

// Column-tiled form of the strided transform for the two passes of a four-step FFT.  The transforms of one pass
// are the columns of a matrix whose rows are contiguous (in_bs == 1): a workgroup takes CB adjacent columns, so
// every global access is a run of CB complex values (128 bytes at CB = 16) instead of one 8-byte element per line,
// transposes them into LDS (one column = one natural-order array, pitch n + COLS_PAD), runs the CB transforms side
// by side (256 / CB threads each; the trip counts and barriers of an engine depend on n only) and stores either
// k-fast (out_es == 1: the transposed layout pass A leaves for pass B) or column-fast (out_bs == 1: final order).
constexpr int COLS_NT = 256;
constexpr int COLS_PAD = 2;
constexpr int COLS_MAXN = 1024;

template <class Engine, bool KFAST>
__global__ __launch_bounds__(COLS_NT) void fft_cols_kernel(const float2* __restrict__ in, float2* __restrict__ out, int n,
                                                           int cb_log, int inverse,
                                                           const float2* __restrict__ tw, int64_t in_os, int64_t in_es,
                                                           int64_t out_os, int64_t out_bs, int64_t out_es, int64_t bign,
                                                           float scale, int flags, int64_t mask_n, int64_t in_valid, Engine eng) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int CB = 1 << cb_log, LP = n + COLS_PAD;
  float2* x = reinterpret_cast<float2*>(lds);
  float2* y = x + CB * LP;
  const int tid = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x << cb_log, o = blockIdx.y;
  const int64_t ibase = o * in_os, obase = o * out_os;
  const int total = n << cb_log;
  for (int idx = tid; idx < total; idx += COLS_NT) {
    const int c = idx & (CB - 1), e = idx >> cb_log;
    const int64_t pos = (int64_t)e * in_es + c0 + c;           // position inside the row (= the bin, for the analytic weights)
    float2 v = fft_load(in, ibase, pos, flags, mask_n, in_valid);
    if (inverse) v.y = -v.y;
    x[c * LP + e] = v;
  }
  __syncthreads();
  const int tpc_log = 8 - cb_log;                              // threads per column
  const int g = tid >> tpc_log, lt = tid & ((1 << tpc_log) - 1);
  const float2* r = eng(x + g * LP, y + g * LP, n, tw, lt, 1 << tpc_log) - g * LP;
  int ln = 0;
  while ((1 << ln) < n) ++ln;
  for (int idx = tid; idx < total; idx += COLS_NT) {
    int c, k;
    if (KFAST && Engine::POW2) { k = idx & (n - 1); c = idx >> ln; }
    else if (KFAST) { c = idx / n; k = idx - c * n; }
    else { c = idx & (CB - 1); k = idx >> cb_log; }
    float2 v = r[c * LP + k];
    if (bign > 0) {
      int64_t e = (c0 + c) * (int64_t)k;
      if (e >= bign) e %= bign;                                // (column * k < bign in a four-step split: never taken there)
      v = cmul(v, four_step_twiddle<Engine::POW2>(e, bign));
    }
    v.x *= scale; v.y *= scale;
    if (inverse) v.y = -v.y;
    fft_store(out, obase + (c0 + c) * out_bs + (int64_t)k * out_es, v, flags);
  }
}

// Behind both _ex entry points: the checks, the choice between column tiles and the row kernel, the launch.  `who` names
// the entry in messages, maxn is its largest n; the two rules in which the entries differ are arguments:
//   row_threads(n)      workgroup size of the row kernel
//   narrow_to_divisor   the tile also narrows (16 -> 8 -> 4 columns) until its width divides `batch`; without it the
//                       width is chosen by size alone and a batch it does not divide goes to the row kernel
template <class Engine>
int fft_strided_launch(const char* who, int maxn, int (*row_threads)(int), bool narrow_to_divisor, const float* in, float* out,
                       int64_t outer, int64_t batch, int n, int inverse, const float* twiddle, int64_t in_os, int64_t in_bs,
                       int64_t in_es, int64_t out_os, int64_t out_bs, int64_t out_es, int64_t bign, float scale, int flags,
                       int64_t mask_n, int64_t in_valid, void* stream) {
  SYG_REQUIRE(in && out && twiddle, "%s: null pointer argument", who);
  SYG_REQUIRE((Engine::POW2 ? is_pow2(n) : n >= 2) && n <= maxn, "%s: n must be %sin [2, %d] (got %d)", who,
              Engine::POW2 ? "a power of two " : "", maxn, n);
  SYG_REQUIRE(batch >= 1 && batch < (int64_t)0x7fffffff && outer >= 1 && outer <= MAX_GRID_Y, "%s: bad batch/outer", who);
  SYG_REQUIRE(in != out, "%s: in-place operation is not supported", who);
  SYG_REQUIRE(flags >= 0 && flags <= 7 && (flags & 5) != 5 && mask_n >= 0 && in_valid >= 0, "%s: bad flags / mask length", who);
  Engine eng;                                                  // (only the mixed engine refuses a length inside the range)
  SYG_REQUIRE(eng.plan(n), "%s: n = %d has a prime factor other than 2, 3, 5, 7", who, n);
  const float2* src = (const float2*)in;
  float2* dst = (float2*)out;
  const float2* tw = (const float2*)twiddle;
  if (in_bs == 1 && (out_es == 1 || out_bs == 1) && n <= COLS_MAXN && n >= 8) {
    const auto cols_lds = [n](int cb_log) { return (size_t)2 * ((size_t)(n + COLS_PAD) << cb_log) * sizeof(float2); };
    int cb_log = 4;                                            // 16 columns = 128-byte runs; at most 4096 points per tile
    while (cb_log > 2 && (((int64_t)n << cb_log) > 4096 || (narrow_to_divisor && batch % (1 << cb_log) != 0))) --cb_log;
    // two workgroups per CU hide too little: above 40 KB of LDS take 8 columns (64-byte runs) -- 758 -> 646 us for the two
    // passes of 1024 x 48000 (200 x 240), 1145 -> 760 us for 1024 x 65536 (256 x 256); 4 columns are slower again
    if (cb_log == 4 && cols_lds(4) > 40 * 1024) cb_log = 3;
    if (batch % (1 << cb_log) == 0) {                          // (n <= COLS_MAXN: 4 columns always fit the 4096 points)
      char cols[64];
      snprintf(cols, sizeof cols, "%s(cols)", who);
      const auto kernel = out_es == 1 ? fft_cols_kernel<Engine, true> : fft_cols_kernel<Engine, false>;   // k-fast store?
      const size_t lds = cols_lds(cb_log);
      if (const int rc = reserve_dynamic_lds(cols, (const void*)kernel, lds)) return rc;
      hipLaunchKernelGGL(kernel, dim3((unsigned)(batch >> cb_log), (unsigned)outer), dim3(COLS_NT), lds, (hipStream_t)stream,
                         src, dst, n, cb_log, inverse, tw, in_os, in_es, out_os, out_bs, out_es, bign, scale, flags, mask_n,
                         in_valid, eng);
      SYG_CHECK_LAUNCH(cols);
      return SYG_OK;
    }
  }
  const size_t lds = (size_t)n * 2 * sizeof(float2);
  if (const int rc = reserve_dynamic_lds(who, (const void*)fft_strided_kernel<Engine>, lds)) return rc;
  hipLaunchKernelGGL(fft_strided_kernel<Engine>, dim3((unsigned)batch, (unsigned)outer), dim3(row_threads(n)), lds,
                     (hipStream_t)stream, src, dst, n, inverse, tw, in_os, in_bs, in_es, out_os, out_bs, out_es, bign, scale,
                     flags, mask_n, in_valid, eng);
  SYG_CHECK_LAUNCH(who);
  return SYG_OK;
}

}  // namespace
}  // namespace syg
