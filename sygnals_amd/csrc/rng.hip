// Device noise generation: raw Philox words, standard normals (rng_dev.h has the generator and the stream layout), and
// the three pointwise steps of power-law ("coloured") noise around the strided FFT entries:
//     noise[r] = irfft(rfft(w_r) g, M)[:L],   g[k] = k^(-alpha / 2)   (Timmer & Koenig 1995)
// g is real and symmetric, so two rows share one complex transform as w_a + i w_b: rng_normal_kernel writes the pair
// interleaved, power_gain_kernel applies g[min(k, M - k)] to the spectrum, unpack_pairs_kernel takes the real and the
// imaginary part of the inverse transform apart.  Rows are paired by ABSOLUTE index (r with r ^ 1): a row's bits never
// depend on the batch it came in.  No atomics anywhere.  The fused white-noise mix is in effects.hip, beside add_noise.
#include "host.h"
#include "rng_dev.h"

namespace syg {
namespace {

constexpr int RNG_THREADS = 256;
constexpr int64_t RNG_COLORED_MAX = (int64_t)1 << 26;     // longest transform of the strided FFT

__global__ __launch_bounds__(RNG_THREADS) void philox_words_kernel(const uint4* __restrict__ ctr, const uint2* __restrict__ key,
                                                                   int64_t n, uint4* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * RNG_THREADS + threadIdx.x;
  if (i < n) out[i] = philox4x32(ctr[i], key[i]);
}

// rows: out + b ld, unit stride; pair rows: row b is component b & 1 of the complex row b >> 1 (ld floats each)
struct NormalArgs {
  float* out; int64_t B, L, ld, offset; uint2 key; uint32_t first_row; int pair, vec;
};

// grid (blocks of RNG_THREADS calls, rows): a thread owns call q of every row its workgroup serves
__global__ __launch_bounds__(RNG_THREADS) void rng_normal_kernel(NormalArgs A) {
  const int64_t q0 = A.offset >> 2, q1 = (A.offset + A.L - 1) >> 2;
  const int64_t q = q0 + (int64_t)blockIdx.x * RNG_THREADS + threadIdx.x;
  if (q > q1) return;
  const int64_t i0 = 4 * q - A.offset;                    // index in the row of the call's first sample: -3 .. L - 1
  const bool whole = i0 >= 0 && i0 + 3 < A.L;
  for (int64_t b = blockIdx.y; b < A.B; b += gridDim.y) {
    const float4 z = rng_normal4(A.key, (uint64_t)q, A.first_row + (uint32_t)b);
    if (A.pair) {
      float2* o = (float2*)(A.out + (b >> 1) * A.ld);
      const int c = (int)(b & 1);
      const float v[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + j >= 0 && i0 + j < A.L) ((float*)(o + i0 + j))[c] = v[j];
    } else {
      float* o = A.out + b * A.ld;
      if (A.vec && whole) {
        *(float4*)(o + i0) = z;
      } else {
        const float v[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (i0 + j >= 0 && i0 + j < A.L) o[i0 + j] = v[j];
      }
    }
  }
}

// X [rows, M][2] *= g[min(k, M - k)], g[k] = k^(-alpha / 2); g[0] = 0 removes the mean (at alpha = 0 nothing diverges
// and g = 1 everywhere: 0^0 = 1, the white row passes unchanged)
__global__ __launch_bounds__(RNG_THREADS) void power_gain_kernel(float2* __restrict__ X, int64_t total, int64_t M, float half_alpha,
                                                                 int keep_dc) {
  const int64_t i = (int64_t)blockIdx.x * RNG_THREADS + threadIdx.x;
  if (i >= total) return;
  const int64_t k = i & (M - 1);
  const int64_t kk = k < M - k ? k : M - k;
  const float g = (kk == 0) ? (keep_dc ? 1.f : 0.f) : powf((float)kk, -half_alpha);
  float2 v = X[i];
  v.x *= g;
  v.y *= g;
  X[i] = v;
}

// out[b, n] = component (R & 1) of Z[(R >> 1) - (R0 >> 1)][n], R = R0 + b the absolute row; n < L
__global__ __launch_bounds__(RNG_THREADS) void unpack_pairs_kernel(const float* __restrict__ Z, int64_t M, int64_t first_row,
                                                                   float* __restrict__ out, int64_t B, int64_t L, int64_t ldo) {
  const int64_t n = (int64_t)blockIdx.x * RNG_THREADS + threadIdx.x;
  if (n >= L) return;
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    const int64_t R = first_row + b;
    out[b * ldo + n] = Z[(((R >> 1) - (first_row >> 1)) * M + n) * 2 + (R & 1)];
  }
}

int check_rows_rng(const char* who, const void* out, int64_t B, int64_t L, int64_t ld, int64_t first_row) {
  SYG_REQUIRE(out, "%s: null pointer argument (out)", who);
  SYG_REQUIRE(B >= 1 && L >= 1 && L < ((int64_t)1 << 39), "%s: bad B / L", who);
  SYG_REQUIRE(ld >= L, "%s: bad row stride (%lld < L = %lld)", who, (long long)ld, (long long)L);
  SYG_REQUIRE(first_row >= 0 && B <= RNG_ROW_LIMIT && first_row <= RNG_ROW_LIMIT - B,
              "%s: rows first_row .. first_row + B - 1 must lie in [0, 2^31) (got first_row = %lld, B = %lld)", who,
              (long long)first_row, (long long)B);
  return SYG_OK;
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_rng_constants(int key) {
  switch (key) {
    case SYG_RNG_ROUNDS: return PHILOX_ROUNDS;
    case SYG_RNG_STREAM_NOISE: return RNG_STREAM_NOISE;
    case SYG_RNG_STREAM_ROW: return RNG_STREAM_ROW;
    case SYG_RNG_ROW_LIMIT: return RNG_ROW_LIMIT;
    case SYG_RNG_COLORED_MAX: return RNG_COLORED_MAX;
    default: return -1;
  }
}

extern "C" int syg_rng_philox_u32(const uint32_t* counter, const uint32_t* key, int64_t n, uint32_t* out, void* stream) {
  SYG_REQUIRE(counter && key && out, "rng_philox: null pointer argument (counter / key / out)");
  SYG_REQUIRE(n >= 1 && n < ((int64_t)1 << 38), "rng_philox: bad n");
  SYG_REQUIRE((((uintptr_t)counter | (uintptr_t)out) & 15) == 0 && ((uintptr_t)key & 7) == 0,
              "rng_philox: counter / out must be 16-byte aligned, key 8-byte aligned");
  hipLaunchKernelGGL(philox_words_kernel, dim3((unsigned)ceil_div(n, RNG_THREADS)), dim3(RNG_THREADS), 0, (hipStream_t)stream,
                     (const uint4*)counter, (const uint2*)key, n, (uint4*)out);
  SYG_CHECK_LAUNCH("rng_philox");
  return SYG_OK;
}

extern "C" int syg_rng_normal_f32(float* out, int64_t B, int64_t L, int64_t ldo, uint64_t seed, int64_t first_row, int64_t offset,
                                  void* stream) {
  if (const int rc = check_rows_rng("rng_normal", out, B, L, ldo, first_row)) return rc;
  SYG_REQUIRE(offset >= 0 && offset < ((int64_t)1 << 62), "rng_normal: offset must be in [0, 2^62) (got %lld)", (long long)offset);
  const int vec = (offset & 3) == 0 && (ldo & 3) == 0 && ((uintptr_t)out & 15) == 0;
  NormalArgs A{out, B, L, ldo, offset, rng_key(seed), (uint32_t)first_row, 0, vec};
  const int64_t calls = ((offset + L - 1) >> 2) - (offset >> 2) + 1;
  hipLaunchKernelGGL(rng_normal_kernel, dim3((unsigned)ceil_div(calls, RNG_THREADS), grid_rows(B)), dim3(RNG_THREADS), 0,
                     (hipStream_t)stream, A);
  SYG_CHECK_LAUNCH("rng_normal");
  return SYG_OK;
}

extern "C" int syg_rng_normal_pairs_c64(float* Z, int64_t P, int64_t M, uint64_t seed, int64_t first_row, void* stream) {
  SYG_REQUIRE(Z, "rng_normal_pairs: null pointer argument (Z)");
  SYG_REQUIRE(P >= 1 && M >= 1 && M <= RNG_COLORED_MAX && P <= RNG_ROW_LIMIT / 2, "rng_normal_pairs: bad P / M");
  SYG_REQUIRE(first_row >= 0 && (first_row & 1) == 0 && first_row <= RNG_ROW_LIMIT - 2 * P,
              "rng_normal_pairs: first_row must be even with rows first_row .. first_row + 2 P - 1 in [0, 2^31) (got %lld, P = %lld)",
              (long long)first_row, (long long)P);
  NormalArgs A{Z, 2 * P, M, 2 * M, 0, rng_key(seed), (uint32_t)first_row, 1, 0};
  hipLaunchKernelGGL(rng_normal_kernel, dim3((unsigned)ceil_div(ceil_div(M, 4), RNG_THREADS), grid_rows(2 * P)), dim3(RNG_THREADS), 0,
                     (hipStream_t)stream, A);
  SYG_CHECK_LAUNCH("rng_normal_pairs");
  return SYG_OK;
}

extern "C" int syg_rng_power_gain_c64(float* X, int64_t rows, int64_t M, double alpha, void* stream) {
  SYG_REQUIRE(X, "rng_power_gain: null pointer argument (X)");
  SYG_REQUIRE(rows >= 1 && M >= 2 && M <= RNG_COLORED_MAX && (M & (M - 1)) == 0 && rows <= ((int64_t)1 << 38) / M,
              "rng_power_gain: bad rows / M (M a power of two in [2, 2^26])");
  SYG_REQUIRE(alpha >= 0.0 && alpha <= 2.0, "rng_power_gain: exponent must be in [0, 2] (got %g)", alpha);
  const int64_t total = rows * M;
  hipLaunchKernelGGL(power_gain_kernel, dim3((unsigned)ceil_div(total, RNG_THREADS)), dim3(RNG_THREADS), 0, (hipStream_t)stream,
                     (float2*)X, total, M, (float)(0.5 * alpha), alpha == 0.0 ? 1 : 0);
  SYG_CHECK_LAUNCH("rng_power_gain");
  return SYG_OK;
}

extern "C" int syg_rng_unpack_pairs_f32(const float* Z, int64_t M, int64_t first_row, float* out, int64_t B, int64_t L, int64_t ldo,
                                        void* stream) {
  SYG_REQUIRE(Z, "rng_unpack_pairs: null pointer argument (Z)");
  if (const int rc = check_rows_rng("rng_unpack_pairs", out, B, L, ldo, first_row)) return rc;
  SYG_REQUIRE(M >= L && M <= RNG_COLORED_MAX, "rng_unpack_pairs: bad M (L <= M <= 2^26)");
  hipLaunchKernelGGL(unpack_pairs_kernel, dim3((unsigned)ceil_div(L, RNG_THREADS), grid_rows(B)), dim3(RNG_THREADS), 0,
                     (hipStream_t)stream, Z, M, first_row, out, B, L, ldo);
  SYG_CHECK_LAUNCH("rng_unpack_pairs");
  return SYG_OK;
}
