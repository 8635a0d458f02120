// What the chunked SOS filters share (sosfilt.hip: zero-phase; sosfilt_causal.hip: causal with state in and out):
// the chunk / tile geometry, the scan step s <- A^CS s + zs on one DPP row per clip, and the host side of A^CS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace syg {
namespace sos {

constexpr int CS = 256;      // samples per chunk
constexpr int TS = 32;       // samples per LDS tile row group
constexpr int MAXS = 8;      // sections of one cascade (one state vector of the scan)
constexpr int MAXD = 2 * MAXS;
constexpr int LSTR = 36;     // LDS tile row stride (floats): one row = the 32 samples of one chunk (+4 pad)
constexpr int AHEAD = 32;    // chunk states the scan keeps in flight: a step is ~150 cycles, memory latency an order more

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte access at 4-byte alignment

// ---- scan: 16 lanes per clip (one DPP row); lane r carries state component r.  The state vector is broadcast
// inside the row with DPP row_newbcast (two 32-bit moves per double) instead of ds_bpermute.
template <int J>
__device__ __forceinline__ double row_bcast(double v) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, 0x150 + J, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), 0x150 + J, 0xF, 0xF, false);
  return __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo));
}
template <int D, int J>
__device__ __forceinline__ void bcast_all(double (&b)[D], double s) {
  if constexpr (J < D) {
    b[J] = row_bcast<J>(s);
    bcast_all<D, J + 1>(b, s);
  }
}

// row . state with four independent partial sums (the serial scan is latency-bound: one accumulator would chain
// D dependent fp64 FMAs per step); fixed summation order, so results are reproducible
template <int D>
__device__ __forceinline__ double row_dot(const double (&arow)[D], double s, double z) {
  double b[D];
  bcast_all<D, 0>(b, s);
  double p0 = z, p1 = 0.0, p2 = 0.0, p3 = 0.0;
#pragma unroll
  for (int j = 0; j < D; j += 4) {
    p0 = fma(arow[j], b[j], p0);
    if (j + 1 < D) p1 = fma(arow[j + 1], b[j + 1], p1);
    if (j + 2 < D) p2 = fma(arow[j + 2], b[j + 2], p2);
    if (j + 3 < D) p3 = fma(arow[j + 3], b[j + 3], p3);
  }
  return (p0 + p1) + (p2 + p3);
}

// ---- host: one step of the cascade (sos5 = b0 b1 b2 a1 a2 per section, a0 = 1) and A^n
inline void host_step(const double* sos5, int S, double* z, double x) {
  double u = x;
  for (int s = 0; s < S; ++s) {
    const double* c = sos5 + 5 * s;  // b0 b1 b2 a1 a2
    const double y = c[0] * u + z[2 * s];
    z[2 * s] = c[1] * u - c[3] * y + z[2 * s + 1];
    z[2 * s + 1] = c[2] * u - c[4] * y;
    u = y;
  }
}

// A: the homogeneous one-step map of the cascade's state, column j = step(e_j, x = 0); row-major, MAXD-strided
inline void one_step_matrix(const double* sos5, int S, double* A1) {
  const int D = 2 * S;
  for (int i = 0; i < MAXD * MAXD; ++i) A1[i] = 0.0;
  for (int j = 0; j < D; ++j) {
    double z[MAXD] = {0};
    z[j] = 1.0;
    host_step(sos5, S, z, 0.0);
    for (int i = 0; i < D; ++i) A1[i * MAXD + j] = z[i];
  }
}

// A^n (row-major D x D in a MAXD-strided array), n >= 0, by square and multiply (n <= 256: at most 16 products)
inline void mat_pow(const double* A1, int D, int n, double* out) {
  double R[MAXD * MAXD] = {0}, Bm[MAXD * MAXD] = {0}, T[MAXD * MAXD];
  auto mul = [&](const double* X, const double* Y, double* Z) {  // Z = X Y (Z may alias X or Y)
    for (int i = 0; i < D; ++i)
      for (int j = 0; j < D; ++j) {
        double acc = 0.0;
        for (int k = 0; k < D; ++k) acc += X[i * MAXD + k] * Y[k * MAXD + j];
        T[i * MAXD + j] = acc;
      }
    for (int i = 0; i < D; ++i)
      for (int j = 0; j < D; ++j) Z[i * MAXD + j] = T[i * MAXD + j];
  };
  for (int i = 0; i < D; ++i) R[i * MAXD + i] = 1.0;
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) Bm[i * MAXD + j] = A1[i * MAXD + j];
  for (int e = n; e > 0; e >>= 1) {
    if (e & 1) mul(R, Bm, R);
    if (e > 1) mul(Bm, Bm, Bm);
  }
  for (int i = 0; i < MAXD * MAXD; ++i) out[i] = R[i];
}

}  // namespace sos
}  // namespace syg
