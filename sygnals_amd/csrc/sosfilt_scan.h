// What the chunked SOS filters share (sosfilt.hip: zero-phase; sosfilt_causal.hip: causal with state in and out;
// loudness.hip: the K-weighted segment powers): the chunk / tile geometry, the scan step s <- A^CS s + zs on one DPP row
// per clip, the host side of A^CS, and the causal scan over a row's chunks with its launcher.
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

struct CausalPow {
  double apow[MAXD * MAXD];  // A^CS, row-major D x D (MAXD-strided)
};

// ---- the scan over a row's chunks (pass B of sosfilt_causal.hip, whose header names the passes; loudness.hip runs the
// same three passes): 16 lanes per (row, segment) (row_dot above), the zero-state end states AHEAD chunks ahead of the
// chain.  A segment is G consecutive chunks of a row; the chain runs s <- A s + zs[c] over its chunks, writing s to
// init[c] in front of each step.  Chunk 0 ran pass A from zi[b]: its report is the state at chunk 1 as it is, and pass C
// never reads init[b, 0].
//   start   [B, nseg, D] state at each segment's first chunk (segment 0: not read), or null = zero
//   init    [B, nch, D] written where given;  ends  [B, nseg, D] the state behind each segment, written where given
// One segment per row (G = nch) is the whole scan.  A long row takes three launches (scan_rows below): every segment
// from a zero state -> ends; the same kernel over the ends as if they were chunks, with A^(CS G) -> the segments' true
// starts; every segment again from its start -> init.  2 G + nch / G serial steps instead of nch.
template <int S>
__global__ __launch_bounds__(256) void causal_scan_kernel(int nch, int G, int nseg, int64_t B, CausalPow P,
                                                          const double* __restrict__ zs, const double* __restrict__ start,
                                                          double* __restrict__ init, double* __restrict__ ends) {
  constexpr int D = 2 * S;
  const int r = threadIdx.x & 15;
  const int64_t np = B * nseg;
  const int64_t p = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = (p < np) && (r < D);
  const int64_t pp = (p < np) ? p : (np - 1);
  const int64_t b = pp / nseg;
  const int cbeg = (int)(pp % nseg) * G;                 // first chunk of the segment
  const int n = (nch - cbeg < G) ? (nch - cbeg) : G;     // its chunks (>= 1: nseg = ceil(nch / G))
  double arow[D];
#pragma unroll
  for (int j = 0; j < D; ++j) arow[j] = 0.0;
#pragma unroll
  for (int rr = 0; rr < D; ++rr)
    if (r == rr) {
#pragma unroll
      for (int j = 0; j < D; ++j) arow[j] = P.apow[rr * MAXD + j];
    }
  const int rc = (r < D) ? r : 0;
  double s = (live && start && cbeg > 0) ? start[pp * D + rc] : 0.0;
  const double* zp = zs + ((int64_t)b * nch + cbeg) * D + rc;
  double* ip = init ? init + ((int64_t)b * nch + cbeg) * D + rc : nullptr;
  const bool fill = live && init;
  double zq[AHEAD];
#pragma unroll
  for (int k = 0; k < AHEAD; ++k) zq[k] = (live && k < n) ? zp[(int64_t)k * D] : 0.0;
#pragma unroll
  for (int k = 0; k < AHEAD; ++k) asm volatile("" : "+v"(zq[k]));      // (landed before the chain starts: see below)
  for (int c0 = 0; c0 < G; c0 += AHEAD) {
    double zn[AHEAD];
#pragma unroll
    for (int k = 0; k < AHEAD; ++k) zn[k] = (live && c0 + AHEAD + k < n) ? zp[(int64_t)(c0 + AHEAD + k) * D] : 0.0;
#pragma unroll
    for (int k = 0; k < AHEAD; ++k) {
      if (c0 + k < G) {                                    // (uniform; a shorter last segment sits its tail out below)
        const bool in = c0 + k < n;
        if (fill && in) ip[(int64_t)(c0 + k) * D] = s;     // (init[b, 0] = 0: never read)
        const double t = (cbeg + c0 + k == 0) ? zq[k] : row_dot<D>(arow, s, zq[k]);
        s = in ? t : s;
      }
    }
    // the look-ahead lands HERE, once per AHEAD steps: left to itself the compiler waits for it inside the chain, step
    // by step with vmcnt(0), and so for each step's own store of init as well (1.8 x the time of a step)
#pragma unroll
    for (int k = 0; k < AHEAD; ++k) {
      zq[k] = zn[k];
      asm volatile("" : "+v"(zq[k]));
    }
  }
  if (live && ends) ends[pp * D + rc] = s;
}

constexpr int TWO_LEVEL = 256;       // rows of more chunks than this take the three-launch scan
// chunks per segment: the whole row up to TWO_LEVEL chunks, above it the multiple of AHEAD next to sqrt(nch / 2), which
// minimises the 2 G + nch / G serial steps.  A function of the row's length alone: so are the bits of a result.
inline int scan_segment(int nch) {
  if (nch <= TWO_LEVEL) return nch;
  int g = AHEAD;
  while ((int64_t)2 * g * g < nch) g += AHEAD;
  return g;
}

// the scan of nb rows of nch > 1 chunks on stream st: zs [nb, nch, D] -> init [nb, nch, D]; ends, segs [nb, nseg, D] are
// the two-level form's scratch (G = scan_segment(nch), nseg = ceil(nch / G), AG = A^(CS G))
template <int S>
inline void scan_rows(int64_t nb, int nch, const CausalPow& A, const CausalPow& AG, const double* zs, double* init,
                      double* ends, double* segs, hipStream_t st) {
  const int G = scan_segment(nch), nseg = (nch + G - 1) / G;
  auto scan_grid = [](int64_t rows) { return dim3((unsigned)((rows + 15) / 16)); };
  if (nseg == 1) {
    hipLaunchKernelGGL((causal_scan_kernel<S>), scan_grid(nb), dim3(256), 0, st, nch, nch, 1, nb, A, zs,
                       (const double*)nullptr, init, (double*)nullptr);
  } else {
    hipLaunchKernelGGL((causal_scan_kernel<S>), scan_grid(nb * nseg), dim3(256), 0, st, nch, G, nseg, nb, A, zs,
                       (const double*)nullptr, (double*)nullptr, ends);
    hipLaunchKernelGGL((causal_scan_kernel<S>), scan_grid(nb), dim3(256), 0, st, nseg, nseg, 1, nb, AG,
                       (const double*)ends, (const double*)nullptr, segs, (double*)nullptr);
    hipLaunchKernelGGL((causal_scan_kernel<S>), scan_grid(nb * nseg), dim3(256), 0, st, nch, G, nseg, nb, A, zs,
                       (const double*)segs, init, (double*)nullptr);
  }
}

}  // namespace sos
}  // namespace syg
