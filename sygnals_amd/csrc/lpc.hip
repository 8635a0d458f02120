// Linear prediction (LPC): Burg's method and the autocorrelation method on frames and on whole rows, and the spectral
// envelope of the coefficients.  The float64 restatement that is the contract lives in tests/lpc_ref.py.
//
//     burg      f = x[1:], b = x[:-1];  k_i = -2 sum f b / (sum (f^2 + b^2) + tiny);  a <- a + k_i reversed(a);
//               f, b <- (f + k_i b)[1:], (b + k_i f)[:-1];  err = sum (f^2 + b^2) / (2 (N - 1 - p)) after p stages
//     autocorr  r[l] = sum_n xw[n] xw[n + l], l = 0 .. p;  Levinson-Durbin on r;  err = (r[0] + sum_j a[j] r[j]) / N
//
// Everything past the load is float64: the rounding of f and b is amplified by the prediction gain (a float32 recurrence
// is 4e-5 off at order 32 on a sine with 1 % noise).
//
// Frame kernel (lpc_frames_kernel<E>), 64 (E - 1) < N <= 64 E samples a frame, E = 1 .. 32 registers per lane for each
// of f and b, so that a short frame does not pay for 2048.  A workgroup of LPC_WAVES waves takes a tile of LPC_TILE
// consecutive frames of one clip.  Where the tile's span of samples, (LPC_TILE - 1) hop + N, is at most LPC_SPAN_MAX floats,
// the workgroup reads it from global memory once into LDS; otherwise every wave reads its frame itself.  One wave holds
// one frame in registers: sample n in lane n % 64, register n / 64 (coalesced loads, no LDS bank conflict, and every
// register number below is known at compile time).
//   Burg.  F[n] = f[n] and V[n] = b[n - 1] (b delayed by one sample) sit in the same lane and register, so a stage is
//   two fused multiply-adds per element; the new b then moves up one sample: a whole-wave DPP rotate by one lane per
//   register and a select that hands lane 0 the lane 63 of the register below.  The sample that leaves the frame at the
//   low end (lane i + 1 of register 0) and the slot after the frame's last sample (register E - 1) are set to zero, so
//   everything outside the frame stays zero and the sums need no mask.  The numerator is summed again every stage; the
//   denominator is carried forward as librosa does, den <- (1 - k^2) den - f_new[0]^2 - b_new[-1]^2, from the two
//   elements that leave: three float64 fma and four 32-bit moves per element and stage.
//   Autocorr.  X stays, a copy moves down one sample per lag (the same rotate and select); a lag is one fma per
//   element.  The lags land in a lane-indexed register (lane l holds r[l + 1]) and the Levinson recursion runs across
//   the lanes: its inner product is one cross-lane read and one wave sum per stage.
//   Both methods keep a[1 ..] and k in lane-indexed registers (lane l: a[l + 1], k[l]); the step-up a <- a + k
//   reversed(a) is one cross-lane read.  The tile's results go to LDS and are stored with the frame index fastest.
// Sums run in one fixed order (a lane's registers, then the DPP tree of wave_sum_d), no atomics: the same call gives the
// same bits and a batch equals its rows.
//
// Whole rows (syg_lpc_rows_f32), any length: Burg stage by stage over a float64 workspace F, G [B, L].  f_i[n] is kept
// at F[n] and b_i[n] at G[n - i]: the pair of a stage is then (F[n], G[n - i]) for the thread that owns n, read and
// written in place by that thread alone, and nothing moves.  Launch i (0 .. p) reduces the partial sums of launch i - 1
// in a fixed order (every workgroup, redundantly), forms k_{i-1}, applies it to its chunk of LPC_STAGE_CHUNK samples and
// leaves the sums of its own pairs plus its first f and last b: the pair across a chunk's border is added by the next
// launch's reduction.  The three sums (f^2, b^2, f b) take each pair at the same place, so a constant row gives k_0 = -1
// exactly.  A last one-wave launch steps k up to a.  Autocorr is one launch of partial lag sums over chunks of
// LPC_ACORR_CHUNK samples and a one-wave launch that adds them in order and runs the Levinson recursion.
//
// Envelope (syg_lpc_envelope_f32): a thread per (clip, bin, frame), Horner's rule in float64 on the unit phasor of a
// float64 host table; P = err / |A|^2 or 10 log10(max(P, amin)).
#include <float.h>
#include <math.h>
#include "host.h"

namespace syg {
namespace {

constexpr int LPC_MAX_FRAME = 2048;       // longest frame of the frame kernel (64 lanes x 32 elements)
constexpr int LPC_MAX_ORDER = 64;         // a[1 ..] and k fit the 64 lanes
constexpr int LPC_WAVES = 4;              // waves of a workgroup of the frame kernel
constexpr int LPC_TILE = 16;              // consecutive frames a workgroup takes, stages and stores together
constexpr int LPC_SPAN_MAX = 12288;       // floats of a tile's span that are staged in LDS
constexpr int LPC_STAGE_CHUNK = 6144;     // samples a workgroup of the stage form owns (48 KiB of float64 in LDS)
constexpr int LPC_STAGE_PER = LPC_STAGE_CHUNK / 256;
constexpr int LPC_ACORR_CHUNK = 4096;     // samples a workgroup of the row autocorrelation owns
constexpr int LPC_PART = 5;               // doubles a workgroup of a stage leaves: ff, bb, fb, its first f, its last b
constexpr int LPC_WAVE_ROL1 = 0x134, LPC_WAVE_ROR1 = 0x13C;   // whole-wave rotate left / right by one lane (gfx9 DPP)
constexpr double LPC_TINY = DBL_MIN;      // the smallest normal float64

// a <- a + k reversed(a) for stage i: lane l holds a[l + 1]; a_new[j] = a[j] + k a[i + 1 - j], j = 1 .. i + 1, a[0] = 1
__device__ __forceinline__ double step_up(double A, double k, int i, int lane) {
  const int src = i - lane - 1;
  double part = __shfl(A, src & 63, 64);
  part = src < 0 ? 1.0 : part;
  return lane <= i ? fma(k, part, A) : A;
}

// Levinson-Durbin on r[0] = r0, r[l + 1] in lane l of R: a[l + 1] -> A, k[l] -> K
__device__ __forceinline__ void levinson_wave(double r0, double R, int p, int lane, double& A, double& K) {
  A = 0.0;
  K = 0.0;
  if (r0 == 0.0) return;
  double E = r0;
  for (int i = 0; i < p; ++i) {
    const double rr = __shfl(R, (i - lane - 1) & 63, 64);      // r[i - l], the partner of a[l + 1]
    const double acc = rl_d(R, i) + wave_sum_d(lane < i ? A * rr : 0.0);
    const double k = E > 0.0 ? -acc / E : 0.0;
    A = step_up(A, k, i, lane);
    if (lane == i) K = k;
    E *= 1.0 - k * k;
  }
}

// b moves up one sample: V[n] = t[n - 1], V[0] = 0; the slot after the frame's last sample (where there is one) stays 0
template <int E>
__device__ __forceinline__ void shift_up(const double (&t)[E], double (&V)[E], int N, int lane) {
  double prev = 0.0;
#pragma unroll
  for (int r = 0; r < E; ++r) {
    const double rot = dpp_d<LPC_WAVE_ROR1>(t[r]);             // lane l gets lane l - 1, lane 0 gets lane 63
    V[r] = lane == 0 ? prev : rot;
    prev = rot;
  }
  if (N < 64 * E && lane == (N & 63)) V[E - 1] = 0.0;
}

// U holds the frame X (sample n in lane n % 64, register n / 64); on return A, K, err of Burg's method
template <int E>
__device__ __forceinline__ void burg_wave(double (&U)[E], double (&V)[E], int N, int p, int lane, double& A, double& K, double& err) {
  shift_up<E>(U, V, N, lane);                                 // V[n] = x[n - 1], the b of f = U[n] = x[n], n >= 1
  if (lane == 0) U[0] = 0.0;
  double ff = 0.0, bb = 0.0, fb = 0.0;
#pragma unroll
  for (int r = 0; r < E; ++r) {
    ff = fma(U[r], U[r], ff);
    bb = fma(V[r], V[r], bb);
    fb = fma(U[r], V[r], fb);
  }
  double den = wave_sum_d(ff) + wave_sum_d(bb), num = wave_sum_d(fb);
  A = 0.0;
  K = 0.0;
  const int ltop = (N - 1) & 63;
  for (int i = 0; i < p; ++i) {
    const double k = -2.0 * num / (den + LPC_TINY);
    A = step_up(A, k, i, lane);
    if (lane == i) K = k;
    // one pass: the pair's update, the new b moved up one sample (lane 0 takes lane 63 of the register below) and the
    // next numerator.  The products at the two slots that are zeroed below are zero already: their other factor is.
    double prev = 0.0, top = 0.0, s = 0.0;
#pragma unroll
    for (int r = 0; r < E; ++r) {
      const double t = fma(k, U[r], V[r]);
      U[r] = fma(k, V[r], U[r]);
      if (r == E - 1) top = rl_d(t, ltop);                    // b_new[-1]
      const double rot = dpp_d<LPC_WAVE_ROR1>(t);
      V[r] = lane == 0 ? prev : rot;
      prev = rot;
      s = fma(U[r], V[r], s);
    }
    if (N < 64 * E && lane == (N & 63)) V[E - 1] = 0.0;
    // f_new[0] leaves the frame: read it, then zero it, so that everything under the frame's low end stays zero
    const int d = i + 1;
    double fd;
    if (d < 64) {
      fd = rl_d(U[0], d);
      if (lane == d) U[0] = 0.0;
    } else {
      fd = rl_d(U[E >= 2 ? 1 : 0], 0);
      if (lane == 0) U[E >= 2 ? 1 : 0] = 0.0;
    }
    den = (1.0 - k * k) * den - fd * fd - top * top;
    if (i + 1 < p) num = wave_sum_d(s);
  }
  err = den / (2.0 * (double)(N - 1 - p));
}

template <int E>
__device__ __forceinline__ void autocorr_wave(double (&U)[E], double (&V)[E], int N, int p, int lane, double& A, double& K,
                                              double& err) {
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < E; ++r) {
    V[r] = U[r];
    s = fma(U[r], U[r], s);
  }
  const double r0 = wave_sum_d(s);
  double R = 0.0;
  for (int l = 1; l <= p; ++l) {
    // the copy moves down one sample: V[n] <- V[n + 1], zero after the last register
    double next = 0.0;
#pragma unroll
    for (int r = E - 1; r >= 0; --r) {
      const double rot = dpp_d<LPC_WAVE_ROL1>(V[r]);           // lane l gets lane l + 1, lane 63 gets lane 0
      V[r] = lane == 63 ? next : rot;
      next = rot;
    }
    s = 0.0;
#pragma unroll
    for (int r = 0; r < E; ++r) s = fma(U[r], V[r], s);
    const double rl = wave_sum_d(s);
    if (lane == l - 1) R = rl;
  }
  levinson_wave(r0, R, p, lane, A, K);
  err = (r0 + wave_sum_d(lane < p ? A * R : 0.0)) / (double)N;
}

struct LpcArgs {
  const float* y; int64_t L, ldy; int N, hop, pad, staged, span_floats; int64_t T, tiles_per_clip, tiles;
  const float* win; int p, method; float *a, *k, *err;
};

template <int E>
__global__ __launch_bounds__(LPC_WAVES * 64, 2) void lpc_frames_kernel(LpcArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lp_smem[];
  float* span = lp_smem;
  float* stage = lp_smem + A.span_floats;                     // [LPC_TILE][2 p + 3]: a[0 .. p], k[0 .. p - 1], err, one of padding
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = A.p, N = A.N, Sp = 2 * p + 3;
  for (int64_t tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
    const int64_t b = tile / A.tiles_per_clip, t0 = (tile - b * A.tiles_per_clip) * LPC_TILE;
    const int cnt = (int)(A.T - t0 < LPC_TILE ? A.T - t0 : LPC_TILE);
    const float* __restrict__ yr = A.y + b * A.ldy;
    const int64_t sbase = t0 * A.hop - A.pad;
    if (A.staged) {
      const int len = (cnt - 1) * A.hop + N;
      for (int q = tid; q < len; q += LPC_WAVES * 64) {
        const int64_t s = sbase + q;
        span[q] = (s >= 0 && s < A.L) ? yr[s] : 0.f;
      }
      __syncthreads();
    }
    for (int tt = w; tt < cnt; tt += LPC_WAVES) {
      double U[E], V[E];
#pragma unroll
      for (int r = 0; r < E; ++r) {
        const int n = 64 * r + lane;
        double x = 0.0;
        if (n < N) {
          float v;
          if (A.staged) {
            v = span[tt * A.hop + n];
          } else {
            const int64_t s = sbase + (int64_t)tt * A.hop + n;
            v = (s >= 0 && s < A.L) ? yr[s] : 0.f;
          }
          x = A.win ? (double)v * (double)A.win[n] : (double)v;
        }
        U[r] = x;
      }
      double Aa, Kk, er;
      if (A.method == SYG_LPC_BURG) burg_wave<E>(U, V, N, p, lane, Aa, Kk, er);
      else autocorr_wave<E>(U, V, N, p, lane, Aa, Kk, er);
      float* row = stage + tt * Sp;
      if (lane == 0) {
        row[0] = 1.f;
        row[2 * p + 1] = (float)er;
      }
      if (lane < p) {
        row[1 + lane] = (float)Aa;
        row[p + 1 + lane] = (float)Kk;
      }
    }
    __syncthreads();
    // ---- the tile's stage to a [B, p + 1, T], k [B, p, T], err [B, T], frames fastest
    for (int i = tid; i < (2 * p + 2) * LPC_TILE; i += LPC_WAVES * 64) {
      const int tt = i & (LPC_TILE - 1), q = i / LPC_TILE;
      if (tt >= cnt) continue;
      const float v = stage[tt * Sp + q];
      const int64_t t = t0 + tt;
      if (q <= p) A.a[(b * (p + 1) + q) * A.T + t] = v;
      else if (q <= 2 * p) { if (A.k) A.k[(b * p + (q - p - 1)) * A.T + t] = v; }
      else if (A.err) A.err[b * A.T + t] = v;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ whole rows, Burg
// sum of three doubles per thread over a workgroup of 256 threads, in a fixed order; red: 12 doubles of LDS
__device__ __forceinline__ void block_sum3(double& a, double& b, double& c, double* red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  a = wave_sum_d(a);
  b = wave_sum_d(b);
  c = wave_sum_d(c);
  __syncthreads();                                            // red may still be read from a call before
  if (lane == 0) {
    red[wv] = a;
    red[4 + wv] = b;
    red[8 + wv] = c;
  }
  __syncthreads();
  a = (red[0] + red[1]) + (red[2] + red[3]);
  b = (red[4] + red[5]) + (red[6] + red[7]);
  c = (red[8] + red[9]) + (red[10] + red[11]);
}

// the sums of a stage over a row from its workgroups' parts: their own pairs, then the pair across each border
__device__ __forceinline__ void reduce_parts(const double* __restrict__ P, int64_t nblk, double* red, double& ff, double& bb, double& fb) {
  ff = 0.0;
  bb = 0.0;
  fb = 0.0;
  for (int64_t c = threadIdx.x; c < nblk; c += 256) {
    const double* q = P + c * LPC_PART;
    ff += q[0];
    bb += q[1];
    fb += q[2];
    if (c > 0) {
      const double f = q[3], b = q[4 - LPC_PART];
      ff = fma(f, f, ff);
      bb = fma(b, b, bb);
      fb = fma(f, b, fb);
    }
  }
  block_sum3(ff, bb, fb, red);
}

struct StageArgs {
  const float* y; int64_t L, ldy; const float* win; int i; int64_t nblk;
  double *F, *G; const double* part_prev; double* part_cur; double* kbuf;
};

__global__ __launch_bounds__(256) void lpc_stage_kernel(StageArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lp_sb[];      // the chunk's new b
  __shared__ double red[12];
  const int tid = threadIdx.x, i = A.i;
  const int64_t b = blockIdx.x / A.nblk, c = blockIdx.x - b * A.nblk;
  const int64_t n0 = c * LPC_STAGE_CHUNK;
  const int cnt = (int)(A.L - n0 < LPC_STAGE_CHUNK ? A.L - n0 : LPC_STAGE_CHUNK);
  double k = 0.0;
  if (i >= 1) {
    double ff, bb, fb;
    reduce_parts(A.part_prev + b * A.nblk * LPC_PART, A.nblk, red, ff, bb, fb);
    k = -2.0 * fb / (ff + bb + LPC_TINY);
    if (c == 0 && tid == 0) A.kbuf[b * LPC_MAX_ORDER + i - 1] = k;
  }
  double* __restrict__ F = A.F + b * A.L;
  double* __restrict__ G = A.G + b * A.L;
  const float* __restrict__ yr = A.y + b * A.ldy;
  double fr[LPC_STAGE_PER];
#pragma unroll
  for (int u = 0; u < LPC_STAGE_PER; ++u) {
    const int q = tid + 256 * u;
    const int64_t n = n0 + q;
    double f = 0.0, g = 0.0;
    if (q < cnt) {
      if (i == 0) {
        f = A.win ? (double)yr[n] * (double)A.win[n] : (double)yr[n];
        g = f;
        F[n] = f;
        G[n] = g;
      } else if (n >= i) {                                    // the pair (f_{i-1}[n], b_{i-1}[n - 1]) -> f_i[n], b_i[n]
        const double f0 = F[n], g0 = G[n - i];
        f = fma(k, g0, f0);
        g = fma(k, f0, g0);
        F[n] = f;
        G[n - i] = g;
      }
      lp_sb[q] = g;
    }
    fr[u] = f;
  }
  __syncthreads();
  // the pairs (f_i[n], b_i[n - 1]) of stage i, n >= i + 1, that lie inside the chunk
  double ff = 0.0, bb = 0.0, fb = 0.0;
#pragma unroll
  for (int u = 0; u < LPC_STAGE_PER; ++u) {
    const int q = tid + 256 * u;
    if (q >= 1 && q < cnt && n0 + q >= i + 1) {
      const double f = fr[u], g = lp_sb[q - 1];
      ff = fma(f, f, ff);
      bb = fma(g, g, bb);
      fb = fma(f, g, fb);
    }
  }
  block_sum3(ff, bb, fb, red);
  if (tid == 0) {
    double* q = A.part_cur + (b * A.nblk + c) * LPC_PART;
    q[0] = ff;
    q[1] = bb;
    q[2] = fb;
    q[3] = fr[0];
    q[4] = lp_sb[cnt - 1];
  }
}

struct FinishArgs {
  int64_t L, nblk; int p; const double* part; const double* kbuf; float *a, *k, *err;
};

// one wave per row: the last sums -> err, k stepped up to a
__global__ __launch_bounds__(64) void lpc_burg_finish_kernel(FinishArgs A) {
  const int lane = threadIdx.x, p = A.p;
  const int64_t b = blockIdx.x;
  const double* P = A.part + b * A.nblk * LPC_PART;
  double ff = 0.0, bb = 0.0;
  for (int64_t c = lane; c < A.nblk; c += 64) {
    const double* q = P + c * LPC_PART;
    ff += q[0];
    bb += q[1];
    if (c > 0) {
      ff = fma(q[3], q[3], ff);
      bb = fma(q[4 - LPC_PART], q[4 - LPC_PART], bb);
    }
  }
  const double den = wave_sum_d(ff) + wave_sum_d(bb);
  double Aa = 0.0, Kk = 0.0;
  for (int i = 0; i < p; ++i) {
    const double k = A.kbuf[b * LPC_MAX_ORDER + i];
    Aa = step_up(Aa, k, i, lane);
    if (lane == i) Kk = k;
  }
  if (lane == 0) {
    A.a[b * (p + 1)] = 1.f;
    if (A.err) A.err[b] = (float)(den / (2.0 * (double)(A.L - 1 - p)));
  }
  if (lane < p) {
    A.a[b * (p + 1) + 1 + lane] = (float)Aa;
    if (A.k) A.k[b * p + lane] = (float)Kk;
  }
}

// ------------------------------------------------------------------------------------------------ whole rows, autocorr
__global__ __launch_bounds__(256) void lpc_acorr_part_kernel(const float* __restrict__ y, int64_t L, int64_t ldy, const float* __restrict__ win,
                                                            int p, int64_t nblk, double* __restrict__ part) {
  __shared__ double xs[LPC_ACORR_CHUNK + LPC_MAX_ORDER];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t b = blockIdx.x / nblk, c = blockIdx.x - b * nblk;
  const int64_t n0 = c * LPC_ACORR_CHUNK;
  const int cnt = (int)(L - n0 < LPC_ACORR_CHUNK ? L - n0 : LPC_ACORR_CHUNK);
  const float* __restrict__ yr = y + b * ldy;
  for (int q = tid; q < LPC_ACORR_CHUNK + LPC_MAX_ORDER; q += 256) {
    const int64_t n = n0 + q;
    xs[q] = n < L ? (win ? (double)yr[n] * (double)win[n] : (double)yr[n]) : 0.0;
  }
  __syncthreads();
  for (int l = w; l <= p; l += 4) {
    double s = 0.0;
    for (int q = lane; q < cnt; q += 64) s = fma(xs[q], xs[q + l], s);
    s = wave_sum_d(s);
    if (lane == 0) part[(b * nblk + c) * (LPC_MAX_ORDER + 1) + l] = s;
  }
}

__global__ __launch_bounds__(64) void lpc_acorr_finish_kernel(int64_t L, int64_t nblk, int p, const double* __restrict__ part, float* a,
                                                             float* kout, float* err) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const double* P = part + b * nblk * (LPC_MAX_ORDER + 1);
  double r0 = 0.0, R = 0.0;
  for (int64_t c = 0; c < nblk; ++c) {
    r0 += P[c * (LPC_MAX_ORDER + 1)];
    if (lane < p) R += P[c * (LPC_MAX_ORDER + 1) + 1 + lane];
  }
  double Aa, Kk;
  levinson_wave(r0, R, p, lane, Aa, Kk);
  const double e = (r0 + wave_sum_d(lane < p ? Aa * R : 0.0)) / (double)L;
  if (lane == 0) {
    a[b * (p + 1)] = 1.f;
    if (err) err[b] = (float)e;
  }
  if (lane < p) {
    a[b * (p + 1) + 1 + lane] = (float)Aa;
    if (kout) kout[b * p + lane] = (float)Kk;
  }
}

// ------------------------------------------------------------------------------------------------ envelope
__global__ __launch_bounds__(256) void lpc_envelope_kernel(const float* __restrict__ a, const float* __restrict__ err, int64_t B, int p, int64_t T,
                                                          int64_t K, const double* __restrict__ ph, int db, float amin, float* __restrict__ out) {
  const int64_t total = B * K * T;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = i % T, bk = i / T, kk = bk % K, b = bk / K;
    const float* __restrict__ ap = a + b * (p + 1) * T + t;
    const double zr = ph[2 * kk], zi = ph[2 * kk + 1];
    double ar = (double)ap[(int64_t)p * T], ai = 0.0;
    for (int j = p - 1; j >= 0; --j) {
      const double nr = fma(ar, zr, -ai * zi) + (double)ap[(int64_t)j * T];
      ai = fma(ar, zi, ai * zr);
      ar = nr;
    }
    const float P = (float)((double)err[b * T + t] / fma(ar, ar, ai * ai));
    out[i] = db ? 10.f * log10f(fmaxf(P, amin)) : P;
  }
}

int check_order(const char* who, int order, int64_t N) {
  const int64_t hi = N - 2 < LPC_MAX_ORDER ? N - 2 : LPC_MAX_ORDER;
  SYG_REQUIRE(order >= 1 && order <= hi, "%s: order=%d is outside 1 ... min(%d, N - 2) = %lld for N = %lld samples", who, order, LPC_MAX_ORDER,
              (long long)hi, (long long)N);
  return SYG_OK;
}
int check_method(const char* who, int method) {
  SYG_REQUIRE(method == SYG_LPC_BURG || method == SYG_LPC_AUTOCORR, "%s: method=%d is neither SYG_LPC_BURG (0) nor SYG_LPC_AUTOCORR (1)", who,
              method);
  return SYG_OK;
}
int64_t stage_blocks(int64_t L) { return ceil_div(L, LPC_STAGE_CHUNK); }
int64_t acorr_blocks(int64_t L) { return ceil_div(L, LPC_ACORR_CHUNK); }
bool rows_ok(int64_t B, int64_t L) { return B >= 1 && L >= 3 && L <= ((int64_t)1 << 26) && B <= ((int64_t)1 << 31) / L; }

template <int E>
void launch_frames(const LpcArgs& A, unsigned blocks, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL(lpc_frames_kernel<E>, dim3(blocks), dim3(LPC_WAVES * 64), lds, s, A);
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_lpc_constants(int key) {
  switch (key) {
    case SYG_LPC_MAX_FRAME: return LPC_MAX_FRAME;
    case SYG_LPC_MAX_ORDER: return LPC_MAX_ORDER;
    case SYG_LPC_WAVES: return LPC_WAVES;
    case SYG_LPC_TILE_FRAMES: return LPC_TILE;
    case SYG_LPC_SPAN_MAX: return LPC_SPAN_MAX;
    case SYG_LPC_STAGE_CHUNK: return LPC_STAGE_CHUNK;
    case SYG_LPC_ACORR_CHUNK: return LPC_ACORR_CHUNK;
    default: set_error("lpc_constants: unknown key %d", key); return -1;
  }
}

extern "C" int syg_lpc_frames_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int frame_length, int hop, int center, int64_t T,
                                  const float* window, int order, int method, float* a, float* k, float* err, void* stream) {
  SYG_REQUIRE(y && a, "lpc_frames: null pointer argument (y / a)");
  if (frame_length > LPC_MAX_FRAME || frame_length < 3) {
    set_error("lpc_frames: frame_length %d is not served by the frame kernel (3 ... %d; longer rows take syg_lpc_rows_f32)", frame_length,
              LPC_MAX_FRAME);
    return SYG_E_UNSUPPORTED;
  }
  if (const int rc = check_method("lpc_frames", method)) return rc;
  if (const int rc = check_order("lpc_frames", order, frame_length)) return rc;
  SYG_REQUIRE(B >= 1 && L >= 1 && ldy >= L, "lpc_frames: bad B / L / ldy");
  SYG_REQUIRE(hop >= 1 && (center == 0 || center == 1), "lpc_frames: bad hop / center");
  const int N = frame_length;
  const bool pow2_rule = is_pow2(N) && N >= 8;               // the frame count of the transform front ends, as for the cepstrogram
  if (const int rc = check_framing("lpc_frames", T, pow2_rule ? frames_expected(L, N, hop, center) : frames_padded(L, N, hop, center)))
    return rc;
  SYG_REQUIRE(T <= ((int64_t)1 << 31) / (order + 1) / B, "lpc_frames: the result of %lld x %d x %lld elements is above 2^31", (long long)B,
              order + 1, (long long)T);
  const int64_t span = (int64_t)(LPC_TILE - 1) * hop + N;
  const int staged = span <= LPC_SPAN_MAX;
  const int span_floats = staged ? (int)span : 0;
  const int64_t tpc = ceil_div(T, LPC_TILE);
  LpcArgs A{y, L, ldy, N, hop, center ? N / 2 : 0, staged, span_floats, T, tpc, B * tpc, window, order, method, a, k, err};
  const size_t lds = sizeof(float) * ((size_t)span_floats + (size_t)LPC_TILE * (size_t)(2 * order + 3));
  hipStream_t s = (hipStream_t)stream;
  switch ((N + 63) / 64) {                                   // registers a lane holds of each of f and b
#define SYG_LPC_CASE(E) case E: launch_frames<E>(A, capped_grid(A.tiles, LPC_FRAMES_WGS_PER_CU), lds, s); break;
    SYG_LPC_CASE(1) SYG_LPC_CASE(2) SYG_LPC_CASE(3) SYG_LPC_CASE(4) SYG_LPC_CASE(5) SYG_LPC_CASE(6) SYG_LPC_CASE(7) SYG_LPC_CASE(8)
    SYG_LPC_CASE(9) SYG_LPC_CASE(10) SYG_LPC_CASE(11) SYG_LPC_CASE(12) SYG_LPC_CASE(13) SYG_LPC_CASE(14) SYG_LPC_CASE(15) SYG_LPC_CASE(16)
    SYG_LPC_CASE(17) SYG_LPC_CASE(18) SYG_LPC_CASE(19) SYG_LPC_CASE(20) SYG_LPC_CASE(21) SYG_LPC_CASE(22) SYG_LPC_CASE(23) SYG_LPC_CASE(24)
    SYG_LPC_CASE(25) SYG_LPC_CASE(26) SYG_LPC_CASE(27) SYG_LPC_CASE(28) SYG_LPC_CASE(29) SYG_LPC_CASE(30) SYG_LPC_CASE(31) SYG_LPC_CASE(32)
#undef SYG_LPC_CASE
  }
  SYG_CHECK_LAUNCH("lpc_frames");
  return SYG_OK;
}

extern "C" int64_t syg_lpc_rows_work_bytes(int64_t B, int64_t L, int order, int method) {
  if (!rows_ok(B, L) || order < 1 || order > LPC_MAX_ORDER || (method != SYG_LPC_BURG && method != SYG_LPC_AUTOCORR)) {
    set_error("lpc_rows_work_bytes: bad B / L / order / method (B >= 1, L in [3, 2^26], B L <= 2^31, order in [1, %d])", LPC_MAX_ORDER);
    return -1;
  }
  if (method == SYG_LPC_AUTOCORR) return 8 * B * acorr_blocks(L) * (LPC_MAX_ORDER + 1);
  return 8 * (2 * B * L + 2 * B * stage_blocks(L) * LPC_PART + B * LPC_MAX_ORDER);
}

extern "C" int syg_lpc_rows_f32(const float* y, int64_t B, int64_t L, int64_t ldy, const float* window, int order, int method, void* work,
                                int64_t work_bytes, float* a, float* k, float* err, void* stream) {
  SYG_REQUIRE(y && a, "lpc_rows: null pointer argument (y / a)");
  if (const int rc = check_method("lpc_rows", method)) return rc;
  SYG_REQUIRE(rows_ok(B, L) && ldy >= L, "lpc_rows: bad B / L / ldy (B >= 1, L in [3, 2^26], B L <= 2^31)");
  if (const int rc = check_order("lpc_rows", order, L)) return rc;
  const int64_t need = syg_lpc_rows_work_bytes(B, L, order, method);
  SYG_REQUIRE(work && work_bytes >= need && ((uintptr_t)work & 7) == 0,
              "lpc_rows: workspace of %lld bytes needed (syg_lpc_rows_work_bytes, 8-byte aligned), got %lld", (long long)need,
              (long long)work_bytes);
  hipStream_t s = (hipStream_t)stream;
  if (method == SYG_LPC_AUTOCORR) {
    const int64_t nblk = acorr_blocks(L);
    SYG_REQUIRE(B * nblk < 0x7fffffff, "lpc_rows: too many blocks");
    double* part = (double*)work;
    hipLaunchKernelGGL(lpc_acorr_part_kernel, dim3((unsigned)(B * nblk)), dim3(256), 0, s, y, L, ldy, window, order, nblk, part);
    hipLaunchKernelGGL(lpc_acorr_finish_kernel, dim3((unsigned)B), dim3(64), 0, s, L, nblk, order, (const double*)part, a, k, err);
    SYG_CHECK_LAUNCH("lpc_rows");
    return SYG_OK;
  }
  const int64_t nblk = stage_blocks(L);
  SYG_REQUIRE(B * nblk < 0x7fffffff, "lpc_rows: too many blocks");
  double* F = (double*)work;
  double* G = F + B * L;
  double* part[2] = {G + B * L, G + B * L + B * nblk * LPC_PART};
  double* kbuf = part[1] + B * nblk * LPC_PART;
  for (int i = 0; i <= order; ++i) {
    StageArgs A{y, L, ldy, window, i, nblk, F, G, part[(i + 1) & 1], part[i & 1], kbuf};
    hipLaunchKernelGGL(lpc_stage_kernel, dim3((unsigned)(B * nblk)), dim3(256), sizeof(double) * LPC_STAGE_CHUNK, s, A);
  }
  FinishArgs Fa{L, nblk, order, part[order & 1], kbuf, a, k, err};
  hipLaunchKernelGGL(lpc_burg_finish_kernel, dim3((unsigned)B), dim3(64), 0, s, Fa);
  SYG_CHECK_LAUNCH("lpc_rows");
  return SYG_OK;
}

extern "C" int syg_lpc_envelope_f32(const float* a, const float* err, int64_t B, int order, int64_t T, int n_fft, const double* phasor, int db,
                                    double amin, float* out, void* stream) {
  SYG_REQUIRE(a && err && phasor && out, "lpc_envelope: null pointer argument (a / err / phasor / out)");
  SYG_REQUIRE(order >= 1 && order <= LPC_MAX_ORDER, "lpc_envelope: order=%d is outside 1 ... %d", order, LPC_MAX_ORDER);
  SYG_REQUIRE(n_fft >= 2 && n_fft <= (1 << 24) && n_fft % 2 == 0, "lpc_envelope: n_fft=%d must be even and in [2, 2^24]", n_fft);
  SYG_REQUIRE(db == 0 || db == 1, "lpc_envelope: db must be 0 or 1");
  SYG_REQUIRE(amin >= 0.0 && amin <= (double)FLT_MAX, "lpc_envelope: amin must be finite and >= 0 (got %g)", amin);
  const int64_t K = n_fft / 2 + 1;
  SYG_REQUIRE(B >= 1 && T >= 1 && T <= ((int64_t)1 << 31) / K / B, "lpc_envelope: bad B / T (each >= 1, B (n_fft / 2 + 1) T <= 2^31)");
  hipLaunchKernelGGL(lpc_envelope_kernel, dim3(capped_grid(ceil_div(B * K * T, 256), LPC_ENVELOPE_WGS_PER_CU)), dim3(256), 0,
                     (hipStream_t)stream, a, err, B, order, T, K, phasor, db, (float)amin, out);
  SYG_CHECK_LAUNCH("lpc_envelope");
  return SYG_OK;
}
