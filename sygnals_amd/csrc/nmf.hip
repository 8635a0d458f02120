// Non-negative matrix factorisation of a spectrogram by multiplicative updates (scikit-learn's solver="mu", which is what
// librosa.decompose.decompose runs when handed NMF(solver="mu")), the divergence of a factorisation and the soft masks of
// its components.  The float64 restatement that is the contract lives in tests/nmf_ref.py.
//
// Frame-major: V [B, T, F] = A [B, T, K] C [B, K, F]; A is sklearn's W (activations), C its H (components).  One
// iteration is the A-step, then the C-step with the new A.  eps = FLT_EPSILON.
//   Frobenius  A <- A (V C^T) / (A (C C^T))            C <- C (A^T V) / ((A^T A) C)
//   KL         A <- A ((V / AC) C^T) / sum_f C         C <- C (A^T (V / AC)) / sum_t A      (AC raised to eps)
// A denominator equal to 0 becomes eps; under KL an entry of the new C below 2^-52 becomes 0, as sklearn has it.
// No [T, F] intermediate exists in memory: V / AC lives in LDS, a tile at a time.
//
// Launches of an iteration (a half step that needs a whole reduction is a launch of its own; nothing waits on another
// workgroup):
//   factor_sums_kernel<of C>   C C^T [K, K] (Frobenius) or sum_f C [K] (KL) per clip -> scratch     one workgroup a clip
//   a_step_kernel              16 frames a workgroup, F in chunks of 64 bins through LDS
//   factor_sums_kernel<of A>   A^T A or sum_t A per clip -> the same scratch
//   c_step_kernel              64 bins a workgroup, T in chunks of 32 frames through LDS
// With the components fixed, their sums are formed once, ahead of the loop.
// The contractions over F (A-step) and T (C-step) exist in two forms, from the same LDS tiles.  FMA: a thread owns up to
// 4 (A-step) or 16 (C-step) outputs and reads both operands from LDS, one of them as a broadcast.  MFMA: 16 x 16 output
// tiles on v_mfma_f32_16x16x4_f32, whose result is an exact k-ordered fp32 fma chain, one LDS read per operand and lane,
// laid out so that the 64 lanes hit 64 banks.  SYG_NMF_FORM_AUTO takes the one that measured faster at that K
// (MFMA_MIN_K; DESIGN.md section 4.28 has both timings per K).  A sum over F or T is kept in two levels (the chunk's
// part, then the total), so its rounding grows with the chunk's length and the number of chunks, not with their product.
// Measured: a single long clip leaves most CUs idle in the per-clip sums and the C-step.
// A clip's arithmetic depends on (T, F, K) alone: a batch equals its clips bit for bit, and no atomics are used.
#include <float.h>
#include <math.h>
#include <algorithm>
#include "host.h"

namespace syg {
namespace {

constexpr int NT = 256;                  // threads of every workgroup here
constexpr int KMAX = 64;                 // components served
constexpr int FMAX = 2049;               // bins served
constexpr int GMAX = 64;                 // mask groups served
constexpr int TT = 16;                   // frames of an A-step tile
constexpr int FC = 64;                   // bins of an A-step chunk
constexpr int FT = 64;                   // bins of a C-step tile
constexpr int TC = 32;                   // frames of a C-step chunk
constexpr int SC = 64;                   // contraction indices of a factor_sums chunk
constexpr float EPS = FLT_EPSILON;
typedef float v4f __attribute__((ext_vector_type(4)));
constexpr float C_FLUSH = 2.220446049250313e-16f;   // KL: sklearn zeroes entries of H below float64's epsilon after its update

struct NmfArgs {
  const float* V; float* A; float* C; float* work;
  int64_t B, T, cstride;                 // cstride: floats from one clip's C to the next (0: one dictionary for all)
  int F, K, wstride;                     // wstride: floats of scratch a clip
};

// ------------------------------------------------------------------ C C^T / A^T A, or the sums of C's rows / A's columns
// X[c][k] over the contraction index c: of C, X[c][k] = C[k][c] (c a bin); of A, X[c][k] = A[c][k] (c a frame).
// Frobenius: work[i K + j] = sum_c X[c][i] X[c][j]; KL: work[K K + k] = sum_c X[c][k].
template <bool OF_A, bool KL>
__global__ __launch_bounds__(NT) void factor_sums_kernel(NmfArgs P) {
  __shared__ float S[SC][KMAX + 1];      // + 1: the transposed store of a C chunk walks c at a fixed k
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int K = P.K;
  const int64_t n = OF_A ? P.T : P.F;
  for (int64_t b = blockIdx.x; b < P.B; b += gridDim.x) {
    const float* X = OF_A ? P.A + b * P.T * K : P.C + b * P.cstride;
    float acc[KMAX / 4];
#pragma unroll
    for (int q = 0; q < KMAX / 4; ++q) acc[q] = 0.f;
    for (int64_t c0 = 0; c0 < n; c0 += SC) {
      for (int idx = tid; idx < SC * K; idx += NT) {
        int c, k;
        if (OF_A) { c = idx / K; k = idx - c * K; } else { k = idx / SC; c = idx - k * SC; }
        const int64_t cc = c0 + c;
        S[c][k] = cc < n ? (OF_A ? X[cc * K + k] : X[(int64_t)k * P.F + cc]) : 0.f;
      }
      __syncthreads();
      if (KL) {
        if (w == 0 && lane < K) {
          float part = 0.f;
#pragma unroll 8
          for (int c = 0; c < SC; ++c) part += S[c][lane];
          acc[0] += part;
        }
      } else if (lane < K) {
#pragma unroll
        for (int q = 0; q < KMAX / 4; ++q) {
          const int i = w + 4 * q;                       // uniform in a wave
          if (i < K) {
            float part = 0.f;
#pragma unroll 8
            for (int c = 0; c < SC; ++c) part = fmaf(S[c][i], S[c][lane], part);
            acc[q] += part;
          }
        }
      }
      __syncthreads();
    }
    float* out = P.work + b * P.wstride;
    if (KL) {
      if (w == 0 && lane < K) out[K * K + lane] = acc[0];
    } else if (lane < K) {
#pragma unroll
      for (int q = 0; q < KMAX / 4; ++q) {
        const int i = w + 4 * q;
        if (i < K) out[i * K + lane] = acc[q];
      }
    }
  }
}

// ------------------------------------------------------------------ A-step
// A workgroup owns TT frames of a clip.  FMA form: thread (tl, kq) owns the outputs (tl, kq + 16 j), j < KJ.
// MFMA form (MF): wave w < KJ owns the 16 x 16 tile of components 16 w .. 16 w + 15 on v_mfma_f32_16x16x4_f32 (an exact
// k-ordered fp32 fma chain): lane (n, kk) supplies bin 16 kk + j at step j, so that the 64 lanes read 64 LDS banks, and
// holds the outputs (frame 4 kk + i, component 16 w + n), i < 4.
template <bool KL, int KJ, bool MF>
__global__ __launch_bounds__(NT) void a_step_kernel(NmfArgs P) {
  __shared__ float As[TT][KMAX];
  __shared__ float Cs[KMAX][FC + 1];     // + 1: 16 lanes read 16 rows at one bin
  __shared__ float Xs[TT][FC + 1];       // V, or V / AC; + 1: 4 lanes of a wave read 4 rows at one bin
  __shared__ float Gs[KL ? 1 : KMAX][KMAX];
  __shared__ float Ds[KMAX];
  const int tid = threadIdx.x, tl = tid >> 4, kq = tid & 15;
  const int w = tid >> 6, n = tid & 15, kk = (tid >> 4) & 3;       // MFMA form
  const int K = P.K, F = P.F;
  const int64_t t0 = (int64_t)blockIdx.x * TT;
  for (int64_t b = blockIdx.y; b < P.B; b += gridDim.y) {
    const float* Vb = P.V + b * P.T * F;
    float* Ab = P.A + b * P.T * K;
    const float* Cb = P.C + b * P.cstride;
    const float* Wb = P.work + b * P.wstride;
    for (int idx = tid; idx < TT * KMAX; idx += NT) {
      const int t = idx / KMAX, k = idx - t * KMAX;
      As[t][k] = (k < K && t0 + t < P.T) ? Ab[(t0 + t) * K + k] : 0.f;
    }
    if (KL) {
      if (tid < KMAX) Ds[tid] = tid < K ? Wb[K * K + tid] : 0.f;
    } else {
      for (int idx = tid; idx < KMAX * KMAX; idx += NT) {
        const int i = idx / KMAX, j = idx - i * KMAX;
        Gs[i][j] = (i < K && j < K) ? Wb[i * K + j] : 0.f;
      }
    }
    float acc[KJ];
#pragma unroll
    for (int j = 0; j < KJ; ++j) acc[j] = 0.f;
    v4f macc = {0.f, 0.f, 0.f, 0.f};
    for (int f0 = 0; f0 < F; f0 += FC) {
      __syncthreads();                                  // the tables above; the previous chunk's readers
      for (int idx = tid; idx < KJ * 16 * FC; idx += NT) {
        const int k = idx / FC, fl = idx - k * FC;
        Cs[k][fl] = (k < K && f0 + fl < F) ? Cb[(int64_t)k * F + f0 + fl] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < TT * FC / NT; ++q) {
        const int idx = tid + q * NT, t = idx / FC, fl = idx - t * FC;
        Xs[t][fl] = (t0 + t < P.T && f0 + fl < F) ? Vb[(t0 + t) * F + f0 + fl] : 0.f;
      }
      __syncthreads();
      if (KL) {
#pragma unroll
        for (int q = 0; q < TT * FC / NT; ++q) {         // the entries this thread loaded: no one else touches them yet
          const int idx = tid + q * NT, t = idx / FC, fl = idx - t * FC;
          float wh = 0.f;
          for (int k = 0; k < K; ++k) wh = fmaf(As[t][k], Cs[k][fl], wh);
          Xs[t][fl] = Xs[t][fl] / fmaxf(wh, EPS);
        }
        __syncthreads();
      }
      if (MF) {
        if (w < KJ) {                                    // uniform in a wave
          v4f p0 = {0.f, 0.f, 0.f, 0.f}, p1 = {0.f, 0.f, 0.f, 0.f};
          const float* xr = &Xs[n][16 * kk];
          const float* cr = &Cs[16 * w + n][16 * kk];
#pragma unroll
          for (int j = 0; j < 16; j += 2) {
            p0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xr[j], cr[j], p0, 0, 0, 0);
            p1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xr[j + 1], cr[j + 1], p1, 0, 0, 0);
          }
          macc += p0 + p1;
        }
      } else {
        float part[KJ];
#pragma unroll
        for (int j = 0; j < KJ; ++j) part[j] = 0.f;
#pragma unroll 8
        for (int fl = 0; fl < FC; ++fl) {
          const float x = Xs[tl][fl];
#pragma unroll
          for (int j = 0; j < KJ; ++j) part[j] = fmaf(x, Cs[kq + 16 * j][fl], part[j]);
        }
#pragma unroll
        for (int j = 0; j < KJ; ++j) acc[j] += part[j];
      }
    }
#pragma unroll
    for (int j = 0; j < (MF ? 4 : KJ); ++j) {
      const int tr = MF ? 4 * kk + j : tl;                // the output's frame in the tile, its component, its numerator
      const int k = MF ? 16 * w + n : kq + 16 * j;
      const float num = MF ? macc[j] : acc[MF ? 0 : j];
      const int64_t t = t0 + tr;
      if ((!MF || w < KJ) && k < K && t < P.T) {
        float d;
        if (KL) {
          d = Ds[k];
        } else {
          d = 0.f;
          for (int i = 0; i < K; ++i) d = fmaf(As[tr][i], Gs[i][k], d);
        }
        if (d == 0.f) d = EPS;
        Ab[t * K + k] = As[tr][k] * (num / d);
      }
    }
    __syncthreads();                                    // As, Gs, Ds are rewritten for the next clip
  }
}

// ------------------------------------------------------------------ C-step
// A workgroup owns FT bins of a clip.  FMA form: thread (wave kg, lane fl) owns the outputs (kg + 4 j, fl), j < KJ.
// MFMA form (MF): wave w owns bins 16 w .. 16 w + 15 and KJ tiles of 16 components; lane (n, kk) supplies frame 4 j + kk
// at step j (rows of 80 floats put the four kk on four groups of 16 banks) and holds the outputs (component
// 16 kt + 4 kk + i, bin 16 w + n).
constexpr int CS = 80;                   // row stride of the C-step's frame-major LDS tiles
template <bool KL, int KJ, bool MF>
__global__ __launch_bounds__(NT) void c_step_kernel(NmfArgs P) {
  __shared__ float Cs[KMAX][FT];
  __shared__ float As[TC][CS];
  __shared__ float Xs[TC][CS];
  __shared__ float Hs[KL ? 1 : KMAX][KMAX];
  __shared__ float Ds[KMAX];
  const int tid = threadIdx.x, fl = tid & 63, kg = tid >> 6;
  const int n = tid & 15, kk = (tid >> 4) & 3;                     // MFMA form (its wave is kg)
  const int K = P.K, F = P.F;
  const int f0 = blockIdx.x * FT;
  for (int64_t b = blockIdx.y; b < P.B; b += gridDim.y) {
    const float* Vb = P.V + b * P.T * F;
    const float* Ab = P.A + b * P.T * K;
    float* Cb = P.C + b * P.cstride;
    const float* Wb = P.work + b * P.wstride;
    for (int idx = tid; idx < KMAX * FT; idx += NT) {
      const int k = idx / FT, f = idx - k * FT;
      Cs[k][f] = (k < K && f0 + f < F) ? Cb[(int64_t)k * F + f0 + f] : 0.f;
    }
    if (KL) {
      if (tid < KMAX) Ds[tid] = tid < K ? Wb[K * K + tid] : 0.f;
    } else {
      for (int idx = tid; idx < KMAX * KMAX; idx += NT) {
        const int i = idx / KMAX, j = idx - i * KMAX;
        Hs[i][j] = (i < K && j < K) ? Wb[i * K + j] : 0.f;
      }
    }
    float acc[MF ? 1 : KJ];
#pragma unroll
    for (int j = 0; j < (MF ? 1 : KJ); ++j) acc[j] = 0.f;
    v4f macc[MF ? KJ : 1];
#pragma unroll
    for (int j = 0; j < (MF ? KJ : 1); ++j) macc[j] = v4f{0.f, 0.f, 0.f, 0.f};
    for (int64_t t0 = 0; t0 < P.T; t0 += TC) {
      __syncthreads();
      for (int idx = tid; idx < TC * KMAX; idx += NT) {
        const int t = idx / KMAX, k = idx - t * KMAX;
        As[t][k] = (k < K && t0 + t < P.T) ? Ab[(t0 + t) * K + k] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < TC * FT / NT; ++q) {
        const int t = kg + 4 * q;
        Xs[t][fl] = (t0 + t < P.T && f0 + fl < F) ? Vb[(t0 + t) * F + f0 + fl] : 0.f;
      }
      __syncthreads();
      if (KL) {
#pragma unroll
        for (int q = 0; q < TC * FT / NT; ++q) {
          const int t = kg + 4 * q;
          float wh = 0.f;
          for (int k = 0; k < K; ++k) wh = fmaf(As[t][k], Cs[k][fl], wh);
          Xs[t][fl] = Xs[t][fl] / fmaxf(wh, EPS);
        }
        __syncthreads();
      }
      if (MF) {
        v4f part[KJ];
#pragma unroll
        for (int j = 0; j < KJ; ++j) part[j] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < TC / 4; ++j) {
          const float x = Xs[4 * j + kk][16 * kg + n];
#pragma unroll
          for (int kt = 0; kt < KJ; ++kt)
            part[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(As[4 * j + kk][16 * kt + n], x, part[kt], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < KJ; ++j) macc[j] += part[j];
      } else {
        float part[KJ];
#pragma unroll
        for (int j = 0; j < KJ; ++j) part[j] = 0.f;
#pragma unroll 4
        for (int t = 0; t < TC; ++t) {
          const float x = Xs[t][fl];
#pragma unroll
          for (int j = 0; j < KJ; ++j) part[j] = fmaf(As[t][kg + 4 * j], x, part[j]);
        }
#pragma unroll
        for (int j = 0; j < KJ; ++j) acc[MF ? 0 : j] += part[j];
      }
    }
#pragma unroll
    for (int j = 0; j < (MF ? 4 * KJ : KJ); ++j) {
      const int k = MF ? 16 * (j >> 2) + 4 * kk + (j & 3) : kg + 4 * j;      // the output's component, bin and numerator
      const int fo = MF ? 16 * kg + n : fl;
      const float num = MF ? macc[MF ? j >> 2 : 0][j & 3] : acc[MF ? 0 : j];
      const int f = f0 + fo;
      if (k < K && f < F) {
        float d;
        if (KL) {
          d = Ds[k];
        } else {
          d = 0.f;
          for (int i = 0; i < K; ++i) d = fmaf(Hs[k][i], Cs[i][fo], d);
        }
        if (d == 0.f) d = EPS;
        float c = Cs[k][fo] * (num / d);
        if (KL && c < C_FLUSH) c = 0.f;
        Cb[(int64_t)k * F + f] = c;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ divergence
// A clip is cut into nb = clamp(ceil(T F / 8192), 1, 256) workgroups -- a function of (T, F) alone -- that take frames
// j, j + nb, ...; AC is formed in float64 from the float32 factors.
inline int div_blocks(int64_t T, int64_t F) { return (int)std::min<int64_t>(256, std::max<int64_t>(1, ceil_div(T * F, 8192))); }

struct DivArgs {
  const float* V; const float* A; const float* C; double* part; double* out;
  int64_t B, T, cstride; int F, K, nb, kl;
};

__global__ __launch_bounds__(NT) void divergence_kernel(DivArgs P) {
  __shared__ double As[KMAX];
  __shared__ double red[NT / 64];
  const int tid = threadIdx.x;
  const int K = P.K, F = P.F;
  for (int64_t b = blockIdx.y; b < P.B; b += gridDim.y) {
    const float* Cb = P.C + b * P.cstride;
    double s = 0.0;
    for (int64_t t = blockIdx.x; t < P.T; t += P.nb) {
      __syncthreads();
      if (tid < K) As[tid] = (double)P.A[(b * P.T + t) * K + tid];
      __syncthreads();
      const float* Vt = P.V + (b * P.T + t) * F;
      for (int f = tid; f < F; f += NT) {
        double wh = 0.0;
        for (int k = 0; k < K; ++k) wh = fma(As[k], (double)Cb[(int64_t)k * F + f], wh);
        const float vf = Vt[f];
        const double v = (double)vf;
        if (P.kl) {
          s += wh;
          if (vf > EPS) s += v * log(v / fmax(wh, (double)EPS)) - v;
        } else {
          const double d = v - wh;
          s += 0.5 * d * d;
        }
      }
    }
    s = wave_sum_d(s);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) P.part[b * P.nb + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

__global__ __launch_bounds__(64) void divergence_sum_kernel(DivArgs P) {
  const int lane = threadIdx.x;
  for (int64_t b = blockIdx.x; b < P.B; b += gridDim.x) {
    double s = 0.0;
    for (int j = lane; j < P.nb; j += 64) s += P.part[b * P.nb + j];
    s = wave_sum_d(s);
    if (lane == 0) P.out[b] = s;
  }
}

// ------------------------------------------------------------------ masks
// out[b, g, t, f] = D[b, t, f] (sum_k G[g, k] A[t, k] C[k, f]) / max(sum_k A[t, k] C[k, f], eps): a workgroup takes MT
// frames by 256 bins; both sums are formed in float64, so that the groups of a partition add up to D to float32 rounding.
constexpr int MT = 8;

struct MaskArgs {
  const float2* D; const float* A; const float* C; const float* G; float2* out;
  int64_t B, T, cstride; int F, K, NG, nft;
};

__global__ __launch_bounds__(NT) void masks_kernel(MaskArgs P) {
  __shared__ float As[KMAX];
  __shared__ float GA[GMAX][KMAX];
  const int tid = threadIdx.x;
  const int K = P.K, F = P.F, NG = P.NG;
  const int ft = blockIdx.x % P.nft;
  const int64_t t0 = (int64_t)(blockIdx.x / P.nft) * MT;
  const int f = ft * NT + tid;
  for (int64_t b = blockIdx.y; b < P.B; b += gridDim.y) {
    const float* Cb = P.C + b * P.cstride;
    for (int64_t t = t0; t < t0 + MT && t < P.T; ++t) {
      __syncthreads();
      if (tid < K) As[tid] = P.A[(b * P.T + t) * K + tid];
      for (int idx = tid; idx < NG * K; idx += NT) {
        const int g = idx / K, k = idx - g * K;
        GA[g][k] = P.G[idx] * P.A[(b * P.T + t) * K + k];
      }
      __syncthreads();
      if (f < F) {
        double tot = 0.0;
        for (int k = 0; k < K; ++k) tot = fma((double)As[k], (double)Cb[(int64_t)k * F + f], tot);
        const double inv = 1.0 / fmax(tot, (double)EPS);
        const float2 d = P.D[(b * P.T + t) * F + f];
        for (int g = 0; g < NG; ++g) {
          double num = 0.0;
          for (int k = 0; k < K; ++k) num = fma((double)GA[g][k], (double)Cb[(int64_t)k * F + f], num);
          const float m = (float)(num * inv);
          P.out[(((b * NG + g) * P.T) + t) * F + f] = make_float2(d.x * m, d.y * m);
        }
      }
    }
  }
}

inline bool shape_ok(int64_t B, int64_t T, int64_t F, int64_t K) {
  return B >= 1 && T >= 1 && F >= 1 && F <= FMAX && K >= 1 && K <= KMAX && T <= ((int64_t)1 << 30) &&
         B <= ((int64_t)1 << 40) / (T * F);
}

inline int64_t step_work_floats(int64_t K) { return K * K + K; }

// The form of the contractions: SYG_NMF_FORM_FMA, SYG_NMF_FORM_MFMA, or the measured choice: the MFMA form was the faster
// one at every K that was timed (8, 16, 32, 64: by 7 to 26 %); below 8 nothing was timed and the
// FMA form stays.
constexpr int MFMA_MIN_K = 8;
inline bool use_mfma(int form, int64_t K) { return form == SYG_NMF_FORM_MFMA || (form == SYG_NMF_FORM_AUTO && K >= MFMA_MIN_K); }

template <bool KL, bool MF>
void launch_a_step(const NmfArgs& P, dim3 grid, hipStream_t s) {
  if (P.K <= 16) hipLaunchKernelGGL((a_step_kernel<KL, 1, MF>), grid, dim3(NT), 0, s, P);
  else if (P.K <= 32) hipLaunchKernelGGL((a_step_kernel<KL, 2, MF>), grid, dim3(NT), 0, s, P);
  else hipLaunchKernelGGL((a_step_kernel<KL, 4, MF>), grid, dim3(NT), 0, s, P);
}

template <bool KL>
void launch_c_step(const NmfArgs& P, dim3 grid, hipStream_t s, bool mf) {
  if (mf) {
    if (P.K <= 16) hipLaunchKernelGGL((c_step_kernel<KL, 1, true>), grid, dim3(NT), 0, s, P);
    else if (P.K <= 32) hipLaunchKernelGGL((c_step_kernel<KL, 2, true>), grid, dim3(NT), 0, s, P);
    else hipLaunchKernelGGL((c_step_kernel<KL, 4, true>), grid, dim3(NT), 0, s, P);
  } else if (P.K <= 4) hipLaunchKernelGGL((c_step_kernel<KL, 1, false>), grid, dim3(NT), 0, s, P);
  else if (P.K <= 8) hipLaunchKernelGGL((c_step_kernel<KL, 2, false>), grid, dim3(NT), 0, s, P);
  else if (P.K <= 16) hipLaunchKernelGGL((c_step_kernel<KL, 4, false>), grid, dim3(NT), 0, s, P);
  else if (P.K <= 32) hipLaunchKernelGGL((c_step_kernel<KL, 8, false>), grid, dim3(NT), 0, s, P);
  else hipLaunchKernelGGL((c_step_kernel<KL, 16, false>), grid, dim3(NT), 0, s, P);
}

template <bool OF_A>
void launch_sums(const NmfArgs& P, bool kl, hipStream_t s) {
  const dim3 grid(grid_rows(P.B));
  if (kl) hipLaunchKernelGGL((factor_sums_kernel<OF_A, true>), grid, dim3(NT), 0, s, P);
  else hipLaunchKernelGGL((factor_sums_kernel<OF_A, false>), grid, dim3(NT), 0, s, P);
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int syg_nmf_constants(int which) {
  switch (which) {
    case 0: return KMAX;
    case 1: return FMAX;
    case 2: return GMAX;
    case 3: return TT;
    case 4: return FC;
    case 5: return FT;
    case 6: return TC;
    case 7: return SC;
    case 8: return MFMA_MIN_K;
    default: return -1;
  }
}

extern "C" int64_t syg_nmf_work_bytes(int64_t B, int64_t T, int64_t F, int64_t K) {
  if (!shape_ok(B, T, F, K)) {
    set_error("nmf_work_bytes: served are B >= 1, T >= 1, F in [1, %d], K in [1, %d] (got B=%lld, T=%lld, F=%lld, K=%lld)", FMAX,
              KMAX, (long long)B, (long long)T, (long long)F, (long long)K);
    return -1;
  }
  const int64_t step = B * step_work_floats(K) * (int64_t)sizeof(float);
  const int64_t div = B * div_blocks(T, F) * (int64_t)sizeof(double);
  return (std::max(step, div) + 7) / 8 * 8;
}

extern "C" int syg_nmf_f32(const float* V, int64_t B, int64_t T, int64_t F, int64_t K, float* A, float* C, int c_shared,
                           int64_t n_iter, int loss, int update_A, int update_C, int form, void* work, void* stream) {
  SYG_REQUIRE(V && A && C && work, "nmf: null pointer argument (V / A / C / work)");
  SYG_REQUIRE(shape_ok(B, T, F, K),
              "nmf: served are B >= 1, T >= 1, F in [1, %d], K in [1, %d] (got B=%lld, T=%lld, F=%lld, K=%lld)", FMAX, KMAX,
              (long long)B, (long long)T, (long long)F, (long long)K);
  SYG_REQUIRE(loss == SYG_NMF_FROBENIUS || loss == SYG_NMF_KL,
              "nmf: loss must be SYG_NMF_FROBENIUS (0) or SYG_NMF_KL (1); Itakura-Saito and other beta are not served (got %d)", loss);
  SYG_REQUIRE(n_iter >= 0 && n_iter <= ((int64_t)1 << 31), "nmf: n_iter must be in [0, 2^31] (got %lld)", (long long)n_iter);
  SYG_REQUIRE((update_A == 0 || update_A == 1) && (update_C == 0 || update_C == 1) && (c_shared == 0 || c_shared == 1),
              "nmf: update_A, update_C and c_shared are 0 or 1");
  SYG_REQUIRE(form >= SYG_NMF_FORM_AUTO && form <= SYG_NMF_FORM_MFMA,
              "nmf: form must be SYG_NMF_FORM_AUTO (-1), SYG_NMF_FORM_FMA (0) or SYG_NMF_FORM_MFMA (1) (got %d)", form);
  const bool mf = use_mfma(form, K);
  SYG_REQUIRE(!(c_shared && update_C), "nmf: a shared dictionary C [1, K, F] cannot be updated (update_C with c_shared)");
  hipStream_t s = (hipStream_t)stream;
  const bool kl = loss == SYG_NMF_KL;
  NmfArgs P{V, A, C, (float*)work, B, T, c_shared ? 0 : K * F, (int)F, (int)K, (int)step_work_floats(K)};
  const dim3 ga((unsigned)ceil_div(T, TT), grid_rows(B)), gc((unsigned)ceil_div(F, FT), grid_rows(B));
  if (n_iter == 0 || (!update_A && !update_C)) return SYG_OK;
  if (update_A && !update_C) {
    launch_sums<false>(P, kl, s);
    SYG_CHECK_LAUNCH("nmf (sums of C)");
  }
  for (int64_t it = 0; it < n_iter; ++it) {
    if (update_A) {
      if (update_C) {
        launch_sums<false>(P, kl, s);
        SYG_CHECK_LAUNCH("nmf (sums of C)");
      }
      if (kl) { if (mf) launch_a_step<true, true>(P, ga, s); else launch_a_step<true, false>(P, ga, s); }
      else { if (mf) launch_a_step<false, true>(P, ga, s); else launch_a_step<false, false>(P, ga, s); }
      SYG_CHECK_LAUNCH("nmf (A-step)");
    }
    if (update_C) {
      if (update_A || it == 0) {
        launch_sums<true>(P, kl, s);
        SYG_CHECK_LAUNCH("nmf (sums of A)");
      }
      if (kl) launch_c_step<true>(P, gc, s, mf); else launch_c_step<false>(P, gc, s, mf);
      SYG_CHECK_LAUNCH("nmf (C-step)");
    }
  }
  return SYG_OK;
}

extern "C" int syg_nmf_divergence_f32(const float* V, const float* A, const float* C, int c_shared, int64_t B, int64_t T,
                                      int64_t F, int64_t K, int loss, double* out, void* work, void* stream) {
  SYG_REQUIRE(V && A && C && out && work, "nmf_divergence: null pointer argument (V / A / C / out / work)");
  SYG_REQUIRE(shape_ok(B, T, F, K),
              "nmf_divergence: served are B >= 1, T >= 1, F in [1, %d], K in [1, %d] (got B=%lld, T=%lld, F=%lld, K=%lld)", FMAX,
              KMAX, (long long)B, (long long)T, (long long)F, (long long)K);
  SYG_REQUIRE(loss == SYG_NMF_FROBENIUS || loss == SYG_NMF_KL,
              "nmf_divergence: loss must be SYG_NMF_FROBENIUS (0) or SYG_NMF_KL (1) (got %d)", loss);
  SYG_REQUIRE(c_shared == 0 || c_shared == 1, "nmf_divergence: c_shared is 0 or 1");
  const int nb = div_blocks(T, F);
  DivArgs P{V, A, C, (double*)work, out, B, T, c_shared ? 0 : K * F, (int)F, (int)K, nb, loss == SYG_NMF_KL};
  hipLaunchKernelGGL(divergence_kernel, dim3((unsigned)nb, grid_rows(B)), dim3(NT), 0, (hipStream_t)stream, P);
  SYG_CHECK_LAUNCH("nmf_divergence");
  hipLaunchKernelGGL(divergence_sum_kernel, dim3(grid_rows(B)), dim3(64), 0, (hipStream_t)stream, P);
  SYG_CHECK_LAUNCH("nmf_divergence (sum)");
  return SYG_OK;
}

extern "C" int syg_nmf_masks_f32(const float* D, const float* A, const float* C, int c_shared, const float* G, int64_t B,
                                 int64_t T, int64_t F, int64_t K, int64_t n_groups, float* out, void* stream) {
  SYG_REQUIRE(D && A && C && G && out, "nmf_masks: null pointer argument (D / A / C / G / out)");
  SYG_REQUIRE(shape_ok(B, T, F, K),
              "nmf_masks: served are B >= 1, T >= 1, F in [1, %d], K in [1, %d] (got B=%lld, T=%lld, F=%lld, K=%lld)", FMAX, KMAX,
              (long long)B, (long long)T, (long long)F, (long long)K);
  SYG_REQUIRE(n_groups >= 1 && n_groups <= GMAX, "nmf_masks: n_groups must be in [1, %d] (got %lld)", GMAX, (long long)n_groups);
  SYG_REQUIRE(c_shared == 0 || c_shared == 1, "nmf_masks: c_shared is 0 or 1");
  SYG_REQUIRE(B * n_groups <= ((int64_t)1 << 40) / (T * F), "nmf_masks: the output is too large");
  const int nft = (int)ceil_div(F, NT);
  MaskArgs P{(const float2*)D, A, C, G, (float2*)out, B, T, c_shared ? 0 : K * F, (int)F, (int)K, (int)n_groups, nft};
  hipLaunchKernelGGL(masks_kernel, dim3((unsigned)(ceil_div(T, MT) * nft), grid_rows(B)), dim3(NT), 0, (hipStream_t)stream, P);
  SYG_CHECK_LAUNCH("nmf_masks");
  return SYG_OK;
}
