// Features back to audio: Griffin-Lim's projection step and the dense inversions of the mel and MFCC maps
// (librosa 0.10 `griffinlim`, `feature.inverse.mfcc_to_mel`; `mel_to_stft` as torchaudio's InverseMelScale defines it).
// The float64 restatement that is the contract lives in tests/inverse_ref.py.  The loop's other two thirds are
// syg_stft2048_c2c_f32 and syg_istft2048_f32 (hpss.hip).  A second load mode of the inverse STFT that projected in
// registers, so that D was never written, measured 1.22 ms against 0.33 + 0.38 ms for the two launches at 1024 clips of
// 65 frames and was deleted ("Feature inversion").
//
// Projection (gl_project_kernel): D = S A / (|A| + tiny), A = R - alpha P, tiny = FLT_MIN (util.tiny of complex64), one
// bin per thread and trip, R / P / S read once, D written once: memory-bound (28 B per bin).  The modulus neither
// underflows nor overflows: A is scaled by the power of two that brings its larger component into [1/2, 1)
// (v_frexp_exp / v_ldexp: exact, denormals included), so the sum of squares lies in [1/4, 2) -- a smaller component whose
// square vanishes is below the rounding of that sum -- and tiny takes the same scale: 2^23 at most (A the smallest
// denormal), 0 once A is above 2^24 tiny, where the sum would round it away anyway.  |D| <= S (1 + 5 * 2^-24) whatever
// the exponent of A (five roundings: sum, root, quotient, two products).  A form that took two bins a thread through
// 16-byte loads measured slower (0.43 against 0.38 ms at 1024 clips of 65 frames) and was not kept.
// A clip is cut into nb = clamp(ceil(T 1025 / 2048), 1, 1024) workgroups -- a function of T alone, so a clip's figures
// do not depend on the batch it sits in.  With `sums` each adds (|R| - S)^2 and S^2 in float64 (the modulus as a float64
// root of the exact sum of squares), lanes strided, then wave_sum_d and the four waves in order, and writes one pair;
// gl_sums_kernel adds a clip's pairs, lanes strided, with one wave.  No atomics: a call repeats its bits.
//
// Dense inversion (inv_dense_kernel): out[b, t, f] = post(sum_m W[f, m] pre(X[b, m, t])) as an LDS-tiled fp32 FMA
// kernel, 32 frames x 64 outputs per workgroup, m in steps of 32 ascending.  pre = db_to_power is ref 2^(x log2(10) / 10)
// with the exponent formed in float64 and split into integer and fraction, so that +200 dB keeps float32's relative
// precision (a float32 exponent of 66 would carry 3e-6 into the power).
#include <float.h>
#include <math.h>
#include <algorithm>
#include "host.h"

namespace syg {
namespace {

constexpr int NB = 1025;

// has_p: P takes part (the first projection of a run has no previous spectrum).  Compiled under contract(off): every
// step is one rounded float32 operation in the order written.
__device__ __forceinline__ float2 gl_project(float2 r, float2 p, bool has_p, float alpha, float s) {
#pragma clang fp contract(off)
  // A: one rounding of the exact r - alpha p
  const float ax = has_p ? __fmaf_rn(-alpha, p.x, r.x) : r.x;
  const float ay = has_p ? __fmaf_rn(-alpha, p.y, r.y) : r.y;
  const float big = fmaxf(fabsf(ax), fabsf(ay));
  if (!(big > 0.f)) return make_float2(0.f, 0.f);               // A = 0: D = S 0 / tiny
  const int e = __builtin_amdgcn_frexp_expf(big);               // big = m 2^e, m in [1/2, 1)
  const float x = ldexpf(ax, -e), y = ldexpf(ay, -e);
  const float t = ldexpf(FLT_MIN, -e);
  const float xx = x * x, yy = y * y;
  const float den = sqrtf(xx + yy) + t;                         // (|A| + tiny) 2^-e
  const float inv = 1.f / den;
  const float qx = x * inv, qy = y * inv;
  return make_float2(s * qx, s * qy);
}

constexpr int PT = 256;                     // threads of a projection workgroup
constexpr int64_t PBINS = 2048;              // bins per workgroup that decide nb
constexpr int PMAXB = 1024;

inline int proj_blocks(int64_t T) { return (int)std::min<int64_t>(PMAXB, std::max<int64_t>(1, ceil_div(T * NB, PBINS))); }

struct ProjArgs {
  const float2* R; const float2* P; const float* S; int64_t n; int nb; float alpha; float2* D; double* part;
};

template <bool SUMS>
__global__ __launch_bounds__(PT) void gl_project_kernel(ProjArgs A) {
  __shared__ double red[2][PT / 64];
  const int64_t b = blockIdx.x / A.nb;
  const int j = (int)(blockIdx.x - b * A.nb);
  const int64_t base = b * A.n;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t i = (int64_t)j * PT + threadIdx.x; i < A.n; i += (int64_t)A.nb * PT) {
    const float2 r = A.R[base + i];
    const float s = A.S[base + i];
    const float2 p = A.P ? A.P[base + i] : make_float2(0.f, 0.f);
    A.D[base + i] = gl_project(r, p, A.P != nullptr, A.alpha, s);
    if (SUMS) {
      const double x = r.x, y = r.y;
      const double d = sqrt(x * x + y * y) - (double)s;      // exact squares, one rounding in the sum, one in the root
      s1 += d * d;
      s2 += (double)s * (double)s;
    }
  }
  if (SUMS) {
    s1 = wave_sum_d(s1);
    s2 = wave_sum_d(s2);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][w] = s1; red[1][w] = s2; }
    __syncthreads();
    if (threadIdx.x < 2) {
      const double* q = red[threadIdx.x];
      A.part[((int64_t)blockIdx.x) * 2 + threadIdx.x] = (q[0] + q[1]) + (q[2] + q[3]);
    }
  }
}

__global__ __launch_bounds__(64) void gl_sums_kernel(const double* part, int nb, double* sums) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  double s1 = 0.0, s2 = 0.0;
  for (int j = lane; j < nb; j += 64) {
    s1 += part[(b * nb + j) * 2];
    s2 += part[(b * nb + j) * 2 + 1];
  }
  s1 = wave_sum_d(s1);
  s2 = wave_sum_d(s2);
  if (lane == 0) { sums[b * 2] = s1; sums[b * 2 + 1] = s2; }
}

// ------------------------------------------------------------------ dense inversions
constexpr int DT = 32, DF = 64, DM = 32, DTHREADS = 256;
constexpr int TPT = DT / (DTHREADS / DF);     // frames per thread: 8

struct DenseArgs {
  const float* X; const float* W; float* out; int64_t T, ntt; int M, F, nft, pre, post, mel_major; float pre_ref, post_arg, inv_power;
};

// ref 10^(x / 10); -inf dB is power 0
__device__ __forceinline__ float db_to_power(float x, float ref) {
  if (x == -INFINITY) return 0.f;
  const double a = (double)x * 0.33219280948873623479;        // log2(10) / 10
  const double n = rint(a);
  const float f = (float)(a - n);                               // |f| <= 1/2, exact to float32's precision
  const float nn = (float)fmin(fmax(n, -300.0), 300.0);
  return ref * ldexpf(exp2f(f), (int)nn);
}

__global__ __launch_bounds__(DTHREADS) void inv_dense_kernel(DenseArgs A) {
  __shared__ __attribute__((aligned(16))) float Xs[DM][DT];
  __shared__ float Ws[DF][DM + 1];             // + 1: the 64 lanes read 64 rows at one m
  const int tid = threadIdx.x, tx = tid & (DF - 1), ty = tid >> 6;
  const int64_t blk = blockIdx.x;
  const int ft = (int)(blk % A.nft);
  const int64_t rest = blk / A.nft;
  const int64_t tt = rest % A.ntt, b = rest / A.ntt;
  const int64_t t0 = tt * DT;
  const int f0 = ft * DF;
  const float* Xb = A.X + b * A.M * A.T;
  float acc[TPT];
#pragma unroll
  for (int j = 0; j < TPT; ++j) acc[j] = 0.f;
  for (int m0 = 0; m0 < A.M; m0 += DM) {
#pragma unroll
    for (int q = 0; q < DM * DT / DTHREADS; ++q) {
      const int idx = tid + q * DTHREADS, mm = idx / DT, tl = idx - mm * DT;
      const int m = m0 + mm;
      const int64_t t = t0 + tl;
      float v = 0.f;
      if (m < A.M && t < A.T) {
        v = Xb[(int64_t)m * A.T + t];
        if (A.pre) v = db_to_power(v, A.pre_ref);
      }
      Xs[mm][tl] = v;
    }
#pragma unroll
    for (int q = 0; q < DF * DM / DTHREADS; ++q) {
      const int idx = tid + q * DTHREADS, fl = idx / DM, mm = idx - fl * DM;
      const int f = f0 + fl, m = m0 + mm;
      Ws[fl][mm] = (f < A.F && m < A.M) ? A.W[(int64_t)f * A.M + m] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int mm = 0; mm < DM; ++mm) {
      const float w = Ws[tx][mm];
      const float4 xa = *reinterpret_cast<const float4*>(&Xs[mm][ty * TPT]);
      const float4 xb = *reinterpret_cast<const float4*>(&Xs[mm][ty * TPT + 4]);
      acc[0] = fmaf(w, xa.x, acc[0]); acc[1] = fmaf(w, xa.y, acc[1]);
      acc[2] = fmaf(w, xa.z, acc[2]); acc[3] = fmaf(w, xa.w, acc[3]);
      acc[4] = fmaf(w, xb.x, acc[4]); acc[5] = fmaf(w, xb.y, acc[5]);
      acc[6] = fmaf(w, xb.z, acc[6]); acc[7] = fmaf(w, xb.w, acc[7]);
    }
    __syncthreads();
  }
  const int f = f0 + tx;
  if (f >= A.F) return;
#pragma unroll
  for (int j = 0; j < TPT; ++j) {
    const int64_t t = t0 + ty * TPT + j;
    if (t >= A.T) break;
    float v = acc[j];
    if (A.post == 1) {
      v = fmaxf(v, 0.f);
      if (A.post_arg == 2.f) v = sqrtf(v);
      else if (A.post_arg != 1.f) v = powf(v, A.inv_power);
    } else if (A.post == 2) {
      v = db_to_power(v, A.post_arg);
    }
    // (mel-major: a lane's neighbour is T floats away; the rows this form writes are an eighth of a spectrum)
    A.out[A.mel_major ? (b * A.F + f) * A.T + t : (b * A.T + t) * A.F + f] = v;
  }
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_gl_project_work_bytes(int64_t B, int64_t T) {
  if (B < 1 || T < 1 || B * T >= ((int64_t)1 << 40) / NB) {
    set_error("gl_project_work_bytes: bad B / T");
    return -1;
  }
  return B * proj_blocks(T) * 2 * (int64_t)sizeof(double);
}

extern "C" int syg_gl_project_f32(const float* R, const float* P, const float* S, int64_t B, int64_t T, float alpha, float* D,
                                  double* sums, void* work, void* stream) {
  SYG_REQUIRE(R && S && D, "gl_project: null pointer argument (R / S / D)");
  SYG_REQUIRE(!sums || work, "gl_project: sums needs the workspace of syg_gl_project_work_bytes");
  SYG_REQUIRE(B >= 1 && T >= 1 && B * T < ((int64_t)1 << 40) / NB, "gl_project: bad B / T");
  SYG_REQUIRE(alpha >= 0.f && alpha < 0.5f, "gl_project: alpha = momentum / (1 + momentum) must be in [0, 0.5) (got %g)",
              (double)alpha);
  const int nb = proj_blocks(T);
  SYG_REQUIRE(B * nb < 0x7fffffff, "gl_project: too many workgroups");
  ProjArgs A{(const float2*)R, (const float2*)P, S, T * NB, nb, alpha, (float2*)D, (double*)work};
  if (sums) {
    hipLaunchKernelGGL(gl_project_kernel<true>, dim3((unsigned)(B * nb)), dim3(PT), 0, (hipStream_t)stream, A);
    SYG_CHECK_LAUNCH("gl_project");
    hipLaunchKernelGGL(gl_sums_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, (const double*)work, nb, sums);
    SYG_CHECK_LAUNCH("gl_project (sums)");
  } else {
    hipLaunchKernelGGL(gl_project_kernel<false>, dim3((unsigned)(B * nb)), dim3(PT), 0, (hipStream_t)stream, A);
    SYG_CHECK_LAUNCH("gl_project");
  }
  return SYG_OK;
}

extern "C" int syg_inv_dense_f32(const float* X, int64_t B, int64_t M, int64_t T, const float* W, int64_t F, int pre,
                                 float pre_ref, int post, float post_arg, float* out, int out_mel_major, void* stream) {
  SYG_REQUIRE(X && W && out, "inv_dense: null pointer argument (X / W / out)");
  SYG_REQUIRE(B >= 1 && T >= 1 && M >= 1 && M <= 4096 && F >= 1 && F <= 65536, "inv_dense: bad B / M / T / F");
  SYG_REQUIRE((pre == 0 || pre == 1) && post >= 0 && post <= 2 && (out_mel_major == 0 || out_mel_major == 1),
              "inv_dense: pre is 0 or 1, post 0, 1 or 2, out_mel_major 0 or 1");
  SYG_REQUIRE(!pre || (pre_ref > 0.f && isfinite(pre_ref)), "inv_dense: pre_ref must be positive and finite");
  SYG_REQUIRE(!post || (post_arg > 0.f && isfinite(post_arg)), "inv_dense: post_arg (power / ref) must be positive and finite");
  const int64_t ntt = ceil_div(T, DT);
  const int nft = (int)ceil_div(F, DF);
  SYG_REQUIRE(B * ntt < 0x7fffffff / nft && B * T < ((int64_t)1 << 40) / std::max(F, M), "inv_dense: too many tiles");
  DenseArgs A{X, W, out, T, ntt, (int)M, (int)F, nft, pre, post, out_mel_major, pre_ref, post_arg, post == 1 ? 1.f / post_arg : 1.f};
  hipLaunchKernelGGL(inv_dense_kernel, dim3((unsigned)(B * ntt * nft)), dim3(DTHREADS), 0, (hipStream_t)stream, A);
  SYG_CHECK_LAUNCH("inv_dense");
  return SYG_OK;
}
