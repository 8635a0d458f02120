// Onset detection after the mel front end: librosa 0.10 `onset.onset_strength` (spectral flux of the log-mel matrix),
// `util.peak_pick` and `onset.onset_detect` as reached from sygnals/core/audio/features.py:555 (detect_onsets), and the
// two clip totals of get_basic_audio_metrics (:508).  The float64 restatement that is the contract lives in
// tests/onset_ref.py.
//
// Strength (onset_flux_kernel): a workgroup owns one clip, or a slice of 256 output frames of a long clip.  It takes the
// clip's largest mel power (its own pass over the clip, or the partial maxima of onset_max_kernel), which fixes the
// top_db floor, then forms d[t] = mean_m max(0, S[m, t + lag] - ref[m, t]) with the clip applied to the powers as they
// are loaded and each rise taken as 10 log10 of the ratio of the two clipped powers: the dB matrix never exists in
// memory, and no two rounded dB values are subtracted.  power_to_db is monotone, so the running maximum
// of the "superflux" reference (max_size > 1) is taken on the powers and converted once; scipy's reflected edges only
// repeat values the clipped window already holds.  A lane owns a frame (loads run along T, coalesced); the four waves
// own a quarter of the mel rows each, summed in row order, and the four partial sums are combined in a fixed order:
// the envelope is bit-identical from run to run.  The clip is not staged in LDS: the second pass re-reads what the
// first pulled into L2 (a 1 s clip is 48 KB).
//
// Detrend (onset_detrend_kernel): lfilter([1, -1], [1, -0.99]) over the padded envelope, one wave per clip, 64 frames
// a step: a Hillis-Steele scan of y[n] = d[n] + 0.99 y[n - 1] in float64, the carry handed from step to step.
//
// Peaks (onset_peaks_kernel): a workgroup owns a clip; a clip of more than 4096 frames has its flags made by one
// workgroup per 4096 frames (each redoes the clip's min / max out of L2) and is picked by a second launch.  Min / max / finiteness reduction; one thread per frame for the
// candidate flags (the window maximum and the non-zero test compare the raw float32 values, which the normalisation
// orders identically, so both are exact; the window mean is a direct float64 sum over the window; a tile of frames and
// its window halo are staged in LDS, since a wave would otherwise wait out one load after another); the flags go to
// the `frames` row itself.  The flags become ballot words in LDS; wave 0 walks the non-empty words (find-first-set, bits up
// to last + wait cleared at once) and compacts the accepted frames in place: an output slot is never ahead of the
// flags still to be read.  Backtracking moves each onset to the nearest local minimum of the energy at or before it.  No atomics.
//
// Clip metrics (clip_metrics_kernel): sum of squares (float64 per thread, fixed-order tree) and peak |y| of a clip.
#include <float.h>
#include <math.h>
#include "host.h"

namespace syg {
namespace {

constexpr int FT = 256;                 // flux kernel threads: four waves
constexpr int FCH = 64;                 // frames per step: one per lane
constexpr int FSL = 256;                // output frames per workgroup of the sliced form
constexpr int MSL = 1024;               // frames per workgroup of the partial-maximum launch
constexpr int64_t T_ONE = 2048;         // clips up to this many frames: one workgroup, its own maximum

struct FluxArgs {
  const float* mel; int64_t B; int M; int64_t T; float amin, top_db; int lag, max_size, pad; int64_t T_out;
  float* env; float* work; int64_t nsl, nmax;
};

__device__ __forceinline__ float block_max4(float v, float* red, int tid) {
  v = wave_max(v);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  const float m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return m;
}

// largest mel power of frames [s MSL, (s + 1) MSL) of clip b -> work[b nmax + s]
__global__ __launch_bounds__(FT) void onset_max_kernel(FluxArgs A) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / A.nmax, s = blockIdx.x % A.nmax;
  const int64_t t0 = s * MSL, t1 = min(t0 + MSL, A.T);
  const float* P = A.mel + b * A.M * A.T;
  float mx = 0.f;
  for (int m = 0; m < A.M; ++m)
    for (int64_t t = t0 + tid; t < t1; t += FT) mx = fmaxf(mx, P[m * A.T + t]);
  mx = block_max4(mx, red, tid);
  if (tid == 0) A.work[b * A.nmax + s] = mx;
}

template <bool OWN_MAX>
__global__ __launch_bounds__(FT) void onset_flux_kernel(FluxArgs A) {
  __shared__ float red[4];
  __shared__ float part[4][FCH];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t b = blockIdx.x / A.nsl, s = blockIdx.x % A.nsl;
  const int M = A.M;
  const int64_t T = A.T;
  const float* P = A.mel + b * M * T;
  float mx = 0.f;
  if (OWN_MAX) {
    const int64_t n = (int64_t)M * T;
    for (int64_t i = tid; i < n; i += FT) mx = fmaxf(mx, P[i]);
  } else {
    for (int64_t i = tid; i < A.nmax; i += FT) mx = fmaxf(mx, A.work[b * A.nmax + i]);
  }
  mx = block_max4(mx, red, tid);
  const float amin = A.amin;
  // The top_db floor as a POWER, max(amin, mx) 10^(-top_db / 10), held as fhi (1 + flo_rel ln 2) (float64, once a
  // thread): the clip to it is the dB clip, power_to_db being monotone.  A rise S[a] - S[b] is then 10 log10 of one
  // ratio, not the difference of two rounded dB values of some tens: r = a / b, its residual by one fma, log2 of the two
  // together.  Its error is relative to the rise itself, and the envelope sums rises that are all >= 0, so the error of
  // a frame is relative to that frame however small it is next to the dB values.
  const double fd = (A.top_db >= 0.f) ? (double)fmaxf(amin, mx) * exp2(-(double)A.top_db / (double)SYG_DB_PER_LOG2) : 0.0;
  const float fhi = (float)fd;
  const float flo_rel = fhi > 0.f ? (float)((fd - (double)fhi) / (double)fhi * 1.4426950408889634) : 0.f;
  auto rise = [&](float xa, float xb) {
    xa = fmaxf(amin, xa); xb = fmaxf(amin, xb);
    // floored: at or below the exact floor (fhi itself is below it only when the remainder is positive)
    const bool fa = xa < fhi || (xa == fhi && flo_rel > 0.f), fb = xb < fhi || (xb == fhi && flo_rel > 0.f);
    const float a = fa ? fhi : xa, b = fb ? fhi : xb;
    const float r = a * __builtin_amdgcn_rcpf(b);
    if (!(r > 0x1p-40f && r < 0x1p40f))          // ratio or reciprocal out of range (an amin far below 1e-30)
      return fmaxf(0.f, SYG_DB_PER_LOG2 * (syg_log2(a) - syg_log2(b)));
    const float e = fmaf(-r, b, a);              // a - r b exactly: a / b = r (1 + e / a)
    float l = syg_log2(r) + 1.44269504f * (e * __builtin_amdgcn_rcpf(a));
    l += fa ? flo_rel : 0.f;
    l -= fb ? flo_rel : 0.f;
    return fmaxf(0.f, SYG_DB_PER_LOG2 * l);
  };
  const int m0 = (w * M) / 4, m1 = ((w + 1) * M) / 4;
  const int k = A.max_size, h = k / 2, lag = A.lag;
  const int64_t j0 = OWN_MAX ? 0 : s * FSL, j1 = OWN_MAX ? A.T_out : min(j0 + FSL, A.T_out);
  const float invM = 1.f / (float)M;
  for (int64_t jc = j0; jc < j1; jc += FCH) {
    const int64_t j = jc + lane, t = j - A.pad;
    const bool valid = j < j1 && t >= 0 && t < T - lag;
    float acc = 0.f;
    if (valid) {
      if (k == 1) {
        for (int m = m0; m < m1; ++m) {
          const float* row = P + (int64_t)m * T + t;
          acc += rise(row[lag], row[0]);
        }
      } else {
        for (int m = m0; m < m1; ++m) {
          const int lo = max(0, m - h), hi = min(M - 1, m - h + k - 1);
          float r = P[(int64_t)lo * T + t];
          for (int q = lo + 1; q <= hi; ++q) r = fmaxf(r, P[(int64_t)q * T + t]);
          acc += rise(P[(int64_t)m * T + t + lag], r);
        }
      }
    }
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0 && j < j1)
      A.env[b * A.T_out + j] = valid ? ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) * invM : 0.f;
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void onset_detrend_kernel(float* env, int64_t T) {
  const int lane = threadIdx.x;
  float* e = env + (int64_t)blockIdx.x * T;
  constexpr double a = 0.99;
  double ap = a;                        // a^(lane + 1): weight of the carry
  for (int i = 0; i < lane; ++i) ap *= a;
  double carry = 0.0, xprev = 0.0;      // y[-1], x[-1]
  for (int64_t c = 0; c < T; c += 64) {
    const int64_t n = c + lane;
    const double x = n < T ? (double)e[n] : 0.0;
    double xl = __shfl_up(x, 1, 64);
    if (lane == 0) xl = xprev;
    double sft = x - xl, ak = a;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double o = __shfl_up(sft, d, 64);
      if (lane >= d) sft += ak * o;
      ak *= ak;
    }
    const double y = sft + ap * carry;
    if (n < T) e[n] = (float)y;
    carry = __shfl(y, 63, 64);
    xprev = __shfl(x, 63, 64);
  }
}

// ------------------------------------------------------------------ peak picking
struct PeakArgs {
  const float* env; const float* energy; int64_t T, ld; int pre_max, post_max, pre_avg, post_avg; double delta;
  int wait, normalize, backtrack; int32_t* frames; int32_t* count; int mode; int64_t nsl;
};

constexpr int PT_MAX = 1024;
constexpr int PHALO = 256;              // window halo a side that is staged in LDS with a tile of frames
constexpr int PW = 2048;                // ballot words (64 flags each) held in LDS for the greedy pass
constexpr int64_t P_ONE = 4096;         // clips up to this many frames: one launch, one workgroup a clip
constexpr int64_t PSL = 4096;           // frames per workgroup of the sliced flag launch
constexpr int P_FUSED = 0, P_FLAGS = 1, P_PICK = 2;                  // chunks of 64 flags in flight in the greedy pass

__global__ __launch_bounds__(PT_MAX) void onset_peaks_kernel(PeakArgs A) {
  __shared__ float rmin[PT_MAX / 64], rmax[PT_MAX / 64];
  __shared__ int rbad[PT_MAX / 64];
  __shared__ int s_count;
  __shared__ float tile[PT_MAX + 2 * PHALO];
  __shared__ unsigned long long words[PW];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, nw = nt >> 6;
  const int64_t T = A.T;
  const int64_t b = A.mode == P_FLAGS ? blockIdx.x / A.nsl : blockIdx.x;
  const int64_t f0 = A.mode == P_FLAGS ? (blockIdx.x % A.nsl) * PSL : 0, f1 = A.mode == P_FLAGS ? min(T, f0 + PSL) : T;
  const float* e = A.env + b * A.ld;
  int32_t* out = A.frames + b * T;
  if (A.mode != P_PICK) {
  // ---- min / max / finiteness of the whole clip (every workgroup of a sliced clip redoes it, out of L2)
  float mn = INFINITY, mx = -INFINITY;
  int bad = 0;
  for (int64_t i = tid; i < T; i += nt) {
    const float v = e[i];
    bad |= !isfinite(v);
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  bad = __ballot(bad) != 0;
  if (lane == 0) { rmin[tid >> 6] = mn; rmax[tid >> 6] = mx; rbad[tid >> 6] = bad; }
  __syncthreads();
  for (int i = 0; i < nw; ++i) { mn = fminf(mn, rmin[i]); mx = fmaxf(mx, rmax[i]); bad |= rbad[i]; }
  if (bad || (mn == 0.f && mx == 0.f)) {         // non-finite or all-zero envelope: no onsets
    for (int64_t i = f0 + tid; i < f1; i += nt) out[i] = A.mode == P_FLAGS ? 0 : -1;
    if (tid == 0 && A.mode == P_FUSED) A.count[b] = 0;
    return;
  }
  // ---- candidate flags
  const double sub = A.normalize ? (double)mn : 0.0;
  const double den = A.normalize ? ((double)mx - (double)mn) + (double)FLT_MIN : 1.0;
  const float zero = A.normalize ? mn : 0.f;     // x[n] == 0 on the raw values
  // a tile of nt frames and its window halo go through LDS (windows wider than PHALO a side read the row itself)
  const int hl = max(A.pre_max, A.pre_avg), hr = max(A.post_max, A.post_avg);
  const bool staged = hl <= PHALO && hr <= PHALO;
  for (int64_t n0 = f0; n0 < f1; n0 += nt) {
    const float* w = e;
    int64_t base = 0;
    if (staged) {
      const int64_t lo = max((int64_t)0, n0 - hl), hi = min(T, min(f1, n0 + nt) + hr);
      __syncthreads();
      for (int64_t i = lo + tid; i < hi; i += nt) tile[i - lo] = e[i];
      __syncthreads();
      w = tile;
      base = lo;
    }
    const int64_t n = n0 + tid;
    if (n >= f1) continue;
    const float v = w[n - base];
    int flag = v != zero;
    if (flag) {
      const int64_t a0 = max((int64_t)0, n - A.pre_max), a1 = min(T, n + A.post_max);
      for (int64_t i = a0; i < a1; ++i) flag &= w[i - base] <= v;
    }
    if (flag) {
      const int64_t a0 = max((int64_t)0, n - A.pre_avg), a1 = min(T, n + A.post_avg);
      double sum = 0.0;
      int64_t i = a0;
      for (; i + 4 <= a1; i += 4) {                // four loads in flight, added in index order
        const float* q = w + (i - base);
        const float x0 = q[0], x1 = q[1], x2 = q[2], x3 = q[3];
        sum += (double)x0; sum += (double)x1; sum += (double)x2; sum += (double)x3;
      }
      for (; i < a1; ++i) sum += (double)w[i - base];
      // (the window is never empty: post_avg >= 1 keeps frame n inside it)
      const double avg = (sum / (double)(a1 - a0) - sub) / den;
      flag = ((double)v - sub) / den >= avg + A.delta;
    }
    out[n] = flag;
  }
  if (A.mode == P_FLAGS) return;
  __syncthreads();
  }
  // ---- greedy pass: a candidate is kept when it lies more than `wait` frames after the last kept one.  All waves
  // turn the flags of up to 64 PW frames into ballot words in LDS; wave 0 then takes 64 words a step, skips the
  // empty ones and walks the set bits.  The words are in LDS before lane 0 reuses the flags' slots, and an output slot
  // is never ahead of the frame it holds, so a later segment's flags are still intact when it is read.
  const int wv = tid >> 6;
  int64_t last = -1 - (int64_t)A.wait;           // the first candidate always passes
  int kept = 0;
  for (int64_t seg0 = 0; seg0 < T; seg0 += (int64_t)64 * PW) {
    const int nwords = (int)min((int64_t)PW, (T - seg0 + 63) / 64);
    for (int wi = wv; wi < nwords; wi += 4 * nw) {
      int v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = out[min(seg0 + (int64_t)64 * (wi + u * nw) + lane, T - 1)];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int wq = wi + u * nw;
        const unsigned long long m = __ballot(seg0 + (int64_t)64 * wq + lane < T && v[u] != 0);
        if (lane == 0 && wq < nwords) words[wq] = m;
      }
    }
    __syncthreads();
    if (wv == 0) {
      for (int w0 = 0; w0 < nwords; w0 += 64) {
        const unsigned long long word = w0 + lane < nwords ? words[w0 + lane] : 0ull;
        unsigned long long nz = __ballot(word != 0ull);
        while (nz) {
          const int j = __builtin_ctzll(nz);
          nz &= nz - 1ull;
          unsigned long long m = __shfl(word, j, 64);
          const int64_t c = seg0 + (int64_t)64 * (w0 + j);
          while (m) {
            const int i = __builtin_ctzll(m);
            const int64_t p = c + i;
            if (p > last + A.wait) {
              last = p;
              if (lane == 0) out[kept] = (int32_t)p;
              ++kept;
              const int64_t upto = (int64_t)i + A.wait;   // bits i .. i + wait are spent
              m = upto >= 63 ? 0ull : m & ~((2ull << upto) - 1ull);
            } else {
              m &= m - 1ull;
            }
          }
        }
      }
    }
    __syncthreads();
  }
  if (tid == 0) { A.count[b] = kept; s_count = kept; }
  __syncthreads();
  const int cnt = s_count;
  for (int64_t i = cnt + tid; i < T; i += nt) out[i] = -1;
  if (!A.backtrack) return;
  // ---- backtrack: nearest i <= onset with e[i] <= e[i - 1] and e[i] < e[i + 1]; frame 0 always qualifies
  const float* g = A.energy ? A.energy + b * A.ld : e;
  for (int q = tid; q < cnt; q += nt) {
    int64_t i = out[q];
    while (i > 0 && !(i <= T - 2 && g[i] <= g[i - 1] && g[i] < g[i + 1])) --i;
    out[q] = (int32_t)i;
  }
}

// ------------------------------------------------------------------ clip totals
constexpr int CT = 1024;

__global__ __launch_bounds__(CT) void clip_metrics_kernel(const float* y, int64_t L, int64_t ldy, float* out) {
  __shared__ double ss[CT];
  __shared__ float pk[CT];
  const int tid = threadIdx.x;
  const float* x = y + (int64_t)blockIdx.x * ldy;
  double s = 0.0;
  float p = 0.f;
  for (int64_t i = tid; i < L; i += CT) {
    const float v = x[i];
    s += (double)v * (double)v;
    p = fmaxf(p, fabsf(v));
  }
  ss[tid] = s;
  pk[tid] = p;
  __syncthreads();
  for (int d = CT / 2; d >= 1; d >>= 1) {
    if (tid < d) { ss[tid] += ss[tid + d]; pk[tid] = fmaxf(pk[tid], pk[tid + d]); }
    __syncthreads();
  }
  if (tid == 0) { out[2 * blockIdx.x] = (float)ss[0]; out[2 * blockIdx.x + 1] = pk[0]; }
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_onset_strength_work_bytes(int64_t B, int M, int64_t T) {
  if (B < 1 || M < 1 || T < 1) return -1;
  return T <= T_ONE ? 0 : B * ceil_div(T, MSL) * (int64_t)sizeof(float);
}

extern "C" int syg_onset_strength_f32(const float* mel, int64_t B, int M, int64_t T, float amin, float top_db, int lag,
                                      int max_size, int pad, int64_t T_out, int detrend, float* env, void* work,
                                      void* stream) {
  SYG_REQUIRE(mel && env, "onset_strength: null pointer argument (mel / env)");
  SYG_REQUIRE(B >= 1 && M >= 1 && T >= 1 && (int64_t)M * T < ((int64_t)1 << 40) / B, "onset_strength: bad B / M / T");
  SYG_REQUIRE(amin > 0.f && isfinite(amin), "onset_strength: amin must be strictly positive");
  SYG_REQUIRE(!isnan(top_db), "onset_strength: top_db is NaN");
  SYG_REQUIRE(lag >= 1, "onset_strength: lag must be a positive integer");
  SYG_REQUIRE(lag < T, "onset_strength: lag = %d needs more than %lld frames", lag, (long long)T);
  SYG_REQUIRE(max_size >= 1, "onset_strength: max_size must be a positive integer");
  SYG_REQUIRE(pad >= 0 && T_out >= 1 && T_out <= pad + T, "onset_strength: bad pad / T_out");
  const int64_t wb = syg_onset_strength_work_bytes(B, M, T);
  SYG_REQUIRE(wb == 0 || work, "onset_strength: %lld frames need a workspace of syg_onset_strength_work_bytes",
              (long long)T);
  FluxArgs A{mel, B, M, T, fmaxf(amin, FLT_MIN), top_db, lag, max_size, pad, T_out, env, (float*)work, 1, 0};
  hipStream_t st = (hipStream_t)stream;
  if (wb == 0) {
    SYG_REQUIRE(B < 0x7fffffff, "onset_strength: too many clips");
    hipLaunchKernelGGL(onset_flux_kernel<true>, dim3((unsigned)B), dim3(FT), 0, st, A);
  } else {
    A.nmax = ceil_div(T, MSL);
    A.nsl = ceil_div(T_out, FSL);
    SYG_REQUIRE(B * A.nsl < 0x7fffffff, "onset_strength: too many slices");
    hipLaunchKernelGGL(onset_max_kernel, dim3((unsigned)(B * A.nmax)), dim3(FT), 0, st, A);
    SYG_CHECK_LAUNCH("onset_strength (maximum)");
    hipLaunchKernelGGL(onset_flux_kernel<false>, dim3((unsigned)(B * A.nsl)), dim3(FT), 0, st, A);
  }
  SYG_CHECK_LAUNCH("onset_strength");
  if (detrend) {
    hipLaunchKernelGGL(onset_detrend_kernel, dim3((unsigned)B), dim3(64), 0, st, env, T_out);
    SYG_CHECK_LAUNCH("onset_strength (detrend)");
  }
  return SYG_OK;
}

extern "C" int syg_onset_peaks_f32(const float* env, int64_t B, int64_t T, int64_t ld, int pre_max, int post_max,
                                   int pre_avg, int post_avg, double delta, int wait, int normalize, int backtrack,
                                   const float* energy, int32_t* frames, int32_t* count, void* stream) {
  SYG_REQUIRE(env && frames && count, "onset_peaks: null pointer argument (env / frames / count)");
  SYG_REQUIRE(B >= 1 && B < 0x7fffffff && T >= 1 && T < 0x7fffffff && ld >= T, "onset_peaks: bad B / T / ld");
  SYG_REQUIRE(pre_max >= 0 && post_max >= 0 && pre_avg >= 0 && post_avg >= 0 && wait >= 0,
              "onset_peaks: windows and wait must be non-negative (got %d, %d, %d, %d, %d)", pre_max, post_max, pre_avg,
              post_avg, wait);
  SYG_REQUIRE(pre_max + (int64_t)post_max >= 1, "onset_peaks: pre_max + post_max must be at least 1");
  SYG_REQUIRE(pre_avg + (int64_t)post_avg >= 1, "onset_peaks: pre_avg + post_avg must be at least 1");
  SYG_REQUIRE(post_max >= 1 && post_avg >= 1, "onset_peaks: post_max and post_avg must be positive");
  SYG_REQUIRE(isfinite(delta) && delta >= 0.0, "onset_peaks: delta must be finite and non-negative");
  PeakArgs A{env, energy, T, ld, pre_max, post_max, pre_avg, post_avg, delta, wait, normalize != 0, backtrack != 0,
             frames, count, P_FUSED, 1};
  if (T <= P_ONE) {
    hipLaunchKernelGGL(onset_peaks_kernel, dim3((unsigned)B), dim3(T <= 256 ? 256 : PT_MAX), 0, (hipStream_t)stream, A);
  } else {                         // a long clip: its flags from many workgroups, then one wave picks
    A.mode = P_FLAGS;
    A.nsl = ceil_div(T, PSL);
    SYG_REQUIRE(B * A.nsl < 0x7fffffff, "onset_peaks: too many slices");
    hipLaunchKernelGGL(onset_peaks_kernel, dim3((unsigned)(B * A.nsl)), dim3(PT_MAX), 0, (hipStream_t)stream, A);
    SYG_CHECK_LAUNCH("onset_peaks (flags)");
    A.mode = P_PICK;
    hipLaunchKernelGGL(onset_peaks_kernel, dim3((unsigned)B), dim3(PT_MAX), 0, (hipStream_t)stream, A);
  }
  SYG_CHECK_LAUNCH("onset_peaks");
  return SYG_OK;
}

extern "C" int syg_clip_metrics_f32(const float* y, int64_t B, int64_t L, int64_t ldy, float* out, void* stream) {
  SYG_REQUIRE(y && out, "clip_metrics: null pointer argument (y / out)");
  SYG_REQUIRE(B >= 1 && B < 0x7fffffff && L >= 1 && ldy >= L, "clip_metrics: bad B / L / ldy");
  hipLaunchKernelGGL(clip_metrics_kernel, dim3((unsigned)B), dim3(CT), 0, (hipStream_t)stream, y, L, ldy, out);
  SYG_CHECK_LAUNCH("clip_metrics");
  return SYG_OK;
}
