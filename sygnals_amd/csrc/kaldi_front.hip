// Kaldi-compatible front end (torchaudio.compliance.kaldi.fbank / mfcc, restated in tests/kaldi_ref.py): samples in, log mel
// filterbank energies or MFCCs out, one launch, no spectrogram in HBM.  The transform and the projection are those of
// stft_mel_pow2.hip: a workgroup takes 16 consecutive frames of one clip, every wave runs whole frames by itself
// (block_fft<WAVE> on the real frame packed as N/2 complex points), a barrier, then v_mfma_f32_16x16x4_f32 projects the 16
// LDS power rows onto the zero-padded filterbank.  What is Kaldi's is the load stage and the epilogue:
//   load      wl samples by the framing rule (snip_edges: frame t starts at t hop; otherwise at t hop + hop/2 - wl/2 with
//             Kaldi's reflection where the frame leaves the clip; the interior takes the unchecked path) are staged in the
//             wave's second FFT buffer; dither (Philox normals keyed by seed, clip, frame, sample) is added there; the frame
//             sum is a float64 wave sum and the mean is rounded once; DC removal, pre-emphasis (the neighbour comes from
//             the staged samples, x[-1] := x[0]) and the window are applied on the way into the packed frame, zero-padded
//             to N; the log-energy is a float64 wave sum of squares, before the pre-emphasis (raw_energy) or behind the
//             window;
//   epilogue  E > eps ? logf(E) : log_eps (the float32 nearest to log(eps), so floor cells are bit-exact), the optional
//             energy column, and for MFCC the num_ceps x M contraction (DCT-II rows with the lifter folded in) on the MFMA
//             from the tile's log rows in LDS.
// The Nyquist bin carries no weight: the power rows have N/2 columns.  Output goes through two strides (frame,
// coefficient), so [B, C, T] and [B, T, C] are both one launch.  No atomics: a call repeats its bits, a batch equals its
// rows.  The grid is capped (capped_grid) and a workgroup loops over the tiles past the cap.
#include "host.h"
#include "rng_dev.h"

namespace syg {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int KALDI_TILE = 16;                 // frames of a workgroup's tile
constexpr int KALDI_N_MIN = 256, KALDI_N_MAX = 2048;
constexpr int KALDI_MEL_MIN = 3, KALDI_MEL_MAX = 256;
constexpr int KALDI_LDS_MAX = 160 * 1024;
constexpr int KALDI_WGS_PER_CU = 2;            // workgroups a CU of the capped grid
constexpr int KALDI_LG_STRIDE = 17;            // row stride of the log tile [band][16 frames]
constexpr float KALDI_EPS = 1.1920929e-07f;    // float32 epsilon: the floor of every logarithm here

struct KaldiArgs {
  const float* y; int64_t B, L, ldy, T;
  int wl, hop, n_fft, snip_edges;
  const float* win;            // [wl]
  const float2* tw;            // [n_fft + n_fft / 2]: W_N^k, then W_{N/2}^k
  const float* basis_p;        // [16 ceil(M / 16), n_fft / 2]
  int n_mels;
  float preemph; int remove_dc, raw_energy, use_power, use_log;
  float log_eps, log_energy_floor;
  float dither; uint2 key;
  const float* dct; int num_ceps;              // [num_ceps, M] (lifter folded in) or null: filterbank output
  int e_col, feat_off, c0_last;                // column of the log-energy (-1: none), first feature column, htk order
  float* out; int64_t sob, sot, soc;
  float* fb; int64_t sfb, sft, sfc;            // MFCC: the log filterbank beside it, or null
  int64_t tiles_per_clip, tiles;
};

// Real-input split: Z = FFT_M(z), z[m] = x[2m] + i x[2m+1]; X[k], k in [0, M);  tw2[k] = W_{2M}^k.
__device__ __forceinline__ float2 rbin(const float2* Z, int M, int k, const float2* __restrict__ tw2) {
  const float2 zk = Z[k], zm = Z[(M - k) & (M - 1)];
  const float2 E = make_float2(zk.x + zm.x, zk.y - zm.y);
  const float2 O = make_float2(zk.y + zm.y, zm.x - zk.x);
  const float2 wO = cmul(tw2[k], O);
  return make_float2(0.5f * (E.x + wO.x), 0.5f * (E.y + wO.y));
}

// Kaldi's reflection of an index outside [0, L): s <- -s - 1 or s <- 2 L - 1 - s until inside, in closed form
__device__ __forceinline__ int64_t reflect(int64_t s, int64_t L) {
  int64_t r = s % (2 * L);
  if (r < 0) r += 2 * L;
  return r < L ? r : 2 * L - 1 - r;
}

// LDS (floats): fft [NW][2][M] complex (MFCC: the log tile [16 n_mt][17] aliases it between the barriers) | P [16][PS] |
// twl [n_fft + M] complex
template <int NW>
__global__ __launch_bounds__(NW * 64) void kaldi_front_kernel(KaldiArgs A, int fft_floats) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int n_fft = A.n_fft, M = n_fft >> 1, PS = M + 4, wl = A.wl;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  float2* fx = reinterpret_cast<float2*>(lds) + (size_t)w * 2 * M;
  float2* fz = fx + M;
  float* stage = reinterpret_cast<float*>(fz);       // the frame's wl raw samples (wl <= n_fft = 2 M floats)
  float* lg = lds;
  float* P = lds + fft_floats;
  float2* twl = reinterpret_cast<float2*>(P + KALDI_TILE * PS);
  for (int i = tid; i < n_fft + M; i += NW * 64) twl[i] = A.tw[i];
  // the columns [M, PS) of the power rows are never read
  const int n_mels = A.n_mels, n_mt = (n_mels + 15) >> 4;
  const int n = lane & 15, kk = lane >> 4;
  const bool mfcc = A.dct != nullptr;
  __syncthreads();

  for (int64_t tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
    const int64_t b = tile / A.tiles_per_clip;
    const int64_t t0 = (tile - b * A.tiles_per_clip) * KALDI_TILE;
    const float* yb = A.y + b * A.ldy;
    // ---- transforms: wave w takes the frames w, w + NW, ... of the tile
    for (int fi = w; fi < KALDI_TILE; fi += NW) {
      const int64_t t = t0 + fi;
      float* prow = P + fi * PS;
      if (t >= A.T) {
        for (int k = lane; k < M; k += 64) prow[k] = 0.f;
        continue;
      }
      const int64_t s0 = t * (int64_t)A.hop + (A.snip_edges ? 0 : (A.hop >> 1) - (wl >> 1));
      if (s0 >= 0 && s0 + wl <= A.L) {
        for (int i = lane; i < wl; i += 64) stage[i] = yb[s0 + i];
      } else {
        for (int i = lane; i < wl; i += 64) stage[i] = yb[reflect(s0 + i, A.L)];
      }
      if (A.dither != 0.f) {
        wave_lds_sync();
        for (int g = lane; 4 * g < wl; g += 64) {
          const float4 z = rng_normal4(A.key, ((uint64_t)t << 9) | (uint64_t)g, (uint32_t)b);
          const float zz[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (4 * g + j < wl) stage[4 * g + j] = fmaf(A.dither, zz[j], stage[4 * g + j]);
        }
      }
      wave_lds_sync();
      float mean = 0.f;
      if (A.remove_dc) {
        double s = 0.0;
        for (int i = lane; i < wl; i += 64) s += (double)stage[i];
        mean = (float)(wave_sum_d(s) / (double)wl);
      }
      // packed frame: lane's complex point m holds the samples 2 m and 2 m + 1
      const bool want_e = A.e_col >= 0, raw_e = want_e && A.raw_energy, win_e = want_e && !A.raw_energy;
      double e2 = 0.0;
      for (int m = lane; m < M; m += 64) {
        const int i0 = 2 * m, i1 = i0 + 1;
        float a = 0.f, c = 0.f;
        if (i0 < wl) {
          const float x0 = stage[i0] - mean;
          const float xm = i0 > 0 ? stage[i0 - 1] - mean : x0;
          a = fmaf(-A.preemph, xm, x0);
          if (raw_e) e2 += (double)x0 * (double)x0;
          a *= A.win[i0];
          if (win_e) e2 += (double)a * (double)a;
          if (i1 < wl) {
            const float x1 = stage[i1] - mean;
            c = fmaf(-A.preemph, x0, x1);
            if (raw_e) e2 += (double)x1 * (double)x1;
            c *= A.win[i1];
            if (win_e) e2 += (double)c * (double)c;
          }
        }
        fx[m] = make_float2(a, c);
      }
      if (want_e) {
        const double es = wave_sum_d(e2);
        const float le = fmaxf(logf(fmaxf((float)es, KALDI_EPS)), A.log_energy_floor);
        if (lane == 0) A.out[b * A.sob + t * A.sot + (int64_t)A.e_col * A.soc] = le;
      }
      wave_lds_sync();                   // the staged samples are read: the transform may write the second buffer
      const float2* Z = block_fft<true>(fx, fz, M, twl + n_fft, lane, 64);
      for (int k = lane; k < M; k += 64) {
        const float2 X = rbin(Z, M, k, twl);
        const float p2 = fmaf(X.x, X.x, X.y * X.y);
        prow[k] = A.use_power ? p2 : sqrtf(p2);
      }
      wave_lds_sync();                   // the buffers are free for the wave's next frame
    }
    __syncthreads();
    // ---- projection: wave w takes the 16-row mel tiles w, w + NW, ...
    for (int mt = w; mt < n_mt; mt += NW) {
      const float* arow = A.basis_p + (size_t)(16 * mt + n) * M + 4 * kk;
      const float* brow = P + n * PS + 4 * kk;
      v4f acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};
      for (int s = 0; s < M; s += 16) {
        const float4 a4 = *reinterpret_cast<const float4*>(arow + s);
        const float4 b4 = *reinterpret_cast<const float4*>(brow + s);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b4.x, acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b4.y, acc2, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b4.z, acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b4.w, acc2, 0, 0, 0);
      }
      acc += acc2;
      // D[row 4 kk + i][col n]: mel row 16 mt + 4 kk + i of frame t0 + n
      const int64_t t = t0 + n;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 16 * mt + 4 * kk + i;
        const float E = acc[i];
        const float v = A.use_log ? (E > KALDI_EPS ? logf(E) : A.log_eps) : E;
        if (mfcc) {
          lg[m * KALDI_LG_STRIDE + n] = m < n_mels ? v : 0.f;      // (the transforms are behind the barrier: the FFT buffers are free)
          if (A.fb != nullptr && m < n_mels && t < A.T) A.fb[b * A.sfb + t * A.sft + (int64_t)m * A.sfc] = v;
        } else if (m < n_mels && t < A.T) {
          A.out[b * A.sob + t * A.sot + (int64_t)(A.feat_off + m) * A.soc] = v;
        }
      }
    }
    __syncthreads();                     // every projection has read the rows: the next tile may overwrite them
    if (!mfcc) continue;
    // ---- cepstra: c[k, t] = sum_m dct[k, m] lg[m, t], wave w takes the 16-row coefficient tiles w, w + NW, ...
    const int nc = A.num_ceps, ktiles = (nc + 15) >> 4;
    for (int kt = w; kt < ktiles; kt += NW) {
      const int krow = kt * 16 + n;
      v4f acc = {0.f, 0.f, 0.f, 0.f};
      for (int m0 = 0; m0 < n_mels; m0 += 4) {
        const int m = m0 + kk;
        const float a = (krow < nc && m < n_mels) ? A.dct[krow * n_mels + m] : 0.f;
        const float bv = (m < n_mels) ? lg[m * KALDI_LG_STRIDE + n] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc, 0, 0, 0);
      }
      const int64_t t = t0 + n;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = kt * 16 + 4 * kk + r;
        if (k < nc && t < A.T) {
          const int col = A.c0_last ? (k ? k - 1 : nc - 1) : k;
          if (col != A.e_col) A.out[b * A.sob + t * A.sot + (int64_t)col * A.soc] = acc[r];
        }
      }
    }
    __syncthreads();                     // the log tile is read: the next tile's transforms may write the FFT buffers
  }
}

inline int waves_of(int n_fft) { return n_fft == 2048 ? 4 : 8; }

inline int fft_floats_of(int n_fft, int n_mels, bool mfcc) {
  const int a = waves_of(n_fft) * 2 * n_fft;                        // NW waves x 2 buffers x M complex
  const int b = mfcc ? 16 * ((n_mels + 15) / 16) * KALDI_LG_STRIDE : 0;
  return a > b ? a : b;
}

inline size_t lds_bytes(int n_fft, int n_mels, bool mfcc) {
  const int M = n_fft / 2;
  return ((size_t)fft_floats_of(n_fft, n_mels, mfcc) + (size_t)KALDI_TILE * (M + 4) + (size_t)2 * (n_fft + M)) * sizeof(float);
}

inline bool finite_f(float v) { return v - v == 0.f; }

const char* const SERVED = "served: n_fft 256, 512, 1024 or 2048, 2 <= wl <= n_fft, hop >= 1, 3 <= num_mel_bins <= 256, "
                           "1 <= num_ceps <= num_mel_bins";

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_kaldi_constants(int key) {
  switch (key) {
    case SYG_KALDI_TILE: return KALDI_TILE;
    case SYG_KALDI_N_MIN: return KALDI_N_MIN;
    case SYG_KALDI_N_MAX: return KALDI_N_MAX;
    case SYG_KALDI_MEL_MIN: return KALDI_MEL_MIN;
    case SYG_KALDI_MEL_MAX: return KALDI_MEL_MAX;
    case SYG_KALDI_LDS_MAX: return KALDI_LDS_MAX;
    case SYG_KALDI_WGS_PER_CU: return KALDI_WGS_PER_CU;
    case SYG_KALDI_LDS_WORST: return (int64_t)lds_bytes(KALDI_N_MAX, KALDI_MEL_MAX, true);
    default: return -1;
  }
}

extern "C" int syg_kaldi_fbank_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int wl, int hop, int n_fft, int snip_edges,
                                   int64_t T, const float* window, const float* twiddle, const float* basis_p, int n_mels,
                                   float preemph, int remove_dc, int raw_energy, int use_power, int use_log, float log_eps,
                                   float energy_floor, float dither, uint64_t seed, int use_energy, int htk_compat,
                                   const float* dct, int num_ceps, float* out, int64_t sob, int64_t sot, int64_t soc, float* fb,
                                   int64_t sfb, int64_t sft, int64_t sfc, void* stream) {
  const char* who = "kaldi_fbank";
  SYG_REQUIRE(y && window && twiddle && basis_p && out, "%s: null pointer argument", who);
  SYG_REQUIRE(n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048, "%s: n_fft = %d is not served (%s)", who, n_fft, SERVED);
  SYG_REQUIRE(wl >= 2 && wl <= n_fft, "%s: wl = %d is not served at n_fft = %d (%s)", who, wl, n_fft, SERVED);
  SYG_REQUIRE(hop >= 1, "%s: hop = %d is not served (%s)", who, hop, SERVED);
  SYG_REQUIRE(n_mels >= KALDI_MEL_MIN && n_mels <= KALDI_MEL_MAX, "%s: num_mel_bins = %d is not served (%s)", who, n_mels, SERVED);
  SYG_REQUIRE(!dct || (num_ceps >= 1 && num_ceps <= n_mels), "%s: num_ceps = %d is not served at num_mel_bins = %d (%s)", who,
              num_ceps, n_mels, SERVED);
  SYG_REQUIRE(dct || !fb, "%s: the filterbank beside the result is served for the MFCC only (dct is null)", who);
  SYG_REQUIRE(!dct || use_log, "%s: the MFCC is taken from the log filterbank (use_log = 0)", who);
  SYG_REQUIRE(B >= 1 && B < RNG_ROW_LIMIT && L >= 1 && L < ((int64_t)1 << 40) && (B == 1 || ldy >= L || ldy == 0),
              "%s: bad B / L / ldy (%lld, %lld, %lld)", who, (long long)B, (long long)L, (long long)ldy);
  const int64_t Texp = snip_edges ? (L >= wl ? 1 + (L - wl) / hop : 0) : (L + hop / 2) / hop;
  SYG_REQUIRE(T >= 1 && T == Texp, "%s: T=%lld does not match the framing rule (%lld; snip_edges: 1 + (L - wl) / hop, else "
              "(L + hop / 2) / hop)", who, (long long)T, (long long)Texp);
  SYG_REQUIRE(finite_f(preemph) && preemph >= 0.f && preemph <= 1.f, "%s: preemphasis_coefficient must be in [0, 1] (got %g)", who,
              (double)preemph);
  SYG_REQUIRE(finite_f(dither) && dither >= 0.f, "%s: dither must be non-negative and finite (got %g)", who, (double)dither);
  SYG_REQUIRE(finite_f(energy_floor) && energy_floor >= 0.f, "%s: energy_floor must be non-negative and finite (got %g)", who,
              (double)energy_floor);
  SYG_REQUIRE(finite_f(log_eps) && log_eps < 0.f, "%s: log_eps must be the float32 nearest to log(eps) (got %g)", who, (double)log_eps);
  const int C = dct ? num_ceps : n_mels + (use_energy ? 1 : 0);
  SYG_REQUIRE(sot >= 1 && soc >= 1 && ((soc == 1 && sot >= C) || (sot == 1 && soc >= T)) && (B == 1 || sob >= (int64_t)C * T),
              "%s: bad output strides (%lld, %lld, %lld) for [T = %lld, C = %d]: one of the frame and coefficient strides is 1", who,
              (long long)sob, (long long)sot, (long long)soc, (long long)T, C);
  if (fb)
    SYG_REQUIRE(sft >= 1 && sfc >= 1 && ((sfc == 1 && sft >= n_mels) || (sft == 1 && sfc >= T)) && (B == 1 || sfb >= (int64_t)n_mels * T),
                "%s: bad filterbank strides (%lld, %lld, %lld) for [T = %lld, M = %d]", who, (long long)sfb, (long long)sft,
                (long long)sfc, (long long)T, n_mels);
  SYG_REQUIRE(((uintptr_t)basis_p) % 16 == 0, "%s: the padded filterbank must be 16-byte aligned", who);
  const size_t lds = lds_bytes(n_fft, n_mels, dct != nullptr);
  SYG_REQUIRE(lds <= (size_t)KALDI_LDS_MAX, "%s: n_fft=%d needs %zu B of LDS", who, n_fft, lds);

  KaldiArgs A;
  A.y = y; A.B = B; A.L = L; A.ldy = ldy; A.T = T;
  A.wl = wl; A.hop = hop; A.n_fft = n_fft; A.snip_edges = snip_edges ? 1 : 0;
  A.win = window; A.tw = (const float2*)twiddle; A.basis_p = basis_p; A.n_mels = n_mels;
  A.preemph = preemph; A.remove_dc = remove_dc ? 1 : 0; A.raw_energy = raw_energy ? 1 : 0; A.use_power = use_power ? 1 : 0;
  A.use_log = use_log ? 1 : 0;
  A.log_eps = log_eps;
  A.log_energy_floor = energy_floor > 0.f ? logf(energy_floor) : -3.4e38f;
  A.dither = dither; A.key = rng_key(seed);
  A.dct = dct; A.num_ceps = dct ? num_ceps : 0;
  A.c0_last = (dct && htk_compat) ? 1 : 0;
  if (dct) {
    A.feat_off = 0;
    A.e_col = use_energy ? (htk_compat ? num_ceps - 1 : 0) : -1;
  } else {
    A.feat_off = (use_energy && !htk_compat) ? 1 : 0;
    A.e_col = use_energy ? (htk_compat ? n_mels : 0) : -1;
  }
  A.out = out; A.sob = sob; A.sot = sot; A.soc = soc;
  A.fb = fb; A.sfb = sfb; A.sft = sft; A.sfc = sfc;
  A.tiles_per_clip = ceil_div(T, KALDI_TILE);
  A.tiles = B * A.tiles_per_clip;
  const int fftf = fft_floats_of(n_fft, n_mels, dct != nullptr);
  const unsigned grid = capped_grid(A.tiles, KALDI_WGS_PER_CU);
  if (n_fft == 2048) {
    auto kern = kaldi_front_kernel<4>;
    if (const int rc = reserve_dynamic_lds(who, (const void*)kern, lds)) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(4 * 64), lds, (hipStream_t)stream, A, fftf);
  } else {
    auto kern = kaldi_front_kernel<8>;
    if (const int rc = reserve_dynamic_lds(who, (const void*)kern, lds)) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(8 * 64), lds, (hipStream_t)stream, A, fftf);
  }
  SYG_CHECK_LAUNCH(who);
  return SYG_OK;
}
