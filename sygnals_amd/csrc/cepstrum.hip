// Cepstral analysis: real cepstrum of frames (the cepstrogram) and of whole rows, complex cepstrum with its phase unwrap,
// the inverse complex cepstrum and the cepstral peak picker.  The float64 restatement that is the contract lives in
// tests/cepstrum_ref.py:
//     real     c = ifft(log(max(|X|, amin))).real,                       X = fft(x, n)
//     complex  c = ifft(log(max(|X|, amin)) + i phi_u).real,             phi_u = unwrap(angle X) - pi ndelay k / center
//
// Fused frame kernel (cepstrogram2048_kernel), n_fft = 2048.  A workgroup of CP_WAVES waves takes a tile of CP_TILE
// consecutive frames of one clip; a wave takes one frame at a time: the frame is read through the centre-padding rule
// and windowed, transformed as a 1024-point complex wave FFT (wave_fft.h) of the even / odd packing with the real-input
// split in registers (the lane that owns bin k also owns 1024 - k), L[k] = log(max(|X[k]|, amin)) is formed in the same
// registers, and the inverse of that real, even spectrum is the forward transform of the conjugate of its packed form
// (the arithmetic of pitch.hip's autocorrelation with L in the product's place).  The Q quefrencies a caller wants go to
// the tile's stage in LDS ([frame][q], rows Qp = 64 ceil(Q / 64) + 64 / CP_TILE floats apart); after a barrier the
// workgroup stores the stage with the frame index fastest, so that a wave writes 64 / CP_TILE rows of [B, Q, T] in runs
// of CP_TILE consecutive floats instead of 64 floats T apart.  Everything is float32 in one fixed order, no atomics: the
// same call gives the same bits, a batch equals its rows, and the arithmetic of a frame does not depend on Q.
//
// Chain form, for every other length (the transforms are the strided FFT's, run by sygnals_amd/ops.py):
//     syg_cepstrum_logmag_c64   D[r, k] = log(max(|X[r, k']|, amin)) - log(amin), k' = k or n - k (a one-sided spectrum
//                               is extended evenly), as a complex row for the inverse transform
//     syg_cepstrum_gather_f32   the real part of the first Q points of every row, log(amin) added back at q = 0, stored
//                               [rows, Q] or transposed into [B, Q, T]
// The floor is taken out before the inverse and put back after it: a frame at or under the floor in every bin is then a
// row of exact zeros for any transform, and its cepstrum is log(amin) at q = 0 and exactly 0 elsewhere.
//
// Phase unwrap (syg_cepstrum_unwrap_c64), three launches, no workgroup waits on another:
//     1  a block takes CP_SCAN bins of one row: phi = atan2f (bin 0: 0 or +pi by the sign of Re X[0] alone), the wrap
//        count M[k] in {-1, 0, 1} of np.unwrap's rule from the float64 difference of neighbours, an inclusive integer
//        scan inside the block; the block's total goes to the row's list of block sums
//     2  one block per row scans the block sums (exclusive, in place) and forms ndelay = rint(phi_u[center] / pi)
//     3  pointwise: log(max(|X|, amin)) - log(amin) + i (float)(phi + 2 pi (count) - pi ndelay k / center), float64 inside
// syg_cepstrum_exp_c64 is the inverse's middle: exp(Re) (cos, sin)(Im + pi ndelay k / center), the angle in float64.
//
// Peak picker (syg_cepstrum_peaks_f32): a thread per frame walks q = qmin .. qmax of the stored float32 cepstrogram
// (frames are the fast axis: coalesced), first maximum, parabolic shift in float64.
#include <float.h>
#include <math.h>
#include "wave_fft.h"
#include "host.h"

namespace syg {
namespace {

constexpr int NF = 2048;                 // frame length of the fused kernel
constexpr int CP_WAVES = 4;              // waves per workgroup
constexpr int CP_TILE = 8;               // frames per tile
constexpr int CP_SCAN = 1024;            // bins a block of the unwrap scans (256 threads x 4)
constexpr int CP_BLOCKS_PER_CU = 4;      // persistent grid of the fused kernel
constexpr double CP_PI = 3.14159265358979323846;

// log of the floor; 0 for amin = 0 (nothing is taken out then)
__device__ __forceinline__ float floor_log(float amin) { return amin > 0.f ? logf(amin) : 0.f; }
__device__ __forceinline__ float log_mag(float2 x, float amin) { return logf(fmaxf(sqrtf(fmaf(x.x, x.x, x.y * x.y)), amin)); }

struct CepLds {
  float2 sc[CP_WAVES][wfft::SC_COMPLEX];  // FFT exchange; between the transforms, the packed log spectrum in two halves
  float2 tw2l[wfft::TW2_COMPLEX];
  float2 tw1l[wfft::TW1_COMPLEX];
  float2 t2048[8][64];                    // W_2048^k of (lane, unit j, pair d), index j * 4 + d
};

// E = zk + conj(zm), O = -i (zk - conj(zm));  X[k] = (E + w O) / 2,  X[1024 - k] = conj(E - w O) / 2
__device__ __forceinline__ void split_fwd(float2 zk, float2 zm, float2 w, float2& xk, float2& xm) {
  const float2 E = make_float2(zk.x + zm.x, zk.y - zm.y);
  const float2 O = make_float2(zk.y + zm.y, zm.x - zk.x);
  const float2 wO = cmul(w, O);
  xk = make_float2(0.5f * (E.x + wO.x), 0.5f * (E.y + wO.y));
  xm = make_float2(0.5f * (E.x - wO.x), -0.5f * (E.y - wO.y));
}
// inverse split of a REAL spectrum (P[k] = pk, P[1024 - k] = pm) into the packed spectrum Zc of c[2m] + i c[2m+1]:
// Ec = (pk + pm) / 2, Oc = (pk - pm) conj(w) / 2, Zc[k] = Ec + i Oc, Zc[1024 - k] = conj(Ec) + i conj(Oc)
__device__ __forceinline__ void split_inv_real(float pk, float pm, float2 w, float2& zk, float2& zm) {
  const float Ec = 0.5f * (pk + pm), D = 0.5f * (pk - pm);
  const float2 Oc = make_float2(D * w.x, -D * w.y);
  zk = make_float2(Ec - Oc.y, Oc.x);
  zm = make_float2(Ec + Oc.y, Oc.x);
}

struct CepArgs {
  const float* y; int64_t L, ldy; int hop, center; int64_t T, tiles_per_clip, tiles;
  const float* win; int Q, Qp; float amin; float* out;
};

__global__ __launch_bounds__(CP_WAVES * 64) void cepstrogram2048_kernel(CepArgs A, const float2* __restrict__ tw) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cp_smem[];
  CepLds& S = *reinterpret_cast<CepLds*>(cp_smem);
  float* stage = reinterpret_cast<float*>(cp_smem + sizeof(CepLds));      // [CP_TILE][Qp]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  wfft::Lane lc;
  wfft::init_lane(lc, lane);
  wfft::init_tables(S.tw2l, S.tw1l, tw, NF, tid, CP_WAVES * 64);
  for (int i = tid; i < 8 * 64; i += CP_WAVES * 64) {
    const int q = i >> 6, l = i & 63;
    S.t2048[q][l] = tw[wfft::bin_of(l, q >> 2, q & 3)];
  }
  __syncthreads();
  float2* sc = S.sc[w];
  const int Q = A.Q, Qp = A.Qp;
  const float2* __restrict__ win2 = reinterpret_cast<const float2*>(A.win);

  for (int64_t tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
    const int64_t b = tile / A.tiles_per_clip, t0 = (tile - b * A.tiles_per_clip) * CP_TILE;
    const int cnt = (int)(A.T - t0 < CP_TILE ? A.T - t0 : CP_TILE);
    const float* __restrict__ yr = A.y + b * A.ldy;
    for (int tt = w; tt < cnt; tt += CP_WAVES) {
      const int64_t s0 = (t0 + tt) * A.hop - (A.center ? NF / 2 : 0);
      auto xat = [&](int n) -> float {
        const int64_t s = s0 + n;
        return (s >= 0 && s < A.L) ? yr[s] : 0.f;
      };
      float2 va[16];
#pragma unroll
      for (int a = 0; a < 16; ++a) {
        const int m = 64 * a + lane;
        const float2 wv = win2[m];
        va[a] = make_float2(xat(2 * m) * wv.x, xat(2 * m + 1) * wv.y);
      }
      float2 ak[2][4], am[2][4], a512;
      wfft::cfft1024(va, lc, sc, S.tw1l, S.tw2l, lane, ak, am, a512);
      // ---- log magnitudes and the inverse split, in the registers that hold the bins
      float2 zk[2][4], zm[2][4], z512 = make_float2(0.f, 0.f);
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const float2 wk = S.t2048[4 * j + d][lane];
          float2 xa, xam;
          split_fwd(ak[j][d], am[j][d], wk, xa, xam);
          split_inv_real(log_mag(xa, A.amin), log_mag(xam, A.amin), wk, zk[j][d], zm[j][d]);
        }
      if (lane == 0) {
        const float2 wk = make_float2(0.f, -1.f);    // W_2048^512
        float2 xa, xam, zmm;
        split_fwd(a512, a512, wk, xa, xam);
        split_inv_real(log_mag(xa, A.amin), log_mag(xam, A.amin), wk, z512, zmm);
      }
      // ---- conjugate into natural order, z[64 a + lane], through the exchange scratch: bins 0 .. 511, then 512 .. 1023
      float2 vc[16];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        auto send = [&](int k, float2 v) {
          if ((k >> 9) == h) sc[fft_swz(k & 511, true)] = make_float2(v.x, -v.y);
        };
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const int k = wfft::bin_of(lane, j, d);
            send(k, zk[j][d]);
            if (k != 0) send(1024 - k, zm[j][d]);
          }
        if (lane == 0) send(512, z512);
        wave_lds_sync();
#pragma unroll
        for (int a = 0; a < 8; ++a) vc[8 * h + a] = sc[fft_swz(64 * a + lane, true)];
        wave_lds_sync();
      }
      float2 ck[2][4], cm_[2][4], c512;
      wfft::cfft1024(vc, lc, sc, S.tw1l, S.tw2l, lane, ck, cm_, c512);
      constexpr float INV = 1.f / 1024.f;
      float* row = stage + tt * Qp;
      auto put = [&](int k, float2 v) {              // c[2k], c[2k + 1]
        if (2 * k < Q) row[2 * k] = v.x * INV;
        if (2 * k + 1 < Q) row[2 * k + 1] = -v.y * INV;
      };
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const int k = wfft::bin_of(lane, j, d);
          put(k, ck[j][d]);
          if (k != 0) put(1024 - k, cm_[j][d]);
        }
      if (lane == 0) put(512, c512);
    }
    __syncthreads();
    // ---- the tile's stage to [B, Q, T], frames fastest
    float* __restrict__ ob = A.out + b * (int64_t)Q * A.T + t0;
    for (int i = tid; i < Q * CP_TILE; i += CP_WAVES * 64) {
      const int tt = i & (CP_TILE - 1), q = i / CP_TILE;
      if (tt < cnt) ob[(int64_t)q * A.T + tt] = stage[tt * Qp + q];
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ chain form
__global__ __launch_bounds__(256) void ceps_logmag_kernel(const float2* __restrict__ X, int64_t rows, int64_t in_bins, int64_t n,
                                                         float amin, float2* __restrict__ Z) {
  const float l0 = floor_log(amin);
  const int64_t total = rows * n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / n, k = i - r * n;
    const int64_t ks = k < in_bins ? k : n - k;
    Z[i] = make_float2(log_mag(X[r * in_bins + ks], amin) - l0, 0.f);
  }
}

// rows of Z [rows, n] complex -> out[(b Q + q) T + t], r = b T + t (T = 1: [rows, Q]); 32 x 32 tiles through LDS when
// the frame index is the fast axis of out
__global__ __launch_bounds__(256) void ceps_gather_kernel(const float2* __restrict__ Z, int64_t rows, int64_t n, int64_t Q, int64_t T,
                                                         float amin, float* __restrict__ out) {
  __shared__ float tile[32][33];
  const float l0 = floor_log(amin);
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t nqb = (Q + 31) / 32;
  const int64_t q0 = ((int64_t)blockIdx.x % nqb) * 32, r0 = ((int64_t)blockIdx.x / nqb) * 32;
  if (T == 1) {
    for (int i = ty; i < 32; i += 8) {
      const int64_t r = r0 + i, q = q0 + tx;
      if (r < rows && q < Q) out[r * Q + q] = Z[r * n + q].x + (q == 0 ? l0 : 0.f);
    }
    return;
  }
  for (int i = ty; i < 32; i += 8) {
    const int64_t r = r0 + i, q = q0 + tx;
    tile[i][tx] = (r < rows && q < Q) ? Z[r * n + q].x + (q == 0 ? l0 : 0.f) : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int64_t r = r0 + tx, q = q0 + i;
    if (r < rows && q < Q) {
      const int64_t b = r / T, t = r - b * T;
      out[(b * Q + q) * T + t] = tile[tx][i];
    }
  }
}

// ------------------------------------------------------------------------------------------------ phase unwrap
// the phase of bin k in float64: float32 atan2f, and at bin 0 the sign of the real part alone
__device__ __forceinline__ double phase_at(const float2* __restrict__ xr, int64_t k) {
  const float2 v = xr[k];
  if (k == 0) return v.x >= 0.f ? 0.0 : CP_PI;
  return (double)atan2f(v.y, v.x);
}
// np.unwrap's correction of a step d between neighbours, in units of 2 pi (its ties at +-pi leave the step alone)
__device__ __forceinline__ int wrap_count(double d) { return d > CP_PI ? -1 : (d < -CP_PI ? 1 : 0); }

// inclusive scan of one int per thread over a block of 256 threads; red: 4 ints of LDS.  Returns the block's total.
__device__ __forceinline__ int block_incl_scan(int& v, int* red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  __syncthreads();                                    // red may still be read from a call before
  if (lane == 63) red[wv] = v;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q < wv) off += red[q];
    tot += red[q];
  }
  v += off;
  return tot;
}

__global__ __launch_bounds__(256) void ceps_wraps_kernel(const float2* __restrict__ X, int64_t n, int64_t nblk, int32_t* __restrict__ S,
                                                        int32_t* __restrict__ bsum) {
  __shared__ int red[4];
  const int64_t b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
  const float2* __restrict__ xr = X + b * n;
  const int64_t k0 = blk * CP_SCAN + 4 * (int64_t)threadIdx.x;
  int m[4];
  double prev = (k0 >= 1 && k0 - 1 < n) ? phase_at(xr, k0 - 1) : 0.0;
  int s = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t k = k0 + u;
    m[u] = 0;
    if (k < n) {
      const double p = phase_at(xr, k);
      if (k >= 1) m[u] = wrap_count(p - prev);
      prev = p;
    }
    s += m[u];
    m[u] = s;                                         // inclusive inside the thread
  }
  int incl = s;
  const int tot = block_incl_scan(incl, red);
  const int base = incl - s;
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (k0 + u < n) S[b * n + k0 + u] = base + m[u];
  if (threadIdx.x == 0) bsum[b * nblk + blk] = tot;
}

__global__ __launch_bounds__(256) void ceps_ndelay_kernel(const float2* __restrict__ X, int64_t n, int64_t nblk, const int32_t* __restrict__ S,
                                                         int32_t* __restrict__ bsum, int32_t* __restrict__ ndelay) {
  __shared__ int red[4];
  const int64_t b = blockIdx.x;
  int32_t* bs = bsum + b * nblk;
  int carry = 0;
  for (int64_t base = 0; base < nblk; base += 256) {     // (block-uniform trip count)
    const int64_t i = base + threadIdx.x;
    const int v = i < nblk ? bs[i] : 0;
    int incl = v;
    const int tot = block_incl_scan(incl, red);
    if (i < nblk) bs[i] = carry + incl - v;
    carry += tot;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t center = (n + 1) / 2;
    const double pu = phase_at(X + b * n, center) + 2.0 * CP_PI * (double)(S[b * n + center] + bs[center / CP_SCAN]);
    ndelay[b] = (int32_t)rint(pu / CP_PI);
  }
}

__global__ __launch_bounds__(256) void ceps_logphase_kernel(const float2* __restrict__ X, int64_t B, int64_t n, int64_t nblk, float amin,
                                                           const int32_t* __restrict__ S, const int32_t* __restrict__ bsum,
                                                           const int32_t* __restrict__ ndelay, float2* __restrict__ Z) {
  const float l0 = floor_log(amin);
  const int64_t total = B * n, center = (n + 1) / 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / n, k = i - b * n;
    const int cnt = S[i] + bsum[b * nblk + k / CP_SCAN];
    const double pu = phase_at(X + b * n, k) + 2.0 * CP_PI * (double)cnt;
    const double ph = pu - CP_PI * (double)ndelay[b] * (double)k / (double)center;
    Z[i] = make_float2(log_mag(X[i], amin) - l0, (float)ph);
  }
}

__global__ __launch_bounds__(256) void ceps_exp_kernel(const float2* __restrict__ Xh, int64_t B, int64_t n, const int32_t* __restrict__ ndelay,
                                                      float2* __restrict__ Z) {
  const int64_t total = B * n, center = (n + 1) / 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / n, k = i - b * n;
    const float2 v = Xh[i];
    const double th = (double)v.y + CP_PI * (double)ndelay[b] * (double)k / (double)center;
    double sn, cs;
    sincos(th, &sn, &cs);
    const float e = expf(v.x);
    Z[i] = make_float2(e * (float)cs, e * (float)sn);
  }
}

// ------------------------------------------------------------------------------------------------ peak picker
struct PeakArgs {
  const float* c; int64_t B, Q, T; int qmin, qmax; double sr, threshold;
  double* f0; float* strength; int32_t* qstar; uint8_t* voiced;
};

__global__ __launch_bounds__(256) void ceps_peaks_kernel(PeakArgs A) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= A.B * A.T) return;
  const int64_t b = f / A.T, t = f - b * A.T;
  const float* __restrict__ c = A.c + b * A.Q * A.T + t;
  float best = c[(int64_t)A.qmin * A.T];
  int qs = A.qmin;
  for (int q = A.qmin + 1; q <= A.qmax; ++q) {
    const float v = c[(int64_t)q * A.T];
    if (v > best) { best = v; qs = q; }                // the first maximum
  }
  double delta = 0.0;
  if (qs > A.qmin && qs < A.qmax) {
    const double a = c[(int64_t)(qs - 1) * A.T], m = best, r = c[(int64_t)(qs + 1) * A.T];
    const double den = a - 2.0 * m + r;
    if (den < 0.0) delta = 0.5 * (a - r) / den;
  }
  const bool v = (double)best >= A.threshold;
  A.f0[f] = v ? A.sr / ((double)qs + delta) : (double)__builtin_nanf("");
  A.strength[f] = best;
  A.qstar[f] = qs;
  A.voiced[f] = v ? 1 : 0;
}

int check_amin(const char* who, double amin) {
  SYG_REQUIRE(amin >= 0.0 && amin <= (double)FLT_MAX, "%s: amin must be finite and >= 0 (got %g)", who, amin);
  return SYG_OK;
}
int check_rows(const char* who, int64_t rows, int64_t n, int64_t n_min) {
  SYG_REQUIRE(rows >= 1 && n >= n_min && n <= ((int64_t)1 << 26) && rows <= ((int64_t)1 << 31) / n,
              "%s: bad rows / n (rows >= 1, n in [%lld, 2^26], rows n <= 2^31)", who, (long long)n_min);
  return SYG_OK;
}
unsigned pointwise_grid(int64_t total) { return capped_grid(ceil_div(total, 256), CEPS_POINTWISE_WGS_PER_CU); }
int stage_pitch(int Q) { return (Q + 63) / 64 * 64 + 64 / CP_TILE; }

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_cepstrum_constants(int key) {
  switch (key) {
    case SYG_CEPS_FRAME: return NF;
    case SYG_CEPS_TILE_FRAMES: return CP_TILE;
    case SYG_CEPS_WAVES: return CP_WAVES;
    case SYG_CEPS_SCAN: return CP_SCAN;
    case SYG_CEPS_LDS_FIXED: return (int64_t)sizeof(CepLds);
    case SYG_CEPS_LDS_MAX: return (int64_t)sizeof(CepLds) + (int64_t)sizeof(float) * CP_TILE * stage_pitch(NF);
    default: set_error("cepstrum_constants: unknown key %d", key); return -1;
  }
}

extern "C" int syg_cepstrogram2048_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int frame_length, int hop, int center,
                                       int64_t T, const float* window, const float* twiddle, int n_ceps, double amin, float* out,
                                       void* stream) {
  if (frame_length != NF) {
    set_error("cepstrogram2048: frame_length %d is not served by the fused kernel (only 2048; other lengths take the chain form)",
              frame_length);
    return SYG_E_UNSUPPORTED;
  }
  SYG_REQUIRE(y && window && twiddle && out, "cepstrogram2048: null pointer argument (y / window / twiddle / out)");
  SYG_REQUIRE(n_ceps >= 1 && n_ceps <= NF, "cepstrogram2048: n_ceps=%d is outside 1 ... n_fft = %d", n_ceps, NF);
  if (const int rc = check_amin("cepstrogram2048", amin)) return rc;
  SYG_REQUIRE(B >= 1 && L >= 1 && ldy >= L, "cepstrogram2048: bad B / L / ldy");
  SYG_REQUIRE(hop >= 1 && (center == 0 || center == 1), "cepstrogram2048: bad hop / center");
  if (const int rc = check_framing("cepstrogram2048", T, frames_expected(L, NF, hop, center))) return rc;
  SYG_REQUIRE(T <= ((int64_t)1 << 31) / n_ceps / B, "cepstrogram2048: the result of %lld x %d x %lld elements is above 2^31",
              (long long)B, n_ceps, (long long)T);
  const int Qp = stage_pitch(n_ceps);
  const int64_t tpc = ceil_div(T, CP_TILE);
  CepArgs A{y, L, ldy, hop, center, T, tpc, B * tpc, window, n_ceps, Qp, (float)amin, out};
  const size_t lds = sizeof(CepLds) + sizeof(float) * (size_t)CP_TILE * (size_t)Qp;
  if (const int rc = reserve_dynamic_lds("cepstrogram2048", (const void*)cepstrogram2048_kernel, lds)) return rc;
  hipLaunchKernelGGL(cepstrogram2048_kernel, dim3(capped_grid(A.tiles, CP_BLOCKS_PER_CU)), dim3(CP_WAVES * 64), lds, (hipStream_t)stream, A,
                     (const float2*)twiddle);
  SYG_CHECK_LAUNCH("cepstrogram2048");
  return SYG_OK;
}

extern "C" int syg_cepstrum_logmag_c64(const float* X, int64_t rows, int64_t in_bins, int64_t n, double amin, float* Z, void* stream) {
  SYG_REQUIRE(X && Z, "cepstrum_logmag: null pointer argument (X / Z)");
  if (const int rc = check_rows("cepstrum_logmag", rows, n, 1)) return rc;
  SYG_REQUIRE(in_bins == n || in_bins == n / 2 + 1, "cepstrum_logmag: in_bins=%lld is neither n = %lld nor n / 2 + 1", (long long)in_bins,
              (long long)n);
  if (const int rc = check_amin("cepstrum_logmag", amin)) return rc;
  SYG_REQUIRE(Z != X || in_bins == n, "cepstrum_logmag: a one-sided spectrum cannot be extended in place");
  hipLaunchKernelGGL(ceps_logmag_kernel, dim3(pointwise_grid(rows * n)), dim3(256), 0, (hipStream_t)stream, (const float2*)X, rows,
                     in_bins, n, (float)amin, (float2*)Z);
  SYG_CHECK_LAUNCH("cepstrum_logmag");
  return SYG_OK;
}

extern "C" int syg_cepstrum_gather_f32(const float* Z, int64_t rows, int64_t n, int64_t n_ceps, int64_t T, double amin, float* out,
                                       void* stream) {
  SYG_REQUIRE(Z && out, "cepstrum_gather: null pointer argument (Z / out)");
  if (const int rc = check_rows("cepstrum_gather", rows, n, 1)) return rc;
  SYG_REQUIRE(n_ceps >= 1 && n_ceps <= n, "cepstrum_gather: n_ceps=%lld is outside 1 ... n_fft = %lld", (long long)n_ceps, (long long)n);
  SYG_REQUIRE(T >= 1 && (rows % T == 0 || rows < T), "cepstrum_gather: rows=%lld is neither a multiple of T=%lld nor a part of one clip",
              (long long)rows, (long long)T);
  if (const int rc = check_amin("cepstrum_gather", amin)) return rc;
  const int64_t blocks = ceil_div(n_ceps, 32) * ceil_div(rows, 32);
  SYG_REQUIRE(blocks < 0x7fffffff, "cepstrum_gather: too many tiles");
  hipLaunchKernelGGL(ceps_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float2*)Z, rows, n, n_ceps, T,
                     (float)amin, out);
  SYG_CHECK_LAUNCH("cepstrum_gather");
  return SYG_OK;
}

extern "C" int64_t syg_cepstrum_unwrap_work_bytes(int64_t B, int64_t n) {
  if (B < 1 || n < 2 || n > ((int64_t)1 << 26) || B > ((int64_t)1 << 31) / n) {
    set_error("cepstrum_unwrap_work_bytes: bad B / n (B >= 1, n in [2, 2^26], B n <= 2^31)");
    return -1;
  }
  return 4 * B * (n + ceil_div(n, CP_SCAN));          // the inclusive counts inside the blocks, then the block sums
}

extern "C" int syg_cepstrum_unwrap_c64(const float* X, int64_t B, int64_t n, double amin, void* work, int64_t work_bytes, float* Z,
                                       int32_t* ndelay, void* stream) {
  SYG_REQUIRE(X && Z && ndelay, "cepstrum_unwrap: null pointer argument (X / Z / ndelay)");
  if (const int rc = check_rows("cepstrum_unwrap", B, n, 2)) return rc;
  if (const int rc = check_amin("cepstrum_unwrap", amin)) return rc;
  const int64_t need = syg_cepstrum_unwrap_work_bytes(B, n);
  SYG_REQUIRE(work && work_bytes >= need, "cepstrum_unwrap: workspace of %lld bytes needed (syg_cepstrum_unwrap_work_bytes), got %lld",
              (long long)need, (long long)work_bytes);
  const int64_t nblk = ceil_div(n, CP_SCAN);
  SYG_REQUIRE(B * nblk < 0x7fffffff, "cepstrum_unwrap: too many blocks");
  int32_t* S = (int32_t*)work;
  int32_t* bsum = S + B * n;
  const float2* X2 = (const float2*)X;
  hipLaunchKernelGGL(ceps_wraps_kernel, dim3((unsigned)(B * nblk)), dim3(256), 0, (hipStream_t)stream, X2, n, nblk, S, bsum);
  hipLaunchKernelGGL(ceps_ndelay_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, X2, n, nblk, (const int32_t*)S, bsum,
                     ndelay);
  hipLaunchKernelGGL(ceps_logphase_kernel, dim3(pointwise_grid(B * n)), dim3(256), 0, (hipStream_t)stream, X2, B, n, nblk, (float)amin,
                     (const int32_t*)S, (const int32_t*)bsum, (const int32_t*)ndelay, (float2*)Z);
  SYG_CHECK_LAUNCH("cepstrum_unwrap");
  return SYG_OK;
}

extern "C" int syg_cepstrum_exp_c64(const float* Xh, int64_t B, int64_t n, const int32_t* ndelay, float* Z, void* stream) {
  SYG_REQUIRE(Xh && ndelay && Z, "cepstrum_exp: null pointer argument (Xh / ndelay / Z)");
  if (const int rc = check_rows("cepstrum_exp", B, n, 2)) return rc;
  hipLaunchKernelGGL(ceps_exp_kernel, dim3(pointwise_grid(B * n)), dim3(256), 0, (hipStream_t)stream, (const float2*)Xh, B, n, ndelay,
                     (float2*)Z);
  SYG_CHECK_LAUNCH("cepstrum_exp");
  return SYG_OK;
}

extern "C" int syg_cepstrum_peaks_f32(const float* ceps, int64_t B, int64_t Q, int64_t T, int qmin, int qmax, double sr, double threshold,
                                      double* f0, float* strength, int32_t* qstar, uint8_t* voiced, void* stream) {
  SYG_REQUIRE(ceps && f0 && strength && qstar && voiced, "cepstrum_peaks: null pointer argument (ceps / f0 / strength / qstar / voiced)");
  SYG_REQUIRE(B >= 1 && Q >= 1 && T >= 1 && Q <= ((int64_t)1 << 26) && T <= ((int64_t)1 << 31) / Q / B,
              "cepstrum_peaks: bad B / Q / T (each >= 1, B Q T <= 2^31)");
  SYG_REQUIRE(qmin >= 1 && qmin <= qmax && qmax < Q, "cepstrum_peaks: need 1 <= qmin <= qmax < Q (got %d, %d, Q=%lld)", qmin, qmax,
              (long long)Q);
  SYG_REQUIRE(sr > 0.0 && sr <= DBL_MAX && threshold == threshold, "cepstrum_peaks: bad sr / threshold");
  PeakArgs A{ceps, B, Q, T, qmin, qmax, sr, threshold, f0, strength, qstar, voiced};
  hipLaunchKernelGGL(ceps_peaks_kernel, dim3((unsigned)ceil_div(B * T, 256)), dim3(256), 0, (hipStream_t)stream, A);
  SYG_CHECK_LAUNCH("cepstrum_peaks");
  return SYG_OK;
}
