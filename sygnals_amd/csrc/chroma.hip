// Tonal features: the chroma fold of a spectrogram (frame-major) or of a constant-Q transform (bin-major) with librosa's
// threshold and per-frame normalisation, the tonnetz transform, CENS, and the tuning histogram behind estimate_tuning.
// The float64 restatement: tests/chroma_ref.py; the host tables: sygnals_amd/_chroma.py.
//
// fold_rows   x [B, T, F(, 2)], the bins contiguous.  A wave takes a tile of CH_ROW_TILE consecutive frames of one clip,
//             one frame at a time: the lanes run along the bins (256 or 512 contiguous bytes an instruction), each keeps
//             CH_GROUP partial sums over its bins k = lane, lane + 64, ... (ascending, fmaf) against the table
//             [n_chroma, F] that the workgroup has staged in LDS once (read from global memory where it does not fit), then
//             a butterfly over the lanes.  The frame's n_chroma sums go to LDS; at the end of the tile the lanes turn to run
//             along the frames and write 64-byte pieces of four output rows an instruction (the output is 0.6 % of the bytes).
// fold_bins   x [B, K, T(, 2)], the frames contiguous.  A lane takes a frame and keeps all n_chroma sums over the K rows
//             (k ascending, fmaf); the weights wt [K, n_chroma] are uniform over the wave.  No cross-lane step.  After the
//             threshold and the norm an optional transform phi [P, n_chroma] of the L1-normalised frame (tonnetz).
// cens        x [B, n_chroma, T]: a workgroup takes CH_CENS_TILE frames of a clip with a halo of the window's reach; the
//             L1 normalisation and the quantiser per frame into LDS, the smoothing out of LDS (j ascending, fmaf, zeros
//             beyond the row), the closing norm.
// tuning      piptrack's peaks of S [B, T, F(, 2)], a wave a frame, written as (mag float64, residual bin) through one
//             integer counter per clip; then a workgroup per clip selects the exact median of mag by radix selection over
//             the keys' bit patterns (integer histograms in LDS) and counts the bins of the peaks at or above it.
//
// Bits.  Every sum has a fixed order that depends on the frame alone, so a batch equals its rows and a call repeats its
// bits.  The only atomics are integer ones (slot counters, histograms), whose results do not depend on order: the
// order of the peak list does, and nothing reads it but the median selection and the count.
#include "host.h"

#pragma clang fp contract(off)

namespace syg {
namespace {

constexpr int CH_WAVE = 64;
constexpr int CH_NC_MAX = 36;                 // n_chroma served
constexpr int CH_GROUP = 12;                  // chroma rows a lane accumulates side by side (fold_rows)
constexpr int CH_ROW_TILE = 16;               // frames of a wave's tile (fold_rows): 64 bytes of an output row, 4 rows a store
constexpr int CH_ROW_LOADS = 9;               // global loads a lane issues before it waits (fold_rows): 2 rounds at F = 1025
constexpr int CH_ROW_WAVES = 8;               // waves of a fold_rows workgroup at most: they share one staged table
constexpr int64_t CH_TABLE_LDS_MAX = 128 * 1024;   // LDS of a fold_rows workgroup, at most (the table and the tile's sums)
constexpr int CH_BIN_LOADS = 4;               // rows a lane loads before it waits (fold_bins)
constexpr int CH_P_MAX = 8;                   // rows of the output transform
constexpr int CH_CENS_TILE = 256;             // frames of a CENS workgroup
constexpr int CH_CENS_WIN_MAX = 257;          // taps of the smoothing window (win_len_smooth + 2)
constexpr int CH_HIST_BINS_MAX = 1024;
constexpr int64_t CH_MAX_ELEMS = (int64_t)1 << 31;
constexpr double CH_TINY = 1.1754943508222875e-38;  // np.finfo(np.float32).tiny

enum { NORM_NONE = 0, NORM_INF = 1, NORM_L1 = 2, NORM_L2 = 3 };

// |z|^power of an interleaved complex value, the formula of cabs_pow_kernel (fft_generic.hip)
__device__ __forceinline__ float cpow_of(float re, float im, int power) {
  const float p = fmaf(re, re, im * im);
  return power == 2 ? p : sqrtf(p);
}

// librosa.util.normalize's length of v[0 .. n) held one per lane (0 beyond n) in float64; every lane returns it
__device__ __forceinline__ double wave_norm_len(float v, int norm) {
  if (norm == NORM_INF) return (double)wave_max(fabsf(v));                   // a maximum of floats is exact in either width
  const double a = wave_sum_d(norm == NORM_L2 ? (double)v * (double)v : fabs((double)v));
  return norm == NORM_L2 ? sqrt(a) : a;
}

struct RowsArgs {
  const float* x; const float* tab; float* out;
  int64_t B, T, units, tiles;
  int F, nc, cplx, power, has_thr, norm, tab_lds;
  float thr;
};

__global__ __launch_bounds__(CH_WAVE * CH_ROW_WAVES) void chroma_fold_rows_kernel(RowsArgs A) {
  extern __shared__ float ch_smem[];
  const int lane = threadIdx.x & (CH_WAVE - 1), w = threadIdx.x >> 6;
  const int F = A.F, nc = A.nc;
  const int ncp = (nc + CH_GROUP - 1) / CH_GROUP * CH_GROUP;
  const int waves = blockDim.x >> 6;                                        // 2 ... CH_ROW_WAVES: the host's choice by grid size
  float* res = ch_smem + (size_t)w * nc * CH_ROW_TILE;                      // [nc][CH_ROW_TILE] of this wave
  float* tl = ch_smem + (size_t)waves * nc * CH_ROW_TILE;            // [ncp][F], rows beyond nc are zero
  if (A.tab_lds) {
    const int n = nc * F, np = ncp * F;
    for (int i = threadIdx.x; i < np; i += blockDim.x) tl[i] = i < n ? A.tab[i] : 0.f;
  }
  __syncthreads();
  const int64_t u = (int64_t)blockIdx.x * waves + w;
  if (u >= A.units) return;                                                  // (no barrier below)
  const int64_t b = u / A.tiles, ti = u - b * A.tiles;
  const int64_t t0 = ti * CH_ROW_TILE;
  const int nt = (int)(A.T - t0 < CH_ROW_TILE ? A.T - t0 : CH_ROW_TILE);
  for (int tt = 0; tt < nt; ++tt) {
    const float* xr = A.x + ((b * A.T + t0 + tt) * (int64_t)F) * (A.cplx ? 2 : 1);
    float mine = 0.f;                                                        // lane c: the frame's sum of row c
    for (int c0 = 0; c0 < nc; c0 += CH_GROUP) {
      float acc[CH_GROUP];
#pragma unroll
      for (int j = 0; j < CH_GROUP; ++j) acc[j] = 0.f;
      // CH_ROW_LOADS loads in flight a lane: one at a time leaves a frame waiting on memory for every 64 bins
      for (int k0 = lane; k0 < F; k0 += CH_WAVE * CH_ROW_LOADS) {
        float v[CH_ROW_LOADS];
#pragma unroll
        for (int q = 0; q < CH_ROW_LOADS; ++q) {
          const int k = k0 + q * CH_WAVE;
          const int kc = k < F ? k : F - 1;
          if (A.cplx) {
            const float2 z = ((const float2*)xr)[kc];
            v[q] = cpow_of(z.x, z.y, A.power);
          } else {
            v[q] = xr[kc];
          }
        }
#pragma unroll
        for (int q = 0; q < CH_ROW_LOADS; ++q) {
          const int k = k0 + q * CH_WAVE;
          if (k >= F) continue;
          if (A.tab_lds) {
            const float* tp = tl + (size_t)c0 * F + k;
#pragma unroll
            for (int j = 0; j < CH_GROUP; ++j) acc[j] = fmaf(tp[(size_t)j * F], v[q], acc[j]);
          } else {
#pragma unroll
            for (int j = 0; j < CH_GROUP; ++j) {
              const int c = c0 + j < nc ? c0 + j : nc - 1;
              const float wv = A.tab[(size_t)c * F + k];
              acc[j] = fmaf(c0 + j < nc ? wv : 0.f, v[q], acc[j]);
            }
          }
        }
      }
      // CH_GROUP independent wave sums: the compiler interleaves their steps
#pragma unroll
      for (int j = 0; j < CH_GROUP; ++j) {
        const float s = wave_sum(acc[j]);
        if (lane == c0 + j) mine = s;
      }
    }
    if (lane >= nc) mine = 0.f;
    if (A.has_thr && mine < A.thr) mine = 0.f;
    if (A.norm != NORM_NONE) {
      const double len = wave_norm_len(mine, A.norm);
      if (!(len < CH_TINY)) mine = (float)((double)mine / len);
    }
    if (lane < nc) res[lane * CH_ROW_TILE + tt] = mine;
  }
  wave_lds_sync();
  float* ob = A.out + b * (int64_t)nc * A.T + t0;
  for (int i = lane; i < nc * CH_ROW_TILE; i += CH_WAVE) {
    const int c = i / CH_ROW_TILE, tt = i - c * CH_ROW_TILE;
    if (tt < nt) ob[(int64_t)c * A.T + tt] = res[i];
  }
}

struct BinsArgs {
  const float* x; const float* wt; const float* phi; float* out;
  int64_t B, K, T, sxb, sxk;
  int nc, cplx, power, has_thr, norm, P;
  float thr;
};

// NCP: n_chroma rounded up to a size the registers are laid out for; rows beyond nc stay zero
template <int NCP>
__global__ __launch_bounds__(CH_WAVE) void chroma_fold_bins_kernel(BinsArgs A) {
  const int64_t t = (int64_t)blockIdx.x * CH_WAVE + threadIdx.x;
  const int64_t b = blockIdx.y;
  if (t >= A.T) return;
  const int nc = A.nc;
  const float* xb = A.x + b * A.sxb + (A.cplx ? 2 * t : t);
  float acc[NCP];
#pragma unroll
  for (int c = 0; c < NCP; ++c) acc[c] = 0.f;
  for (int64_t k0 = 0; k0 < A.K; k0 += CH_BIN_LOADS) {                        // CH_BIN_LOADS rows in flight a lane
    float v[CH_BIN_LOADS];
#pragma unroll
    for (int q = 0; q < CH_BIN_LOADS; ++q) {
      const int64_t k = k0 + q < A.K ? k0 + q : A.K - 1;
      if (A.cplx) {
        const float2 z = *(const float2*)(xb + k * A.sxk);
        v[q] = cpow_of(z.x, z.y, A.power);
      } else {
        v[q] = xb[k * A.sxk];
      }
    }
#pragma unroll
    for (int q = 0; q < CH_BIN_LOADS; ++q) {
      if (k0 + q >= A.K) break;
      const float* wk = A.wt + (k0 + q) * nc;                                  // uniform over the wave
#pragma unroll
      for (int c = 0; c < NCP; ++c)
        if (c < nc) acc[c] = fmaf(wk[c], v[q], acc[c]);
    }
  }
  if (A.has_thr) {
#pragma unroll
    for (int c = 0; c < NCP; ++c)
      if (acc[c] < A.thr) acc[c] = 0.f;
  }
  if (A.norm != NORM_NONE) {
    double len = 0.0;
#pragma unroll
    for (int c = 0; c < NCP; ++c) {
      const double a = fabs((double)acc[c]);
      if (A.norm == NORM_INF) len = a > len ? a : len;
      else if (A.norm == NORM_L1) len = len + a;
      else len = len + a * a;
    }
    if (A.norm == NORM_L2) len = sqrt(len);
    if (!(len < CH_TINY)) {
#pragma unroll
      for (int c = 0; c < NCP; ++c) acc[c] = (float)((double)acc[c] / len);
    }
  }
  if (A.P == 0) {
    float* ob = A.out + b * (int64_t)nc * A.T + t;
#pragma unroll
    for (int c = 0; c < NCP; ++c)
      if (c < nc) ob[(int64_t)c * A.T] = acc[c];
    return;
  }
  double len = 0.0;
#pragma unroll
  for (int c = 0; c < NCP; ++c) len = len + fabs((double)acc[c]);
  if (!(len < CH_TINY)) {
#pragma unroll
    for (int c = 0; c < NCP; ++c) acc[c] = (float)((double)acc[c] / len);
  }
  float* ob = A.out + b * (int64_t)A.P * A.T + t;
  for (int p = 0; p < A.P; ++p) {
    const float* pp = A.phi + p * nc;
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NCP; ++c)
      if (c < nc) s = fmaf(pp[c], acc[c], s);
    ob[(int64_t)p * A.T] = s;
  }
}

struct CensArgs {
  const float* x; const float* win; float* out;
  int64_t B, T, sxb, sxk, tiles;
  int nc, nw, left, region, norm;
};

// out[c, t] = sum_j win[j] q[c, t - left + j], q = 0 outside [0, T)
__global__ __launch_bounds__(CH_CENS_TILE) void chroma_cens_kernel(CensArgs A) {
  extern __shared__ float ch_smem[];
  __shared__ float wl[CH_CENS_WIN_MAX];
  const int64_t b = blockIdx.x / A.tiles, ti = blockIdx.x - b * A.tiles;
  const int64_t t0 = ti * CH_CENS_TILE;
  const int nt = (int)(A.T - t0 < CH_CENS_TILE ? A.T - t0 : CH_CENS_TILE);
  const int region = A.region, nc = A.nc, nw = A.nw;
  for (int j = threadIdx.x; j < nw; j += blockDim.x) wl[j] = A.win[j];
  const float* xb = A.x + b * A.sxb;
  for (int r = threadIdx.x; r < region; r += blockDim.x) {
    const int64_t t = t0 - A.left + r;
    const bool in = t >= 0 && t < A.T;
    double len = 0.0;
    if (in)
      for (int c = 0; c < nc; ++c) len = len + fabs((double)xb[c * A.sxk + t]);
    const bool unit = len < CH_TINY;
    for (int c = 0; c < nc; ++c) {
      float q = 0.f;
      if (in) {
        const float v = xb[c * A.sxk + t];
        const float n = unit ? v : (float)((double)v / len);
        q = (n > 0.4f ? 0.25f : 0.f) + (n > 0.2f ? 0.25f : 0.f) + (n > 0.1f ? 0.25f : 0.f) + (n > 0.05f ? 0.25f : 0.f);
      }
      ch_smem[c * region + r] = q;
    }
  }
  __syncthreads();
  const int tt = threadIdx.x;
  if (tt >= nt) return;
  double len = 0.0;
  for (int c = 0; c < nc; ++c) {
    const float* qp = ch_smem + c * region + tt;
    float s = 0.f;
    for (int j = 0; j < nw; ++j) s = fmaf(wl[j], qp[j], s);
    const double a = fabs((double)s);
    if (A.norm == NORM_INF) len = a > len ? a : len;
    else if (A.norm == NORM_L1) len = len + a;
    else len = len + a * a;
  }
  if (A.norm == NORM_L2) len = sqrt(len);
  const bool unit = A.norm == NORM_NONE || len < CH_TINY;
  float* ob = A.out + b * (int64_t)nc * A.T + t0 + tt;
  for (int c = 0; c < nc; ++c) {
    const float* qp = ch_smem + c * region + tt;
    float s = 0.f;
    for (int j = 0; j < nw; ++j) s = fmaf(wl[j], qp[j], s);                 // the same sum, the same bits
    ob[(int64_t)c * A.T] = unit ? s : (float)((double)s / len);
  }
}

struct TuneArgs {
  const float* x; const double* edges; double* keys; int* pbin; int* npk; float* pitch_out; float* mag_out;
  int64_t B, T, cap;
  int F, cplx, power, n_fft, k_lo, k_hi, n_bins;
  double sr, threshold, bpo;
};

__device__ __forceinline__ float tune_load(const TuneArgs& A, const float* xr, int k) {
  if (A.cplx) {
    const float2 z = ((const float2*)xr)[k];
    return cpow_of(z.x, z.y, A.power);
  }
  return xr[k];
}

// a wave a frame: the peaks of librosa.piptrack with their float64 (pitch, mag); the list of the clip's admissible peaks
// (mag, residual bin) grows through npk[b]; pitch_out / mag_out (optional) [B, T, F] are the dense float32 pair
__global__ __launch_bounds__(CH_WAVE * 4) void tuning_peaks_kernel(TuneArgs A) {
  const int lane = threadIdx.x & (CH_WAVE - 1);
  const int64_t fr = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (fr >= A.B * A.T) return;
  const int64_t b = fr / A.T;
  const int F = A.F;
  const float* xr = A.x + fr * (int64_t)F * (A.cplx ? 2 : 1);
  float mx = -INFINITY;
#pragma unroll 6
  for (int k = lane; k < F; k += CH_WAVE) {
    const float v = tune_load(A, xr, k);
    mx = v > mx ? v : mx;
  }
  mx = wave_max(mx);
  const double ref = A.threshold * (double)mx;
  for (int k = lane; k < F; k += CH_WAVE) {
    const int km = k > 0 ? k - 1 : 0, kp = k + 1 < F ? k + 1 : F - 1;
    const double s0 = (double)tune_load(A, xr, k), sm = (double)tune_load(A, xr, km), sp = (double)tune_load(A, xr, kp);
    const double x0 = s0 > ref ? s0 : 0.0, xm = sm > ref ? sm : 0.0, xp = sp > ref ? sp : 0.0;
    const bool peak = x0 > xm && x0 >= xp && k >= A.k_lo && k < A.k_hi;
    double pitch = 0.0, mag = 0.0;
    if (peak) {
      double shift = 0.0, avg;
      if (k > 0 && k + 1 < F) {
        const double a = sp + sm - 2.0 * s0, bb = (sp - sm) / 2.0;
        if (fabs(bb) < fabs(a)) shift = -bb / a;
        avg = (sp - sm) / 2.0;
      } else {
        avg = k == 0 ? sp - s0 : s0 - sm;                                    // np.gradient's one-sided edges
      }
      pitch = ((double)k + shift) * A.sr / (double)A.n_fft;
      mag = s0 + 0.5 * avg * shift;
      if (A.keys) {
        double r = A.bpo * log2(pitch / (440.0 / 16.0));
        r = r - floor(r);
        if (r >= 0.5) r = r - 1.0;
        int lo = 0, hi = A.n_bins;                                           // edges[lo] <= r < edges[lo + 1]
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (r >= A.edges[mid]) lo = mid; else hi = mid;
        }
        const int slot = atomicAdd(A.npk + b, 1);
        if (slot < A.cap) {
          A.keys[b * A.cap + slot] = mag;
          A.pbin[b * A.cap + slot] = lo;
        }
      }
    }
    if (A.pitch_out) {
      A.pitch_out[fr * F + k] = (float)pitch;
      A.mag_out[fr * F + k] = (float)mag;
    }
  }
}

__device__ __forceinline__ unsigned long long key_of(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);                       // ascending as unsigned integers
}
__device__ __forceinline__ double value_of(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// the key of rank `rank` (0-based, ascending) among keys[0 .. n): eight passes over a byte each, most significant first
__device__ unsigned long long radix_select(const double* keys, int64_t n, int64_t rank, unsigned int* hist, unsigned long long* pick) {
  unsigned long long prefix = 0, mask = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
      const unsigned long long k = key_of(keys[i]);
      if ((k & mask) == prefix) atomicAdd(hist + (int)((k >> shift) & 255), 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t left = rank;
      int d = 0;
      for (; d < 255; ++d) {
        if (left < (int64_t)hist[d]) break;
        left -= hist[d];
      }
      pick[0] = (unsigned long long)d;
      pick[1] = (unsigned long long)left;
    }
    __syncthreads();
    prefix |= pick[0] << shift;
    mask |= 255ull << shift;
    rank = (int64_t)pick[1];
    __syncthreads();
  }
  return prefix;
}

// a workgroup a clip: th = the exact median of the clip's mags, counts[b, i] = peaks of bin i with mag >= th
__global__ __launch_bounds__(256) void tuning_hist_kernel(const double* __restrict__ keys, const int* __restrict__ pbin,
                                                          const int* __restrict__ npk, int64_t cap, int n_bins, int* counts) {
  __shared__ unsigned int hist[256];
  __shared__ unsigned long long pick[2];
  __shared__ int cnt[CH_HIST_BINS_MAX];
  const int64_t b = blockIdx.x;
  int64_t n = npk[b];
  if (n > cap) n = cap;
  for (int i = threadIdx.x; i < n_bins; i += blockDim.x) cnt[i] = 0;
  __syncthreads();
  if (n > 0) {
    const double* kb = keys + b * cap;
    const double lo = value_of(radix_select(kb, n, (n - 1) / 2, hist, pick));
    const double hi = (n & 1) ? lo : value_of(radix_select(kb, n, n / 2, hist, pick));
    const double th = (lo + hi) / 2.0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x)
      if (kb[i] >= th) atomicAdd(cnt + pbin[b * cap + i], 1);
    __syncthreads();
  }
  for (int i = threadIdx.x; i < n_bins; i += blockDim.x) counts[b * n_bins + i] = cnt[i];
}

int check_fold(const char* who, const float* x, const float* tab, const float* out, int64_t B, int64_t rows, int64_t cols, int nc,
               int cplx, int power, int norm) {
  SYG_REQUIRE(x && tab && out, "%s: null pointer argument (x / table / out)", who);
  SYG_REQUIRE(B >= 1 && rows >= 1 && cols >= 1, "%s: empty input (B = %lld and a spectrogram of %lld x %lld; each must be at least 1)",
              who, (long long)B, (long long)rows, (long long)cols);
  SYG_REQUIRE(nc >= 1 && nc <= CH_NC_MAX, "%s: n_chroma must be in [1, %d] (got %d)", who, CH_NC_MAX, nc);
  SYG_REQUIRE((cplx == 0 || cplx == 1) && (power == 1 || power == 2), "%s: complex must be 0 or 1 and power 1 or 2", who);
  SYG_REQUIRE(!cplx || ((uintptr_t)x & 7) == 0, "%s: a complex input must be aligned to 8 bytes", who);
  SYG_REQUIRE(norm >= NORM_NONE && norm <= NORM_L2, "%s: unknown norm %d (served: 0 none, 1 inf, 2 L1, 3 L2)", who, norm);
  const long double total = (long double)B * (long double)rows * (long double)cols;
  SYG_REQUIRE(total <= (long double)CH_MAX_ELEMS, "%s: an input of %.0Lf elements is above 2^31 = %lld", who, total,
              (long long)CH_MAX_ELEMS);
  return SYG_OK;
}

inline int64_t rows_lds_bytes(int nc, int F, bool table, int waves = CH_ROW_WAVES) {
  const int ncp = (nc + CH_GROUP - 1) / CH_GROUP * CH_GROUP;
  return ((int64_t)waves * nc * CH_ROW_TILE + (table ? (int64_t)ncp * F : 0)) * (int64_t)sizeof(float);
}

inline int64_t tuning_cap(int64_t T, int k_lo, int k_hi) { return T * ((k_hi - k_lo + 1) / 2); }

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_chroma_constants(int key) {
  switch (key) {
    case SYG_CHROMA_NC_MAX: return CH_NC_MAX;
    case SYG_CHROMA_ROW_TILE: return CH_ROW_TILE;
    case SYG_CHROMA_TABLE_LDS_MAX: return CH_TABLE_LDS_MAX;
    case SYG_CHROMA_P_MAX: return CH_P_MAX;
    case SYG_CHROMA_CENS_TILE: return CH_CENS_TILE;
    case SYG_CHROMA_CENS_WIN_MAX: return CH_CENS_WIN_MAX;
    case SYG_CHROMA_HIST_BINS_MAX: return CH_HIST_BINS_MAX;
    case SYG_CHROMA_MAX_ELEMS: return CH_MAX_ELEMS;
    default: return -1;
  }
}

extern "C" int syg_chroma_fold_rows_f32(const float* x, int64_t B, int64_t T, int F, int cplx, int power, const float* tab, int n_chroma,
                                        int has_threshold, float threshold, int norm, float* out, void* stream) {
  const char* who = "chroma_fold_rows";
  if (const int rc = check_fold(who, x, tab, out, B, T, F, n_chroma, cplx, power, norm)) return rc;
  RowsArgs A;
  A.x = x; A.tab = tab; A.out = out; A.B = B; A.T = T; A.F = F; A.nc = n_chroma; A.cplx = cplx; A.power = power;
  A.has_thr = has_threshold ? 1 : 0; A.thr = threshold; A.norm = norm;
  A.tiles = ceil_div(T, CH_ROW_TILE);
  A.units = B * A.tiles;
  A.tab_lds = rows_lds_bytes(n_chroma, F, true) <= CH_TABLE_LDS_MAX;
  // fewer waves a workgroup while the grid would leave CUs idle (one row of 2^24 samples is 1025 tiles): the bits are the same
  const int64_t cus = device_cu_count();
  int waves = CH_ROW_WAVES;
  while (waves > 2 && A.units < 2 * cus * waves) waves >>= 1;
  const size_t lds = (size_t)rows_lds_bytes(n_chroma, F, A.tab_lds != 0, waves);
  if (const int rc = reserve_dynamic_lds(who, (const void*)chroma_fold_rows_kernel, lds)) return rc;
  hipLaunchKernelGGL(chroma_fold_rows_kernel, dim3((unsigned)ceil_div(A.units, waves)), dim3(CH_WAVE * waves), lds,
                     (hipStream_t)stream, A);
  SYG_CHECK_LAUNCH(who);
  return SYG_OK;
}

extern "C" int syg_chroma_fold_bins_f32(const float* x, int64_t B, int64_t K, int64_t T, int64_t sxb, int64_t sxk, int cplx, int power,
                                        const float* wt, int n_chroma, int has_threshold, float threshold, int norm, const float* phi,
                                        int P, float* out, void* stream) {
  const char* who = "chroma_fold_bins";
  if (const int rc = check_fold(who, x, wt, out, B, K, T, n_chroma, cplx, power, norm)) return rc;
  const int64_t w = cplx ? 2 * T : T;
  SYG_REQUIRE(sxb >= 0 && sxk >= 0 && (K == 1 || sxk >= w) && (B == 1 || sxb >= (K - 1) * sxk + w) && (!cplx || (sxb % 2 == 0 && sxk % 2 == 0)),
              "%s: bad input strides (%lld, %lld; in floats, even for complex input) for rows of %lld floats", who, (long long)sxb,
              (long long)sxk, (long long)w);
  SYG_REQUIRE(P >= 0 && P <= CH_P_MAX && (P == 0 || phi), "%s: the output transform must have 0 .. %d rows and a table (got P = %d)",
              who, CH_P_MAX, P);
  SYG_REQUIRE(B <= MAX_GRID_Y, "%s: at most 65535 clips a call (got %lld)", who, (long long)B);
  BinsArgs A;
  A.x = x; A.wt = wt; A.phi = phi; A.out = out; A.B = B; A.K = K; A.T = T; A.sxb = sxb; A.sxk = sxk; A.nc = n_chroma; A.cplx = cplx;
  A.power = power; A.has_thr = has_threshold ? 1 : 0; A.thr = threshold; A.norm = norm; A.P = P;
  const dim3 grid((unsigned)ceil_div(T, CH_WAVE), (unsigned)B);
  if (n_chroma <= 12) hipLaunchKernelGGL(chroma_fold_bins_kernel<12>, grid, dim3(CH_WAVE), 0, (hipStream_t)stream, A);
  else if (n_chroma <= 24) hipLaunchKernelGGL(chroma_fold_bins_kernel<24>, grid, dim3(CH_WAVE), 0, (hipStream_t)stream, A);
  else hipLaunchKernelGGL(chroma_fold_bins_kernel<36>, grid, dim3(CH_WAVE), 0, (hipStream_t)stream, A);
  SYG_CHECK_LAUNCH(who);
  return SYG_OK;
}

extern "C" int syg_chroma_cens_f32(const float* x, int64_t B, int n_chroma, int64_t T, int64_t sxb, int64_t sxk, const float* win, int n_win,
                                   int left, int norm, float* out, void* stream) {
  const char* who = "chroma_cens";
  SYG_REQUIRE(x && win && out, "%s: null pointer argument (x / win / out)", who);
  SYG_REQUIRE(B >= 1 && T >= 1, "%s: empty input (B = %lld, T = %lld; each must be at least 1)", who, (long long)B, (long long)T);
  SYG_REQUIRE(n_chroma >= 1 && n_chroma <= CH_NC_MAX, "%s: n_chroma must be in [1, %d] (got %d)", who, CH_NC_MAX, n_chroma);
  SYG_REQUIRE(norm >= NORM_NONE && norm <= NORM_L2, "%s: unknown norm %d (served: 0 none, 1 inf, 2 L1, 3 L2)", who, norm);
  SYG_REQUIRE(n_win >= 1 && n_win <= CH_CENS_WIN_MAX && left >= 0 && left < n_win,
              "%s: the window must have 1 .. %d taps and 0 <= left < taps (got %d taps, left = %d)", who, CH_CENS_WIN_MAX, n_win, left);
  SYG_REQUIRE(sxb >= 0 && sxk >= 0 && (n_chroma == 1 || sxk >= T) && (B == 1 || sxb >= (n_chroma - 1) * sxk + T),
              "%s: bad input strides (%lld, %lld) for T = %lld", who, (long long)sxb, (long long)sxk, (long long)T);
  const long double total = (long double)B * (long double)n_chroma * (long double)T;
  SYG_REQUIRE(total <= (long double)CH_MAX_ELEMS, "%s: an input of %.0Lf elements is above 2^31 = %lld", who, total,
              (long long)CH_MAX_ELEMS);
  CensArgs A;
  A.x = x; A.win = win; A.out = out; A.B = B; A.T = T; A.sxb = sxb; A.sxk = sxk; A.nc = n_chroma; A.nw = n_win; A.left = left; A.norm = norm;
  A.tiles = ceil_div(T, CH_CENS_TILE);
  A.region = CH_CENS_TILE + n_win - 1;
  SYG_REQUIRE(B * A.tiles < (int64_t)0x7fffffff, "%s: grid too large", who);
  const size_t lds = (size_t)n_chroma * A.region * sizeof(float);
  if (const int rc = reserve_dynamic_lds(who, (const void*)chroma_cens_kernel, lds)) return rc;
  hipLaunchKernelGGL(chroma_cens_kernel, dim3((unsigned)(B * A.tiles)), dim3(CH_CENS_TILE), lds, (hipStream_t)stream, A);
  SYG_CHECK_LAUNCH(who);
  return SYG_OK;
}

extern "C" int64_t syg_tuning_hist_work_bytes(int64_t B, int64_t T, int k_lo, int k_hi) {
  if (B < 1 || T < 1 || k_lo < 0 || k_hi < k_lo) return -1;
  const int64_t cap = tuning_cap(T, k_lo, k_hi);
  return B * cap * 12 + 16;                                                  // keys float64, then bins int32
}

extern "C" int syg_tuning_hist_f32(const float* x, int64_t B, int64_t T, int F, int cplx, int power, double sr, int n_fft, int k_lo,
                                   int k_hi, double threshold, double bins_per_octave, const double* edges, int n_bins, int* counts,
                                   int* n_peaks, float* pitch_out, float* mag_out, void* work, int64_t work_bytes, void* stream) {
  const char* who = "tuning_hist";
  SYG_REQUIRE(x, "%s: null pointer argument (x)", who);
  SYG_REQUIRE(B >= 1 && T >= 1 && F >= 2, "%s: empty input (B = %lld, T = %lld, F = %d; B and T at least 1, F at least 2)", who,
              (long long)B, (long long)T, F);
  SYG_REQUIRE((cplx == 0 || cplx == 1) && (power == 1 || power == 2), "%s: complex must be 0 or 1 and power 1 or 2", who);
  SYG_REQUIRE(!cplx || ((uintptr_t)x & 7) == 0, "%s: a complex input must be aligned to 8 bytes", who);
  SYG_REQUIRE(sr > 0 && n_fft >= 2 && F == 1 + n_fft / 2, "%s: F = %d is not 1 + n_fft / 2 for n_fft = %d (sr must be positive)", who, F,
              n_fft);
  SYG_REQUIRE(k_lo >= 0 && k_lo <= k_hi && k_hi <= F, "%s: the admissible bins [%d, %d) must lie within [0, %d]", who, k_lo, k_hi, F);
  SYG_REQUIRE(threshold >= 0 && threshold == threshold, "%s: threshold must be a number >= 0", who);
  const long double total = (long double)B * (long double)T * (long double)F;
  SYG_REQUIRE(total <= (long double)CH_MAX_ELEMS, "%s: an input of %.0Lf elements is above 2^31 = %lld", who, total,
              (long long)CH_MAX_ELEMS);
  const bool hist = counts != nullptr;
  SYG_REQUIRE(hist || (pitch_out && mag_out), "%s: nothing to write (counts, or pitch_out and mag_out)", who);
  SYG_REQUIRE((pitch_out == nullptr) == (mag_out == nullptr), "%s: pitch_out and mag_out go together", who);
  if (hist) {
    SYG_REQUIRE(n_peaks && edges, "%s: null pointer argument (n_peaks / edges)", who);
    SYG_REQUIRE(n_bins >= 1 && n_bins <= CH_HIST_BINS_MAX, "%s: the histogram must have 1 .. %d bins (got %d)", who, CH_HIST_BINS_MAX,
                n_bins);
    SYG_REQUIRE(bins_per_octave >= 1, "%s: bins_per_octave must be at least 1", who);
    SYG_REQUIRE(work && work_bytes >= syg_tuning_hist_work_bytes(B, T, k_lo, k_hi), "%s: the histogram needs `work` of %lld bytes", who,
                (long long)syg_tuning_hist_work_bytes(B, T, k_lo, k_hi));
    SYG_REQUIRE(((uintptr_t)work & 7) == 0, "%s: `work` must be aligned to 8 bytes", who);
  }
  TuneArgs A;
  A.x = x; A.edges = edges; A.B = B; A.T = T; A.F = F; A.cplx = cplx; A.power = power; A.n_fft = n_fft; A.k_lo = k_lo; A.k_hi = k_hi;
  A.n_bins = n_bins; A.sr = sr; A.threshold = threshold; A.bpo = bins_per_octave; A.pitch_out = pitch_out; A.mag_out = mag_out;
  A.cap = tuning_cap(T, k_lo, k_hi);
  A.keys = hist ? (double*)work : nullptr;
  A.pbin = hist ? (int*)((double*)work + B * A.cap) : nullptr;
  A.npk = n_peaks;
  if (hist) {
    const hipError_t e = hipMemsetAsync(n_peaks, 0, (size_t)B * sizeof(int), (hipStream_t)stream);
    if (e != hipSuccess) {
      set_error("%s: cannot clear the peak counters: %s", who, hipGetErrorString(e));
      return SYG_E_LAUNCH;
    }
  }
  hipLaunchKernelGGL(tuning_peaks_kernel, dim3((unsigned)ceil_div(B * T, 4)), dim3(CH_WAVE * 4), 0, (hipStream_t)stream, A);
  SYG_CHECK_LAUNCH(who);
  if (hist) {
    hipLaunchKernelGGL(tuning_hist_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, A.keys, A.pbin, A.npk, A.cap, n_bins,
                       counts);
    SYG_CHECK_LAUNCH(who);
  }
  return SYG_OK;
}
