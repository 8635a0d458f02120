// Per-channel energy normalisation (librosa.pcen) of S [B, M, T] float32 rows, frames fastest, one smoother per (b, m) row:
//   ref = S, or the running maximum of max_size bands (scipy.ndimage.maximum_filter1d, mode reflect, origin 0)
//   y[0] = b ref[0] + z,  y[t] = y[t-1] + b (ref[t] - y[t-1]),  z' = (1 - b) y[T-1]     (scipy.signal.lfilter's state)
//   out  = the pointwise law of (S, y): pcen_law below.
//
// The smoother state is float64 in a register and is rounded to float32 once per frame for the pointwise law, which is
// float32.  (Carried in float32 as b x + (1 - b) y it drifts by 1e-4 of a row's peak at b = 1e-4.)
//
// Resident form: a workgroup holds up to PCEN_BANDS consecutive bands of one clip plus the max_size - 1 halo bands
// (reflected at the band edges) in LDS, loaded and stored coalesced along T; a lane runs one row's recurrence out of
// LDS (row stride odd: no bank collisions) and the running maximum is taken from the same tile; all lanes then apply
// the law.  Tiled form: a wave takes PCEN_TILE frames of one row, cut by frame index alone; a lane runs 16 consecutive
// frames, the lanes' affine maps (a, c) are composed by a wave scan, and with more than one tile a row a first launch
// leaves every tile's closing state from rest in `work`; the second launch folds those in index order.
// No atomics: the same call repeats its bits and a batch equals its rows.
#include "host.h"

#include <math.h>

#pragma clang fp contract(off)

namespace syg {
namespace {

constexpr int PCEN_WAVE = 64;
constexpr int PCEN_THREADS = 256;
constexpr int PCEN_UNITS = PCEN_THREADS / PCEN_WAVE;   // tiles (waves) of a workgroup of the tiled form
constexpr int PCEN_BANDS = 64;                         // bands of a workgroup of the resident form, at most
constexpr int PCEN_TILE = 1024;                        // frames of a tile of the tiled form
constexpr int PCEN_RUN = PCEN_TILE / PCEN_WAVE;        // consecutive frames of a lane
constexpr int PCEN_TILE_LDS = PCEN_TILE + PCEN_TILE / PCEN_RUN;   // a word of padding after every run: lane stride 17
constexpr int64_t PCEN_LDS_MAX = 80 * 1024;            // LDS of a workgroup: two fit a CU's 160 KiB
constexpr int PCEN_PRM = 8;                            // float32 words a band's law takes in LDS
constexpr int64_t PCEN_RESIDENT_T = 155;               // longest row of which PCEN_BANDS bands (no halo) fit PCEN_LDS_MAX
constexpr int PCEN_GRID_MAX = 4096;                    // workgroups of a launch, at most: each loops over its share
constexpr int64_t PCEN_MAX_OUT = (int64_t)1 << 31;

// row stride in LDS: odd, so that lanes on consecutive rows at one frame hit distinct banks
constexpr int64_t padded(int64_t T) { return T | 1; }
constexpr int64_t resident_bytes(int64_t rows, int64_t halo, int64_t T) {
  return ((2 * rows + halo) * padded(T) + rows * PCEN_PRM) * 4;
}
static_assert(resident_bytes(PCEN_BANDS, 0, PCEN_RESIDENT_T) <= PCEN_LDS_MAX, "the resident limit does not fit");
static_assert(resident_bytes(PCEN_BANDS, 0, PCEN_RESIDENT_T + 1) > PCEN_LDS_MAX, "the resident limit is not the largest");
static_assert(PCEN_UNITS * 2 * PCEN_TILE_LDS * 4 <= PCEN_LDS_MAX, "the tiled form's LDS");

// a band's parameters as the kernels read them (tab: [M] of these; sygnals_amd/_pcen.py packs it)
struct PcenBand { double b, a_tile, eps, gain, power, bias, bias_pow, mode; };
enum { LAW_GENERAL = 0, LAW_POWER0 = 1, LAW_BIAS0 = 2 };

struct PcenArgs {
  const float* x; float* out; const PcenBand* tab; const double* zi; double* zf; double* work;
  PcenBand sc;
  double scale;
  int64_t sxb, sxk, sob, sok, B, M, T, tiles, units;
  int ms, left, rows, pass;
  float inv_T;
};

__device__ __forceinline__ PcenBand band_of(const PcenArgs& A, int64_t k) { return A.tab ? A.tab[k] : A.sc; }

// scipy's reflect: (d c b a | a b c d | d c b a); max_size <= M keeps one reflection enough
__device__ __forceinline__ int64_t reflect(int64_t k, int64_t M) { return k < 0 ? -k - 1 : (k >= M ? 2 * M - 1 - k : k); }

__device__ __forceinline__ float load_scaled(const float* p, double scale) { return (float)((double)(*p) * scale); }

// smooth = exp(-gain log(eps + m)) (= exp(-gain (log eps + log1p(m / eps))), one rounding less); then librosa's three cases
__device__ __forceinline__ float pcen_law(float s, float m, float gain, float bias, float power, float eps, float bias_pow, int mode) {
  const float ls = -gain * logf(eps + m);
  if (mode == LAW_BIAS0) return expf(power * (logf(s) + ls));       // s = 0: exp(-inf) = 0 exactly
  const float r = s * expf(ls);
  if (mode == LAW_POWER0) return log1pf(r);
  return bias_pow * expm1f(power * log1pf(r / bias));
}

// e = j * T + t with 0 <= t < T, for e < 2^22: a float quotient and one correction either way
__device__ __forceinline__ void split(int e, int T, float inv_T, int& j, int& t) {
  j = (int)((float)e * inv_T);
  t = e - j * T;
  if (t < 0) { --j; t += T; }
  else if (t >= T) { ++j; t -= T; }
}

__global__ __launch_bounds__(PCEN_THREADS) void pcen_resident_kernel(PcenArgs A) {
  extern __shared__ float pcen_smem[];
  const int T = (int)A.T, Tp = (int)padded(A.T), R = A.rows, halo = A.ms - 1;
  float* xs = pcen_smem;                               // [R + halo][Tp]: S, row 0 is band k0 - left
  float* ys = xs + (size_t)(R + halo) * Tp;            // [R][Tp]: the smoother
  float* prm = ys + (size_t)R * Tp;                    // [R][PCEN_PRM]
  const int tid = threadIdx.x;
  const int64_t per_clip = (A.M + R - 1) / R;
  for (int64_t w = blockIdx.x; w < A.units; w += gridDim.x) {
    const int64_t b = w / per_clip, k0 = (w - b * per_clip) * R;
    const int live = (int)(A.M - k0 < R ? A.M - k0 : R);
    const float* xb = A.x + b * A.sxb;
    const int n_in = (live + halo) * T;
    for (int e = tid; e < n_in; e += PCEN_THREADS) {
      int j, t;
      split(e, T, A.inv_T, j, t);
      const int64_t k = reflect(k0 - A.left + j, A.M);
      xs[j * Tp + t] = load_scaled(xb + k * A.sxk + t, A.scale);
    }
    double y = 0.0, a = 0.0, bb = 0.0;
    if (tid < live) {
      const PcenBand P = band_of(A, k0 + tid);
      float* p = prm + tid * PCEN_PRM;
      p[0] = (float)P.gain; p[1] = (float)P.bias; p[2] = (float)P.power; p[3] = (float)P.eps; p[4] = (float)P.bias_pow;
      p[5] = (float)P.mode;
      bb = P.b; a = 1.0 - P.b;
    }
    __syncthreads();
#if defined(SYG_PCEN_WAVE_ROW)
    // The mapping the measurement dropped, kept for the A/B: a wave a row, a run of frames a lane, the
    // runs' affine maps composed by a wave scan.  A build with it reports itself through syg_build_variant().
    for (int j = tid >> 6; j < live; j += PCEN_THREADS / PCEN_WAVE) {
      const int lane = tid & (PCEN_WAVE - 1);
      const PcenBand P = band_of(A, k0 + j);
      const double wb = P.b, wa = 1.0 - P.b;
      const double z = A.zi ? A.zi[b * A.M + k0 + j] : wa;
      const int run = (T + PCEN_WAVE - 1) / PCEN_WAVE, i0 = lane * run;
      const int len = T - i0 < 0 ? 0 : (T - i0 < run ? T - i0 : run);
      const float* xr = xs + j * Tp + i0;
      float* yr = ys + j * Tp + i0;
      double ak = 1.0, c = 0.0;
      for (int q = 0; q < len; ++q) {
        float r = xr[q];
        for (int h = 1; h <= halo; ++h) r = fmaxf(r, xr[h * Tp + q]);
        yr[q] = r;
        c = q ? fma(wb, (double)r - c, c) : fma(wb, (double)r, lane == 0 ? z : 0.0);
        ak = ak * wa;
      }
#pragma unroll
      for (int d = 1; d < PCEN_WAVE; d <<= 1) {
        const double pa = __shfl_up(ak, d), pc = __shfl_up(c, d);
        if (lane >= d) { c = fma(ak, pc, c); ak = ak * pa; }
      }
      const double y_in = __shfl_up(c, 1);
      double yw = 0.0;
      for (int q = 0; q < len; ++q) {
        const double v = (double)yr[q];
        yw = q ? fma(wb, v - yw, yw) : fma(wb, v, lane == 0 ? z : wa * y_in);
        yr[q] = (float)yw;
      }
      if (A.zf && len > 0 && i0 + len == T) A.zf[b * A.M + k0 + j] = wa * yw;
    }
#else
    if (tid < live) {                                  // a lane a row, frame by frame out of LDS
      const double z = A.zi ? A.zi[b * A.M + k0 + tid] : a;
      const float* xr = xs + tid * Tp;
      float* yr = ys + tid * Tp;
      for (int t = 0; t < T; ++t) {
        float r = xr[t];
        for (int q = 1; q <= halo; ++q) r = fmaxf(r, xr[q * Tp + t]);
        const double v = (double)r;
        y = t ? fma(bb, v - y, y) : fma(bb, v, z);
        yr[t] = (float)y;
      }
      if (A.zf) A.zf[b * A.M + k0 + tid] = a * y;
    }
#endif
    __syncthreads();
    float* ob = A.out + b * A.sob + k0 * A.sok;
    const int n_out = live * T;
    for (int e = tid; e < n_out; e += PCEN_THREADS) {
      int j, t;
      split(e, T, A.inv_T, j, t);
      const float* p = prm + j * PCEN_PRM;
      ob[(int64_t)j * A.sok + t] = pcen_law(xs[(j + A.left) * Tp + t], ys[j * Tp + t], p[0], p[1], p[2], p[3], p[4], (int)p[5]);
    }
    __syncthreads();                                   // the next share's loads write the tile again
  }
}

// index of frame i of a tile in LDS
__device__ __forceinline__ int slot(int i) { return i + i / PCEN_RUN; }

// pass 0: work[row][tile] = the tile's closing y from rest (z = 0).  pass 1: the output and zf; with more than one tile a
// row the incoming z is folded from work in index order: z' = a^PCEN_TILE z + a y_rest.
__global__ __launch_bounds__(PCEN_THREADS) void pcen_tiled_kernel(PcenArgs A) {
  __shared__ float pcen_tile[PCEN_UNITS][2][PCEN_TILE_LDS];
  const int lane = threadIdx.x & (PCEN_WAVE - 1), w = threadIdx.x >> 6;
  float* ss = pcen_tile[w][0];
  float* rs = pcen_tile[w][1];
  for (int64_t base = (int64_t)blockIdx.x * PCEN_UNITS; base < A.units; base += (int64_t)gridDim.x * PCEN_UNITS) {
    int64_t u = base + w;
    const bool live = u < A.units;                     // a spare wave repeats the last unit and stores nothing
    if (!live) u = A.units - 1;
    const int64_t row = u / A.tiles, ti = u - row * A.tiles;
    const int64_t b = row / A.M, k = row - b * A.M;
    const int64_t t0 = ti * PCEN_TILE;
    const int n = (int)(A.T - t0 < PCEN_TILE ? A.T - t0 : PCEN_TILE);
    const float* xb = A.x + b * A.sxb + t0;
    const PcenBand P = band_of(A, k);
    const double bb = P.b, a = 1.0 - P.b;
    for (int i = lane; i < n; i += PCEN_WAVE) {
      const float s = load_scaled(xb + k * A.sxk + i, A.scale);
      float r = s;
      if (A.ms > 1)                                    // the neighbouring bands come from global memory (L2)
        for (int q = 0; q < A.ms; ++q) r = fmaxf(r, load_scaled(xb + reflect(k - A.left + q, A.M) * A.sxk + i, A.scale));
      ss[slot(i)] = s;
      rs[slot(i)] = r;
    }
    double z = 0.0;
    if (A.pass) {
      z = A.zi ? A.zi[row] : a;
      const double* wk = A.work + row * A.tiles;
      for (int64_t c0 = 0; c0 < ti; c0 += PCEN_WAVE) {
        const double v = c0 + lane < ti ? wk[c0 + lane] : 0.0;
        const int cnt = (int)(ti - c0 < PCEN_WAVE ? ti - c0 : PCEN_WAVE);
        for (int j = 0; j < cnt; ++j) z = fma(P.a_tile, z, a * __shfl(v, j));
      }
    }
    __syncthreads();
    const int i0 = lane * PCEN_RUN;
    const int len = n - i0 < 0 ? 0 : (n - i0 < PCEN_RUN ? n - i0 : PCEN_RUN);
    const float* run = rs + slot(i0);
    // the lane's run as an affine map of the y in front of it: y_end = ak y_in + c (lane 0 takes z, not a y_in)
    double ak = 1.0, c = 0.0;
    for (int q = 0; q < len; ++q) {
      const double v = (double)run[q];
      c = q ? fma(bb, v - c, c) : fma(bb, v, lane == 0 ? z : 0.0);
      ak = ak * a;
    }
#pragma unroll
    for (int d = 1; d < PCEN_WAVE; d <<= 1) {
      const double pa = __shfl_up(ak, d), pc = __shfl_up(c, d);
      if (lane >= d) { c = fma(ak, pc, c); ak = ak * pa; }
    }
    if (!A.pass) {
      if (live && lane == PCEN_WAVE - 1) A.work[u] = c;
    } else {
      const double y_in = __shfl_up(c, 1);             // the y that closes the lanes in front
      double y = 0.0;
      float* dst = rs + slot(i0);
      for (int q = 0; q < len; ++q) {
        const double v = (double)dst[q];
        y = q ? fma(bb, v - y, y) : fma(bb, v, lane == 0 ? z : a * y_in);
        dst[q] = (float)y;
      }
      if (live && A.zf && len > 0 && t0 + i0 + len == A.T) A.zf[row] = a * y;
    }
    __syncthreads();
    if (A.pass && live) {
      float* o = A.out + b * A.sob + k * A.sok + t0;
      const float gain = (float)P.gain, bias = (float)P.bias, power = (float)P.power, eps = (float)P.eps, bp = (float)P.bias_pow;
      const int mode = (int)P.mode;
      for (int i = lane; i < n; i += PCEN_WAVE) o[i] = pcen_law(ss[slot(i)], rs[slot(i)], gain, bias, power, eps, bp, mode);
    }
    __syncthreads();
  }
}

inline int64_t span(int64_t B, int64_t K, int64_t T, int64_t sb, int64_t sk) { return (B - 1) * sb + (K - 1) * sk + T; }

inline bool overlaps(const float* a, int64_t na, const float* b, int64_t nb) { return a < b + nb && b < a + na; }

// bands of a resident workgroup at this T and max_size: 0 if not even one fits
inline int64_t resident_rows(int64_t T, int64_t M, int64_t max_size) {
  const int64_t halo = max_size - 1, Tp = padded(T);
  const int64_t room = PCEN_LDS_MAX / 4 - halo * Tp;
  if (room <= 0) return 0;
  int64_t r = room / (2 * Tp + PCEN_PRM);
  if (r > PCEN_BANDS) r = PCEN_BANDS;
  return r > M ? M : r;
}

// 0 resident, 1 tiled: the library's rule
inline int form_rule(int64_t T, int64_t M, int64_t max_size) {
  return T <= PCEN_RESIDENT_T && resident_rows(T, M, max_size) >= 1 ? 0 : 1;
}

inline bool finite_d(double v) { return v - v == 0.0; }

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_pcen_constants(int key) {
  switch (key) {
    case SYG_PCEN_TILE: return PCEN_TILE;
    case SYG_PCEN_BANDS: return PCEN_BANDS;
    case SYG_PCEN_RESIDENT_T: return PCEN_RESIDENT_T;
    case SYG_PCEN_LDS_MAX: return PCEN_LDS_MAX;
    case SYG_PCEN_GRID_MAX: return PCEN_GRID_MAX;
    case SYG_PCEN_UNITS: return PCEN_UNITS;
    case SYG_PCEN_MAX_OUT: return PCEN_MAX_OUT;
    case SYG_PCEN_TABLE_WORDS: return (int64_t)(sizeof(PcenBand) / sizeof(double));
    default: return -1;
  }
}

extern "C" int syg_pcen_form(int64_t T, int64_t M, int64_t max_size) {
  if (T < 1 || M < 1 || max_size < 1 || max_size > M) return -1;
  return form_rule(T, M, max_size);
}

extern "C" int64_t syg_pcen_work_bytes(int64_t B, int64_t M, int64_t T) {
  if (B < 1 || M < 1 || T < 1) return -1;
  const int64_t tiles = ceil_div(T, PCEN_TILE);
  return tiles > 1 ? B * M * tiles * (int64_t)sizeof(double) : 0;
}

extern "C" int syg_pcen_f32(const float* x, int64_t B, int64_t M, int64_t T, int64_t sxb, int64_t sxk, float* out, int64_t sob,
                            int64_t sok, double gain, double bias, double power, double eps, double b, const double* tab,
                            int64_t max_size, double scale, const double* zi, double* zf, int form, void* work, int64_t work_bytes,
                            void* stream) {
  const char* who = "pcen";
  SYG_REQUIRE(x && out, "%s: null pointer argument (x / out)", who);
  SYG_REQUIRE(B >= 1 && M >= 1 && T >= 1, "%s: empty input (B = %lld, M = %lld, T = %lld; each must be at least 1)", who, (long long)B,
              (long long)M, (long long)T);
  SYG_REQUIRE(sxb >= 0 && sxk >= 0 && (M == 1 || sxk >= T || sxk == 0), "%s: bad input strides (%lld, %lld) for T = %lld", who,
              (long long)sxb, (long long)sxk, (long long)T);
  SYG_REQUIRE(sok >= T && sob >= M * sok - (sok - T), "%s: bad output strides (%lld, %lld) for %lld rows of T = %lld", who,
              (long long)sob, (long long)sok, (long long)M, (long long)T);
  const long double total = (long double)B * (long double)M * (long double)T;
  SYG_REQUIRE(total <= (long double)PCEN_MAX_OUT, "%s: a result of %.0Lf elements is above 2^31 = %lld", who, total,
              (long long)PCEN_MAX_OUT);
  if (!tab) {                                          // a table's values are its maker's to check (sygnals_amd/_pcen.py)
    SYG_REQUIRE(gain >= 0.0 && finite_d(gain), "%s: gain must be non-negative (got %g)", who, gain);
    SYG_REQUIRE(bias >= 0.0 && finite_d(bias), "%s: bias must be non-negative (got %g)", who, bias);
    SYG_REQUIRE(power >= 0.0 && finite_d(power), "%s: power must be non-negative (got %g)", who, power);
    SYG_REQUIRE(eps > 0.0 && finite_d(eps), "%s: eps must be strictly positive (got %g)", who, eps);
    SYG_REQUIRE(b > 0.0 && b <= 1.0, "%s: b must be in (0, 1] (got %g)", who, b);
  }
  SYG_REQUIRE(max_size >= 1 && max_size <= M, "%s: max_size must be an integer in [1, M = %lld] (got %lld)", who, (long long)M,
              (long long)max_size);
  SYG_REQUIRE(scale > 0.0 && finite_d(scale), "%s: scale must be positive and finite (got %g)", who, scale);
  SYG_REQUIRE(form >= 0 && form <= 2, "%s: form must be 0 (the rule), 1 (resident) or 2 (tiled)", who);
  const bool alias = out == x && sob == sxb && sok == sxk;
  SYG_REQUIRE((alias && max_size == 1) || !overlaps(x, span(B, M, T, sxb, sxk), out, span(B, M, T, sob, sok)),
              "%s: out overlaps x (only out = x itself with max_size = 1 is served: neighbouring bands are read)", who);
  const int tiled = form ? form - 1 : form_rule(T, M, max_size);

  PcenArgs A;
  A.x = x; A.out = out; A.tab = (const PcenBand*)tab; A.zi = zi; A.zf = zf; A.work = (double*)work;
  A.sc.b = b; A.sc.a_tile = pow(1.0 - b, (double)PCEN_TILE); A.sc.eps = eps; A.sc.gain = gain; A.sc.power = power; A.sc.bias = bias;
  A.sc.bias_pow = pow(bias, power);
  A.sc.mode = power == 0.0 ? LAW_POWER0 : (bias == 0.0 ? LAW_BIAS0 : LAW_GENERAL);
  A.scale = scale;
  A.sxb = sxb; A.sxk = sxk; A.sob = sob; A.sok = sok; A.B = B; A.M = M; A.T = T;
  A.ms = (int)max_size; A.left = (int)(max_size / 2); A.inv_T = 1.0f / (float)T;
  if (!tiled) {
    const int64_t rows = resident_rows(T, M, max_size);
    SYG_REQUIRE(rows >= 1, "%s: a row of T = %lld with max_size = %lld does not fit the resident form (%lld B of LDS a band, at most %lld)",
                who, (long long)T, (long long)max_size, (long long)resident_bytes(1, max_size - 1, T), (long long)PCEN_LDS_MAX);
    const size_t lds = (size_t)resident_bytes(rows, max_size - 1, T);
    if (const int rc = reserve_dynamic_lds(who, (const void*)pcen_resident_kernel, lds)) return rc;
    A.rows = (int)rows; A.tiles = 1; A.units = B * ceil_div(M, rows); A.pass = 1;
    const int64_t grid = A.units < PCEN_GRID_MAX ? A.units : PCEN_GRID_MAX;
    hipLaunchKernelGGL(pcen_resident_kernel, dim3((unsigned)grid), dim3(PCEN_THREADS), lds, (hipStream_t)stream, A);
    SYG_CHECK_LAUNCH(who);
    return SYG_OK;
  }
  A.rows = 0; A.tiles = ceil_div(T, PCEN_TILE); A.units = B * M * A.tiles;
  if (A.tiles > 1)
    SYG_REQUIRE(work && work_bytes >= syg_pcen_work_bytes(B, M, T), "%s: rows of more than one tile need `work` of %lld bytes", who,
                (long long)syg_pcen_work_bytes(B, M, T));
  const int64_t blocks = ceil_div(A.units, PCEN_UNITS);
  const int64_t grid = blocks < PCEN_GRID_MAX ? blocks : PCEN_GRID_MAX;
  for (int pass = A.tiles > 1 ? 0 : 1; pass < 2; ++pass) {
    A.pass = pass;
    hipLaunchKernelGGL(pcen_tiled_kernel, dim3((unsigned)grid), dim3(PCEN_THREADS), 0, (hipStream_t)stream, A);
    SYG_CHECK_LAUNCH(who);
  }
  return SYG_OK;
}
