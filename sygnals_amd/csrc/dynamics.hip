// Feature dynamics along T of [B, K, T] float32 rows (frames fastest): CMVN (global or Kaldi's centred sliding window),
// Savitzky-Golay deltas (librosa.feature.delta = scipy.signal.savgol_filter) and context stacking.
//
// One kernel serves cmvn, delta and their fusion.  A UNIT is one wave's work: a row's frames [t0, t1) with the region
// [t0 - halo, t1 + halo) (clipped to the row) in LDS.  Resident form: the unit is the whole row.  Tiled form: the row is
// cut every DYN_TILE frames; the halo is `width` frames for the deltas (the interp edge frames read the first / last
// `width` samples, which a halo of width always covers) plus W frames for a sliding window.  A workgroup is up to four
// waves, each with a unit of its own: at T = 65 four rows share a workgroup and its lanes, at T = 3001 three workgroups
// share a CU's LDS.
//
// Bits.  A delta frame is one float32 dot product, j ascending, of values that do not depend on the cut: both forms
// give the same bits.  Global statistics are float64 sums over chunks of DYN_TILE frames cut by frame index alone
// (chunk_sum: lane-strided, then a butterfly), combined in index order; the resident form sums the same chunks out of
// LDS that the tiled form's first two launches sum out of global memory, so the forms agree bit for bit there too.
// Sliding statistics: W <= DYN_DIRECT_W sums every window explicitly (W = 1 is exact); above it float64 prefix sums of
// x and x^2 over the unit's region, which start where the region starts, so the forms may differ in the last bits of
// float64 (at most 2 ulp of the float32 result).  No atomics.
#include "host.h"

#pragma clang fp contract(off)

namespace syg {
namespace {

constexpr int DYN_WAVE = 64;
constexpr int DYN_UNITS = 4;                  // waves (units) of a workgroup, at most
constexpr int DYN_FRAMES = 4;                 // interior frames a lane filters side by side
constexpr int DYN_LOADS = 8;                  // global loads a lane issues before it waits
constexpr int DYN_TILE = 1024;                // frames of a tile, and of a chunk of the global sums
constexpr int DYN_WIDTH_MAX = 255;
constexpr int DYN_ORDER_MAX = 4;
constexpr int DYN_DIRECT_W = 32;              // sliding windows up to this are summed explicitly
constexpr int DYN_WINDOW_MAX = 1024;          // longest sliding window below T
constexpr int64_t DYN_RESIDENT_T = 3072;      // longest resident row (4 bytes a frame, 4 units in 48 KiB)
constexpr int64_t DYN_RESIDENT_T_SLIDING = 2048;  // 20 bytes a frame with the prefix sums: one unit in 40 KiB
constexpr int64_t DYN_LDS_SHARED = 64 * 1024; // LDS of a workgroup that up to four units share
constexpr int64_t DYN_LDS_MAX = 80 * 1024;    // LDS of a workgroup of one unit: two workgroups a CU (160 KiB)
constexpr int64_t DYN_MAX_OUT = (int64_t)1 << 31;
constexpr double DYN_VAR_FLOOR = 1e-20;

enum { MODE_INTERP = 0, MODE_NEAREST = 1, MODE_MIRROR = 2, MODE_WRAP = 3, MODE_CONSTANT = 4 };

struct DynArgs {
  const float* x; float* out; const float* tab; const double* part;
  int64_t sxb, sxk, sob, sok, B, K, T, W, tiles, units, unit_bytes;
  int tile, halo, region, cm, variance, statics, nd, width, mode, resident, direct;
  float cval;
};

// float64 sum of p[0 .. n) (sq: of (p[i] - m)^2): lane-strided partial sums, then a butterfly; every lane returns it
__device__ __forceinline__ double chunk_sum(const float* p, int n, int lane, double m, bool sq) {
  double a = 0.0;
  for (int i = lane; i < n; i += DYN_WAVE) {
    double v = (double)p[i];
    if (sq) { v = v - m; v = v * v; }
    a = a + v;
  }
  return wave_sum_d(a);
}

// Kaldi's centred window of frame t: [s, e)
__device__ __forceinline__ void window_of(int64_t t, int64_t W, int64_t T, int64_t& s, int64_t& e) {
  s = t - W / 2; e = s + W;
  if (s < 0) { e -= s; s = 0; }
  if (e > T) { s -= e - T; e = T; }
  if (s < 0) s = 0;
}

// index of the row that position idx (outside [0, T)) stands for; -1: the constant
__device__ __forceinline__ int64_t map_index(int64_t idx, int64_t T, int mode) {
  if (idx >= 0 && idx < T) return idx;
  if (mode == MODE_NEAREST) return idx < 0 ? 0 : T - 1;
  if (mode == MODE_WRAP) { int64_t r = idx % T; return r < 0 ? r + T : r; }
  if (mode == MODE_MIRROR) {
    if (T == 1) return 0;
    const int64_t p = 2 * (T - 1);
    int64_t r = idx % p;
    if (r < 0) r += p;
    return r < T ? r : p - r;
  }
  return -1;
}

// work: part [rows][2][tiles] float64, then stat [rows][2].  Pass 0 writes the chunk sums of x, pass 1 those of (x - m)^2
// with m = stat[row][0]; dyn_combine_kernel turns a pass's chunk sums into stat[row][pass] = their sum in index order / T.
__global__ __launch_bounds__(DYN_WAVE * DYN_UNITS) void dyn_stats_kernel(const float* __restrict__ x, int64_t sxb, int64_t sxk, int64_t K,
                                                                         int64_t T, int64_t tiles, int64_t units, double* part,
                                                                         const double* stat, int pass) {
  const int lane = threadIdx.x & (DYN_WAVE - 1);
  const int64_t u = (int64_t)blockIdx.x * DYN_UNITS + (threadIdx.x >> 6);
  if (u >= units) return;
  const int64_t row = u / tiles, c = u - row * tiles;
  const int64_t b = row / K, k = row - b * K;
  const float* xr = x + b * sxb + k * sxk;
  const int64_t t0 = c * DYN_TILE;
  const int n = (int)(T - t0 < DYN_TILE ? T - t0 : DYN_TILE);
  const double m = pass ? stat[row * 2] : 0.0;
  const double s = chunk_sum(xr + t0, n, lane, m, pass != 0);
  if (lane == 0) part[(row * 2 + pass) * tiles + c] = s;
}

// one wave a row: 64 chunk sums at a time into the lanes, added one by one in index order
__global__ __launch_bounds__(DYN_WAVE * DYN_UNITS) void dyn_combine_kernel(const double* __restrict__ part, int64_t tiles, int64_t rows,
                                                                           int64_t T, double* stat, int pass) {
  const int lane = threadIdx.x & (DYN_WAVE - 1);
  const int64_t row = (int64_t)blockIdx.x * DYN_UNITS + (threadIdx.x >> 6);
  if (row >= rows) return;
  const double* pr = part + (row * 2 + pass) * tiles;
  double s = 0.0;
  for (int64_t base = 0; base < tiles; base += DYN_WAVE) {
    const double v = base + lane < tiles ? pr[base + lane] : 0.0;
    const int cnt = (int)(tiles - base < DYN_WAVE ? tiles - base : DYN_WAVE);
    for (int j = 0; j < cnt; ++j) s = s + __shfl(v, j);
  }
  if (lane == 0) stat[row * 2 + pass] = s / (double)T;
}

__global__ __launch_bounds__(DYN_WAVE * DYN_UNITS) void dyn_kernel(DynArgs A) {
  extern __shared__ double dyn_smem[];
  const int lane = threadIdx.x & (DYN_WAVE - 1), w = threadIdx.x >> 6;
  int64_t u = (int64_t)blockIdx.x * (blockDim.x >> 6) + w;
  const bool live = u < A.units;                // a spare wave repeats the last unit and stores nothing: barriers stay uniform
  if (!live) u = A.units - 1;
  const int64_t row = u / A.tiles, ti = u - row * A.tiles;
  const int64_t b = row / A.K, k = row - b * A.K;
  const float* xr = A.x + b * A.sxb + k * A.sxk;
  const int64_t T = A.T, t0 = ti * A.tile;
  const int64_t t1 = T - t0 < A.tile ? T : t0 + A.tile;
  const int64_t lo = t0 - A.halo > 0 ? t0 - A.halo : 0;
  const int64_t hi = T - t1 < A.halo ? T : t1 + A.halo;
  const int n = (int)(hi - lo);
  char* base = (char*)dyn_smem + (size_t)w * A.unit_bytes;
  const bool prefix = A.cm == 2 && !A.direct;
  double* S = (double*)base;
  double* Q = S + A.region + 1;
  float* xs = (float*)(base + (prefix ? (size_t)(2 * (A.region + 1)) * 8 : 0));
  float* ys = (A.cm == 2 && A.direct) ? xs + A.region : xs;

  // DYN_LOADS loads in flight a lane: with one, a CU's few resident waves leave HBM idle
  for (int i0 = lane; i0 < n; i0 += DYN_WAVE * DYN_LOADS) {
    float v[DYN_LOADS];
#pragma unroll
    for (int q = 0; q < DYN_LOADS; ++q) {
      const int i = i0 + q * DYN_WAVE;
      v[q] = i < n ? xr[lo + i] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < DYN_LOADS; ++q) {
      const int i = i0 + q * DYN_WAVE;
      if (i < n) xs[i] = v[q];
    }
  }
  __syncthreads();

  if (A.cm == 1) {
    double m, inv = 1.0;
    if (A.resident) {                           // the region is the whole row
      const int chunks = (int)((T + DYN_TILE - 1) / DYN_TILE);
      double s = 0.0;
      for (int c = 0; c < chunks; ++c) {
        const int len = (int)(T - (int64_t)c * DYN_TILE < DYN_TILE ? T - (int64_t)c * DYN_TILE : DYN_TILE);
        s = s + chunk_sum(xs + c * DYN_TILE, len, lane, 0.0, false);
      }
      m = s / (double)T;
      if (A.variance) {
        double q = 0.0;
        for (int c = 0; c < chunks; ++c) {
          const int len = (int)(T - (int64_t)c * DYN_TILE < DYN_TILE ? T - (int64_t)c * DYN_TILE : DYN_TILE);
          q = q + chunk_sum(xs + c * DYN_TILE, len, lane, m, true);
        }
        const double v = q / (double)T;
        inv = 1.0 / sqrt(v > DYN_VAR_FLOOR ? v : DYN_VAR_FLOOR);
      }
    } else {
      m = A.part[row * 2];                      // stat [rows][2]: the mean and the variance
      if (A.variance) {
        const double v = A.part[row * 2 + 1];
        inv = 1.0 / sqrt(v > DYN_VAR_FLOOR ? v : DYN_VAR_FLOOR);
      }
    }
    __syncthreads();
    for (int i = lane; i < n; i += DYN_WAVE) xs[i] = (float)(((double)xs[i] - m) * inv);
    __syncthreads();
  } else if (A.cm == 2) {
    const int dh = A.nd ? A.width : 0;          // the deltas read normalised frames this far outside [t0, t1)
    const int64_t a0 = t0 - dh > lo ? t0 - dh : lo;
    const int64_t a1 = hi - t1 < dh ? hi : t1 + dh;
    if (A.direct) {
      for (int64_t t = a0 + lane; t < a1; t += DYN_WAVE) {
        int64_t s, e;
        window_of(t, A.W, T, s, e);
        const double nn = (double)(e - s);
        double a = 0.0;
        for (int64_t i = s; i < e; ++i) a = a + (double)xs[i - lo];
        const double m = a / nn;
        double y = (double)xs[t - lo] - m;
        if (A.variance) {
          double q = 0.0;
          for (int64_t i = s; i < e; ++i) { const double d = (double)xs[i - lo] - m; q = q + d * d; }
          const double v = q / nn;
          y = y / sqrt(v > DYN_VAR_FLOOR ? v : DYN_VAR_FLOOR);
        }
        ys[t - lo] = (float)y;
      }
    } else {
      // exclusive float64 prefix sums of x and x^2 over the region: a run per lane, a wave scan of the run totals
      const int R = (n + DYN_WAVE - 1) / DYN_WAVE;
      const int i0 = lane * R < n ? lane * R : n, i1 = i0 + R < n ? i0 + R : n;
      double a = 0.0, q = 0.0;
      for (int i = i0; i < i1; ++i) { const double v = (double)xs[i]; a = a + v; q = q + v * v; }
#pragma unroll
      for (int d = 1; d < DYN_WAVE; d <<= 1) {
        const double ta = __shfl_up(a, d), tq = __shfl_up(q, d);
        if (lane >= d) { a = a + ta; q = q + tq; }
      }
      double ra = __shfl_up(a, 1), rq = __shfl_up(q, 1);
      if (lane == 0) { ra = 0.0; rq = 0.0; }
      for (int i = i0; i < i1; ++i) {
        S[i] = ra; Q[i] = rq;
        const double v = (double)xs[i];
        ra = ra + v; rq = rq + v * v;
      }
      if (i0 < n && i1 == n) { S[n] = ra; Q[n] = rq; }
      __syncthreads();
      for (int64_t t = a0 + lane; t < a1; t += DYN_WAVE) {
        int64_t s, e;
        window_of(t, A.W, T, s, e);
        const double nn = (double)(e - s);
        const double m = (S[e - lo] - S[s - lo]) / nn;
        double y = (double)xs[t - lo] - m;
        if (A.variance) {
          const double v = (Q[e - lo] - Q[s - lo]) / nn - m * m;
          y = y / sqrt(v > DYN_VAR_FLOOR ? v : DYN_VAR_FLOOR);
        }
        ys[t - lo] = (float)y;                  // in place: the windows read S and Q alone
      }
    }
    __syncthreads();
  }

  if (!live) return;
  const int width = A.width, h = width / 2;
  float* ob = A.out + b * A.sob;
  // Interior frames [bb0, bb1), DYN_FRAMES a lane at a time: a weight is fetched once for all of them and their sums run
  // side by side, each still j ascending, so the bits are those of the frame-by-frame loop below, which takes the rest.
  int64_t bb0 = t0 >= h ? t0 : t0 + (h - t0 + DYN_WAVE - 1) / DYN_WAVE * DYN_WAVE, bb1 = bb0;
  if (A.nd) {
    const int64_t i1 = t1 < T - h ? t1 : T - h;
    if (i1 > bb0) bb1 = bb0 + (i1 - bb0) / (DYN_WAVE * DYN_FRAMES) * (DYN_WAVE * DYN_FRAMES);
    for (int64_t tb = bb0; tb < bb1; tb += DYN_WAVE * DYN_FRAMES) {
      const float* sp = ys + (tb + lane - h - lo);
      float* op = ob + k * A.sok + tb + lane;
      if (A.statics) {
#pragma unroll
        for (int r = 0; r < DYN_FRAMES; ++r) op[r * DYN_WAVE] = sp[h + r * DYN_WAVE];
      }
      for (int d = 0; d < A.nd; ++d) {
        const float* wt = A.tab + (size_t)d * width * width;
        float acc[DYN_FRAMES];
#pragma unroll
        for (int r = 0; r < DYN_FRAMES; ++r) acc[r] = 0.f;
#pragma unroll 4
        for (int j = 0; j < width; ++j) {
          const float wj = wt[j];
#pragma unroll
          for (int r = 0; r < DYN_FRAMES; ++r) acc[r] = fmaf(wj, sp[j + r * DYN_WAVE], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < DYN_FRAMES; ++r) op[(int64_t)(d + A.statics) * A.K * A.sok + r * DYN_WAVE] = acc[r];
      }
    }
  }
  for (int64_t t = t0 + lane; t < t1; t += DYN_WAVE) {
    if (t >= bb0 && t < bb1) continue;
    if (A.statics) ob[k * A.sok + t] = ys[t - lo];
    for (int d = 0; d < A.nd; ++d) {
      const float* wt = A.tab + (size_t)d * width * width;      // w [width], then the left and right edge rows [h][width]
      float acc = 0.f;
      if (A.mode == MODE_INTERP && t < h) {
        const float* e = wt + width + (size_t)t * width;
        for (int j = 0; j < width; ++j) acc = fmaf(e[j], ys[j - lo], acc);
      } else if (A.mode == MODE_INTERP && t >= T - h) {
        const float* e = wt + width + (size_t)(h + (t - (T - h))) * width;
        const float* sp = ys + (T - width - lo);
        for (int j = 0; j < width; ++j) acc = fmaf(e[j], sp[j], acc);
      } else if (t >= h && t < T - h) {
        const float* sp = ys + (t - h - lo);
        for (int j = 0; j < width; ++j) acc = fmaf(wt[j], sp[j], acc);
      } else {
        for (int j = 0; j < width; ++j) {
          const int64_t idx = map_index(t - h + j, T, A.mode);
          const float v = idx < 0 ? A.cval : (idx >= lo && idx < hi ? ys[idx - lo] : xr[idx]);
          acc = fmaf(wt[j], v, acc);
        }
      }
      ob[((int64_t)(d + A.statics) * A.K + k) * A.sok + t] = acc;
    }
  }
}

// out [B, n_steps K, T] contiguous: out[b, i K + k, t] = x[b, k, t - i delay], 0 outside [0, T)
__global__ __launch_bounds__(256) void stack_memory_kernel(const float* __restrict__ x, int64_t sxb, int64_t sxk, int64_t B, int64_t K,
                                                           int64_t T, int64_t n_steps, int64_t delay, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const int64_t rows = B * n_steps * K;
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const int64_t b = r / (n_steps * K), ik = r - b * n_steps * K;
    const int64_t i = ik / K, k = ik - i * K;
    const int64_t src = t - i * delay;
    out[r * T + t] = (src >= 0 && src < T) ? x[b * sxb + k * sxk + src] : 0.f;
  }
}

int check_rows_dyn(const char* who, const float* x, const float* out, int64_t B, int64_t K, int64_t T, int64_t sxb, int64_t sxk) {
  SYG_REQUIRE(x && out, "%s: null pointer argument (x / out)", who);
  SYG_REQUIRE(B >= 1 && K >= 1 && T >= 1, "%s: empty input (B = %lld, K = %lld, T = %lld; each must be at least 1)", who,
              (long long)B, (long long)K, (long long)T);
  SYG_REQUIRE(sxb >= 0 && sxk >= 0 && (K == 1 || sxk >= T || sxk == 0), "%s: bad input strides (%lld, %lld) for T = %lld", who,
              (long long)sxb, (long long)sxk, (long long)T);
  return SYG_OK;
}

int check_out_size(const char* who, int64_t B, int64_t rows_per_clip, int64_t T) {
  const long double total = (long double)B * (long double)rows_per_clip * (long double)T;
  SYG_REQUIRE(total <= (long double)DYN_MAX_OUT, "%s: a result of %.0Lf elements is above 2^31 = %lld", who, total,
              (long long)DYN_MAX_OUT);
  return SYG_OK;
}

inline int64_t span(int64_t B, int64_t K, int64_t T, int64_t sb, int64_t sk) { return (B - 1) * sb + (K - 1) * sk + T; }

inline bool overlaps(const float* a, int64_t na, const float* b, int64_t nb) { return a < b + nb && b < a + na; }

inline bool sliding(int64_t W, int64_t T) { return W >= 1 && W < T; }

// 0 resident, 1 tiled: the library's rule
inline int form_rule(int64_t T, int64_t W) { return T <= (sliding(W, T) ? DYN_RESIDENT_T_SLIDING : DYN_RESIDENT_T) ? 0 : 1; }

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_dynamics_constants(int key) {
  switch (key) {
    case SYG_DYN_TILE: return DYN_TILE;
    case SYG_DYN_RESIDENT_T: return DYN_RESIDENT_T;
    case SYG_DYN_RESIDENT_T_SLIDING: return DYN_RESIDENT_T_SLIDING;
    case SYG_DYN_WINDOW_MAX: return DYN_WINDOW_MAX;
    case SYG_DYN_DIRECT_WINDOW: return DYN_DIRECT_W;
    case SYG_DYN_WIDTH_MAX: return DYN_WIDTH_MAX;
    case SYG_DYN_ORDER_MAX: return DYN_ORDER_MAX;
    case SYG_DYN_UNITS: return DYN_UNITS;
    case SYG_DYN_MAX_OUT: return DYN_MAX_OUT;
    case SYG_DYN_LDS_MAX: return DYN_LDS_MAX;
    default: return -1;
  }
}

extern "C" int syg_dynamics_form(int64_t T, int64_t window) {
  if (T < 1 || window < 0) return -1;
  return form_rule(T, window);
}

extern "C" int64_t syg_dynamics_work_bytes(int64_t B, int64_t K, int64_t T) {
  if (B < 1 || K < 1 || T < 1) return -1;
  return B * K * 2 * (ceil_div(T, DYN_TILE) + 1) * (int64_t)sizeof(double);
}

extern "C" int syg_dynamics_f32(const float* x, int64_t B, int64_t K, int64_t T, int64_t sxb, int64_t sxk, float* out, int64_t sob,
                                int64_t sok, int cmvn, int64_t window, int variance, int statics, int n_delta, int width, int mode,
                                float cval, const float* tab, int form, void* work, int64_t work_bytes, void* stream) {
  const char* who = "dynamics";
  if (const int rc = check_rows_dyn(who, x, out, B, K, T, sxb, sxk)) return rc;
  SYG_REQUIRE(n_delta >= 0 && n_delta <= 2 && (statics == 0 || statics == 1) && statics + n_delta >= 1 && (cmvn == 0 || cmvn == 1),
              "%s: bad block selection (cmvn 0 / 1, statics 0 / 1, n_delta 0 .. 2, at least one block)", who);
  SYG_REQUIRE(form >= 0 && form <= 2, "%s: form must be 0 (the rule), 1 (resident) or 2 (tiled)", who);
  const int64_t blocks = statics + n_delta;
  SYG_REQUIRE(sok >= T && sob >= blocks * K * sok - (sok - T), "%s: bad output strides (%lld, %lld) for %lld rows of T = %lld", who,
              (long long)sob, (long long)sok, (long long)(blocks * K), (long long)T);
  if (const int rc = check_out_size(who, B, blocks * K, T)) return rc;
  if (n_delta) {
    SYG_REQUIRE(tab, "%s: null pointer argument (tab)", who);
    SYG_REQUIRE(width >= 3 && width <= DYN_WIDTH_MAX && (width & 1), "%s: width must be odd in [3, %d] (got %d)", who, DYN_WIDTH_MAX,
                width);
    SYG_REQUIRE(mode >= MODE_INTERP && mode <= MODE_CONSTANT,
                "%s: unknown mode %d (served: 0 interp, 1 nearest, 2 mirror, 3 wrap, 4 constant)", who, mode);
    SYG_REQUIRE(mode != MODE_INTERP || T >= width,
                "%s: if mode is 'interp', window_length (%d) must be less than or equal to the size of x (%lld)", who, width,
                (long long)T);
  } else {
    width = 1;
  }
  SYG_REQUIRE(!cmvn || window >= 0, "%s: window must be 0 (all frames) or at least 1 (got %lld)", who, (long long)window);
  const bool slide = cmvn && sliding(window, T);
  const int64_t nx = span(B, K, T, sxb, sxk), no = span(B, blocks * K, T, sob, sok);
  const bool alias = out == x && sob == sxb && sok == sxk;
  if (n_delta || !statics || !alias)
    SYG_REQUIRE(!overlaps(x, nx, out, no), "%s: out overlaps x (only cmvn alone may write onto its input, out = x)", who);
  int tiled = form ? form - 1 : form_rule(T, cmvn ? window : 0);
  if (slide && tiled)
    SYG_REQUIRE(window <= DYN_WINDOW_MAX,
                "%s: a sliding window of %lld frames below T = %lld does not fit beside a tile: the bound is %d (or T <= %lld)", who,
                (long long)window, (long long)T, DYN_WINDOW_MAX, (long long)DYN_RESIDENT_T_SLIDING);
  SYG_REQUIRE(!(slide && tiled && alias), "%s: a sliding window in the tiled form cannot write onto its input", who);
  const int direct = slide && window <= DYN_DIRECT_W;
  const int64_t tiles = tiled ? ceil_div(T, DYN_TILE) : 1;
  SYG_REQUIRE(!(cmvn && n_delta && mode == MODE_WRAP && tiles > 1),
              "%s: mode wrap with CMVN is served in one call only where a row is one unit (T <= %d here, or the resident form)", who,
              DYN_TILE);
  const int halo = tiled ? (n_delta ? width : 0) + (slide ? (int)window : 0) : 0;
  const int64_t region = tiled ? (int64_t)DYN_TILE + 2 * halo : T;
  const int64_t per_frame = slide ? (direct ? 8 : 4) : 4;
  int64_t unit_bytes = region * per_frame + (slide && !direct ? 2 * (region + 1) * 8 : 0);
  unit_bytes = (unit_bytes + 15) & ~(int64_t)15;
  SYG_REQUIRE(unit_bytes <= DYN_LDS_MAX, "%s: a row of T = %lld does not fit the resident form (%lld B of LDS, at most %lld)", who,
              (long long)T, (long long)unit_bytes, (long long)DYN_LDS_MAX);
  int upw = (int)(DYN_LDS_SHARED / unit_bytes);
  upw = upw < 1 ? 1 : (upw > DYN_UNITS ? DYN_UNITS : upw);
  const int64_t rows = B * K, units = rows * tiles;
  const bool global_tiled = cmvn && !slide && tiled;
  if (global_tiled)
    SYG_REQUIRE(work && work_bytes >= syg_dynamics_work_bytes(B, K, T), "%s: the tiled form needs `work` of %lld bytes", who,
                (long long)syg_dynamics_work_bytes(B, K, T));
  const size_t lds = (size_t)unit_bytes * upw;
  if (const int rc = reserve_dynamic_lds(who, (const void*)dyn_kernel, lds)) return rc;

  double* part = (double*)work;
  double* stat = part + rows * 2 * tiles;
  if (global_tiled) {
    for (int pass = 0; pass < (variance ? 2 : 1); ++pass) {
      hipLaunchKernelGGL(dyn_stats_kernel, dim3((unsigned)ceil_div(units, DYN_UNITS)), dim3(DYN_WAVE * DYN_UNITS), 0,
                         (hipStream_t)stream, x, sxb, sxk, K, T, tiles, units, part, stat, pass);
      SYG_CHECK_LAUNCH(who);
      hipLaunchKernelGGL(dyn_combine_kernel, dim3((unsigned)ceil_div(rows, DYN_UNITS)), dim3(DYN_WAVE * DYN_UNITS), 0,
                         (hipStream_t)stream, part, tiles, rows, T, stat, pass);
      SYG_CHECK_LAUNCH(who);
    }
  }
  DynArgs A;
  A.x = x; A.out = out; A.tab = tab; A.part = stat;
  A.sxb = sxb; A.sxk = sxk; A.sob = sob; A.sok = sok; A.B = B; A.K = K; A.T = T; A.W = window; A.tiles = tiles; A.units = units;
  A.unit_bytes = unit_bytes;
  A.tile = tiled ? DYN_TILE : (int)T; A.halo = halo; A.region = (int)region; A.cm = cmvn ? (slide ? 2 : 1) : 0;
  A.variance = variance ? 1 : 0; A.statics = statics; A.nd = n_delta; A.width = width; A.mode = mode; A.resident = !tiled;
  A.direct = direct; A.cval = cval;
  hipLaunchKernelGGL(dyn_kernel, dim3((unsigned)ceil_div(units, upw)), dim3(DYN_WAVE * upw), lds, (hipStream_t)stream, A);
  SYG_CHECK_LAUNCH(who);
  return SYG_OK;
}

extern "C" int syg_stack_memory_f32(const float* x, int64_t B, int64_t K, int64_t T, int64_t sxb, int64_t sxk, float* out,
                                    int64_t n_steps, int64_t delay, void* stream) {
  const char* who = "stack_memory";
  if (const int rc = check_rows_dyn(who, x, out, B, K, T, sxb, sxk)) return rc;
  SYG_REQUIRE(n_steps >= 1, "%s: n_steps must be at least 1 (got %lld)", who, (long long)n_steps);
  SYG_REQUIRE(delay != 0, "%s: delay must be a non-zero integer, either sign", who);
  SYG_REQUIRE(n_steps <= DYN_MAX_OUT, "%s: a result of more than 2^31 = %lld elements", who, (long long)DYN_MAX_OUT);
  if (const int rc = check_out_size(who, B, n_steps * K, T)) return rc;
  SYG_REQUIRE(!overlaps(x, span(B, K, T, sxb, sxk), out, B * n_steps * K * T), "%s: out overlaps x", who);
  const int64_t rows = B * n_steps * K;
  hipLaunchKernelGGL(stack_memory_kernel, dim3((unsigned)ceil_div(T, 256), grid_rows(rows)), dim3(256), 0,
                     (hipStream_t)stream, x, sxb, sxk, B, K, T, n_steps, delay, out);
  SYG_CHECK_LAUNCH(who);
  return SYG_OK;
}
