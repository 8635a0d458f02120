// Structure analysis of a recurrence matrix and of the feature sequence behind it: the rest of librosa.segment.  The
// float64 restatement that is the contract lives in tests/structure_ref.py.
//
//   lag_shear_kernel      recurrence_to_lag / lag_to_recurrence, both axes, padded or not: one gather, a read and a write
//                         an element, consecutive lanes on consecutive output columns.
//   path_enhance_kernel   librosa.segment.path_enhance: out = max over filters of a sparse 2-D correlation.  A workgroup
//                         owns a tile of 16 x 64 outputs and stages tile plus halo in LDS through the boundary rule (a
//                         periodic index map, so a matrix far smaller than the filter folds as often as needed).  The
//                         filters arrive as lists of (row offset, column offset, weight) of their non-zero taps; a tap is
//                         the same for every lane and is read with scalar loads.  A thread carries four outputs (rows
//                         4 ty + q) and four partial sums each: tap e of a filter goes to partial sum e mod 4, the sums
//                         are combined as (s0 + s1) + (s2 + s3), and the maximum over filters is taken in registers.  That
//                         order is the kernel's definition: no atomics, the same call gives the same bits and a batch
//                         equals its rows.
//   diag_median_kernel    timelag_filter(median_filter, size=(1, w)) without the lag matrix: a thread an output, its w
//                         values as order-preserving keys in a column of LDS of its own, the middle one found by a
//                         32-step bisection over the key bits.  -0 orders below +0; the result is an input value bit
//                         for bit.
//   agglomerative_kernel  Ward clustering of a chain: a workgroup a span, segment sums in a float64 workspace, the live
//                         boundary costs and the links in LDS, a block-wide (value, index) argmin a merge (the leftmost
//                         on ties), two costs recomputed a merge.
//   segment_sync_kernel   librosa.util.sync for mean (summed in float64, ascending), max and min.
#include <float.h>
#include <limits.h>
#include <math.h>
#include <cmath>
#include "host.h"

namespace syg {
namespace {

constexpr int NT = 256;                       // threads of every workgroup here but the median's
constexpr int SHEAR_T_MAX = 32768;            // 2 t t output elements stay below 2^31
constexpr int PT_R = 16, PT_C = 64, PQ = 4;   // path_enhance: outputs of a tile, outputs of a thread (rows 4 ty + q)
constexpr int PATH_SPAN_MAX = 160;            // widest extent of the tap offsets (max - min) along either axis
constexpr int PATH_DIM_MAX = 1 << 20;         // rows / columns of a matrix
constexpr int MED_NT = 128;                   // threads of a median workgroup: 63 x 128 keys are 32 KiB
constexpr int MED_W_MAX = 63;
constexpr int AGG_T_MAX = 8192;               // frames of a span: 16 bytes of LDS a frame, 128 KiB of the 160
constexpr int AGG_WGS_PER_CU = 8;             // agglomerative_kernel: a workgroup loops over the spans past the grid
constexpr int SYNC_FT = 64;                 // features of a segment_sync workgroup

// scipy.ndimage's boundary rules as index maps: the source index of position x of an axis of n, -1 where the constant fills
__device__ __forceinline__ int64_t bmap(int64_t x, int64_t n, int mode) {
  if (x >= 0 && x < n) return x;
  if (mode == SYG_BOUNDARY_NEAREST) return x < 0 ? 0 : n - 1;
  if (mode == SYG_BOUNDARY_CONSTANT) return -1;
  if (mode == SYG_BOUNDARY_MIRROR && n == 1) return 0;
  const int64_t per = mode == SYG_BOUNDARY_WRAP ? n : (mode == SYG_BOUNDARY_REFLECT ? 2 * n : 2 * n - 2);
  int64_t p = x % per;
  if (p < 0) p += per;
  if (p < n) return p;
  return mode == SYG_BOUNDARY_REFLECT ? per - 1 - p : per - p;      // (wrap never gets here: per = n)
}

__device__ __forceinline__ uint32_t ord_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_float(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }

// ------------------------------------------------------------------ shear
// axis 1 (librosa's -1): forward out [n, t], out[y, x] = in~[(y + x) mod n, x]; inverse out [t, t], out[y, x] = in[(y - x) mod n, x].
// axis 0: forward out [t, n], out[y, x] = in~[y, (x + y) mod n]; inverse out[y, x] = in[y, (x - y) mod n].  in~ is `in`
// [t, t] with zeros past t; n = 2 t (padded) or t.
__global__ __launch_bounds__(NT) void lag_shear_kernel(const float* in, float* out, int64_t B, int t, int n, int64_t ldi, int64_t bsi,
                                                       int inverse, int axis) {
  const int rows = (!inverse && axis == 1) ? n : t, cols = (!inverse && axis == 0) ? n : t;
  const int64_t E = (int64_t)rows * cols;
  const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (e >= E) return;
  const int y = (int)(e / cols), x = (int)(e % cols);
  const int a = axis == 1 ? y : x, i = axis == 1 ? x : y;           // a: the sheared coordinate, i: the time index
  int s = inverse ? a - i : a + i;                                   // in [-(t - 1), 3 t)
  if (s < 0) s += n;
  if (s >= n) s -= n;
  const int64_t src = axis == 1 ? (int64_t)s * ldi + i : (int64_t)i * ldi + s;
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y)
    out[b * E + e] = (inverse || s < t) ? in[b * bsi + src] : 0.f;
}

// ------------------------------------------------------------------ path enhancement
template <int PITCH>
__global__ __launch_bounds__(NT) void path_enhance_kernel(const float* __restrict__ R, const int4* __restrict__ taps,
                                                          const int* __restrict__ fstart, float* __restrict__ out, int64_t B, int64_t T,
                                                          int64_t Tc, int64_t ldr, int64_t bsr, int n_taps, int nf, int dr0, int dr1,
                                                          int dc0, int dc1, int mode, float cval, int clip, int tiles_c) {
  extern __shared__ float tile[];                                    // [PT_R + dr1 - dr0][PITCH]
  const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
  const int H = PT_R + dr1 - dr0, W = PT_C + dc1 - dc0;              // W <= PITCH (the host picks PITCH)
  const int64_t r0 = (int64_t)(blockIdx.x / tiles_c) * PT_R, c0 = (int64_t)(blockIdx.x % tiles_c) * PT_C;
  const int base = (ty * PQ) * PITCH + tx;
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    const float* Rb = R + b * bsr;
    __syncthreads();                                                 // the previous matrix's readers
    for (int e = tid; e < H * W; e += NT) {
      const int lr = e / W, lc = e - lr * W;
      const int64_t mr = bmap(r0 + dr0 + lr, T, mode), mc = bmap(c0 + dc0 + lc, Tc, mode);
      tile[lr * PITCH + lc] = (mr < 0 || mc < 0) ? cval : Rb[mr * ldr + mc];
    }
    __syncthreads();
    float best[PQ];
    for (int f = 0; f < nf; ++f) {
      int lo = fstart[f], hi = fstart[f + 1];
      lo = min(max(lo, 0), n_taps);
      hi = min(max(hi, lo), n_taps);
      float acc[4][PQ];
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < PQ; ++q) acc[p][q] = 0.f;
      // a tap's offsets are clamped into the staged halo (scalar work): a table that does not match its spans reads
      // staged values, never past the tile
      auto tap = [&](int e, float (&a)[PQ]) {
        const int4 tp = taps[e];
        const int dr = min(max(tp.x, dr0), dr1) - dr0, dc = min(max(tp.y, dc0), dc1) - dc0;
        const float w = __int_as_float(tp.z);
        const float* src = tile + base + (dr * PITCH + dc);
#pragma unroll
        for (int q = 0; q < PQ; ++q) a[q] = fmaf(w, src[q * PITCH], a[q]);
      };
      int e = lo;
      for (; e + 4 <= hi; e += 4) {
        tap(e, acc[0]);
        tap(e + 1, acc[1]);
        tap(e + 2, acc[2]);
        tap(e + 3, acc[3]);
      }
      if (e < hi) tap(e, acc[0]);
      if (e + 1 < hi) tap(e + 1, acc[1]);
      if (e + 2 < hi) tap(e + 2, acc[2]);
#pragma unroll
      for (int q = 0; q < PQ; ++q) {
        const float v = (acc[0][q] + acc[1][q]) + (acc[2][q] + acc[3][q]);
        best[q] = f == 0 ? v : fmaxf(best[q], v);
      }
    }
    const int64_t c = c0 + tx;
#pragma unroll
    for (int q = 0; q < PQ; ++q) {
      const int64_t r = r0 + ty * PQ + q;
      if (r < T && c < Tc) out[(b * T + r) * Tc + c] = clip ? fmaxf(best[q], 0.f) : best[q];
    }
  }
}

// ------------------------------------------------------------------ diagonal median
// Output (y, x); axis 1: time index i = x, row r = y; axis 0: i = y, r = x.  c_j = m(i + j - w / 2); the sample is
// R~[(r - i + c_j) mod n, c_j] (axis 0: its transpose), R~ zero past t, cval where the constant fills.
__global__ __launch_bounds__(MED_NT) void diag_median_kernel(const float* R, float* out, int64_t B, int t, int n, int64_t ldr,
                                                             int64_t bsr, int w, int axis, int mode, float cval) {
  extern __shared__ uint32_t keys[];                                 // [w][MED_NT]: a thread reads what it wrote
  const int tid = threadIdx.x;
  const int64_t E = (int64_t)t * t;
  const int64_t e = (int64_t)blockIdx.x * MED_NT + tid;
  if (e >= E) return;
  const int y = (int)(e / t), x = (int)(e % t);
  const int i = axis == 1 ? x : y, r = axis == 1 ? y : x;
  const int h = w / 2, m = w / 2;                                    // rank of the median of an odd window
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    const float* Rb = R + b * bsr;
    for (int j = 0; j < w; ++j) {
      const int64_t cj = bmap((int64_t)i + j - h, t, mode);
      float v = cval;
      if (cj >= 0) {
        int s = (r - i + (int)cj) % n;                               // |r - i + cj| < 2 t <= 2 n
        if (s < 0) s += n;
        v = s < t ? (axis == 1 ? Rb[(int64_t)s * ldr + cj] : Rb[cj * ldr + s]) : 0.f;
      }
      keys[j * MED_NT + tid] = ord_key(v);
    }
    uint32_t v = 0;
    for (int bit = 31; bit >= 0; --bit) {                            // the largest v with #(keys < v) <= m is the key of rank m
      const uint32_t trial = v | (1u << bit);
      int below = 0;
      for (int j = 0; j < w; ++j) below += keys[j * MED_NT + tid] < trial ? 1 : 0;
      if (below <= m) v = trial;
    }
    out[b * E + e] = ord_float(v);
  }
}

// ------------------------------------------------------------------ chain Ward
struct AggArgs {
  const float* X; const int* offset; const int* length; const int* k; int* bounds; int* count; double* S;
  int64_t B, T, ldx, bsx, n_spans; int D, k_max, max_len;
};

// the Ward cost of merging the neighbouring segments a (na frames) and b (nb frames): one wave, every lane returns it
__device__ __forceinline__ double ward_cost(const double* Sa, const double* Sb, int na, int nb, int D, int lane) {
  const double ia = 1.0 / (double)na, ib = 1.0 / (double)nb;
  double acc = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double df = Sa[d] * ia - Sb[d] * ib;
    acc = fma(df, df, acc);
  }
  return ((double)na * (double)nb / (double)(na + nb)) * wave_sum_d(acc);
}

__global__ __launch_bounds__(NT) void agglomerative_kernel(AggArgs P) {
  extern __shared__ double agg_lds[];                                // cost [max_len] float64, next [max_len], prev [max_len]
  __shared__ double rv[NT / 64];
  __shared__ int rj[NT / 64];
  double* cost = agg_lds;
  int* next = (int*)(cost + P.max_len);
  int* prev = next + P.max_len;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t frames = P.B * P.T;
  for (int64_t s = blockIdx.x; s < P.n_spans; s += gridDim.x) {
    int64_t off = P.offset[s];
    off = off < 0 ? 0 : (off >= frames ? frames - 1 : off);
    const int64_t bb = off / P.T, t0 = off % P.T;
    int L = P.length[s];
    L = L < 1 ? 1 : L;
    if (L > P.T - t0) L = (int)(P.T - t0);                           // a span stays inside its clip ...
    if (L > P.max_len) L = P.max_len;                                // ... and inside the LDS plan
    int k = P.k[s];
    k = k < 1 ? 1 : (k > L ? L : k);
    if (k > P.k_max) k = P.k_max;
    const float* X0 = P.X + bb * P.bsx + t0 * P.ldx;
    double* S = P.S + off * P.D;
    int* bo = P.bounds + s * P.k_max;
    __syncthreads();                                                 // the previous span's readers
    for (int i = tid; i < L; i += NT) {
      next[i] = i + 1;
      prev[i] = i - 1;
      if (i == L - 1) cost[i] = INFINITY;
    }
    for (int64_t e = tid; e < (int64_t)L * P.D; e += NT) S[e] = (double)X0[(e / P.D) * P.ldx + e % P.D];
    for (int j = k + tid; j < P.k_max; j += NT) bo[j] = -1;
    __syncthreads();
    for (int i = wave; i < L - 1; i += NT / 64) {
      const double c = ward_cost(S + (int64_t)i * P.D, S + (int64_t)(i + 1) * P.D, 1, 1, P.D, lane);
      if (lane == 0) cost[i] = c;
    }
    __syncthreads();
    for (int live = L; live > k; --live) {
      double v = INFINITY;
      int j = INT_MAX;
      for (int i = tid; i < L; i += NT) take_better<false>(v, j, cost[i], i);
      wave_pick<false>(v, j);
      if (lane == 0) { rv[wave] = v; rj[wave] = j; }
      __syncthreads();
      v = rv[0]; j = rj[0];
#pragma unroll
      for (int q = 1; q < NT / 64; ++q) take_better<false>(v, j, rv[q], rj[q]);
      const int a = j < L - 1 ? j : 0;                               // (a live boundary always exists while live > 1)
      const int bseg = next[a];
      const int c = bseg < L ? next[bseg] : L;
      const int p = prev[a];
      __syncthreads();                                               // every thread has read the links and the winners
      if (bseg < L) {
        double* Sa = S + (int64_t)a * P.D;
        const double* Sb = S + (int64_t)bseg * P.D;
        for (int d = tid; d < P.D; d += NT) Sa[d] += Sb[d];
        if (tid == 0) {
          next[a] = c;
          if (c < L) prev[c] = a;
          cost[bseg] = INFINITY;
        }
      }
      __syncthreads();                                               // the merged sums and links are in
      if (wave == 0) {
        double cc = INFINITY;
        if (c < L) cc = ward_cost(S + (int64_t)a * P.D, S + (int64_t)c * P.D, c - a, next[c] - c, P.D, lane);
        if (lane == 0) cost[a] = cc;
      } else if (wave == 1 && p >= 0) {
        const double cc = ward_cost(S + (int64_t)p * P.D, S + (int64_t)a * P.D, a - p, c - a, P.D, lane);
        if (lane == 0) cost[p] = cc;
      }
      __syncthreads();
    }
    if (tid == 0) {
      int a = 0;
      for (int j = 0; j < k && a < L; ++j) {
        bo[j] = a;
        a = next[a];
      }
      P.count[s] = k;
    }
  }
}

// ------------------------------------------------------------------ segment aggregation
// Row (b, j) of the grid's y: segment j of clip b, frames [edges[j], edges[j + 1]) clamped into [0, T]; a lane a feature.
__global__ __launch_bounds__(SYNC_FT) void segment_sync_kernel(const float* X, const int* edges, float* out, int64_t B, int64_t T,
                                                               int64_t ldx, int64_t bsx, int64_t n_seg, int64_t edge_bs, int D,
                                                               int agg) {
  const int d = blockIdx.x * SYNC_FT + threadIdx.x;
  if (d >= D) return;
  for (int64_t row = blockIdx.y; row < B * n_seg; row += gridDim.y) {
    const int64_t b = row / n_seg, j = row % n_seg;
    int64_t lo = edges[b * edge_bs + j], hi = edges[b * edge_bs + j + 1];
    lo = lo < 0 ? 0 : (lo > T ? T : lo);
    hi = hi < lo ? lo : (hi > T ? T : hi);
    const float* x = X + b * bsx + d;
    float res = 0.f;
    if (hi > lo) {
      if (agg == SYG_SYNC_MEAN) {
        double sum = 0.0;
        for (int64_t t = lo; t < hi; ++t) sum += (double)x[t * ldx];
        res = (float)(sum / (double)(hi - lo));
      } else {
        res = x[lo * ldx];
        for (int64_t t = lo + 1; t < hi; ++t) res = agg == SYG_SYNC_MAX ? fmaxf(res, x[t * ldx]) : fminf(res, x[t * ldx]);
      }
    }
    out[row * D + d] = res;
  }
}

inline bool mode_ok(int mode) { return mode >= SYG_BOUNDARY_REFLECT && mode <= SYG_BOUNDARY_CONSTANT; }
inline bool flag_ok(int v) { return v == 0 || v == 1; }
const char* const MODES = "SYG_BOUNDARY_REFLECT (0), _MIRROR (1), _NEAREST (2), _WRAP (3) or _CONSTANT (4)";

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_structure_constants(int key) {
  switch (key) {
    case SYG_STRUCT_AGG_T_MAX: return AGG_T_MAX;
    case SYG_STRUCT_MEDIAN_W_MAX: return MED_W_MAX;
    case SYG_STRUCT_PATH_TILE_ROWS: return PT_R;
    case SYG_STRUCT_PATH_TILE_COLS: return PT_C;
    case SYG_STRUCT_PATH_SPAN_MAX: return PATH_SPAN_MAX;
    case SYG_STRUCT_SHEAR_T_MAX: return SHEAR_T_MAX;
    default: return -1;
  }
}

extern "C" int syg_lag_shear_f32(const float* in, int64_t B, int64_t t, int64_t ldi, int64_t bsi, int inverse, int axis, int pad,
                                 float* out, void* stream) {
  SYG_REQUIRE(in && out, "lag_shear: null pointer argument (in / out)");
  SYG_REQUIRE(B >= 1 && t >= 1 && t <= SHEAR_T_MAX && B <= ((int64_t)1 << 40) / (2 * t * t),
              "lag_shear: served are B >= 1 and square matrices of t in [1, %d] with 2 B t t <= 2^40 (got B=%lld, t=%lld)", SHEAR_T_MAX,
              (long long)B, (long long)t);
  SYG_REQUIRE(flag_ok(inverse) && flag_ok(axis) && flag_ok(pad), "lag_shear: inverse, axis and pad are 0 or 1 (got %d, %d, %d)", inverse,
              axis, pad);
  const int64_t n = pad ? 2 * t : t;
  const int64_t in_cols = (inverse && axis == 0) ? n : t;
  SYG_REQUIRE(ldi >= in_cols && bsi >= 0, "lag_shear: the row stride is smaller than the row (%lld < %lld), or the batch stride negative",
              (long long)ldi, (long long)in_cols);
  const int64_t E = inverse ? t * t : n * t;
  hipLaunchKernelGGL(lag_shear_kernel, dim3((unsigned)ceil_div(E, NT), grid_rows(B)), dim3(NT), 0, (hipStream_t)stream, in, out, B, (int)t,
                     (int)n, ldi, bsi, inverse, axis);
  SYG_CHECK_LAUNCH("lag_shear");
  return SYG_OK;
}

extern "C" int syg_path_enhance_f32(const float* R, int64_t B, int64_t T, int64_t Tc, int64_t ldr, int64_t bsr, const int* taps,
                                    int64_t n_taps, const int* fstart, int n_filters, int dr_min, int dr_max, int dc_min, int dc_max,
                                    int mode, float cval, int clip, float* out, void* stream) {
  SYG_REQUIRE(R && taps && fstart && out, "path_enhance: null pointer argument (R / taps / fstart / out)");
  SYG_REQUIRE(B >= 1 && T >= 1 && Tc >= 1 && T <= PATH_DIM_MAX && Tc <= PATH_DIM_MAX && B <= ((int64_t)1 << 40) / T / Tc,
              "path_enhance: served are B >= 1, T and T' in [1, 2^20] with B T T' <= 2^40 (got B=%lld, T=%lld, T'=%lld)", (long long)B,
              (long long)T, (long long)Tc);
  SYG_REQUIRE(n_filters >= 1 && n_filters <= 4096 && n_taps >= 1 && n_taps <= ((int64_t)1 << 28),
              "path_enhance: n_filters must be in [1, 4096] and n_taps in [1, 2^28] (got %d, %lld)", n_filters, (long long)n_taps);
  SYG_REQUIRE(dr_min <= dr_max && dc_min <= dc_max && (int64_t)dr_max - dr_min <= PATH_SPAN_MAX && (int64_t)dc_max - dc_min <= PATH_SPAN_MAX &&
                  std::abs((int64_t)dr_min) <= PATH_DIM_MAX && std::abs((int64_t)dc_min) <= PATH_DIM_MAX,
              "path_enhance: the tap offsets must span at most %d rows and columns (got rows %d..%d, columns %d..%d)", PATH_SPAN_MAX,
              dr_min, dr_max, dc_min, dc_max);
  SYG_REQUIRE(mode_ok(mode), "path_enhance: mode must be %s (got %d)", MODES, mode);
  SYG_REQUIRE(flag_ok(clip) && std::isfinite(cval), "path_enhance: clip is 0 or 1 and cval finite");
  SYG_REQUIRE(ldr >= Tc && bsr >= 0, "path_enhance: the row stride is smaller than T'=%lld (ldr=%lld), or the batch stride negative",
              (long long)Tc, (long long)ldr);
  const int span_c = dc_max - dc_min, H = PT_R + dr_max - dr_min;
  const int pitch = span_c <= 32 ? 96 : (span_c <= 96 ? 160 : 224);
  const size_t lds = (size_t)H * pitch * sizeof(float);
  const int tiles_c = (int)ceil_div(Tc, PT_C);
  const dim3 grid((unsigned)(ceil_div(T, PT_R) * tiles_c), grid_rows(B));
  hipStream_t s = (hipStream_t)stream;
#define SYG_PATH_LAUNCH(PITCH)                                                                                                   \
  do {                                                                                                                           \
    const int rc = reserve_dynamic_lds("path_enhance", (const void*)path_enhance_kernel<PITCH>, lds);                            \
    if (rc != SYG_OK) return rc;                                                                                                 \
    hipLaunchKernelGGL((path_enhance_kernel<PITCH>), grid, dim3(NT), lds, s, R, (const int4*)taps, fstart, out, B, T, Tc, ldr, bsr, \
                       (int)n_taps, n_filters, dr_min, dr_max, dc_min, dc_max, mode, cval, clip, tiles_c);                      \
  } while (0)
  if (pitch == 96) SYG_PATH_LAUNCH(96);
  else if (pitch == 160) SYG_PATH_LAUNCH(160);
  else SYG_PATH_LAUNCH(224);
#undef SYG_PATH_LAUNCH
  SYG_CHECK_LAUNCH("path_enhance");
  return SYG_OK;
}

extern "C" int syg_diag_median_f32(const float* R, int64_t B, int64_t t, int64_t ldr, int64_t bsr, int w, int axis, int pad, int mode,
                                   float cval, float* out, void* stream) {
  SYG_REQUIRE(R && out, "diag_median: null pointer argument (R / out)");
  SYG_REQUIRE(B >= 1 && t >= 1 && t <= SHEAR_T_MAX && B <= ((int64_t)1 << 40) / (t * t),
              "diag_median: served are B >= 1 and square matrices of t in [1, %d] with B t t <= 2^40 (got B=%lld, t=%lld)", SHEAR_T_MAX,
              (long long)B, (long long)t);
  SYG_REQUIRE(w >= 1 && w <= MED_W_MAX && (w & 1), "diag_median: w must be odd and in [1, %d] (got %d)", MED_W_MAX, w);
  SYG_REQUIRE(flag_ok(axis) && flag_ok(pad), "diag_median: axis and pad are 0 or 1 (got %d, %d)", axis, pad);
  SYG_REQUIRE(mode_ok(mode), "diag_median: mode must be %s (got %d)", MODES, mode);
  SYG_REQUIRE(std::isfinite(cval), "diag_median: cval must be finite");
  SYG_REQUIRE(ldr >= t && bsr >= 0, "diag_median: the row stride is smaller than t=%lld (ldr=%lld), or the batch stride negative",
              (long long)t, (long long)ldr);
  hipLaunchKernelGGL(diag_median_kernel, dim3((unsigned)ceil_div(t * t, MED_NT), grid_rows(B)), dim3(MED_NT),
                     (size_t)w * MED_NT * sizeof(uint32_t), (hipStream_t)stream, R, out, B, (int)t, (int)(pad ? 2 * t : t), ldr, bsr, w, axis,
                     mode, cval);
  SYG_CHECK_LAUNCH("diag_median");
  return SYG_OK;
}

static bool agg_shape_ok(int64_t B, int64_t T, int64_t D) {
  return B >= 1 && T >= 1 && D >= 1 && D <= (1 << 20) && T <= ((int64_t)1 << 30) && B <= (((int64_t)1 << 31) - 1) / T &&
         B * T <= ((int64_t)1 << 36) / D;
}

extern "C" int64_t syg_agglomerative_work_bytes(int64_t B, int64_t T, int64_t D) {
  if (!agg_shape_ok(B, T, D)) {
    set_error("agglomerative_work_bytes: served are B, T >= 1 with B T < 2^31, D in [1, 2^20] and B T D <= 2^36 (got B=%lld, T=%lld, D=%lld)",
              (long long)B, (long long)T, (long long)D);
    return -1;
  }
  return B * T * D * (int64_t)sizeof(double);
}

extern "C" int syg_agglomerative_f32(const float* X, int64_t B, int64_t T, int64_t D, int64_t ldx, int64_t bsx, const int* offset,
                                     const int* length, const int* k, int64_t n_spans, int64_t max_len, int64_t k_max, int* bounds,
                                     int* count, void* work, int64_t work_bytes, void* stream) {
  SYG_REQUIRE(X && offset && length && k && bounds && count && work,
              "agglomerative: null pointer argument (X / offset / length / k / bounds / count / work)");
  SYG_REQUIRE(agg_shape_ok(B, T, D),
              "agglomerative: served are B, T >= 1 with B T < 2^31, D in [1, 2^20] and B T D <= 2^36 (got B=%lld, T=%lld, D=%lld)",
              (long long)B, (long long)T, (long long)D);
  SYG_REQUIRE(n_spans >= 1 && n_spans <= B * T, "agglomerative: n_spans must be in [1, B T] (got %lld)", (long long)n_spans);
  SYG_REQUIRE(max_len >= 1 && max_len <= AGG_T_MAX && max_len <= T,
              "agglomerative: a span holds 1 to %d frames, and no more than T (got max_len=%lld, T=%lld)", AGG_T_MAX, (long long)max_len,
              (long long)T);
  SYG_REQUIRE(k_max >= 1 && k_max <= max_len, "agglomerative: k_max must be in [1, max_len] (got %lld)", (long long)k_max);
  SYG_REQUIRE(ldx >= D && bsx >= 0, "agglomerative: the frame stride is smaller than D=%lld (ldx=%lld), or the batch stride negative",
              (long long)D, (long long)ldx);
  SYG_REQUIRE(work_bytes >= B * T * D * (int64_t)sizeof(double), "agglomerative: the workspace is too small (%lld bytes; needed %lld)",
              (long long)work_bytes, (long long)(B * T * D * (int64_t)sizeof(double)));
  const size_t lds = (size_t)max_len * (sizeof(double) + 2 * sizeof(int));
  const int rc = reserve_dynamic_lds("agglomerative", (const void*)agglomerative_kernel, lds);
  if (rc != SYG_OK) return rc;
  AggArgs P{X, offset, length, k, bounds, count, (double*)work, B, T, ldx, bsx, n_spans, (int)D, (int)k_max, (int)max_len};
  hipLaunchKernelGGL(agglomerative_kernel, dim3(capped_grid(n_spans, AGG_WGS_PER_CU)), dim3(NT), lds, (hipStream_t)stream, P);
  SYG_CHECK_LAUNCH("agglomerative");
  return SYG_OK;
}

extern "C" int syg_segment_sync_f32(const float* X, int64_t B, int64_t T, int64_t D, int64_t ldx, int64_t bsx, const int* edges,
                                    int64_t n_seg, int64_t edge_bs, int aggregate, float* out, void* stream) {
  SYG_REQUIRE(X && edges && out, "segment_sync: null pointer argument (X / edges / out)");
  SYG_REQUIRE(agg_shape_ok(B, T, D),
              "segment_sync: served are B, T >= 1 with B T < 2^31, D in [1, 2^20] and B T D <= 2^36 (got B=%lld, T=%lld, D=%lld)",
              (long long)B, (long long)T, (long long)D);
  SYG_REQUIRE(n_seg >= 1 && n_seg <= T && B * n_seg <= ((int64_t)1 << 36) / D,
              "segment_sync: n_seg must be in [1, T] (got %lld)", (long long)n_seg);
  SYG_REQUIRE(edge_bs == 0 || edge_bs == n_seg + 1, "segment_sync: the batch stride of edges is 0 (shared) or n_seg + 1 (got %lld)",
              (long long)edge_bs);
  SYG_REQUIRE(aggregate == SYG_SYNC_MEAN || aggregate == SYG_SYNC_MAX || aggregate == SYG_SYNC_MIN,
              "segment_sync: aggregate must be SYG_SYNC_MEAN (0), SYG_SYNC_MAX (1) or SYG_SYNC_MIN (2); median is not served (got %d)",
              aggregate);
  SYG_REQUIRE(ldx >= D && bsx >= 0, "segment_sync: the frame stride is smaller than D=%lld (ldx=%lld), or the batch stride negative",
              (long long)D, (long long)ldx);
  hipLaunchKernelGGL(segment_sync_kernel, dim3((unsigned)ceil_div(D, SYNC_FT), grid_rows(B * n_seg)), dim3(SYNC_FT), 0,
                     (hipStream_t)stream, X, edges, out, B, T, ldx, bsx, n_seg, edge_bs, (int)D, aggregate);
  SYG_CHECK_LAUNCH("segment_sync");
  return SYG_OK;
}
