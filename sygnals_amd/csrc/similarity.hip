// Self-similarity of feature sequences: k nearest frames of every frame (librosa.segment.recurrence_matrix /
// cross_similarity without the dense distance matrix), the dense recurrence matrix scattered from those lists,
// librosa.decompose.nn_filter over them, and the two soft masks of REPET-SIM.  The float64 restatement that is the
// contract lives in tests/similarity_ref.py.
//
// Frame-major: X [B, T, D] are the query frames, Y [B, T', D] the frames searched (X itself for self-similarity, where the
// candidates of row i are the j with |i - j| >= width).  x_len / y_len [B] cut ragged clips: frames past a length are
// neither queries nor candidates.
//
// sim_knn_kernel is the fused form: a workgroup owns RT = 16 query rows of a clip and streams tiles of CT = 64 candidate
// columns.  A tile's 16 x 64 dot products are formed on v_mfma_f32_16x16x4_f32 (exact fp32, a fixed k-ordered chain), one
// 16 x 16 tile a wave, from chunks of DC = 64 features staged in LDS (rows of DC + 1 floats, so that the 64 lanes of an
// operand read hit 64 banks).  With the squared norms of a pre-pass the products become the selection value (squared
// distance ||x||^2 + ||y||^2 - 2 x.y, or the cosine distance), go through LDS to the wave that owns the row, and a value
// that beats the row's current k-th entry is inserted into the row's sorted list of 64-bit keys (value bits made
// orderable, then the column index: equal values resolve to the smaller index).  The 16 lists are 16 x 256 x 8 B = 32 KiB
// of LDS; nothing of size T T' passes through memory.
// The selection value loses near-duplicate frames to cancellation, so the kept entries of a row are recomputed from the
// frames themselves in float64 (sum of (x - y)^2, or 1 - x.y / sqrt(|x|^2 |y|^2), in a fixed order) and the list is put in
// the order of the recomputed values, then of the index.  Every value depends on the two frames alone, never on the tile or the
// workgroup they land in: equal frames give bit-equal distances.
#include <float.h>
#include <math.h>
#include <algorithm>
#include <cmath>
#include "host.h"

namespace syg {
namespace {

constexpr int NT = 256;                  // threads of a sim_knn workgroup (4 waves)
constexpr int K_MAX = 256;               // neighbours a row keeps at most
constexpr int RT = 16;                   // query rows of a workgroup
constexpr int CT = 64;                   // candidate columns of a tile (16 a wave)
constexpr int DC = 64;                   // features of a staged chunk
constexpr int FT = 64;                   // bins of an nn_filter tile (one wave)
constexpr int NORM_WGS_PER_CU = 16;      // sim_norms_kernel
constexpr int POINT_WGS_PER_CU = 16;     // repet_masks_kernel
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

// float bits that order as unsigned integers, and back
__device__ __forceinline__ uint32_t ord_bits(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_value(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }
__device__ __forceinline__ u64 lane_u64(u64 v, int src) {
  const int lo = __shfl((int)(uint32_t)v, src), hi = __shfl((int)(uint32_t)(v >> 32), src);
  return ((u64)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ int clip_len(const int* len, int64_t b, int64_t n) {
  if (!len) return (int)n;
  const int v = len[b];
  return v < 0 ? 0 : (v > n ? (int)n : v);
}

struct KnnArgs {
  const float* X; const float* Y; const int* xlen; const int* ylen;
  float* nx; float* ny;                  // squared norms [B, T], [B, Ty]
  int* idx; float* dist; int* count;
  int64_t B, T, Ty, ldx, ldy, bsx, bsy;
  int D, k, width, metric, self;
};

// ------------------------------------------------------------------ squared norms: a wave a frame, a fixed order
__global__ __launch_bounds__(NT) void sim_norms_kernel(const float* X, const int* len, float* out, int64_t B, int64_t T, int64_t ld,
                                                       int64_t bs, int D) {
  const int lane = threadIdx.x & 63;
  const int64_t rows = B * T;
  for (int64_t r = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * (NT / 64)) {
    const int64_t b = r / T, t = r - b * T;
    float s = 0.f;
    if (t < clip_len(len, b, T)) {
      const float* x = X + b * bs + t * ld;
      for (int d = lane; d < D; d += 64) s = fmaf(x[d], x[d], s);
    }
    s = wave_sum(s);
    if (lane == 0) out[r] = s;
  }
}

// The distance of two frames from the frames themselves, in float64 and a fixed order: one wave, every lane returns it.
// Cosine forms x.y, |x|^2 and |y|^2 in the same order, so that equal frames are at exactly 0, and near-duplicates keep
// their relative accuracy (1 - cos of a pair 1e-7 apart is all cancellation in float32).
__device__ __forceinline__ float exact_distance(const float* x, const float* y, int D, int metric, int lane) {
  if (metric == SYG_SIM_COSINE) {
    double xy = 0.0, xx = 0.0, yy = 0.0;
    for (int d = lane; d < D; d += 64) {
      const double a = (double)x[d], b = (double)y[d];
      xy = fma(a, b, xy); xx = fma(a, a, xx); yy = fma(b, b, yy);
    }
    xy = wave_sum_d(xy); xx = wave_sum_d(xx); yy = wave_sum_d(yy);
    return (float)(1.0 - xy / fmax(sqrt(xx * yy), (double)FLT_MIN));
  }
  double s = 0.0;
  for (int d = lane; d < D; d += 64) { const double e = (double)x[d] - (double)y[d]; s = fma(e, e, s); }
  s = wave_sum_d(s);
  return (float)(metric == SYG_SIM_EUCLIDEAN ? sqrt(s) : s);
}

// ------------------------------------------------------------------ k nearest frames
// Wave w forms the products of columns 16 w .. 16 w + 15 of a tile: lane (n, kk) supplies feature 16 kk + j at step j and
// holds the outputs (row 4 kk + i, column 16 w + n), i < 4.  Then wave w owns rows 4 w .. 4 w + 3 of the lists.
__global__ __launch_bounds__(NT) void sim_knn_kernel(KnnArgs P) {
  __shared__ u64 Ls[RT][K_MAX];
  __shared__ float Xs[RT][DC + 1];
  __shared__ float Ys[CT][DC + 1];
  __shared__ float Ds[RT][CT + 1];
  __shared__ float nxs[RT];
  __shared__ float nys[CT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = tid & 15, kk = (tid >> 4) & 3;
  const int D = P.D, k = P.k;
  const int64_t i0 = (int64_t)blockIdx.x * RT;
  for (int64_t b = blockIdx.y; b < P.B; b += gridDim.y) {
    const float* Xb = P.X + b * P.bsx;
    const float* Yb = P.self ? Xb : P.Y + b * P.bsy;
    const int64_t ldy = P.self ? P.ldx : P.ldy;
    const int xlen = clip_len(P.xlen, b, P.T);
    const int ylen = P.self ? xlen : clip_len(P.ylen, b, P.Ty);
    const float* nxb = P.nx + b * P.T;
    const float* nyb = P.self ? nxb : P.ny + b * P.Ty;
    __syncthreads();                                    // the previous clip's readers
    for (int q = tid; q < RT * K_MAX; q += NT) (&Ls[0][0])[q] = ~(u64)0;
    if (tid < RT) nxs[tid] = i0 + tid < xlen ? nxb[i0 + tid] : 0.f;
    __syncthreads();                                    // a row's sentinels come from all four waves: they are in before
                                                        // its wave reads them, also where no tile follows
    const bool any_row = i0 < xlen;                     // uniform in the workgroup
    for (int64_t j0 = 0; any_row && j0 < ylen; j0 += CT) {
      v4f acc = {0.f, 0.f, 0.f, 0.f};
      for (int d0 = 0; d0 < D; d0 += DC) {
        __syncthreads();                                // the previous chunk's and tile's readers
#pragma unroll
        for (int q = 0; q < RT * DC / NT; ++q) {
          const int e = tid + q * NT, r = e / DC, dl = e - r * DC;
          Xs[r][dl] = (i0 + r < xlen && d0 + dl < D) ? Xb[(i0 + r) * P.ldx + d0 + dl] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < CT * DC / NT; ++q) {
          const int e = tid + q * NT, r = e / DC, dl = e - r * DC;
          Ys[r][dl] = (j0 + r < ylen && d0 + dl < D) ? Yb[(j0 + r) * ldy + d0 + dl] : 0.f;
        }
        if (d0 == 0 && tid < CT) nys[tid] = j0 + tid < ylen ? nyb[j0 + tid] : 0.f;
        __syncthreads();
        v4f p0 = {0.f, 0.f, 0.f, 0.f}, p1 = {0.f, 0.f, 0.f, 0.f};
        const float* xr = &Xs[n][16 * kk];
        const float* yr = &Ys[16 * w + n][16 * kk];
#pragma unroll
        for (int j = 0; j < 16; j += 2) {
          p0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xr[j], yr[j], p0, 0, 0, 0);
          p1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xr[j + 1], yr[j + 1], p1, 0, 0, 0);
        }
        acc += p0 + p1;
      }
      {
        const float yn = nys[16 * w + n];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float xn = nxs[4 * kk + i];
          Ds[4 * kk + i][16 * w + n] = P.metric == SYG_SIM_COSINE ? 1.f - acc[i] / fmaxf(sqrtf(xn) * sqrtf(yn), FLT_MIN)
                                                                  : (xn + yn) - 2.f * acc[i];
        }
      }
      __syncthreads();
      for (int rr = 0; rr < 4; ++rr) {
        const int r = 4 * w + rr;
        const int64_t i = i0 + r;
        if (i >= xlen) continue;                         // uniform in the wave
        u64* L = &Ls[r][0];
        const float dv = Ds[r][lane];
        const int64_t j = j0 + lane;
        const int64_t gap = i > j ? i - j : j - i;
        const bool ok = j < ylen && (!P.self || gap >= P.width) && dv == dv;
        const u64 key = ((u64)ord_bits(dv) << 32) | (uint32_t)j;
        u64 thr = L[k - 1];
        u64 m = __ballot(ok && key < thr);
        while (m) {                                     // survivors in index order; the threshold falls as they go in
          const int sel = __builtin_ctzll(m);
          const u64 ck = lane_u64(key, sel);
          u64 v[K_MAX / 64];
          int pos = 0;
#pragma unroll
          for (int q = 0; q < K_MAX / 64; ++q) {
            const int p = lane + 64 * q;
            v[q] = p < k ? L[p] : ~(u64)0;
            pos += __popcll(__ballot(p < k && v[q] < ck));
          }
          wave_lds_sync();                              // every entry is read before one is moved
#pragma unroll
          for (int q = 0; q < K_MAX / 64; ++q) {
            const int p = lane + 64 * q;
            if (p + 1 < k && v[q] > ck) L[p + 1] = v[q];
          }
          if (lane == 0) L[pos] = ck;                   // pos < k: the k-th entry was larger than ck
          wave_lds_sync();
          thr = L[k - 1];
          m = __ballot(ok && lane > sel && key < thr);
        }
      }
    }
    // the kept entries again, from the frames themselves; then the list in the order of those values
    for (int rr = 0; rr < 4; ++rr) {
      const int r = 4 * w + rr;
      const int64_t i = i0 + r;
      if (i >= P.T) continue;                            // uniform in the wave
      u64* L = &Ls[r][0];
      int c = 0;                                         // the entries that were filled; a row past x_len keeps none
#pragma unroll
      for (int q = 0; q < K_MAX / 64; ++q) c += __popcll(__ballot(lane + 64 * q < k && L[lane + 64 * q] != ~(u64)0));
      if (i >= xlen) c = 0;
      const int64_t o = (b * P.T + i) * k;
      for (int e = 0; e < c; ++e) {
        const uint32_t j = (uint32_t)L[e];
        const float dv = exact_distance(Xb + i * P.ldx, Yb + (int64_t)j * ldy, D, P.metric, lane);
        if (lane == 0) L[e] = ((u64)ord_bits(dv) << 32) | j;
      }
      wave_lds_sync();
#pragma unroll
      for (int q = 0; q < K_MAX / 64; ++q) {
        const int p = lane + 64 * q;
        if (p < c) {
          const u64 key = L[p];
          int rank = 0;
          for (int e = 0; e < c; ++e) rank += L[e] < key ? 1 : 0;
          P.idx[o + rank] = (int)(uint32_t)key;
          P.dist[o + rank] = ord_value((uint32_t)(key >> 32));
        } else if (p < k) {
          P.idx[o + p] = -1;
          P.dist[o + p] = INFINITY;
        }
      }
      if (lane == 0) P.count[b * P.T + i] = c;
    }
  }
}

// ------------------------------------------------------------------ dense recurrence matrix from the lists
struct DenseArgs {
  const int* idx; const float* dist; const int* count; const double* bandwidth;
  float* out; float* rowmax;
  int64_t B, T, Ty; int k, mode, sym, self;
};

// A workgroup a row: zero fill, then one thread a list entry.  sym keeps (i, j) only if i is in j's list.  rowmax: the
// largest kept distance of the row, -1 where nothing is kept.  out may be null (the row maxima alone).
__global__ __launch_bounds__(NT) void sim_dense_kernel(DenseArgs P) {
  __shared__ float red[NT / 64];
  const int tid = threadIdx.x;
  const int64_t i = blockIdx.x;
  for (int64_t b = blockIdx.y; b < P.B; b += gridDim.y) {
    float* row = P.out ? P.out + (b * P.T + i) * P.Ty : nullptr;
    if (row) {
      for (int64_t j = tid; j < P.Ty; j += NT) row[j] = 0.f;
    }
    __syncthreads();                                    // the zeros are in before an entry lands on them; red is free
    const int64_t lo = (b * P.T + i) * P.k;
    int c = P.count[b * P.T + i];
    c = c < 0 ? 0 : (c > P.k ? P.k : c);
    float mx = -1.f;
    if (tid < c) {
      const int j = P.idx[lo + tid];
      bool keep = j >= 0 && j < P.Ty;
      if (keep && P.sym) {
        const int64_t lj = (b * P.T + j) * P.k;
        int cj = P.count[b * P.T + j];
        cj = cj < 0 ? 0 : (cj > P.k ? P.k : cj);
        bool found = false;
        for (int e = 0; e < cj; ++e) found = found || P.idx[lj + e] == (int)i;
        keep = found;
      }
      if (keep) {
        const float d = P.dist[lo + tid];
        mx = d;
        if (row) {
          row[j] = P.mode == SYG_SIM_CONNECTIVITY ? 1.f
                 : P.mode == SYG_SIM_DISTANCE   ? d
                                                : (float)exp(-(double)d / P.bandwidth[b]);
        }
      }
    }
    if (P.rowmax) {
      mx = wave_max(mx);
      if ((tid & 63) == 0) red[tid >> 6] = mx;
    }
    __syncthreads();                                    // the entries are in before the diagonal
    if (tid == 0) {
      if (P.rowmax) P.rowmax[b * P.T + i] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
      if (row && P.self && i < P.Ty) row[i] = P.mode == SYG_SIM_DISTANCE ? 0.f : 1.f;
    }
  }
}

// ------------------------------------------------------------------ nn_filter
struct FilterArgs {
  const float* S; const int* idx; const int* count; const float* weights; const double* bandwidth; float* out;
  int64_t B, T, lds, bss; int F, k, nft;
};

// A wave takes FT bins of a frame.  mean / average: gather and accumulate in float64, in list order.  median: the
// neighbours' values of the tile as orderable bits in LDS [k][FT]; each lane finds the middle value(s) of its column by a
// 32-step bisection over the bits, so the result is an input value bit for bit at odd counts.
template <int AGG>
__global__ __launch_bounds__(64) void nn_filter_kernel(FilterArgs P) {
  extern __shared__ uint32_t tile[];                    // median: [k][FT]
  const int lane = threadIdx.x;
  const int ft = blockIdx.x % P.nft;
  const int64_t i = blockIdx.x / P.nft;
  const int f = ft * FT + lane;
  const bool in = f < P.F;
  for (int64_t b = blockIdx.y; b < P.B; b += gridDim.y) {
    const float* Sb = P.S + b * P.bss;
    const int64_t lo = (b * P.T + i) * P.k;
    int c = P.count[b * P.T + i];
    c = c < 0 ? 0 : (c > P.k ? P.k : c);
    const float own = in ? Sb[i * P.lds + f] : 0.f;
    float res = own;
    if (AGG == SYG_NN_MEDIAN) {
      wave_lds_sync();                                  // the previous clip's readers
      for (int e = 0; e < c; ++e) {
        int j = P.idx[lo + e];
        j = j < 0 ? 0 : (j >= P.T ? (int)(P.T - 1) : j);
        tile[e * FT + lane] = ord_bits(in ? Sb[(int64_t)j * P.lds + f] : 0.f);
      }
      wave_lds_sync();
      if (c > 0) {
        const int m = (c - 1) >> 1;                     // rank of the lower middle value
        uint32_t v = 0;
        for (int bit = 31; bit >= 0; --bit) {           // the largest v with #(values < v) <= m is the value of rank m
          const uint32_t trial = v | (1u << bit);
          int below = 0;
          for (int e = 0; e < c; ++e) below += tile[e * FT + lane] < trial ? 1 : 0;
          if (below <= m) v = trial;
        }
        if (c & 1) {
          res = ord_value(v);
        } else {                                        // the upper middle: v again if it fills rank m + 1, else the next value
          int upto = 0;
          uint32_t next = 0xFFFFFFFFu;
          for (int e = 0; e < c; ++e) {
            const uint32_t t = tile[e * FT + lane];
            upto += t <= v ? 1 : 0;
            if (t > v && t < next) next = t;
          }
          const float a = ord_value(v), hi = ord_value(upto > m + 1 ? v : next);
          res = (float)(((double)a + (double)hi) * 0.5);
        }
      }
    } else {
      double num = 0.0, den = 0.0;
      for (int e = 0; e < c; ++e) {
        int j = P.idx[lo + e];
        j = j < 0 ? 0 : (j >= P.T ? (int)(P.T - 1) : j);
        double wgt = 1.0;
        if (AGG == SYG_NN_AVERAGE) wgt = P.bandwidth ? exp(-(double)P.weights[lo + e] / P.bandwidth[b]) : (double)P.weights[lo + e];
        num = fma(wgt, in ? (double)Sb[(int64_t)j * P.lds + f] : 0.0, num);
        den += wgt;
      }
      if (c > 0 && den != 0.0) res = (float)(num / den);
    }
    if (in) P.out[(b * P.T + i) * P.F + f] = res;
  }
}

// ------------------------------------------------------------------ REPET-SIM masks
// librosa.util.softmask(X, X_ref, power, split_zeros=False) for one cell
__device__ __forceinline__ float softmask_cell(float X, float Xr, float power) {
  const float Z = fmaxf(X, Xr);
  if (Z < FLT_MIN) return 0.f;
  const float a = X / Z, r = Xr / Z;
  float m, q;
  if (power == 1.f) { m = a; q = r; }
  else if (power == 2.f) { m = a * a; q = r * r; }
  else { m = powf(a, power); q = powf(r, power); }
  return m / (m + q);
}

__global__ __launch_bounds__(NT) void repet_masks_kernel(const float* S, const float* R, float* Mf, float* Mb, int64_t n, float mb,
                                                         float mf, float power) {
  for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) {
    const float s = S[e], sf = fminf(s, R[e]), rest = s - sf;
    Mb[e] = softmask_cell(sf, mb * rest, power);
    Mf[e] = softmask_cell(rest, mf * sf, power);
  }
}

inline bool knn_shape_ok(int64_t B, int64_t T, int64_t Ty, int64_t D) {
  const int64_t big = (int64_t)1 << 30;
  return B >= 1 && T >= 1 && Ty >= 1 && D >= 1 && T <= big && Ty <= big && D <= big && B <= ((int64_t)1 << 40) / std::max(T, Ty);
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int syg_sim_k_max(void) { return K_MAX; }

extern "C" int64_t syg_sim_knn_work_bytes(int64_t B, int64_t T, int64_t Ty, int has_y) {
  if (!knn_shape_ok(B, T, Ty, 1) || (has_y != 0 && has_y != 1)) {
    set_error("sim_knn_work_bytes: served are B >= 1, T and T' in [1, 2^30], has_y 0 or 1 (got B=%lld, T=%lld, T'=%lld, has_y=%d)",
              (long long)B, (long long)T, (long long)Ty, has_y);
    return -1;
  }
  return (B * (T + (has_y ? Ty : 0)) * (int64_t)sizeof(float) + 7) / 8 * 8;
}

extern "C" int syg_sim_knn_f32(const float* X, const float* Y, int64_t B, int64_t T, int64_t Ty, int64_t D, int64_t ldx, int64_t ldy,
                               int64_t bsx, int64_t bsy, const int* x_len, const int* y_len, int64_t k, int64_t width, int metric,
                               int* idx, float* dist, int* count, void* work, void* stream) {
  SYG_REQUIRE(X && idx && dist && count && work, "sim_knn: null pointer argument (X / idx / dist / count / work)");
  if (!Y) Ty = T;
  SYG_REQUIRE(knn_shape_ok(B, T, Ty, D), "sim_knn: served are B >= 1, T, T' and D in [1, 2^30] (got B=%lld, T=%lld, T'=%lld, D=%lld)",
              (long long)B, (long long)T, (long long)Ty, (long long)D);
  SYG_REQUIRE(k >= 1 && k <= K_MAX, "sim_knn: k must be in [1, %d] (got %lld)", K_MAX, (long long)k);
  SYG_REQUIRE(width >= 1 && width <= ((int64_t)1 << 30), "sim_knn: width must be in [1, 2^30] (got %lld)", (long long)width);
  SYG_REQUIRE(!Y || width == 1, "sim_knn: width applies to self-similarity; with Y it must be 1 (got %lld)", (long long)width);
  SYG_REQUIRE(metric == SYG_SIM_EUCLIDEAN || metric == SYG_SIM_SQEUCLIDEAN || metric == SYG_SIM_COSINE,
              "sim_knn: metric must be SYG_SIM_EUCLIDEAN (0), SYG_SIM_SQEUCLIDEAN (1) or SYG_SIM_COSINE (2); cityblock has no "
              "contraction form and is not served (got %d)", metric);
  SYG_REQUIRE(ldx >= D && (!Y || ldy >= D), "sim_knn: a row stride is smaller than D=%lld (ldx=%lld, ldy=%lld)", (long long)D,
              (long long)ldx, (long long)ldy);
  SYG_REQUIRE(bsx >= 0 && bsy >= 0, "sim_knn: negative batch stride");
  SYG_REQUIRE(Y || !y_len, "sim_knn: y_len needs Y (self-similarity takes x_len for both)");
  hipStream_t s = (hipStream_t)stream;
  float* nx = (float*)work;
  float* ny = Y ? nx + B * T : nx;
  hipLaunchKernelGGL(sim_norms_kernel, dim3(capped_grid(ceil_div(B * T, NT / 64), NORM_WGS_PER_CU)), dim3(NT), 0, s, X, x_len, nx, B, T,
                     ldx, bsx, (int)D);
  SYG_CHECK_LAUNCH("sim_knn (norms of X)");
  if (Y) {
    hipLaunchKernelGGL(sim_norms_kernel, dim3(capped_grid(ceil_div(B * Ty, NT / 64), NORM_WGS_PER_CU)), dim3(NT), 0, s, Y, y_len, ny, B,
                       Ty, ldy, bsy, (int)D);
    SYG_CHECK_LAUNCH("sim_knn (norms of Y)");
  }
  KnnArgs P{X, Y, x_len, y_len, nx, ny, idx, dist, count, B, T, Ty, ldx, ldy, bsx, bsy, (int)D, (int)k, (int)width, metric, Y ? 0 : 1};
  hipLaunchKernelGGL(sim_knn_kernel, dim3((unsigned)ceil_div(T, RT), grid_rows(B)), dim3(NT), 0, s, P);
  SYG_CHECK_LAUNCH("sim_knn");
  return SYG_OK;
}

extern "C" int syg_sim_dense_f32(const int* idx, const float* dist, const int* count, int64_t B, int64_t T, int64_t Ty, int64_t k,
                                 int mode, int sym, int self, const double* bandwidth, float* out, float* rowmax, void* stream) {
  SYG_REQUIRE(idx && dist && count && (out || rowmax), "sim_dense: null pointer argument (idx / dist / count, and out or rowmax)");
  SYG_REQUIRE(knn_shape_ok(B, T, Ty, 1), "sim_dense: served are B >= 1, T and T' in [1, 2^30] (got B=%lld, T=%lld, T'=%lld)",
              (long long)B, (long long)T, (long long)Ty);
  SYG_REQUIRE(k >= 1 && k <= K_MAX, "sim_dense: k must be in [1, %d] (got %lld)", K_MAX, (long long)k);
  SYG_REQUIRE(mode == SYG_SIM_CONNECTIVITY || mode == SYG_SIM_DISTANCE || mode == SYG_SIM_AFFINITY,
              "sim_dense: mode must be SYG_SIM_CONNECTIVITY (0), SYG_SIM_DISTANCE (1) or SYG_SIM_AFFINITY (2) (got %d)", mode);
  SYG_REQUIRE((sym == 0 || sym == 1) && (self == 0 || self == 1), "sim_dense: sym and self are 0 or 1");
  SYG_REQUIRE(!(sym || self) || T == Ty, "sim_dense: sym and self need a square matrix (T=%lld, T'=%lld)", (long long)T, (long long)Ty);
  SYG_REQUIRE(!out || mode != SYG_SIM_AFFINITY || bandwidth, "sim_dense: SYG_SIM_AFFINITY needs bandwidth [B]");
  SYG_REQUIRE(B <= ((int64_t)1 << 40) / T / Ty || !out, "sim_dense: the output is too large");
  DenseArgs P{idx, dist, count, bandwidth, out, rowmax, B, T, Ty, (int)k, mode, sym, self};
  hipLaunchKernelGGL(sim_dense_kernel, dim3((unsigned)T, grid_rows(B)), dim3(NT), 0, (hipStream_t)stream, P);
  SYG_CHECK_LAUNCH("sim_dense");
  return SYG_OK;
}

extern "C" int syg_nn_filter_f32(const float* S, int64_t B, int64_t T, int64_t F, int64_t lds, int64_t bss, const int* idx,
                                 const int* count, int64_t k, const float* weights, const double* bandwidth, int aggregate, float* out,
                                 void* stream) {
  SYG_REQUIRE(S && idx && count && out, "nn_filter: null pointer argument (S / idx / count / out)");
  SYG_REQUIRE(knn_shape_ok(B, T, T, F) && T * ceil_div(F, FT) < ((int64_t)1 << 31),
              "nn_filter: served are B >= 1, T and F in [1, 2^30] with T ceil(F / 64) < 2^31 (got B=%lld, T=%lld, F=%lld)", (long long)B,
              (long long)T, (long long)F);
  SYG_REQUIRE(k >= 1 && k <= K_MAX, "nn_filter: k must be in [1, %d] (got %lld)", K_MAX, (long long)k);
  SYG_REQUIRE(aggregate == SYG_NN_MEAN || aggregate == SYG_NN_AVERAGE || aggregate == SYG_NN_MEDIAN,
              "nn_filter: aggregate must be SYG_NN_MEAN (0), SYG_NN_AVERAGE (1) or SYG_NN_MEDIAN (2) (got %d)", aggregate);
  SYG_REQUIRE(aggregate != SYG_NN_AVERAGE || weights, "nn_filter: SYG_NN_AVERAGE needs weights [B, T, k]");
  SYG_REQUIRE(lds >= F && bss >= 0, "nn_filter: the row stride is smaller than F=%lld (lds=%lld), or the batch stride negative",
              (long long)F, (long long)lds);
  const int nft = (int)ceil_div(F, FT);
  FilterArgs P{S, idx, count, weights, bandwidth, out, B, T, lds, bss, (int)F, (int)k, nft};
  const dim3 grid((unsigned)(T * nft), grid_rows(B));
  hipStream_t s = (hipStream_t)stream;
  if (aggregate == SYG_NN_MEDIAN)
    hipLaunchKernelGGL((nn_filter_kernel<SYG_NN_MEDIAN>), grid, dim3(64), (size_t)k * FT * sizeof(uint32_t), s, P);
  else if (aggregate == SYG_NN_AVERAGE) hipLaunchKernelGGL((nn_filter_kernel<SYG_NN_AVERAGE>), grid, dim3(64), 0, s, P);
  else hipLaunchKernelGGL((nn_filter_kernel<SYG_NN_MEAN>), grid, dim3(64), 0, s, P);
  SYG_CHECK_LAUNCH("nn_filter");
  return SYG_OK;
}

extern "C" int syg_repet_masks_f32(const float* S, const float* Sf, int64_t n, double margin_b, double margin_f, double power,
                                   float* mask_f, float* mask_b, void* stream) {
  SYG_REQUIRE(S && Sf && mask_f && mask_b, "repet_masks: null pointer argument (S / Sf / mask_f / mask_b)");
  SYG_REQUIRE(n >= 1 && n <= ((int64_t)1 << 40), "repet_masks: n must be in [1, 2^40] (got %lld)", (long long)n);
  SYG_REQUIRE(margin_b > 0 && margin_f > 0 && power > 0 && std::isfinite(margin_b) && std::isfinite(margin_f) && std::isfinite(power),
              "repet_masks: margin_b, margin_f and power must be positive and finite");
  hipLaunchKernelGGL(repet_masks_kernel, dim3(capped_grid(ceil_div(n, NT), POINT_WGS_PER_CU)), dim3(NT), 0, (hipStream_t)stream, S, Sf,
                     mask_f, mask_b, n, (float)margin_b, (float)margin_f, (float)power);
  SYG_CHECK_LAUNCH("repet_masks");
  return SYG_OK;
}
