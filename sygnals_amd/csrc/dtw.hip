// Dynamic time warping, librosa.sequence.dtw with its default step set [[1,1],[0,1],[1,0]]:
//     C[n, m] = metric(X[:, n], Y[:, m])                                            (dtw_cost_kernel, float32)
//     D[n, m] = min_k ( D[n - s0_k, m - s1_k] + (w_mul_k C[n, m] + w_add_k) )       (dtw_accum_kernel, float64)
//     path    = the steps walked back from the end cell                              (dtw_backtrack_kernel)
// The float64 restatement that is the contract lives in tests/dtw_ref.py.
//
// Cost.  The three difference metrics are sums of f(x_k - y_k) over k in ascending order, never the
// |x|^2 + |y|^2 - 2 x.y form: a frame against itself costs exactly 0.  A block owns a 64 x 64 tile of one pair and
// stages DC_KC features of its 64 X frames and 64 Y frames in LDS at a time; a thread holds 4 x 4 cells.  Features
// past K and frames past a pair's length are staged as zeros, which add exactly nothing to any of the four sums.
//
// Recurrence.  A cell is librosa's inner loop word for word: it starts from its preset (C on the first cell, on the
// whole first row under subseq, infinity elsewhere) and takes the three candidates in the order diagonal, left, up, a
// later one only if strictly smaller.  A neighbour outside the matrix is infinity, so no cell needs a border case.
// The accumulators are float64 and the file is compiled with contraction off: t = w_mul C, t = t + w_add, t = D + t
// are three roundings as in NumPy, so with the default weights D equals a float64 NumPy evaluation bit for bit.
//
// One wave owns a tile (the whole matrix of a pair in the pair-resident form).  Lane l owns the R columns
// [l R, (l + 1) R) of the tile and keeps row n - 1 of them in registers.  At step t lane l does row t - l: the skew of
// one lane a step makes the cell to the left of a lane's run the value its left neighbour finished one step earlier,
// which crosses lanes with one whole-wave DPP shift of the two halves of the double; the diagonal neighbour is the
// value received the step before.  Only that live diagonal is ever held: 2 R + 2 doubles a lane.  C rows are fetched
// DW_P steps ahead into registers.  A tile of h rows takes h + lanes - 1 steps.
//
// Tiled form.  The matrix is cut into tiles of `tile` x `tile` cells and the tiles of one block anti-diagonal run in
// one launch, tn + tm - 1 launches in all on the caller's stream; no workgroup ever waits for another inside a launch.
// A tile hands its last row and last column on through a float64 workspace in which every tile row has a row of M
// values of its own and every tile column a column of N values: no cell of the workspace is written twice, so a tile
// that reads its corner D[n0 - 1, m0 - 1] cannot meet a tile of the same launch writing there.  The left column of a
// tile is staged in LDS (one coalesced read) instead of one dependent global read a step.
//
// Step codes are one byte a cell, not two bits: lanes of a wave are on different rows at the same moment and tiles of
// one launch border each other, so with packed codes two writers would share a byte and every store would become a
// read-modify-write across lanes and across tiles.  A byte a cell is 1/4 of the bytes of the C read.
//
// No atomics; every cell is computed once by one lane in an order that does not depend on the batch: the same call gives
// the same bits and a batch equals its pairs.
#include <math.h>
#include "host.h"

#pragma clang fp contract(off)

namespace syg {
namespace {

constexpr int DC_T = 64;                   // cost kernel: tile edge
constexpr int DC_KC = 16;                  // cost kernel: features per LDS stage
constexpr int DW_WAVES = 4;                // recurrence: waves per workgroup, each with a tile of its own
constexpr int DW_RMAX = 16;                // recurrence: longest column run of a lane
constexpr int DW_COLS_MAX = 64 * DW_RMAX;  // widest tile: the pair-resident form's widest matrix
constexpr int DW_TILE = 256;               // tiled form: product tile edge
constexpr int DW_P = 4;                    // recurrence: steps a C row is fetched ahead
constexpr int64_t DW_LAUNCH_MAX = 16384;   // tiled form: most launches (block anti-diagonals) of a call
constexpr int64_t DW_DIM_MAX = (int64_t)1 << 30;

enum { DTW_EUCLIDEAN = 0, DTW_SQEUCLIDEAN = 1, DTW_CITYBLOCK = 2, DTW_COSINE = 3 };

struct DcArgs {
  const float* X; const float* Y;
  int64_t K, N, M, ldx, ldy, bsx, bsy;
  const int32_t* x_len; const int32_t* y_len;
  float* C;
};

// a pair's length: the caller's, held inside [1, full] whatever the device array says
__device__ __forceinline__ int64_t dtw_len(const int32_t* len, int64_t b, int64_t full) {
  if (!len) return full;
  const int64_t v = len[b];
  return v < 1 ? 1 : (v > full ? full : v);
}

template <int METRIC>
__global__ __launch_bounds__(256) void dtw_cost_kernel(DcArgs A) {
  __shared__ float xs[DC_KC][DC_T];
  __shared__ float ys[DC_KC][DC_T];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t b = blockIdx.z, n0 = (int64_t)blockIdx.y * DC_T, m0 = (int64_t)blockIdx.x * DC_T;
  const int64_t xl = dtw_len(A.x_len, b, A.N), yl = dtw_len(A.y_len, b, A.M);
  const float* __restrict__ Xb = A.X + b * A.bsx;
  const float* __restrict__ Yb = A.Y + b * A.bsy;
  float acc[4][4], nx[4], ny[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    nx[i] = 0.f; ny[i] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  }
  const bool live = n0 < xl && m0 < yl;    // block-uniform: a tile in a pair's padding only writes zeros
  if (live) {
    for (int64_t k0 = 0; k0 < A.K; k0 += DC_KC) {
#pragma unroll
      for (int r = 0; r < DC_KC * DC_T / 256; ++r) {
        const int idx = tid + 256 * r, kk = idx >> 6, c = idx & 63;
        const int64_t k = k0 + kk, n = n0 + c, m = m0 + c;
        xs[kk][c] = (k < A.K && n < xl) ? Xb[k * A.ldx + n] : 0.f;
        ys[kk][c] = (k < A.K && m < yl) ? Yb[k * A.ldy + m] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < DC_KC; ++kk) {
        float xv[4], yv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { xv[i] = xs[kk][4 * ty + i]; yv[i] = ys[kk][tx + 16 * i]; }
        if (METRIC == DTW_COSINE) {
#pragma unroll
          for (int i = 0; i < 4; ++i) { nx[i] = fmaf(xv[i], xv[i], nx[i]); ny[i] = fmaf(yv[i], yv[i], ny[i]); }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float d = xv[i] - yv[j];
            if (METRIC == DTW_CITYBLOCK) acc[i][j] = acc[i][j] + fabsf(d);
            else if (METRIC == DTW_COSINE) acc[i][j] = fmaf(xv[i], yv[j], acc[i][j]);
            else acc[i][j] = fmaf(d, d, acc[i][j]);
          }
      }
      __syncthreads();
    }
  }
  float* __restrict__ Cb = A.C + b * A.N * A.M;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t n = n0 + 4 * ty + i, m = m0 + tx + 16 * j;
      if (n >= A.N || m >= A.M) continue;
      float v = acc[i][j];
      if (METRIC == DTW_EUCLIDEAN) v = sqrtf(v);
      if (METRIC == DTW_COSINE) v = 1.f - v / (sqrtf(nx[i]) * sqrtf(ny[j]));      // a zero-norm frame: 0 / 0, NaN as cdist
      Cb[n * A.M + m] = (n < xl && m < yl) ? v : 0.f;
    }
}

struct DwArgs {
  const float* C; int64_t ldc, bsc;
  int64_t B, N, M;
  const int32_t* x_len; const int32_t* y_len;
  double wm0, wm1, wm2, wa0, wa1, wa2;
  int subseq;
  double* D; uint8_t* steps; double* cost; int32_t* end_col;
  double* rowws; double* colws;            // [B, tn, M] last rows of the tile rows | [B, tm, N] last columns
  int64_t th, tw;                          // tile height and width (the whole matrix in the pair-resident form)
  int64_t tn, tm;                          // tile grid
  int64_t diag, i_lo, cnt;                 // this launch: tiles (i, diag - i), i in [i_lo, i_lo + cnt)
};

__device__ __forceinline__ double dw_shr1(double v) {      // lane l receives lane l - 1's value (lane 0: unused)
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), DPP_WAVE_SHR1, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), DPP_WAVE_SHR1, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

typedef float dw_f32x4 __attribute__((ext_vector_type(4)));

// R: columns a lane.  UNITW: the weights are 1 and 0.  VEC (R >= 4; the host's dw_vec_ok): every row of C, D and the
// step codes starts 16-byte aligned at every lane's run and every tile is a multiple of four columns wide, so a lane moves
// its run in 16-byte pieces.  Lanes of a wave are on 64 different rows, so every memory instruction touches 64 cache
// lines whatever its width: four times fewer instructions are four times fewer line accesses, which is what bounds a
// step (measured: the recurrence of 256 pairs of 1000 x 1000 with step codes, 6.3 ms with one element an instruction).
template <int R, bool UNITW, bool VEC>
__global__ __launch_bounds__(64 * DW_WAVES) void dtw_accum_kernel(DwArgs A) {
  __shared__ double left_s[DW_WAVES][DW_COLS_MAX];         // D[n0 .. n0 + h, m0 - 1] of the tile (tiled form only)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * DW_WAVES + wv;
  if (w >= A.B * A.cnt) return;                            // wave-uniform, and no workgroup barrier below
  const int64_t b = w / A.cnt, i = A.i_lo + w % A.cnt, j = A.diag - i;
  const int64_t xl = dtw_len(A.x_len, b, A.N), yl = dtw_len(A.y_len, b, A.M);
  const int64_t n0 = i * A.th, m0 = j * A.tw;
  if (n0 >= xl || m0 >= yl) return;                        // a tile in the pair's padding
  const int64_t h = (xl - n0 < A.th) ? xl - n0 : A.th, wd = (yl - m0 < A.tw) ? yl - m0 : A.tw;
  const int64_t mend = m0 + wd;                            // one past the tile's last column
  const int used = (int)((wd + R - 1) / R);                // lanes that own a column
  const int64_t mc = m0 + (int64_t)lane * R;               // this lane's first column
  const bool has_cols = lane < used;
  const double INF = __builtin_inf();

  const bool from_left = j > 0 && A.colws, from_top = i > 0 && A.rowws;
  if (from_left) {
    const double* __restrict__ lc = A.colws + (b * A.tm + (j - 1)) * A.N + n0;
    for (int64_t r = lane; r < h; r += 64) left_s[wv][r] = lc[r];
    wave_lds_sync();
  }
  const double* __restrict__ top = from_top ? A.rowws + (b * A.tn + (i - 1)) * A.M : nullptr;
  double prev[R];                                          // D[n - 1, mc + jj]
#pragma unroll
  for (int jj = 0; jj < R; ++jj) prev[jj] = (top && mc + jj < mend) ? top[mc + jj] : INF;
  double Lcur = (top && has_cols && mc >= 1) ? top[mc - 1] : INF;      // D[n - 1, mc - 1] at the lane's first row
  double last = INF;                                       // D[n, mc + R - 1] of the row this lane finished last
  double bv = INF; int bi = 0x7fffffff;                    // subseq: least value of the pair's last row in this lane's run

  const float* __restrict__ Cb = A.C + b * A.bsc;
  double* __restrict__ Db = A.D ? A.D + b * A.N * A.M : nullptr;
  uint8_t* __restrict__ Sb = A.steps ? A.steps + b * A.N * A.M : nullptr;
  double* __restrict__ roww = (A.rowws && i < A.tn - 1) ? A.rowws + (b * A.tn + i) * A.M : nullptr;
  double* __restrict__ colw = (A.colws && j < A.tm - 1) ? A.colws + (b * A.tm + j) * A.N : nullptr;
  const int64_t nsteps = h + used - 1;

  const int nv = has_cols ? (int)(mend - mc < R ? mend - mc : R) : 0;     // columns of this lane's run inside the tile
  const int64_t mcl = has_cols ? mc : mend - 1;            // a column of the tile whatever the lane
  const int jtop = nv > 0 ? nv - 1 : 0;
  // C of the row this lane does at step t.  Unconditional, at addresses held inside the tile (a lane outside its rows or
  // columns fetches a cell it does not use): a fixed count of loads a step lets a step wait for the loads of DW_P steps
  // ago alone instead of for everything in flight.
  auto load = [&](int64_t t, float (&cb)[R]) {
    int64_t nl = t - lane;
    nl = nl < 0 ? 0 : (nl > h - 1 ? h - 1 : nl);
    if (VEC) {
      const float* __restrict__ row = Cb + (n0 + nl) * A.ldc;
#pragma unroll
      for (int g = 0; g < R / 4; ++g) {
        const dw_f32x4 v = *(const dw_f32x4*)(row + (4 * g < nv ? mc + 4 * g : mend - 4));
#pragma unroll
        for (int e = 0; e < 4; ++e) cb[4 * g + e] = v[e];
      }
    } else {
      const float* __restrict__ row = Cb + (n0 + nl) * A.ldc + mcl;
#pragma unroll
      for (int jj = 0; jj < R; ++jj) cb[jj] = row[jj < jtop ? jj : jtop];
    }
  };
  auto step = [&](int64_t t, const float (&cb)[R]) {
    const double recv = dw_shr1(last);                     // every lane takes part in the shift
    const int64_t nl = t - lane;
    if (nl < 0 || nl >= h || !has_cols) return;
    const int64_t n = n0 + nl;
    const double Lprev = Lcur;
    Lcur = lane == 0 ? (from_left ? left_s[wv][nl] : INF) : recv;
    double dg = Lprev, lf = Lcur;
    const bool pre_row = n == 0 && A.subseq, pre_first = n == 0 && mc == 0;
    int code[R];
    // every cell of the run, also past the tile's last column (only the last lane with columns has such cells: what they
    // hold goes nowhere); the stores below are the only thing that asks where the tile ends.  min() takes the lesser
    // value as the strict comparisons of the loops do; the code is what those comparisons would have left.
#pragma unroll
    for (int jj = 0; jj < R; ++jj) {
      const double c = (double)cb[jj], up = prev[jj];
      const double pre = (pre_row || (jj == 0 && pre_first)) ? c : INF;
      double t0, t1, t2;
      if (UNITW) {                                         // weights 1 and 0: 1 c is c, and c + 0 is formed once
        const double cw = c + 0.0;
        t0 = dg + cw; t1 = lf + cw; t2 = up + cw;
      } else {
        t0 = A.wm0 * c; t0 = t0 + A.wa0; t0 = dg + t0;
        t1 = A.wm1 * c; t1 = t1 + A.wa1; t1 = lf + t1;
        t2 = A.wm2 * c; t2 = t2 + A.wa2; t2 = up + t2;
      }
      const double b0 = fmin(pre, t0), b1 = fmin(b0, t1), best = fmin(b1, t2);
      int k = t1 < b0 ? 1 : 0;
      k = t2 < b1 ? 2 : k;
      prev[jj] = best; code[jj] = k; dg = up; lf = best;
    }
    last = lf;
    if (Db) {
      double* __restrict__ drow = Db + n * A.M + mc;
      if (VEC) {
#pragma unroll
        for (int q = 0; q < R / 2; ++q)
          if (2 * q < nv) *(double2*)(drow + 2 * q) = make_double2(prev[2 * q], prev[2 * q + 1]);
      } else {
#pragma unroll
        for (int jj = 0; jj < R; ++jj)
          if (jj < nv) drow[jj] = prev[jj];
      }
    }
    if (Sb) {
      uint8_t* __restrict__ srow = Sb + n * A.M + mc;
      if (VEC) {
#pragma unroll
        for (int g = 0; g < R / 4; ++g)
          if (4 * g < nv)
            *(uint32_t*)(srow + 4 * g) = (uint32_t)code[4 * g] | ((uint32_t)code[4 * g + 1] << 8) |
                                         ((uint32_t)code[4 * g + 2] << 16) | ((uint32_t)code[4 * g + 3] << 24);
      } else {
#pragma unroll
        for (int jj = 0; jj < R; ++jj)
          if (jj < nv) srow[jj] = (uint8_t)code[jj];
      }
    }
    if (lane == used - 1) {                                // the owner of the tile's last column (stores under their own
#pragma unroll                                             // condition: a chain of selects would index prev[] in scratch)
      for (int jj = 0; jj < R; ++jj)
        if (jj == nv - 1) {
          if (colw) colw[n] = prev[jj];
          if (!A.subseq && n == xl - 1 && mend == yl) { A.cost[b] = prev[jj]; A.end_col[b] = (int32_t)(yl - 1); }
        }
    }
    if (roww && nl == h - 1) {
#pragma unroll
      for (int jj = 0; jj < R; ++jj)
        if (jj < nv) roww[mc + jj] = prev[jj];
    }
    if (A.subseq && n == xl - 1) {
#pragma unroll
      for (int jj = 0; jj < R; ++jj)
        if (jj < nv && prev[jj] < bv) { bv = prev[jj]; bi = (int)(mc + jj); }
    }
  };

  float cb[DW_P][R];
#pragma unroll
  for (int u = 0; u < DW_P; ++u) {
#pragma unroll
    for (int jj = 0; jj < R; ++jj) cb[u][jj] = 0.f;
    load(u, cb[u]);
  }
  for (int64_t t0 = 0; t0 < nsteps; t0 += DW_P) {
#pragma unroll
    for (int u = 0; u < DW_P; ++u) {
      const int64_t t = t0 + u;
      if (t < nsteps) {                                    // wave-uniform
        step(t, cb[u]);
        load(t + DW_P, cb[u]);
      }
    }
  }

  if (A.subseq && n0 + h == xl) {                          // the tile holds part of the pair's last row
    // first arg-min as np.argmin: the lesser value, the lesser column on a tie
    wave_pick<false>(bv, bi);
    // the tiles of a tile row run in launches of their own, left to right: a later one replaces only if strictly less
    if (lane == 0 && (j == 0 || bv < A.cost[b])) { A.cost[b] = bv; A.end_col[b] = bi; }
  }
}

struct BtArgs {
  const uint8_t* steps; int64_t B, N, M;
  const int32_t* x_len; const int32_t* y_len; const int32_t* end_col;
  int subseq;
  int32_t* path; int32_t* path_len;
};

// one lane walks a pair: at most N + M - 1 dependent one-byte reads
__global__ __launch_bounds__(64) void dtw_backtrack_kernel(BtArgs A) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= A.B) return;
  const int64_t xl = dtw_len(A.x_len, b, A.N), yl = dtw_len(A.y_len, b, A.M), cap = A.N + A.M - 1;
  int64_t n = xl - 1, m = yl - 1;
  if (A.subseq) { m = A.end_col[b]; m = m < 0 ? 0 : (m > yl - 1 ? yl - 1 : m); }
  const uint8_t* __restrict__ Sb = A.steps + b * A.N * A.M;
  int2* __restrict__ p = (int2*)A.path + b * cap;
  int64_t len = 0;
  p[len++] = make_int2((int)n, (int)m);
  while (A.subseq ? n > 0 : (n > 0 || m > 0)) {
    const int code = Sb[n * A.M + m] & 3;
    n -= (code != 1); m -= (code != 2);                    // 0: (1, 1)   1: (0, 1)   2: (1, 0)
    if (n < 0 || m < 0 || len >= cap) break;               // librosa: stop where the walk leaves the matrix
    p[len++] = make_int2((int)n, (int)m);
  }
  A.path_len[b] = (int32_t)len;
  for (int64_t q = len; q < cap; ++q) p[q] = make_int2(-1, -1);
}

int dtw_check_shape(int64_t B, int64_t N, int64_t M) {
  SYG_REQUIRE(N >= 1 && M >= 1 && N <= DW_DIM_MAX && M <= DW_DIM_MAX, "dtw: N=%lld and M=%lld must be in [1, 2^30]",
              (long long)N, (long long)M);
  SYG_REQUIRE(B >= 1 && B <= MAX_GRID_Y, "dtw: B=%lld must be in [1, 65535] a call", (long long)B);
  SYG_REQUIRE(N * M <= ((int64_t)1 << 56) / B, "dtw: B N M is too large");
  return SYG_OK;
}

int dtw_check_lens(const char* who, const int32_t* dev, const int32_t* host, int64_t B, int64_t full, const char* name) {
  SYG_REQUIRE((dev == nullptr) == (host == nullptr), "%s: %s and %s_host go together (the lengths on the device and their host copy)",
              who, name, name);
  if (!host) return SYG_OK;
  for (int64_t b = 0; b < B; ++b)
    SYG_REQUIRE(host[b] >= 1 && host[b] <= full, "%s: %s[%lld]=%d is outside [1, %lld]", who, name, (long long)b, (int)host[b],
                (long long)full);
  return SYG_OK;
}

// form: -1 the rule, 0 pair-resident, 1 tiled.  The rule: pair-resident wherever a row fits one wave's column runs.
inline bool dtw_is_tiled(int64_t M, int form) { return form >= 0 ? form == 1 : M > DW_COLS_MAX; }

int dtw_check_form(int64_t M, int form, int tile) {
  SYG_REQUIRE(form >= -1 && form <= 1, "dtw: form must be -1 (the rule), 0 (pair-resident) or 1 (tiled), got %d", form);
  SYG_REQUIRE(tile >= 0 && tile <= DW_COLS_MAX, "dtw: tile=%d must be 0 (the product tile, %d) or in [1, %d]", tile, DW_TILE,
              DW_COLS_MAX);
  SYG_REQUIRE(form != 0 || M <= DW_COLS_MAX, "dtw: the pair-resident form serves M <= %d columns, got M=%lld", DW_COLS_MAX,
              (long long)M);
  return SYG_OK;
}

// what the 16-byte form of the recurrence asks of a call: base pointers, row starts and tile seams on 16 bytes, and no
// per-pair width (a pair's own last column may fall anywhere)
bool dw_vec_ok(const DwArgs& A) {
  return (((uintptr_t)A.C | (uintptr_t)A.D) & 15) == 0 && ((uintptr_t)A.steps & 3) == 0 && A.ldc % 4 == 0 && A.bsc % 4 == 0 &&
         A.M % 4 == 0 && A.tw % 4 == 0 && !A.y_len;
}

template <int R, bool VEC>
int dtw_launch(const DwArgs& A, hipStream_t st) {
  const int64_t blocks = ceil_div(A.B * A.cnt, DW_WAVES);
  SYG_REQUIRE(blocks < 0x7fffffff, "dtw: too many work items");
  const bool unit = A.wm0 == 1.0 && A.wm1 == 1.0 && A.wm2 == 1.0 && A.wa0 == 0.0 && A.wa1 == 0.0 && A.wa2 == 0.0;
  if (unit) hipLaunchKernelGGL((dtw_accum_kernel<R, true, VEC>), dim3((unsigned)blocks), dim3(64 * DW_WAVES), 0, st, A);
  else hipLaunchKernelGGL((dtw_accum_kernel<R, false, VEC>), dim3((unsigned)blocks), dim3(64 * DW_WAVES), 0, st, A);
  SYG_CHECK_LAUNCH("dtw");
  return SYG_OK;
}

int dtw_launch_r(int64_t width, const DwArgs& A, hipStream_t st) {
  const bool vec = dw_vec_ok(A);
  if (width <= 64) return dtw_launch<1, false>(A, st);
  if (width <= 128) return dtw_launch<2, false>(A, st);
  if (width <= 256) return vec ? dtw_launch<4, true>(A, st) : dtw_launch<4, false>(A, st);
  if (width <= 512) return vec ? dtw_launch<8, true>(A, st) : dtw_launch<8, false>(A, st);
  return vec ? dtw_launch<16, true>(A, st) : dtw_launch<16, false>(A, st);
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int syg_dtw_tile(void) { return DW_TILE; }
extern "C" int syg_dtw_tile_max(void) { return DW_COLS_MAX; }
extern "C" int syg_dtw_resident_max_cols(void) { return DW_COLS_MAX; }
extern "C" int syg_dtw_run_max(void) { return DW_RMAX; }
extern "C" int syg_dtw_cost_tile(void) { return DC_T; }

extern "C" int syg_dtw_form(int64_t B, int64_t N, int64_t M, int form) {
  if (dtw_check_shape(B, N, M) || dtw_check_form(M, form, 0)) return -1;
  return dtw_is_tiled(M, form) ? 1 : 0;
}

extern "C" int64_t syg_dtw_work_bytes(int64_t B, int64_t N, int64_t M, int form, int tile) {
  if (dtw_check_shape(B, N, M) || dtw_check_form(M, form, tile)) return -1;
  if (!dtw_is_tiled(M, form)) return 0;
  const int64_t t = tile > 0 ? tile : DW_TILE;
  return B * (ceil_div(N, t) * M + ceil_div(M, t) * N) * (int64_t)sizeof(double);
}

extern "C" int syg_dtw_cost_f32(const float* X, const float* Y, int64_t B, int64_t K, int64_t N, int64_t M, int64_t ldx,
                                int64_t ldy, int64_t bsx, int64_t bsy, const int32_t* x_len, const int32_t* y_len,
                                const int32_t* x_len_host, const int32_t* y_len_host, int metric, float* C, void* stream) {
  SYG_REQUIRE(X && Y && C, "dtw_cost: null pointer argument (X / Y / C)");
  if (const int rc = dtw_check_shape(B, N, M)) return rc;
  SYG_REQUIRE(K >= 1 && K <= ((int64_t)1 << 24), "dtw_cost: K=%lld must be in [1, 2^24]", (long long)K);
  SYG_REQUIRE(ldx >= N && ldy >= M, "dtw_cost: a length is above its row stride (N=%lld, ldx=%lld, M=%lld, ldy=%lld)", (long long)N,
              (long long)ldx, (long long)M, (long long)ldy);
  SYG_REQUIRE(bsx >= 0 && bsy >= 0, "dtw_cost: the batch strides must be >= 0 (0 shares one sequence among the pairs)");
  SYG_REQUIRE(metric >= 0 && metric <= 3, "dtw_cost: metric must be 0 (euclidean), 1 (sqeuclidean), 2 (cityblock) or 3 (cosine), got %d",
              metric);
  if (const int rc = dtw_check_lens("dtw_cost", x_len, x_len_host, B, N, "x_len")) return rc;
  if (const int rc = dtw_check_lens("dtw_cost", y_len, y_len_host, B, M, "y_len")) return rc;
  const int64_t gx = ceil_div(M, DC_T), gy = ceil_div(N, DC_T);
  SYG_REQUIRE(gy <= MAX_GRID_Y && gx < 0x7fffffff, "dtw_cost: N=%lld is above %d rows a call", (long long)N, (int)(MAX_GRID_Y * DC_T));
  DcArgs A{X, Y, K, N, M, ldx, ldy, bsx, bsy, x_len, y_len, C};
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)B), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (metric) {
    case DTW_EUCLIDEAN: hipLaunchKernelGGL(dtw_cost_kernel<DTW_EUCLIDEAN>, grid, block, 0, st, A); break;
    case DTW_SQEUCLIDEAN: hipLaunchKernelGGL(dtw_cost_kernel<DTW_SQEUCLIDEAN>, grid, block, 0, st, A); break;
    case DTW_CITYBLOCK: hipLaunchKernelGGL(dtw_cost_kernel<DTW_CITYBLOCK>, grid, block, 0, st, A); break;
    default: hipLaunchKernelGGL(dtw_cost_kernel<DTW_COSINE>, grid, block, 0, st, A); break;
  }
  SYG_CHECK_LAUNCH("dtw_cost");
  return SYG_OK;
}

extern "C" int syg_dtw_f32(const float* C, int64_t B, int64_t N, int64_t M, int64_t ldc, int64_t bsc, const int32_t* x_len,
                           const int32_t* y_len, const int32_t* x_len_host, const int32_t* y_len_host,
                           const double* weights_mul_host, const double* weights_add_host, int subseq, int form, int tile,
                           double* D, uint8_t* steps, double* cost, int32_t* end_col, int32_t* path, int32_t* path_len,
                           void* work, int64_t work_bytes, void* stream) {
  SYG_REQUIRE(C && cost && end_col, "dtw: null pointer argument (C / cost / end_col)");
  if (const int rc = dtw_check_shape(B, N, M)) return rc;
  if (const int rc = dtw_check_form(M, form, tile)) return rc;
  SYG_REQUIRE(ldc >= M, "dtw: M=%lld is above the row stride ldc=%lld", (long long)M, (long long)ldc);
  SYG_REQUIRE(bsc >= 0, "dtw: the batch stride must be >= 0");
  if (const int rc = dtw_check_lens("dtw", x_len, x_len_host, B, N, "x_len")) return rc;
  if (const int rc = dtw_check_lens("dtw", y_len, y_len_host, B, M, "y_len")) return rc;
  double wm[3] = {1.0, 1.0, 1.0}, wa[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < 3; ++k) {
    if (weights_mul_host) wm[k] = weights_mul_host[k];
    if (weights_add_host) wa[k] = weights_add_host[k];
    SYG_REQUIRE(isfinite(wm[k]) && isfinite(wa[k]), "dtw: the step weights must be finite");
  }
  SYG_REQUIRE((path == nullptr) == (path_len == nullptr), "dtw: path and path_len go together");
  SYG_REQUIRE(!path || steps, "dtw: the backtrack walks the step codes: path needs steps");
  const bool tiled = dtw_is_tiled(M, form);
  const int64_t need = syg_dtw_work_bytes(B, N, M, form, tile);
  SYG_REQUIRE(need >= 0 && (need == 0 || (work && work_bytes >= need)),
              "dtw: the tiled form needs a workspace of syg_dtw_work_bytes() = %lld bytes, got %lld", (long long)need,
              (long long)(work ? work_bytes : 0));
  SYG_REQUIRE(((uintptr_t)work & 7) == 0 && ((uintptr_t)D & 7) == 0 && ((uintptr_t)path & 7) == 0,
              "dtw: D, path and work must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DwArgs A{C, ldc, bsc, B, N, M, x_len, y_len, wm[0], wm[1], wm[2], wa[0], wa[1], wa[2], subseq ? 1 : 0,
           D, steps, cost, end_col, nullptr, nullptr, N, M, 1, 1, 0, 0, 1};
  if (!tiled) {
    if (const int rc = dtw_launch_r(M, A, st)) return rc;
  } else {
    const int64_t t = tile > 0 ? tile : DW_TILE;
    A.th = t; A.tw = t; A.tn = ceil_div(N, t); A.tm = ceil_div(M, t);
    SYG_REQUIRE(A.tn + A.tm - 1 <= DW_LAUNCH_MAX, "dtw: tile=%lld cuts this matrix into more than %lld block anti-diagonals",
                (long long)t, (long long)DW_LAUNCH_MAX);
    A.rowws = (double*)work; A.colws = A.rowws + B * A.tn * M;
    for (int64_t d = 0; d < A.tn + A.tm - 1; ++d) {
      A.diag = d;
      A.i_lo = d - (A.tm - 1) > 0 ? d - (A.tm - 1) : 0;
      const int64_t i_hi = d < A.tn - 1 ? d : A.tn - 1;
      A.cnt = i_hi - A.i_lo + 1;
      if (const int rc = dtw_launch_r(t, A, st)) return rc;
    }
  }
  if (path) {
    BtArgs T{steps, B, N, M, x_len, y_len, end_col, subseq ? 1 : 0, path, path_len};
    hipLaunchKernelGGL(dtw_backtrack_kernel, dim3((unsigned)ceil_div(B, 64)), dim3(64), 0, st, T);
    SYG_CHECK_LAUNCH("dtw");
  }
  return SYG_OK;
}
