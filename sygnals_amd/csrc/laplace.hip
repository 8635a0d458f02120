// Numerical Laplace transform of sygnals/core/transforms.py:159-199:
//     F[b, i] = t_step sum_{n < L} x[b, n] exp(-s_i n t_step),     s_i = sigma_i + j omega_i,
// float32 rows in, complex float64 out, for any list of s-values (an arbitrary-point z-transform at z = exp(s t_step)).
// The float64 restatement that is the contract lives in tests/laplace_ref.py; the gate is 1e-5 of the natural scale
// A[b, i] = |t_step| sum_n |x[b, n]| exp(-sigma_i n t_step).
//
// Chunked form.  With z = exp(-s t_step) and chunks of LP_C samples, F = t_step sum_k Z^k P_k, P_k = sum_{j < C}
// x[kC + j] z^j, Z = z^C.  The table z^j is the same for every chunk and clip: the host forms it in float64 and rounds it
// once to float32 (sygnals_amd/_laplace.py).  P is then a real GEMM, [chunks, C] x [C, 2 S] (the table's real and
// imaginary parts as columns), on v_mfma_f32_16x16x4_f32, which is an exact k-ordered float32 fma chain.  The phase
// omega n t_step reaches 1e7 rad on a long row, so everything across chunks is float64: a lane turns its accumulators
// into sum_r Z^r P_{k0 + r} with float64 factors from the host and walks the tiles of its segment from the last to the
// first in Horner form, h <- h Z^16 + tile.  |z| <= 1 for every column that gets here, so no power overflows.
//
// Reversed form.  A column with sigma t_step < 0 grows along the row.  It is served as the decaying transform of the
// reversed row, F = exp(-s (L - 1) t_step) t_step sum_m x[L - 1 - m] v^m with v = exp(+s t_step), |v| < 1: chunks are
// counted from the row's end (chunk k is samples [L - (k + 1) C, L - k C), the zero padding lies before sample 0), the
// table entry of in-memory position i is v^(C - 1 - i), and the one factor that can be large, the end anchor
// exp(-s (L - 1) t_step), is finite wherever the reference's own exp is (|sigma t_step| (L - 1) <= 700) and multiplies a
// finite sum once.  Both directions run the same kernel: only the chunk's base sample and the table differ.  A column
// tile (16 s-values) shares the A operand, so the host groups the columns by direction and pads each group to 16.
//
// Steep columns.  Where |sigma t_step| (C - 1) > 40 the float32 table would leave the normal range inside one chunk (a
// row that starts with zeros then loses the samples that carry its whole sum).  For those only the first (or, reversed,
// last) LP_STEEP samples can matter at all: further on exp() is below the smallest float64.  lap_steep_kernel serves
// them with one lane per (clip, column) and a float64 recurrence over at most LP_STEEP samples.
//
// Tile and operand layout.  One wave owns (clip, segment, column tile).  A tile is LP_R = 16 consecutive chunks (4 KiB of
// the row, contiguous) by 16 columns.  MFMA step t = 4 u + e (u, e < 4) sums over k = lane >> 4, and the order of j
// inside a chunk is free as long as A and the table agree: position i = 16 u + 4 (lane >> 4) + e.  So lane (row r = lane
// & 15, q = lane >> 4) loads four 16-byte vectors, x[base_r + 16 u + 4 q ..+3], each instruction reading 64 contiguous
// bytes per chunk, and element e of vector u is the A operand of step 4 u + e.  The B operand (32 registers: 16 steps,
// real and imaginary) is loaded once per wave.  The real table goes to one accumulator and the imaginary one to another
// with the same map (column lane & 15, rows 4 (lane >> 4) + reg), so a lane holds both parts of the same (chunk, s).
// A row that is not 16-byte aligned, the end-aligned grid of the reversed form and the row's edges take guarded scalar
// loads.  A clip with fewer chunks than a tile has rows pads the tile with zero chunks; a tile never spans clips.
//
// Launch forms.  Whole-row: one wave walks every tile of its row and writes F.  Segmented, where whole rows would leave
// the device underfilled (lp_segmented): the row is cut into segments of LP_SEG_CH chunks, a wave writes its segment's
// float64 sum into `work`, and lap_combine_kernel adds them in Horner form with Z^LP_SEG_CH, in a fixed order.  No
// atomics anywhere: the same call gives the same bits.
#include <math.h>
#include "host.h"

namespace syg {
namespace {

constexpr int LP_C = 64;                   // samples per chunk
constexpr int LP_R = 16;                   // chunks per tile (MFMA rows)
constexpr int LP_N = 16;                   // s-values per column tile (MFMA columns)
constexpr int LP_SEG_CH = 256;             // chunks per segment of the segmented form
constexpr int LP_STEEP = 1280;             // samples a steep column reads: exp(-40 / 63 * 1280) < the least float64
constexpr int LP_WAVES = 4;                // waves per workgroup, each with a (clip, segment, column tile) of its own
// per column, float64: Z^r for r < 16 (re, im) | Z^16 | Z^LP_SEG_CH | z        (Z = z^LP_C)
constexpr int LP_FAC = 38, LP_F_Z16 = 32, LP_F_ZSEG = 34, LP_F_Z1 = 36;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct LpArgs {
  const float* x; int64_t B, L, ldx;
  const float* table; const double* fac; const double* anchor; const int32_t* col;
  int nfwd, nrev;                          // column tiles of the forward and of the reversed group
  int64_t nsf, nsr;                        // steep columns, forward and reversed
  int64_t S; double t_step; double2* out;
  double2* work;                           // null in the whole-row form
  int64_t nseg, seg_ch;                    // whole-row form: nseg = 1, seg_ch = every chunk of the row
};

// F = t_step * anchor * h, written if the column is one of the caller's S (padding columns carry -1)
__device__ __forceinline__ void lp_store(const LpArgs& A, int64_t b, int64_t colg, double hr, double hi) {
  const int32_t o = A.col[colg];
  if (o < 0 || o >= A.S) return;
  const double ar = A.anchor[2 * colg], ai = A.anchor[2 * colg + 1];
  A.out[b * A.S + o] = make_double2(A.t_step * fma(ar, hr, -(ai * hi)), A.t_step * fma(ar, hi, ai * hr));
}

// four samples from n of the row; outside [0, L) reads as zero
__device__ __forceinline__ f32x4 lp_load4(const float* __restrict__ xr, int64_t n, int64_t L, bool live) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!live) return v;
  if (n >= 0 && n + 4 <= L && (((uintptr_t)(xr + n)) & 15) == 0) return *(const f32x4*)(xr + n);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (n + e >= 0 && n + e < L) v[e] = xr[n + e];
  return v;
}

struct LpTile { f32x4 a[4]; };

// the A operand of the tile whose first chunk is k0: this lane's chunk is k0 + (lane & 15), dead at k_hi and beyond
__device__ __forceinline__ LpTile lp_load_tile(const float* __restrict__ xr, int64_t L, bool rev, int64_t k0, int64_t k_hi,
                                               int lane) {
  const int64_t k = k0 + (lane & 15);
  const int64_t n0 = (rev ? L - (k + 1) * LP_C : k * LP_C) + 4 * (lane >> 4);
  LpTile t;
#pragma unroll
  for (int u = 0; u < 4; ++u) t.a[u] = lp_load4(xr, n0 + 16 * u, L, k < k_hi);
  return t;
}

__global__ __launch_bounds__(64 * LP_WAVES) void lap_tile_kernel(LpArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * LP_WAVES + (threadIdx.x >> 6);
  const int nct = A.nfwd + A.nrev;
  if (w >= A.B * A.nseg * nct) return;
  const int ct = (int)(w % nct);
  const int64_t rest = w / nct, sg = rest % A.nseg, b = rest / A.nseg;
  const bool rev = ct >= A.nfwd;
  const int c = lane & 15, q = lane >> 4;
  const int64_t n16 = (int64_t)nct * LP_N, colg = (int64_t)ct * LP_N + c;

  float tre[16], tim[16];                  // B operand: table[i][part][column], i = 16 u + 4 q + e at step 4 u + e
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int i = 16 * (t >> 2) + 4 * q + (t & 3);
    tre[t] = A.table[(int64_t)(2 * i) * n16 + colg];
    tim[t] = A.table[(int64_t)(2 * i + 1) * n16 + colg];
  }
  const double* __restrict__ f = A.fac + colg * LP_FAC;
  double zr[4], zi[4];                     // Z^(4 q + r): the chunks of this lane's accumulator registers
#pragma unroll
  for (int r = 0; r < 4; ++r) { zr[r] = f[2 * (4 * q + r)]; zi[r] = f[2 * (4 * q + r) + 1]; }
  const double z16r = f[LP_F_Z16], z16i = f[LP_F_Z16 + 1];

  const int64_t K = (A.L + LP_C - 1) / LP_C, k_lo = sg * A.seg_ch, k_hi = (K - k_lo > A.seg_ch) ? k_lo + A.seg_ch : K;
  const int64_t ntile = (k_hi - k_lo + LP_R - 1) / LP_R;
  const float* __restrict__ xr = A.x + b * A.ldx;
  double hr = 0.0, hi = 0.0;
  LpTile cur = lp_load_tile(xr, A.L, rev, k_lo + (ntile - 1) * LP_R, k_hi, lane);
  for (int64_t tl = ntile - 1; tl >= 0; --tl) {
    LpTile nxt = cur;
    if (tl > 0) nxt = lp_load_tile(xr, A.L, rev, k_lo + (tl - 1) * LP_R, k_hi, lane);     // in flight under the MFMAs
    f32x4 are = {0.f, 0.f, 0.f, 0.f}, aim = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        are = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[u][e], tre[4 * u + e], are, 0, 0, 0);
        aim = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[u][e], tim[4 * u + e], aim, 0, 0, 0);
      }
    double pr = 0.0, pi = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double xr_ = (double)are[r], xi_ = (double)aim[r];
      pr = fma(zr[r], xr_, fma(-zi[r], xi_, pr));
      pi = fma(zr[r], xi_, fma(zi[r], xr_, pi));
    }
    const double nr = fma(hr, z16r, fma(-hi, z16i, pr)), ni = fma(hr, z16i, fma(hi, z16r, pi));
    hr = nr; hi = ni;
    cur = nxt;
  }
  // the four lane groups hold rows 4 q .. 4 q + 3: add them (a + b is b + a bit for bit, so every lane agrees)
  hr += __shfl_xor(hr, 16); hi += __shfl_xor(hi, 16);
  hr += __shfl_xor(hr, 32); hi += __shfl_xor(hi, 32);
  if (q != 0) return;
  if (A.work) A.work[(b * A.nseg + sg) * n16 + colg] = make_double2(hr, hi);
  else lp_store(A, b, colg, hr, hi);
}

// F[b, column] = t_step anchor sum_sg Z^(LP_SEG_CH sg) work[b, sg, column], Horner from the last segment
__global__ __launch_bounds__(256) void lap_combine_kernel(LpArgs A) {
  const int64_t n16 = (int64_t)(A.nfwd + A.nrev) * LP_N;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= A.B * n16) return;
  const int64_t b = idx / n16, colg = idx - b * n16;
  const double zsr = A.fac[colg * LP_FAC + LP_F_ZSEG], zsi = A.fac[colg * LP_FAC + LP_F_ZSEG + 1];
  const double2* __restrict__ p = A.work + b * A.nseg * n16 + colg;
  double hr = 0.0, hi = 0.0;
  auto step = [&](double2 v) {
    const double nr = fma(hr, zsr, fma(-hi, zsi, v.x)), ni = fma(hr, zsi, fma(hi, zsr, v.y));
    hr = nr; hi = ni;
  };
  constexpr int U = 8;                     // loads of U segments in flight ahead of the serial chain
  int64_t sg = A.nseg;
  for (; sg >= U; sg -= U) {
    double2 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = p[(sg - 1 - u) * n16];
#pragma unroll
    for (int u = 0; u < U; ++u) step(v[u]);
  }
  for (; sg >= 1; --sg) step(p[(sg - 1) * n16]);
  lp_store(A, b, colg, hr, hi);
}

// steep columns: one lane per (clip, column), lanes of a wave share the clip (the row's loads are broadcasts)
__global__ __launch_bounds__(64) void lap_steep_kernel(LpArgs A) {
  const int64_t j = (int64_t)blockIdx.y * 64 + threadIdx.x, b = blockIdx.x;
  if (j >= A.nsf + A.nsr) return;
  const bool rev = j >= A.nsf;
  const int64_t colg = (int64_t)(A.nfwd + A.nrev) * LP_N + j;
  const double zr = A.fac[colg * LP_FAC + LP_F_Z1], zi = A.fac[colg * LP_FAC + LP_F_Z1 + 1];
  const float* __restrict__ xr = A.x + b * A.ldx;
  const int64_t N = A.L < LP_STEEP ? A.L : LP_STEEP;
  double er = 1.0, ei = 0.0, hr = 0.0, hi = 0.0;
  for (int64_t m = 0; m < N; ++m) {
    const double v = (double)xr[rev ? A.L - 1 - m : m];
    hr = fma(v, er, hr); hi = fma(v, ei, hi);
    const double nr = fma(er, zr, -(ei * zi)), ni = fma(er, zi, ei * zr);
    er = nr; ei = ni;
  }
  lp_store(A, b, colg, hr, hi);
}

// form: -1 the rule, 0 whole-row, 1 segmented.  The rule: rows longer than a segment, and fewer than two waves a SIMD
// (eight a CU) in the whole-row form.
inline bool lp_segmented(int64_t B, int64_t L, int64_t n16, int form, int cus) {
  if (form >= 0) return form == 1;
  return ceil_div(L, LP_C) > LP_SEG_CH && B * (n16 / LP_N) < (int64_t)cus * 8;
}

int lp_check_shape(int64_t B, int64_t L, int64_t n16, int form) {
  SYG_REQUIRE(B >= 1 && L >= 1 && B < ((int64_t)1 << 31) && L < ((int64_t)1 << 40) && B * L < ((int64_t)1 << 44),
              "laplace: bad B / L");
  SYG_REQUIRE(n16 >= 0 && n16 % LP_N == 0 && n16 <= ((int64_t)1 << 24),
              "laplace: S_fwd / S_rev must be multiples of %d (padded column groups) and at most 2^24", LP_N);
  SYG_REQUIRE(form >= -1 && form <= 1, "laplace: form must be -1 (the rule), 0 (whole-row) or 1 (segmented), got %d", form);
  return SYG_OK;
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int syg_laplace_chunk(void) { return LP_C; }
extern "C" int syg_laplace_tile_rows(void) { return LP_R; }
extern "C" int syg_laplace_tile_cols(void) { return LP_N; }
extern "C" int64_t syg_laplace_segment(void) { return (int64_t)LP_SEG_CH * LP_C; }
extern "C" int syg_laplace_steep(void) { return LP_STEEP; }
extern "C" int syg_laplace_fac_stride(void) { return LP_FAC; }

extern "C" int64_t syg_laplace_work_bytes(int64_t B, int64_t L, int64_t S16, int form) {
  if (lp_check_shape(B, L, S16, form)) return -1;
  if (S16 == 0 || !lp_segmented(B, L, S16, form, device_cu_count())) return 0;
  return B * ceil_div(ceil_div(L, LP_C), LP_SEG_CH) * S16 * (int64_t)sizeof(double2);
}

extern "C" int syg_laplace_f32(const float* x, int64_t B, int64_t L, int64_t ldx, const float* table, const double* fac,
                               const double* anchor, const int32_t* col, int64_t S_fwd, int64_t S_rev, int64_t S_steep_fwd,
                               int64_t S_steep_rev, int64_t S, double t_step, double* out, void* work, int form,
                               void* stream) {
  SYG_REQUIRE(x && fac && anchor && col && out, "laplace: null pointer argument (x / fac / anchor / col / out)");
  SYG_REQUIRE(S_fwd >= 0 && S_rev >= 0 && S_fwd <= ((int64_t)1 << 24) && S_rev <= ((int64_t)1 << 24) &&
                  S_fwd % LP_N == 0 && S_rev % LP_N == 0,
              "laplace: S_fwd / S_rev must be multiples of %d (padded column groups) and at most 2^24", LP_N);
  const int64_t n16 = S_fwd + S_rev;
  if (const int rc = lp_check_shape(B, L, n16, form)) return rc;
  SYG_REQUIRE(ldx >= L, "laplace: ldx=%lld is less than L=%lld", (long long)ldx, (long long)L);
  SYG_REQUIRE(S >= 1 && S <= ((int64_t)1 << 24) && S_steep_fwd >= 0 && S_steep_rev >= 0 && S_steep_fwd <= S && S_steep_rev <= S &&
                  n16 + S_steep_fwd + S_steep_rev >= S && n16 + S_steep_fwd + S_steep_rev <= S + 2 * (LP_N - 1),
              "laplace: bad S (S=%lld must be in [1, 2^24] and the column groups must hold S columns and the padding)",
              (long long)S);
  SYG_REQUIRE(table || n16 == 0, "laplace: null pointer argument (table)");
  SYG_REQUIRE(isfinite(t_step), "laplace: t_step must be finite");
  const bool seg = n16 > 0 && lp_segmented(B, L, n16, form, device_cu_count());
  SYG_REQUIRE(work || !seg, "laplace: this shape takes the segmented form and needs `work` (syg_laplace_work_bytes)");
  SYG_REQUIRE(((uintptr_t)work & 15) == 0 && ((uintptr_t)out & 15) == 0, "laplace: `out` and `work` must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t K = ceil_div(L, LP_C);
  LpArgs A{x, B, L, ldx, table, fac, anchor, col, (int)(S_fwd / LP_N), (int)(S_rev / LP_N), S_steep_fwd, S_steep_rev,
           S, t_step, (double2*)out, seg ? (double2*)work : nullptr, 1, K};
  if (seg) { A.nseg = ceil_div(K, LP_SEG_CH); A.seg_ch = LP_SEG_CH; }
  const int64_t blocks = ceil_div(B * A.nseg * (n16 / LP_N), LP_WAVES), nsteep = S_steep_fwd + S_steep_rev;
  SYG_REQUIRE(blocks < 0x7fffffff && ceil_div(B * n16, 256) < 0x7fffffff && ceil_div(nsteep, 64) < 65536,
              "laplace: too many work items");
  if (n16 > 0) {
    hipLaunchKernelGGL(lap_tile_kernel, dim3((unsigned)blocks), dim3(64 * LP_WAVES), 0, st, A);
    SYG_CHECK_LAUNCH("laplace");
    if (seg) {
      hipLaunchKernelGGL(lap_combine_kernel, dim3((unsigned)ceil_div(B * n16, 256)), dim3(256), 0, st, A);
      SYG_CHECK_LAUNCH("laplace");
    }
  }
  if (nsteep > 0) {
    hipLaunchKernelGGL(lap_steep_kernel, dim3((unsigned)B, (unsigned)ceil_div(nsteep, 64)), dim3(64), 0, st, A);
    SYG_CHECK_LAUNCH("laplace");
  }
  return SYG_OK;
}
