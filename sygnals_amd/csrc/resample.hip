// Polyphase resampling, scipy.signal.resample_poly in index form (the float64 restatement that is the contract lives in
// tests/resample_ref.py; the plan comes from sygnals_amd/_resample.py):
//     t = (n + n_pre_remove) down,  p = t mod up,  q = t div up,      y[b, n] = sum_{j < Kp} tab[p][j] x~[b, q - j],
// x~ = x inside [0, L) and the pad rule outside.  float32 rows in, float32 rows out, float32 accumulation with j
// ascending.  Every output is independent: no recurrence, no atomics, the same bits on every call and for every batch
// size.  The statistic pad types (mean, minimum, maximum) are the constant rule on a shifted row and never get here.
//
// One kernel family.  The grid is (output tiles, rows).  A block takes a tile of RS_TILE consecutive outputs of one row
// (a tile never spans rows).  t passes 2^32 inside a long row, so a tile forms its base t0 = (n0 + n_pre_remove)
// down, q0 = t0 div up and p0 = t0 mod up once in 64 bits and every output of the tile works from p0 + i down, which
// stays below 2^31 (up, down <= RS_RATE_MAX = 2^20, i < 1024).  The tile's input span q_first - Kp + 1 ... q_last is
// staged into LDS through the pad rule (the periodic index maps: a row may be many times shorter than the filter), so
// the tap loop is two LDS reads and one fma with a descending x address the compiler folds into immediate offsets.
//
// Table placement.  A table of at most RS_TAB_LDS_RULE bytes (up Kp 4) sits in LDS beside the span, rows at an odd stride
// (Kp | 1: the lanes of a wave sit on different phases, and an odd stride spreads their rows over the banks): loading
// it costs a block at most one word per output.  A larger one, up to RS_TAB_MAX bytes, is read from global memory,
// where it is read-only and stays in L1 / L2; measured, that is the faster place for it (the
// 37 KB table of 160/441 leaves three blocks a CU and costs each block its load).  `form` forces either placement;
// LDS takes tables up to RS_TAB_LDS_MAX bytes (up (Kp | 1) 4).
//
// Span fallback.  A strong decimation (one tile of outputs reading more than RS_SPAN_MAX input samples, e.g. 1/64) does
// not stage: the taps read x through the pad rule from global memory.  Same arithmetic, same order.
//
// Lane mapping.  A thread owns RS_PER = 4 outputs of the tile and runs their four fma chains
// side by side, taps unrolled by four, so that 20 or 32 LDS reads are in flight instead of two.  Consecutive lanes take
// consecutive outputs (stores coalesce, the lanes of a wave sit on different phases, their x addresses advance by
// down / up).  Which four outputs a thread owns is the measured choice:
//   shared taps, the product where up <= RS_TILE / 4: the four are a multiple of `up` apart, so they share one phase and
//     each tap is read once for four fmas (5 LDS reads per 4 fmas);
//   own taps, everywhere else (and everywhere with -DSYG_RESAMPLE_SHARE=0, the form measured against it): the four are
//     RS_THREADS apart and each reads its own row of the table (8 reads per 4 fmas).
// Neither changes a value: every output is the same chain of fmas, j ascending.
#include "host.h"

#ifndef SYG_RESAMPLE_SHARE
#define SYG_RESAMPLE_SHARE 1
#endif

namespace syg {
namespace {

constexpr int RS_TILE = 1024;                          // outputs per tile
constexpr int RS_THREADS = 256;
constexpr int64_t RS_TAB_LDS_RULE = 4 * 1024;          // up Kp 4 bytes at most: the rule puts the table in LDS
constexpr int64_t RS_TAB_LDS_MAX = 64 * 1024;          // up (Kp | 1) 4 bytes at most: form 0 may put it there
constexpr int64_t RS_TAB_MAX = 4 << 20;                // up Kp 4 bytes at most: served at all
constexpr int RS_SPAN_MAX = 16384;                     // input samples a tile stages at most
constexpr int RS_RATE_MAX = 1 << 20;                   // up, down at most (p0 + i down stays below 2^31)
enum { RS_PAD_CONSTANT = 0, RS_PAD_EDGE, RS_PAD_WRAP, RS_PAD_SYMMETRIC, RS_PAD_REFLECT, RS_PAD_COUNT };
constexpr int RS_PER = 4;                              // outputs a thread owns
constexpr bool RS_SHARE_TAPS = SYG_RESAMPLE_SHARE != 0;

struct RsArgs {
  const float* x; int64_t L, ldx;
  int up, down; int64_t npr; int Kp;
  const float* tab; int pad; float cval;
  int64_t n_out; float* y; int64_t ldy;
  int tstride, xs_words, step;
};

// x~[i]: the row inside [0, L), the pad rule outside (periodic maps: |i| may exceed L many times over)
__device__ __forceinline__ float rs_fetch(const float* __restrict__ xr, int64_t i, int64_t L, int pad, float cval) {
  if (i >= 0 && i < L) return xr[i];
  if (pad == RS_PAD_CONSTANT) return cval;
  if (pad == RS_PAD_EDGE) return xr[i < 0 ? 0 : L - 1];
  const int64_t P = pad == RS_PAD_WRAP ? L : (pad == RS_PAD_SYMMETRIC ? 2 * L : 2 * L - 2);   // reflect needs L >= 2 (host)
  int64_t m = i % P;
  if (m < 0) m += P;
  if (m >= L) m = (pad == RS_PAD_SYMMETRIC ? P - 1 : P) - m;
  return xr[m];
}

template <bool TAB_LDS, bool STAGE, bool SHARE>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(RsArgs A) {
  extern __shared__ __align__(16) float rs_smem[];
  float* xs = rs_smem;                                 // [xs_words]
  float* ts = rs_smem + A.xs_words;                    // [up, tstride] where TAB_LDS
  const int tid = threadIdx.x;
  const float* __restrict__ xr = A.x + (int64_t)blockIdx.y * A.ldx;
  float* __restrict__ yr = A.y + (int64_t)blockIdx.y * A.ldy;
  const int up = A.up, down = A.down, Kp = A.Kp, step = A.step;

  if (TAB_LDS) {                                       // a wave per phase row, lanes along the taps
    for (int p = tid >> 6; p < up; p += RS_THREADS / 64)
      for (int j = tid & 63; j < Kp; j += 64) ts[p * A.tstride + j] = A.tab[(int64_t)p * Kp + j];
  }
  const int64_t n0 = (int64_t)blockIdx.x * RS_TILE;
  const int cnt = (int)(A.n_out - n0 < RS_TILE ? A.n_out - n0 : RS_TILE);
  const int64_t t0 = (n0 + A.npr) * down, q0 = t0 / up;
  const uint32_t p0 = (uint32_t)(t0 - q0 * up);
  const int64_t lo = q0 - (Kp - 1);                  // first sample of the span
  if (STAGE) {
    const int span = (int)((p0 + (uint32_t)(cnt - 1) * (uint32_t)down) / (uint32_t)up) + Kp;
    for (int s = tid; s < span; s += RS_THREADS) xs[s] = rs_fetch(xr, lo + s, A.L, A.pad, A.cval);
  }
  __syncthreads();

  // thread e owns the outputs e + k step, k < RS_PER (step: a multiple of `up` where SHARE, RS_THREADS otherwise)
  for (int e = tid; e < step && e < cnt; e += RS_THREADS) {
    const float* tp[RS_PER];
    int top[RS_PER];                                 // local sample of tap 0: ql + Kp - 1
    bool ok[RS_PER];
#pragma unroll
    for (int k = 0; k < RS_PER; ++k) {
      ok[k] = e + k * step < cnt;
      const int i = ok[k] ? e + k * step : e;        // an output past the end repeats the first and is not stored
      if (SHARE && k > 0) {                          // (i - e) down is a multiple of up: the same phase, q further on
        tp[k] = tp[0];
        top[k] = top[0] + (i - e) / up * down;
      } else {
        const uint32_t tt = p0 + (uint32_t)i * (uint32_t)down, ql = tt / (uint32_t)up, p = tt - ql * (uint32_t)up;
        tp[k] = TAB_LDS ? ts + p * A.tstride : A.tab + (int64_t)p * Kp;
        top[k] = (int)ql + Kp - 1;
      }
    }
    float acc[RS_PER] = {0.f, 0.f, 0.f, 0.f};
    auto tap = [&](int j) {
      float t[RS_PER];
#pragma unroll
      for (int k = 0; k < RS_PER; ++k) t[k] = (SHARE && k > 0) ? t[0] : tp[k][j];
#pragma unroll
      for (int k = 0; k < RS_PER; ++k) {
        const float v = STAGE ? xs[top[k] - j] : rs_fetch(xr, lo + top[k] - j, A.L, A.pad, A.cval);
        acc[k] = fmaf(t[k], v, acc[k]);
      }
    };
    int j = 0;
    for (; j + 4 <= Kp; j += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) tap(j + u);
    }
    for (; j < Kp; ++j) tap(j);
#pragma unroll
    for (int k = 0; k < RS_PER; ++k)
      if (ok[k]) yr[n0 + e + k * step] = acc[k];
  }
}

// words of LDS the span of a full tile takes, -1 where it is not staged
inline int rs_span_words(int up, int down, int Kp) {
  const int64_t span = ((int64_t)(RS_TILE - 1) * down + up - 1) / up + Kp;
  return span > RS_SPAN_MAX ? -1 : (int)span;
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int syg_resample_tile(void) { return RS_TILE; }
extern "C" int64_t syg_resample_table_lds_rule(void) { return RS_TAB_LDS_RULE; }
extern "C" int64_t syg_resample_table_lds_max(void) { return RS_TAB_LDS_MAX; }
extern "C" int64_t syg_resample_table_max(void) { return RS_TAB_MAX; }
extern "C" int syg_resample_span_max(void) { return RS_SPAN_MAX; }
extern "C" int syg_resample_rate_max(void) { return RS_RATE_MAX; }

extern "C" int syg_resample_poly_f32(const float* x, int64_t B, int64_t L, int64_t ldx, int up, int down, int64_t n_pre_remove,
                                     int Kp, const float* table, int pad, float cval, int form, int64_t n_out, float* y,
                                     int64_t ldy, void* stream) {
  SYG_REQUIRE(x && table && y, "resample_poly: null pointer argument (x / table / y)");
  SYG_REQUIRE(up >= 1 && down >= 1 && up <= RS_RATE_MAX && down <= RS_RATE_MAX,
              "resample_poly: up=%d and down=%d must be in [1, %d]", up, down, RS_RATE_MAX);
  SYG_REQUIRE(B >= 1 && B <= MAX_GRID_Y && L >= 1 && L < ((int64_t)1 << 40), "resample_poly: bad B / L (B in [1, 65535], L in [1, 2^40))");
  SYG_REQUIRE(n_out == ceil_div(L * up, down), "resample_poly: n_out=%lld is not ceil(L up / down) = %lld", (long long)n_out,
              (long long)ceil_div(L * up, down));
  SYG_REQUIRE(ldx >= L, "resample_poly: ldx=%lld is less than L=%lld", (long long)ldx, (long long)L);
  SYG_REQUIRE(ldy >= n_out, "resample_poly: ldy=%lld is less than n_out=%lld", (long long)ldy, (long long)n_out);
  SYG_REQUIRE(pad >= 0 && pad < RS_PAD_COUNT, "resample_poly: unknown pad code %d (0 constant, 1 edge, 2 wrap, 3 symmetric, 4 reflect)",
              pad);
  SYG_REQUIRE(pad != RS_PAD_REFLECT || L >= 2, "resample_poly: the reflect pad rule needs at least two samples");
  SYG_REQUIRE(Kp >= 1 && n_pre_remove >= 0 && n_pre_remove < ((int64_t)1 << 40), "resample_poly: bad Kp / n_pre_remove");
  const int64_t tab_bytes = (int64_t)up * Kp * 4;
  SYG_REQUIRE(tab_bytes <= RS_TAB_MAX, "resample_poly: the table of up=%d, down=%d takes %lld bytes, above the bound of %lld",
              up, down, (long long)tab_bytes, (long long)RS_TAB_MAX);
  SYG_REQUIRE(form >= -1 && form <= 1, "resample_poly: form must be -1 (the rule), 0 (table in LDS) or 1 (table in global memory), got %d",
              form);
  const int64_t lds_bytes = (int64_t)up * (Kp | 1) * 4;          // with the odd row stride
  SYG_REQUIRE(form != 0 || lds_bytes <= RS_TAB_LDS_MAX, "resample_poly: form 0 needs a table of at most %lld bytes in LDS, this one takes %lld",
              (long long)RS_TAB_LDS_MAX, (long long)lds_bytes);
  const bool tab_lds = form < 0 ? tab_bytes <= RS_TAB_LDS_RULE : form == 0;
  const int span_words = rs_span_words(up, down, Kp);
  const bool stage = span_words >= 0;
  const bool share = RS_SHARE_TAPS && up <= RS_TILE / RS_PER;
  // shared taps: the least multiple of `up` whose RS_PER-fold covers the tile
  const int step = share ? (int)ceil_div(ceil_div(RS_TILE, up), RS_PER) * up : RS_THREADS;
  RsArgs A{x, L, ldx, up, down, n_pre_remove, Kp, table, pad, cval, n_out, y, ldy, Kp | 1, stage ? span_words : 0, step};
  const int64_t gx = ceil_div(n_out, RS_TILE);
  SYG_REQUIRE(gx < 0x7fffffff, "resample_poly: too many tiles");
  const size_t lds = sizeof(float) * ((size_t)A.xs_words + (tab_lds ? (size_t)up * A.tstride : 0));
  void (*k)(RsArgs) = nullptr;
  switch ((tab_lds ? 4 : 0) | (stage ? 2 : 0) | (share ? 1 : 0)) {
    case 0: k = resample_kernel<false, false, false>; break;
    case 1: k = resample_kernel<false, false, true>; break;
    case 2: k = resample_kernel<false, true, false>; break;
    case 3: k = resample_kernel<false, true, true>; break;
    case 4: k = resample_kernel<true, false, false>; break;
    case 5: k = resample_kernel<true, false, true>; break;
    case 6: k = resample_kernel<true, true, false>; break;
    default: k = resample_kernel<true, true, true>; break;
  }
  if (const int rc = reserve_dynamic_lds("resample_poly", (const void*)k, lds)) return rc;
  hipLaunchKernelGGL(k, dim3((unsigned)gx, (unsigned)B), dim3(RS_THREADS), lds, (hipStream_t)stream, A);
  SYG_CHECK_LAUNCH("resample_poly");
  return SYG_OK;
}
