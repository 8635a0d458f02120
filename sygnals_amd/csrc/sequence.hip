// Viterbi decoding of a hidden Markov chain (librosa.sequence.viterbi and its discriminative and binary variants):
// emissions [B, S, T] in any element strides, log-transitions [S, S] (row = source) shared or per sequence.
//   value[0, j] = lp[0, j] + linit[j];  ptr[t, j] = first argmax_i value[t-1, i] + ltrans[i, j];
//   value[t, j] = lp[t, j] + (value[t-1, ptr] + ltrans[ptr, j]);  the path is walked back from the first argmax of
//   value[len-1] in the same launch.  lp = emission (log_domain) or log(emission + eps), minus lmarg[j] where given.
// Everything is float64 and only additions and comparisons touch a score, in the order written above, so the result
// is the float64 restatement's (tests/sequence_ref.py) bit for bit when it is fed the same logs.  No atomics.
// Two forms:
//   wide    one workgroup a sequence, one thread a destination state; the previous scores double-buffered in LDS; the
//           table in LDS up to VT_S_LDS states, read from global memory (coalesced along j) beyond; emissions staged
//           through LDS in tiles of VT_TILE frames, the next tile fetched into registers under the current one's steps;
//           back pointers uint8 (S <= 256) or uint16 in workspace order [B, T, S]; the walk reads them back in LDS slabs.
//   narrow  S <= VT_S_NARROW: one lane owns a sequence (64 sequences a wave), scores and the S^2 logs in registers,
//           emissions staged through LDS so that neighbouring lanes' rows are read in whole lines; the S two-bit back
//           pointers of a step are one byte, four steps a word in workspace order [T / 4, B].
#include <float.h>
#include <math.h>
#include "host.h"

namespace syg {
namespace {

constexpr int VT_S_MAX = 1024;           // largest S (one thread a state, one workgroup)
constexpr int VT_TILE = 16;              // frames of an emission tile
constexpr int VT_S_NARROW = 4;           // largest S of the narrow form (two bits a back pointer, a byte a step)
constexpr int VT_LDS_MAX = 160 * 1024;
constexpr int64_t VT_MAX_CELLS = (int64_t)1 << 40;   // B * T * S at most

__host__ __device__ constexpr int vt_row(int S) { return S | 1; }        // odd row stride of the wide form's tile
// LDS bytes of the wide form: two score rows, the emission tile, the table where it lives in LDS
__host__ __device__ constexpr int64_t vt_wide_lds(int64_t S, bool table) {
  return 8 * (2 * S + (int64_t)VT_TILE * (S | 1) + (table ? S * S : 0));
}
constexpr int vt_s_lds() {
  int s = 1;
  while (vt_wide_lds(s + 1, true) <= VT_LDS_MAX) ++s;
  return s;
}
constexpr int VT_S_LDS = vt_s_lds();     // 134: 8 S^2 + 16 S + 128 (S | 1) <= 160 KiB
constexpr int VT_NARROW_ROW = 65;        // doubles of a (frame, state) row of the narrow form's tile: 64 lanes + 1

struct VtArgs {
  const void* em;
  int em_f64, log_domain;
  int64_t sb, ss, st;
  int64_t B, T;
  int S;
  const int32_t* lengths;
  const double* ltrans; int64_t trans_bs;
  const double* linit;  int64_t init_bs;
  const double* lmarg;  int64_t marg_bs;
  double eps;
  void* work;
  int32_t* states;
  double* logp;
  int lds_bytes;
};

__device__ __forceinline__ double vt_load(const VtArgs& A, int64_t off) {
  return A.em_f64 ? static_cast<const double*>(A.em)[off] : (double)static_cast<const float*>(A.em)[off];
}
// the log-probability of a raw emission of state j of sequence b
__device__ __forceinline__ double vt_lp(const VtArgs& A, double raw, int64_t b, int j) {
  const double v = A.log_domain ? raw : log(raw + A.eps);
  return A.lmarg ? v - A.lmarg[b * A.marg_bs + j] : v;
}
__device__ __forceinline__ int64_t vt_len(const VtArgs& A, int64_t b) {
  int64_t len = A.lengths ? (int64_t)A.lengths[b] : A.T;
  return len < 1 ? 1 : (len > A.T ? A.T : len);      // the host refuses such a length; no access depends on that
}

template <bool WAVE>
__device__ __forceinline__ void vt_sync() {
  if (WAVE) wave_lds_sync(); else __syncthreads();
}

template <bool WAVE, bool TABLE_LDS, typename PT>
__global__ __launch_bounds__(WAVE ? 64 : 1024) void viterbi_wide_kernel(VtArgs A) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int S = A.S, SR = vt_row(S), tid = threadIdx.x, nt = blockDim.x;
  const int64_t b = blockIdx.x, T = A.T, len = vt_len(A, b);
  double* sc0 = sm;
  double* sc1 = sm + S;
  double* tile = sm + 2 * S;                       // [VT_TILE][SR]
  double* tab = tile + VT_TILE * SR;               // [S][S] (TABLE_LDS)
  const double* ltg = A.ltrans + b * A.trans_bs;
  PT* ptr = static_cast<PT*>(A.work) + b * T * S;
  const bool time_fast = A.st <= A.ss;             // which axis of the tile a thread's elements run along
  static_assert(VT_TILE == 16, "the time-fast mapping shifts by 4");

  if (TABLE_LDS)
    for (int i = tid; i < S * S; i += nt) tab[i] = ltg[i];
  // element k of a thread, VT_TILE of them cover the tile (nt >= S): along time, 16 neighbouring lanes take the 16
  // frames of a state's row; along the states, a lane takes its own state at frame k
  const int j0 = time_fast ? tid >> 4 : tid, dj = time_fast ? nt >> 4 : 0;
  const int tt0 = time_fast ? tid & (VT_TILE - 1) : 0, dt = time_fast ? 0 : 1;
  auto where = [&](int k, int& j, int& tt) { j = j0 + k * dj; tt = tt0 + k * dt; };
  const int64_t off0 = b * A.sb + (int64_t)j0 * A.ss + (int64_t)tt0 * A.st, dk = (int64_t)dj * A.ss + (int64_t)dt * A.st;
  auto fetch = [&](int64_t t0, double (&raw)[VT_TILE]) {
    const int64_t off = off0 + t0 * A.st;
    if (A.em_f64) {
      const double* p = static_cast<const double*>(A.em) + off;
#pragma unroll
      for (int k = 0; k < VT_TILE; ++k) raw[k] = (j0 + k * dj < S && t0 + tt0 + k * dt < T) ? p[k * dk] : 1.0;
    } else {
      const float* p = static_cast<const float*>(A.em) + off;
#pragma unroll
      for (int k = 0; k < VT_TILE; ++k) raw[k] = (j0 + k * dj < S && t0 + tt0 + k * dt < T) ? (double)p[k * dk] : 1.0;
    }
  };
  auto stage = [&](const double (&raw)[VT_TILE]) {
#pragma unroll
    for (int k = 0; k < VT_TILE; ++k) {
      int j, tt;
      where(k, j, tt);
      if (j < S) tile[tt * SR + j] = raw[k];
    }
    if (A.log_domain && !A.lmarg) return;
    // a thread turns its own elements into log-probabilities in place, one at a time: sixteen float64 logs unrolled
    // side by side would take more registers than a workgroup of 1024 threads has
#pragma unroll 1
    for (int k = 0; k < VT_TILE; ++k) {
      int j, tt;
      where(k, j, tt);
      if (j < S) tile[tt * SR + j] = vt_lp(A, tile[tt * SR + j], b, j);
    }
  };
  double raw[VT_TILE];
  fetch(0, raw);
  stage(raw);
  vt_sync<WAVE>();

  const int j = tid;
  const double li = j < S ? A.linit[b * A.init_bs + j] : 0.0;
  for (int64_t t0 = 0; t0 < len; t0 += VT_TILE) {
    const bool more = t0 + VT_TILE < len;
    if (more) fetch(t0 + VT_TILE, raw);            // in flight under this tile's steps
    const int steps = (int)(len - t0 < VT_TILE ? len - t0 : VT_TILE);
    for (int tt = 0; tt < steps; ++tt) {
      const int64_t t = t0 + tt;
      double* cur = (t & 1) ? sc1 : sc0;
      const double* prv = (t & 1) ? sc0 : sc1;
      if (j < S) {
        const double e = tile[tt * SR + j];
        double v;
        if (t == 0) {
          v = e + li;
        } else {
          double best = prv[0] + (TABLE_LDS ? tab[j] : ltg[j]);
          int arg = 0, i = 1;
          if (!TABLE_LDS) {
            // eight rows of the table in flight at a time (the loop is bound by the latency of these loads); the
            // comparisons stay in the order of i
            for (; i + 8 <= S; i += 8) {
              double l[8];
#pragma unroll
              for (int u = 0; u < 8; ++u) l[u] = ltg[(int64_t)(i + u) * S + j];
#pragma unroll
              for (int u = 0; u < 8; ++u) {
                const double c = prv[i + u] + l[u];
                if (c > best) { best = c; arg = i + u; }
              }
            }
          }
#pragma unroll 4
          for (; i < S; ++i) {
            const double c = prv[i] + (TABLE_LDS ? tab[i * S + j] : ltg[(int64_t)i * S + j]);
            if (c > best) { best = c; arg = i; }
          }
          v = e + best;
          ptr[t * S + j] = (PT)arg;
        }
        cur[j] = v;
      }
      vt_sync<WAVE>();
    }
    if (more) {
      stage(raw);
      vt_sync<WAVE>();
    }
  }

  // the path: the first argmax of the last scores, then back through the pointers, read in LDS slabs
  __syncthreads();                                 // the pointers of every lane are visible to the workgroup
  const double* fin = ((len - 1) & 1) ? sc1 : sc0;
  int s = 0;
  if (tid == 0) {
    double best = fin[0];
    for (int i = 1; i < S; ++i)
      if (fin[i] > best) { best = fin[i]; s = i; }
    A.logp[b] = best;
  }
  int32_t* out = A.states + b * T;
  for (int64_t t = len + tid; t < T; t += nt) out[t] = -1;
  PT* slab = reinterpret_cast<PT*>(tile);
  const int64_t room = ((int64_t)A.lds_bytes - 16 * (int64_t)S) / ((int64_t)S * (int64_t)sizeof(PT));
  const int64_t W = room < 4096 ? room : 4096;     // steps of a slab: at least 64, the tile alone holds that many
  for (int64_t hi = len - 1; hi >= 1; hi -= W) {
    const int64_t lo = hi - W > 0 ? hi - W : 0;    // steps lo + 1 .. hi
    const int64_t n = (hi - lo) * S;
    const PT* src = ptr + (lo + 1) * S;
    __syncthreads();
    for (int64_t i = tid; i < n; i += nt) slab[i] = src[i];
    __syncthreads();
    if (tid == 0)
      for (int64_t t = hi; t > lo; --t) {
        out[t] = s;
        s = (int)slab[(t - lo - 1) * S + s];
      }
  }
  if (tid == 0) out[0] = s;
}

template <int S>
__global__ __launch_bounds__(64) void viterbi_narrow_kernel(VtArgs A) {
  extern __shared__ __attribute__((aligned(16))) double tile[];   // [VT_TILE][S][VT_NARROW_ROW]
  const int lane = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * 64, T = A.T, B = A.B;
  const bool live = b0 + lane < B;
  const int64_t b = live ? b0 + lane : B - 1;      // an idle lane reads the last sequence and writes nothing
  const int64_t len = vt_len(A, b);
  double lt[S][S], val[S];
#pragma unroll
  for (int i = 0; i < S; ++i)
#pragma unroll
    for (int j = 0; j < S; ++j) lt[i][j] = A.ltrans[b * A.trans_bs + i * S + j];
#pragma unroll
  for (int j = 0; j < S; ++j) val[j] = A.linit[b * A.init_bs + j];
  uint32_t* words = static_cast<uint32_t*>(A.work);              // [ceil(T / 4)][B]
  uint32_t word = 0;
  constexpr int PER_SEQ = S * VT_TILE;
  for (int64_t t0 = 0; t0 < T; t0 += VT_TILE) {
    wave_lds_sync();                               // the previous tile is read
    for (int idx = lane; idx < 64 * PER_SEQ; idx += 64) {
      const int seq = idx / PER_SEQ, r = idx % PER_SEQ, j = r / VT_TILE, tt = r % VT_TILE;
      const int64_t bs = b0 + seq < B ? b0 + seq : B - 1;
      if (t0 + tt < T)
        tile[(tt * S + j) * VT_NARROW_ROW + seq] =
            vt_lp(A, vt_load(A, bs * A.sb + (int64_t)j * A.ss + (t0 + tt) * A.st), bs, j);
    }
    wave_lds_sync();
    const int steps = (int)(T - t0 < VT_TILE ? T - t0 : VT_TILE);
    for (int tt = 0; tt < steps; ++tt) {
      const int64_t t = t0 + tt;
      uint32_t bits = 0;
      if (t == 0) {
#pragma unroll
        for (int j = 0; j < S; ++j) val[j] = tile[(tt * S + j) * VT_NARROW_ROW + lane] + val[j];
      } else if (t < len) {
        double nv[S];
#pragma unroll
        for (int j = 0; j < S; ++j) {
          double best = val[0] + lt[0][j];
          uint32_t arg = 0;
#pragma unroll
          for (int i = 1; i < S; ++i) {
            const double c = val[i] + lt[i][j];
            if (c > best) { best = c; arg = i; }
          }
          nv[j] = tile[(tt * S + j) * VT_NARROW_ROW + lane] + best;
          bits |= arg << (2 * j);
        }
#pragma unroll
        for (int j = 0; j < S; ++j) val[j] = nv[j];
      }
      word |= bits << (8 * (int)(t & 3));
      if ((t & 3) == 3 || t == T - 1) {
        if (live) words[(t >> 2) * B + b] = word;
        word = 0;
      }
    }
  }
  if (!live) return;
  double best = val[0];
  uint32_t s = 0;
#pragma unroll
  for (int i = 1; i < S; ++i)
    if (val[i] > best) { best = val[i]; s = i; }
  A.logp[b] = best;
  int32_t* out = A.states + b * T;
  for (int64_t t = len; t < T; ++t) out[t] = -1;
  word = words[((len - 1) >> 2) * B + b];          // this lane's own stores
  for (int64_t t = len - 1; t >= 1; --t) {
    out[t] = (int32_t)s;
    s = (word >> (8 * (int)(t & 3) + 2 * s)) & 3u;
    if ((t & 3) == 0) word = words[((t - 1) >> 2) * B + b];
  }
  out[0] = (int32_t)s;
}

int64_t vt_ptr_bytes(int64_t S) { return S <= 256 ? 1 : 2; }

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_viterbi_constants(int key) {
  switch (key) {
    case SYG_VITERBI_S_MAX: return VT_S_MAX;
    case SYG_VITERBI_S_LDS: return VT_S_LDS;
    case SYG_VITERBI_S_NARROW: return VT_S_NARROW;
    case SYG_VITERBI_TILE: return VT_TILE;
    default: return -1;
  }
}

// The back pointers of either form: B T S pointers of one or two bytes, or (narrow) a byte a step in words of four
// steps; 4 B bytes on top cover the last word of the narrow form, and the size is a multiple of 8.
extern "C" int64_t syg_viterbi_work_bytes(int64_t B, int64_t S, int64_t T) {
  if (B < 1 || B >= 0x7fffffff || S < 1 || S > VT_S_MAX || T < 1 || T >= 0x7fffffff) return -1;
  if ((long double)B * (long double)T * (long double)S > (long double)VT_MAX_CELLS) return -1;
  return (B * T * S * vt_ptr_bytes(S) + 4 * B + 7) / 8 * 8;
}

extern "C" int syg_viterbi_f32(const void* emission, int dtype, int log_domain, int64_t stride_b, int64_t stride_s,
                               int64_t stride_t, int64_t B, int64_t S, int64_t T, const int32_t* lengths,
                               const double* log_trans, int64_t trans_bs, const double* log_init, int64_t init_bs,
                               const double* log_marginal, int64_t marginal_bs, double eps, void* work, int64_t work_bytes,
                               int32_t* states, double* logp, int form, void* stream) {
  SYG_REQUIRE(emission && log_trans && log_init && work && states && logp,
              "viterbi: null pointer argument (emission / log_trans / log_init / work / states / logp)");
  SYG_REQUIRE(dtype == SYG_VITERBI_F32 || dtype == SYG_VITERBI_F64,
              "viterbi: dtype %d is not served (SYG_VITERBI_F32 = 0, SYG_VITERBI_F64 = 1)", dtype);
  SYG_REQUIRE(S >= 1 && S <= VT_S_MAX, "viterbi: S = %lld is outside 1 .. %d states", (long long)S, VT_S_MAX);
  SYG_REQUIRE(B >= 1 && B < 0x7fffffff && T >= 1 && T < 0x7fffffff, "viterbi: bad B / T (each 1 .. 2^31 - 2)");
  const int64_t wb = syg_viterbi_work_bytes(B, S, T);
  SYG_REQUIRE(wb >= 0, "viterbi: B T S = %lld x %lld x %lld is more than 2^40 back pointers; decode the batch in pieces",
              (long long)B, (long long)T, (long long)S);
  SYG_REQUIRE(work_bytes >= wb, "viterbi: the workspace holds %lld bytes, syg_viterbi_work_bytes asks for %lld",
              (long long)work_bytes, (long long)wb);
  SYG_REQUIRE(stride_b >= 0 && stride_s >= 0 && stride_t >= 0, "viterbi: negative emission stride");
  SYG_REQUIRE(trans_bs == 0 || trans_bs == S * S, "viterbi: the batch stride of log_trans must be 0 (shared) or S S");
  SYG_REQUIRE(init_bs == 0 || init_bs == S, "viterbi: the batch stride of log_init must be 0 (shared) or S");
  SYG_REQUIRE(!log_marginal || marginal_bs == 0 || marginal_bs == S,
              "viterbi: the batch stride of log_marginal must be 0 (shared) or S");
  SYG_REQUIRE(log_domain || (isfinite(eps) && eps >= 0.0), "viterbi: eps must be finite and not negative");
  SYG_REQUIRE(form == SYG_VITERBI_AUTO || form == SYG_VITERBI_WIDE || form == SYG_VITERBI_NARROW,
              "viterbi: form %d is not served (0 automatic, 1 wide, 2 narrow)", form);
  SYG_REQUIRE(form != SYG_VITERBI_NARROW || S <= VT_S_NARROW, "viterbi: the narrow form serves S <= %d, not S = %lld",
              VT_S_NARROW, (long long)S);
  if (form == SYG_VITERBI_AUTO) form = syg_viterbi_form(B, S);

  VtArgs A{emission, dtype == SYG_VITERBI_F64, log_domain != 0, stride_b, stride_s, stride_t, B, T, (int)S, lengths,
           log_trans, trans_bs, log_init, init_bs, log_marginal, log_marginal ? marginal_bs : 0, eps, work, states, logp, 0};
  hipStream_t st = (hipStream_t)stream;
  if (form == SYG_VITERBI_NARROW) {
    const size_t lds = (size_t)VT_TILE * S * VT_NARROW_ROW * sizeof(double);
    const dim3 grid((unsigned)ceil_div(B, 64)), block(64);
    switch ((int)S) {
      case 1: hipLaunchKernelGGL(viterbi_narrow_kernel<1>, grid, block, lds, st, A); break;
      case 2: hipLaunchKernelGGL(viterbi_narrow_kernel<2>, grid, block, lds, st, A); break;
      case 3: hipLaunchKernelGGL(viterbi_narrow_kernel<3>, grid, block, lds, st, A); break;
      default: hipLaunchKernelGGL(viterbi_narrow_kernel<4>, grid, block, lds, st, A); break;
    }
    SYG_CHECK_LAUNCH("viterbi (narrow)");
    return SYG_OK;
  }
  const bool table = S <= VT_S_LDS;
  const size_t lds = (size_t)vt_wide_lds(S, table);
  A.lds_bytes = (int)lds;
  const dim3 grid((unsigned)B), block((unsigned)(ceil_div(S, 64) * 64));
  SYG_REQUIRE(B * (int64_t)block.x < ((int64_t)1 << 32),
              "viterbi: %lld sequences of %u threads are more than 2^32 threads a launch; decode the batch in pieces",
              (long long)B, block.x);
#define SYG_VT_LAUNCH(...)                                                                          \
  do {                                                                                              \
    if (const int rc = reserve_dynamic_lds("viterbi", (const void*)__VA_ARGS__, lds)) return rc;    \
    hipLaunchKernelGGL((__VA_ARGS__), grid, block, lds, st, A);                                     \
  } while (0)
  if (S <= 64) SYG_VT_LAUNCH(viterbi_wide_kernel<true, true, uint8_t>);
  else if (table) SYG_VT_LAUNCH(viterbi_wide_kernel<false, true, uint8_t>);
  else if (S <= 256) SYG_VT_LAUNCH(viterbi_wide_kernel<false, false, uint8_t>);
  else SYG_VT_LAUNCH(viterbi_wide_kernel<false, false, uint16_t>);
#undef SYG_VT_LAUNCH
  SYG_CHECK_LAUNCH("viterbi (wide)");
  return SYG_OK;
}

// The form the automatic rule takes, from profiles/viterbi_bench.json: the narrow form runs B / 64 waves where the wide
// one runs B workgroups, so it wins only on a batch that fills the device with them.  Measured on MI355X at T = 65:
// B = 12 288 narrow 1.91, 1.41 and 1.02 times faster at S = 1, 2, 3 and 0.88 at S = 4; B = 64 and B = 1024 wide 2 to 4
// times faster.  Where between 1024 and 12 288 sequences the forms cross was not measured: the rule takes the narrow
// form only where it was measured faster.
constexpr int VT_NARROW_RULE_S = 3;
constexpr int64_t VT_NARROW_RULE_B = 12288;
extern "C" int syg_viterbi_form(int64_t B, int64_t S) {
  if (B < 1 || S < 1 || S > VT_S_MAX) return -1;
  return (S <= VT_NARROW_RULE_S && B >= VT_NARROW_RULE_B) ? SYG_VITERBI_NARROW : SYG_VITERBI_WIDE;
}
