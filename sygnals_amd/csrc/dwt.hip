// Multi-level discrete wavelet transform and its inverse: PyWavelets 1.x `wavedec` / `waverec` as reached from
// sygnals/core/transforms.py:22 (discrete_wavelet_transform) and :81 (inverse_discrete_wavelet_transform), for the
// orthogonal filter banks of sygnals_amd/_wavelets.py (Daubechies, F = 2 ... 20 taps) and the extension modes zero,
// constant, symmetric, reflect and periodic.  The float64 restatement that is the contract lives in tests/dwt_ref.py.
//
// Analysis, one level of a length-N input: K = (N + F - 1) / 2 outputs,
//     cA[o] = sum_{j < F} dec_lo[j] ext(x)[2 o + 1 - j],   cD[o] = the same sum with dec_hi,
// both from the same F samples, read once.  The F samples of output o are the F / 2 aligned pairs that start at the even
// index 2 o + 2 - F: out of LDS a lane reads them as 8-byte words, consecutive lanes consecutive words (no bank
// conflict; a 4-byte read at stride 2 would be a 2-way one).  Only outputs whose samples leave 0 ... N - 1 take the
// extension rule (ext_index), which holds however many times F - 1 exceeds N.  The taps are read from their device
// arrays at compile-time offsets, i.e. once a wave into scalar registers; the kernels are instantiated per F so that the
// tap loops unroll.  Every sum is a chain of F fused multiply-adds in the order j = 0 ... F - 1, in every form, so the
// forms below agree bit for bit.
//
//   * clip-resident form (dwt_clip_kernel): one workgroup a clip runs all levels in one launch.  Level 1 streams x from
//     global memory, every cD goes straight to its place in the packed row, and the running approximation ping-pongs
//     between two LDS buffers (level 1, 3, ... write buffer A of max(n_1, F - 1) floats rounded up to even, level 2, 4,
//     ... buffer B of max(n_2, F - 1): the lengths of an input shorter than the filter rise towards F - 1); the last
//     level's cA goes to the row.  Fit rule (dwt_fits, exported as syg_dwt_fits): A + B <= 40960 floats, the 160 KiB of
//     a CU's LDS.
//   * streaming form, for rows that do not fit: one level a pass (dwt_level_kernel: 1024 outputs a workgroup, four a
//     thread), the approximations through the caller's workspace, each pass applying the extension rule to its own
//     level's input; as soon as what is left fits, the clip-resident kernel runs the remaining levels from the workspace
//     in one launch.
//
// Synthesis, one level of K approximation and K detail coefficients: 2 K - F + 2 outputs, the middle of the full
// up-sampled convolution, in polyphase form: with m = n / 2 and p = n % 2,
//     y[2 m + p] = sum_{i < F / 2} a[m + F / 2 - 1 - i] rec_lo[2 i + p] + d[m + F / 2 - 1 - i] rec_hi[2 i + p],
// F / 2 taps a phase and no products with inserted zeros; a thread owns m and writes both phases.  No output touches an
// edge, so there is no extension.  idwt_clip_kernel takes the coarse levels (its first level reads the packed row, the
// last one writes global memory, what lies between ping-pongs in LDS) for as long as a level's input and the input of
// the level before it fit the 40960 floats together -- the mirror of the analysis rule; idwt_level_kernel runs the finer
// levels of a longer row one a pass through the workspace.
#include "host.h"

namespace syg {
namespace {

constexpr int DWT_LDS_FLOATS = 160 * 1024 / 4;
constexpr int DWT_MAXLEV = 64;
constexpr int DWT_FMAX = 20;
constexpr int RT = 1024, DU = 4;                 // clip-resident kernels: up to 16 waves; outputs a thread and step
constexpr int DT = 256, DPT = 4, DTILE = DT * DPT;   // streaming kernels: outputs (pairs, for the inverse) a workgroup

// index of ext(x)[i] inside 0 ... N - 1, or -1 for a zero (i is outside the range)
template <typename I>
__device__ __forceinline__ I ext_index(I i, I N, int mode) {
  switch (mode) {
    case SYG_DWT_ZERO: return -1;
    case SYG_DWT_CONSTANT: return i < 0 ? 0 : N - 1;
    case SYG_DWT_PERIODIC: { const I m = i % N; return m < 0 ? m + N : m; }
    case SYG_DWT_REFLECT: {
      if (N == 1) return 0;
      const I P = 2 * N - 2;
      I m = i % P;
      if (m < 0) m += P;
      return m >= N ? P - m : m;
    }
    default: {                                   // SYG_DWT_SYMMETRIC
      const I P = 2 * N;
      I m = i % P;
      if (m < 0) m += P;
      return m >= N ? P - 1 - m : m;
    }
  }
}

typedef __attribute__((address_space(3))) volatile uint64_t lds_u64;

template <int F>
struct Taps {
  float lo[F], hi[F];
  __device__ __forceinline__ Taps(const float* __restrict__ l, const float* __restrict__ h) {
#pragma unroll
    for (int j = 0; j < F; ++j) { lo[j] = l[j]; hi[j] = h[j]; }
  }
};

// One output whose samples leave 0 ... N - 1: the same chain of fused multiply-adds as analyse(), as a rolled loop with
// the taps read from memory (a 64-bit modulo per sample is too much code to unroll F times for the few edge outputs).
template <typename I, typename P>
__device__ __forceinline__ void analyse_edge(P in, I N, I o, int F, int mode, const float* __restrict__ lo,
                                             const float* __restrict__ hi, float& a, float& d) {
  a = 0.f;
  d = 0.f;
#pragma unroll 1
  for (int j = 0; j < F; ++j) {
    const I i = 2 * o + 1 - j;
    const I k = (i >= 0 && i < N) ? i : ext_index<I>(i, N, mode);
    const float x = k < 0 ? 0.f : in[k];
    a = fmaf(lo[j], x, a);
    d = fmaf(hi[j], x, d);
  }
}

template <int F>
__device__ __forceinline__ void analyse(const Taps<F>& t, const float (&xs)[F], float& a, float& d) {
  a = 0.f;
  d = 0.f;
#pragma unroll
  for (int j = 0; j < F; ++j) { a = fmaf(t.lo[j], xs[j], a); d = fmaf(t.hi[j], xs[j], d); }
}

// xs[j] = in[2 o + 1 - j] for an interior output o: straight from global memory, or out of LDS as F / 2 aligned pairs
template <int F>
__device__ __forceinline__ void load_global(const float* __restrict__ g, int64_t o, float (&xs)[F]) {
#pragma unroll
  for (int j = 0; j < F; ++j) xs[j] = g[2 * o + 1 - j];
}
template <int F>
__device__ __forceinline__ void load_lds(const float* cur, int o, float (&xs)[F]) {
  // (volatile: the pairs stay single 8-byte reads; merged into two-address reads they run at half the LDS rate)
  const lds_u64* p = (const lds_u64*)cur + (o + 1 - F / 2);
#pragma unroll
  for (int q = 0; q < F / 2; ++q) {
    const uint64_t v = p[q];
    xs[F - 1 - 2 * q] = __uint_as_float((uint32_t)v);
    xs[F - 2 - 2 * q] = __uint_as_float((uint32_t)(v >> 32));
  }
}

template <int F>
__global__ __launch_bounds__(RT) void dwt_clip_kernel(const float* __restrict__ src, int64_t ldsrc, int N0, int nlev,
                                                      const float* __restrict__ lo, const float* __restrict__ hi,
                                                      int mode, float* __restrict__ out, int64_t ldout, int64_t dend,
                                                      int capA) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Taps<F> t(lo, hi);
  const int tid = threadIdx.x, nt = blockDim.x;
  const float* g = src + (int64_t)blockIdx.x * ldsrc;
  float* row = out + (int64_t)blockIdx.x * ldout;
  int N = N0;
  for (int lev = 0; lev < nlev; ++lev) {
    const int K = (N + F - 1) >> 1;
    const bool last = lev == nlev - 1;
    float* dD = row + (dend - K);
    const float* cur = (lev & 1) ? lds : lds + capA;         // what the level before wrote (lev >= 1)
    float* nxt = (lev & 1) ? lds + capA : lds;
    // outputs [oi0, oi1) read samples 0 ... N - 1 only; the others (at most F - 1, or all K of an input shorter than
    // the filter) take the extension rule
    const int oi0 = F / 2 - 1, oi1 = max(oi0, N >> 1);
    // DU outputs a thread and step, the loads of all of them issued before the first sum and free of branches (a step
    // past the end repeats the last interior output and drops the result): with one workgroup a CU (its LDS holds one
    // clip) the waves alone do not keep enough of level 1's global loads in flight
    for (int o0 = oi0 + tid; o0 < oi1; o0 += DU * nt) {
      float xs[DU][F];
      if (lev == 0) {
#pragma unroll
        for (int u = 0; u < DU; ++u) load_global<F>(g, min(o0 + u * nt, oi1 - 1), xs[u]);
      } else {
#pragma unroll
        for (int u = 0; u < DU; ++u) load_lds<F>(cur, min(o0 + u * nt, oi1 - 1), xs[u]);
      }
#pragma unroll
      for (int u = 0; u < DU; ++u) {
        const int o = o0 + u * nt;
        float a, d;
        analyse<F>(t, xs[u], a, d);
        if (o < oi1) {
          dD[o] = d;
          if (last) row[o] = a; else nxt[o] = a;
        }
      }
    }
    for (int e = tid; e < oi0 + K - oi1; e += nt) {
      const int o = e < oi0 ? e : oi1 + (e - oi0);
      float a, d;
      if (lev == 0) analyse_edge<int>(g, N, o, F, mode, lo, hi, a, d);
      else analyse_edge<int>(cur, N, o, F, mode, lo, hi, a, d);
      dD[o] = d;
      if (last) row[o] = a; else nxt[o] = a;
    }
    dend -= K;
    N = K;
    __syncthreads();
  }
}

template <int F>
__global__ __launch_bounds__(DT) void dwt_level_kernel(const float* __restrict__ src, int64_t ldsrc, int64_t N,
                                                       const float* __restrict__ lo, const float* __restrict__ hi,
                                                       int mode, float* __restrict__ dA, int64_t ldA,
                                                       float* __restrict__ dD, int64_t ldD, int64_t ntiles) {
  const Taps<F> t(lo, hi);
  const int64_t b = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
  const int64_t K = (N + F - 1) >> 1;
  const int64_t oi0 = F / 2 - 1, oi1 = max(oi0, N >> 1);     // the interior outputs, as in dwt_clip_kernel
  const float* g = src + b * ldsrc;
  float xs[DPT][F];
  if (oi1 > oi0) {                                 // every load of the thread's four outputs before the first sum
#pragma unroll
    for (int u = 0; u < DPT; ++u)
      load_global<F>(g, min(max(tile * DTILE + u * DT + threadIdx.x, oi0), oi1 - 1), xs[u]);
  }
#pragma unroll
  for (int u = 0; u < DPT; ++u) {
    const int64_t o = tile * DTILE + u * DT + threadIdx.x;
    float a, d;
    if (oi1 > oi0) analyse<F>(t, xs[u], a, d);
    if (o >= K) continue;
    if (o < oi0 || o >= oi1) analyse_edge<int64_t>(g, N, o, F, mode, lo, hi, a, d);
    dA[b * ldA + o] = a;
    dD[b * ldD + o] = d;
  }
}

// ------------------------------------------------------------------ synthesis
// av[i], dv[i] = a[m + i], d[m + i], i < F / 2: what the pair of outputs 2 m, 2 m + 1 reads
template <int F, typename PA>
__device__ __forceinline__ void synth_load(PA a, const float* __restrict__ d, int64_t m, float (&av)[F / 2],
                                           float (&dv)[F / 2]) {
#pragma unroll
  for (int i = 0; i < F / 2; ++i) { av[i] = a[m + i]; dv[i] = d[m + i]; }
}
template <int F>
__device__ __forceinline__ void synth_pair(const Taps<F>& t, const float (&av)[F / 2], const float (&dv)[F / 2], float& y0,
                                           float& y1) {
  y0 = 0.f;
  y1 = 0.f;
#pragma unroll
  for (int i = 0; i < F / 2; ++i) {
    const float a = av[F / 2 - 1 - i], d = dv[F / 2 - 1 - i];
    y0 = fmaf(a, t.lo[2 * i], y0);
    y0 = fmaf(d, t.hi[2 * i], y0);
    y1 = fmaf(a, t.lo[2 * i + 1], y1);
    y1 = fmaf(d, t.hi[2 * i + 1], y1);
  }
}

struct IdwtK { int32_t K[DWT_MAXLEV]; };

template <int F>
__global__ __launch_bounds__(RT) void idwt_clip_kernel(const float* __restrict__ coeffs, int64_t ldc, int64_t a0, IdwtK P,
                                                       int nlev, const float* __restrict__ rl,
                                                       const float* __restrict__ rh, float* __restrict__ y, int64_t ldy,
                                                       int capA) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Taps<F> t(rl, rh);
  const int tid = threadIdx.x, nt = blockDim.x;
  const float* row = coeffs + (int64_t)blockIdx.x * ldc;
  float* yr = y + (int64_t)blockIdx.x * ldy;
  int64_t doff = a0;
  for (int lev = 0; lev < nlev; ++lev) {
    const int K = P.K[lev], M = K - F / 2 + 1;
    const bool last = lev == nlev - 1;
    const float* d = row + doff;
    const float* cur = (lev & 1) ? lds : lds + capA;
    float* nxt = (lev & 1) ? lds + capA : lds;
    for (int m0 = tid; m0 < M; m0 += DU * nt) {    // DU pairs a thread and step, their loads first (see dwt_clip_kernel)
      float av[DU][F / 2], dv[DU][F / 2];
#pragma unroll
      for (int u = 0; u < DU; ++u) {                // (a step past the end repeats the last pair and drops the result)
        const int m = min(m0 + u * nt, M - 1);
        if (lev == 0) synth_load<F>(row, d, m, av[u], dv[u]);
        else synth_load<F>(cur, d, m, av[u], dv[u]);
      }
#pragma unroll
      for (int u = 0; u < DU; ++u) {
        const int m = m0 + u * nt;
        float y0, y1;
        synth_pair<F>(t, av[u], dv[u], y0, y1);
        if (m >= M) continue;
        if (last) { yr[2 * m] = y0; yr[2 * m + 1] = y1; }
        else *reinterpret_cast<float2*>(nxt + 2 * m) = make_float2(y0, y1);
      }
    }
    doff += K;
    __syncthreads();
  }
}

template <int F>
__global__ __launch_bounds__(DT) void idwt_level_kernel(const float* __restrict__ a, int64_t lda,
                                                        const float* __restrict__ d, int64_t ldd, int64_t K,
                                                        const float* __restrict__ rl, const float* __restrict__ rh,
                                                        float* __restrict__ y, int64_t ldy, int64_t ntiles) {
  const Taps<F> t(rl, rh);
  const int64_t b = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
  const int64_t M = K - F / 2 + 1;
  const float* ar = a + b * lda;
  const float* dr = d + b * ldd;
  float* yr = y + b * ldy;
  float av[DPT][F / 2], dv[DPT][F / 2];
#pragma unroll
  for (int u = 0; u < DPT; ++u) synth_load<F>(ar, dr, min(tile * DTILE + u * DT + threadIdx.x, M - 1), av[u], dv[u]);
#pragma unroll
  for (int u = 0; u < DPT; ++u) {
    const int64_t m = tile * DTILE + u * DT + threadIdx.x;
    float y0, y1;
    synth_pair<F>(t, av[u], dv[u], y0, y1);
    if (m >= M) continue;
    yr[2 * m] = y0;
    yr[2 * m + 1] = y1;
  }
}

// ------------------------------------------------------------------ host side
int64_t level_len(int64_t N, int F) { return (N + F - 1) / 2; }
int64_t even_up(int64_t n) { return (n + 1) & ~(int64_t)1; }

// Sizes (floats) of the two ping-pong buffers for the approximations of a length-N input: a_1, a_3, ... and a_2, a_4, ...
// The lengths fall from level to level while they exceed F - 1 and rise towards F - 1 from below (an input shorter than
// the filter), so n_1 and n_2 bound their buffers unless F - 1 does.
void dwt_buffers(int64_t N, int F, int64_t* capA, int64_t* capB) {
  const int64_t n1 = level_len(N, F), n2 = level_len(n1, F);
  *capA = even_up(n1 > F - 1 ? n1 : F - 1);
  *capB = n2 > F - 1 ? n2 : F - 1;
}
// the clip-resident analysis kernel can take a length-N input: the two buffers fit the LDS
bool dwt_fits(int64_t N, int F) {
  if (option(SYG_OPT_DWT_FORM) == 0) return false;
  int64_t ca, cb;
  dwt_buffers(N, F, &ca, &cb);
  return ca + cb <= DWT_LDS_FLOATS;
}
bool filter_ok(int F) { return F >= 2 && F <= DWT_FMAX && (F & 1) == 0; }

#define DWT_BY_F(F, CALL)                                                                                     \
  switch (F) {                                                                                                \
    case 2: CALL(2); break;   case 4: CALL(4); break;   case 6: CALL(6); break;   case 8: CALL(8); break;     \
    case 10: CALL(10); break; case 12: CALL(12); break; case 14: CALL(14); break; case 16: CALL(16); break;   \
    case 18: CALL(18); break; default: CALL(20); break;                                                       \
  }

int block_for(int64_t n) { return (int)(n >= RT ? RT : (n <= 64 ? 64 : ceil_div(n, 64) * 64)); }

// the levels [0, nlev) of a length-N input by the clip-resident kernel; dend: end of the first level's cD in the row
int launch_dwt_clip(const float* src, int64_t ldsrc, int64_t B, int64_t N, int nlev, const float* lo, const float* hi,
                    int F, int mode, float* out, int64_t ldout, int64_t dend, hipStream_t st) {
  const int64_t n1 = level_len(N, F);
  int64_t ca, cb;
  dwt_buffers(N, F, &ca, &cb);
  const int capA = (int)ca;
  const size_t bytes = nlev == 1 ? 0 : (nlev == 2 ? (size_t)ca * 4 : (size_t)(ca + cb) * 4);
#define CALL(FF)                                                                                               \
  {                                                                                                            \
    const int rc = reserve_dynamic_lds("dwt", (const void*)dwt_clip_kernel<FF>, bytes);                        \
    if (rc != SYG_OK) return rc;                                                                               \
    hipLaunchKernelGGL(dwt_clip_kernel<FF>, dim3((unsigned)B), dim3(block_for(n1)), bytes, st, src, ldsrc, (int)N, \
                       nlev, lo, hi, mode, out, ldout, dend, capA);                                            \
  }
  DWT_BY_F(F, CALL)
#undef CALL
  SYG_CHECK_LAUNCH("dwt (clip-resident)");
  return SYG_OK;
}

// lens (host): [a_n, d_n, ..., d_1]; K[i], out[i]: pairs and output length of synthesis level i (coarsest first)
int idwt_plan(const int64_t* lens, int levels, int F, int64_t* K, int64_t* outl) {
  SYG_REQUIRE(lens[0] >= 1, "idwt: inconsistent lens: lens[0] = %lld", (long long)lens[0]);
  int64_t a = lens[0];
  for (int i = 0; i < levels; ++i) {
    const int64_t d = lens[i + 1];
    SYG_REQUIRE(d >= F / 2, "idwt: inconsistent lens: level %d has %lld detail coefficients, fewer than F / 2 = %d", i,
                (long long)d, F / 2);
    SYG_REQUIRE(a == d || a == d + 1,
                "idwt: inconsistent lens: level %d has %lld approximation and %lld detail coefficients", i, (long long)a,
                (long long)d);
    K[i] = d;
    outl[i] = a = 2 * d - F + 2;
  }
  return SYG_OK;
}

// leading synthesis levels that the clip-resident kernel takes, and its two LDS buffer sizes
int idwt_resident_levels(const int64_t* K, const int64_t* outl, int levels, int64_t* capA, int64_t* capB) {
  int r = 0;
  int64_t ca = 0, cb = 0;
  // level r joins while its input and the input of the level before it fit together (the mirror of dwt_fits; the
  // bound on K[0] and K[1] keeps a long row's fine levels out of a one-workgroup kernel)
  while (r < levels && option(SYG_OPT_DWT_FORM) != 0 && K[r] + (r >= 1 ? K[r - 1] : 0) <= DWT_LDS_FLOATS) {
    // taking level r too makes out[r - 1] an LDS intermediate
    int64_t na = ca, nb = cb;
    if (r >= 1) { if ((r - 1) & 1) nb = nb > outl[r - 1] ? nb : outl[r - 1]; else na = na > outl[r - 1] ? na : outl[r - 1]; }
    if (na + nb > DWT_LDS_FLOATS) break;
    ca = na; cb = nb;
    ++r;
  }
  *capA = ca; *capB = cb;
  return r;
}

// workspace of the streaming synthesis levels r ... levels - 1: ping-pong buffers for out[r - 1] ... out[levels - 2]
void idwt_work_floats(const int64_t* outl, int levels, int r, int64_t* w0, int64_t* w1) {
  *w0 = *w1 = 0;
  if (r >= levels) return;
  for (int i = (r >= 1 ? r - 1 : 0); i <= levels - 2; ++i) {
    int64_t* w = (i & 1) ? w1 : w0;
    if (outl[i] > *w) *w = outl[i];
  }
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_dwt_lengths(int64_t L, int F, int levels, int64_t* lens_host) {
  if (!lens_host) { set_error("dwt_lengths: null pointer argument (lens)"); return -1; }
  if (L < 1 || levels < 1 || levels > DWT_MAXLEV) { set_error("dwt_lengths: bad L / levels (levels must be 1 ... %d)", DWT_MAXLEV); return -1; }
  if (!filter_ok(F)) { set_error("dwt_lengths: F must be even and in 2 ... %d (got %d)", DWT_FMAX, F); return -1; }
  int64_t n = L, total = 0;
  for (int l = 1; l <= levels; ++l) {
    n = level_len(n, F);
    lens_host[levels - l + 1] = n;
    total += n;
  }
  lens_host[0] = n;
  return total + n;
}

extern "C" int syg_dwt_fits(int64_t L, int F, int levels) {
  if (L < 1 || levels < 1 || levels > DWT_MAXLEV || !filter_ok(F)) return 0;
  return dwt_fits(L, F) ? 1 : 0;
}

extern "C" int64_t syg_dwt_work_bytes(int64_t B, int64_t L, int F, int levels) {
  if (B < 1 || L < 1 || levels < 1 || levels > DWT_MAXLEV || !filter_ok(F)) return -1;
  if (dwt_fits(L, F) || levels == 1) return 0;
  int64_t ca, cb;
  dwt_buffers(L, F, &ca, &cb);
  return B * (ca + cb) * (int64_t)sizeof(float);
}

extern "C" int syg_dwt_f32(const float* x, int64_t B, int64_t L, int64_t ldx, const float* dec_lo, const float* dec_hi,
                           int F, int mode, int levels, float* out, int64_t ldout, void* work, void* stream) {
  SYG_REQUIRE(x && dec_lo && dec_hi && out, "dwt: null pointer argument (x / dec_lo / dec_hi / out)");
  SYG_REQUIRE(B >= 1 && L >= 1 && B < 0x7fffffff, "dwt: bad B / L");
  SYG_REQUIRE(levels >= 1 && levels <= DWT_MAXLEV, "dwt: levels must be 1 ... %d (got %d)", DWT_MAXLEV, levels);
  SYG_REQUIRE(filter_ok(F), "dwt: F must be even and in 2 ... %d (got %d)", DWT_FMAX, F);
  SYG_REQUIRE(mode >= SYG_DWT_ZERO && mode <= SYG_DWT_PERIODIC, "dwt: unknown mode %d", mode);
  SYG_REQUIRE(ldx >= L, "dwt: ldx = %lld is smaller than the row (%lld)", (long long)ldx, (long long)L);
  int64_t n[DWT_MAXLEV + 1];
  n[0] = L;
  int64_t total = 0;
  for (int l = 1; l <= levels; ++l) { n[l] = level_len(n[l - 1], F); total += n[l]; }
  total += n[levels];
  SYG_REQUIRE(ldout >= total, "dwt: ldout = %lld is smaller than the packed row (%lld)", (long long)ldout,
              (long long)total);
  hipStream_t st = (hipStream_t)stream;
  if (dwt_fits(L, F)) return launch_dwt_clip(x, ldx, B, L, levels, dec_lo, dec_hi, F, mode, out, ldout, total, st);
  SYG_REQUIRE(levels == 1 || work, "dwt: %lld samples need a workspace of syg_dwt_work_bytes", (long long)L);
  int64_t ca, cb;
  dwt_buffers(L, F, &ca, &cb);
  float* w[2] = {(float*)work, (float*)work + B * ca};       // a_1, a_3, ... | a_2, a_4, ...
  const int64_t ldw[2] = {ca, cb};
  const float* src = x;
  int64_t lds_ = ldx, dend = total;
  for (int l = 1; l <= levels; ++l) {
    if (l > 1 && dwt_fits(n[l - 1], F))
      return launch_dwt_clip(src, lds_, B, n[l - 1], levels - l + 1, dec_lo, dec_hi, F, mode, out, ldout, dend, st);
    const int64_t K = n[l], ntiles = ceil_div(K, DTILE);
    SYG_REQUIRE(B * ntiles < 0x7fffffff, "dwt: too many tiles");
    const bool last = l == levels;
    float* dA = last ? out : w[(l - 1) & 1];
    const int64_t ldA = last ? ldout : ldw[(l - 1) & 1];
#define CALL(FF)                                                                                                   \
  hipLaunchKernelGGL(dwt_level_kernel<FF>, dim3((unsigned)(B * ntiles)), dim3(DT), 0, st, src, lds_, n[l - 1], dec_lo, \
                     dec_hi, mode, dA, ldA, out + (dend - K), ldout, ntiles);
    DWT_BY_F(F, CALL)
#undef CALL
    SYG_CHECK_LAUNCH("dwt (streaming)");
    dend -= K;
    src = dA;
    lds_ = ldA;
  }
  return SYG_OK;
}

extern "C" int64_t syg_idwt_length(const int64_t* lens_host, int levels, int F) {
  if (!lens_host) { set_error("idwt_length: null pointer argument (lens)"); return -1; }
  if (levels < 1 || levels > DWT_MAXLEV) { set_error("idwt_length: levels must be 1 ... %d", DWT_MAXLEV); return -1; }
  if (!filter_ok(F)) { set_error("idwt_length: F must be even and in 2 ... %d (got %d)", DWT_FMAX, F); return -1; }
  int64_t K[DWT_MAXLEV], outl[DWT_MAXLEV];
  if (idwt_plan(lens_host, levels, F, K, outl) != SYG_OK) return -1;
  return outl[levels - 1];
}

extern "C" int64_t syg_idwt_work_bytes(int64_t B, const int64_t* lens_host, int levels, int F) {
  if (B < 1 || !lens_host || levels < 1 || levels > DWT_MAXLEV || !filter_ok(F)) return -1;
  int64_t K[DWT_MAXLEV], outl[DWT_MAXLEV], ca, cb, w0, w1;
  if (idwt_plan(lens_host, levels, F, K, outl) != SYG_OK) return -1;
  const int r = idwt_resident_levels(K, outl, levels, &ca, &cb);
  idwt_work_floats(outl, levels, r, &w0, &w1);
  return B * (w0 + w1) * (int64_t)sizeof(float);
}

extern "C" int syg_idwt_f32(const float* coeffs, int64_t B, int64_t ldc, const int64_t* lens_host, int levels,
                            const float* rec_lo, const float* rec_hi, int F, float* y, int64_t ldy, void* work,
                            void* stream) {
  SYG_REQUIRE(coeffs && lens_host && rec_lo && rec_hi && y, "idwt: null pointer argument (coeffs / lens / rec_lo / rec_hi / y)");
  SYG_REQUIRE(B >= 1 && B < 0x7fffffff, "idwt: bad B");
  SYG_REQUIRE(levels >= 1 && levels <= DWT_MAXLEV, "idwt: levels must be 1 ... %d (got %d)", DWT_MAXLEV, levels);
  SYG_REQUIRE(filter_ok(F), "idwt: F must be even and in 2 ... %d (got %d)", DWT_FMAX, F);
  int64_t K[DWT_MAXLEV], outl[DWT_MAXLEV];
  const int prc = idwt_plan(lens_host, levels, F, K, outl);
  if (prc != SYG_OK) return prc;
  int64_t total = lens_host[0];
  for (int i = 0; i < levels; ++i) total += K[i];
  SYG_REQUIRE(ldc >= total, "idwt: ldc = %lld is smaller than the packed row (%lld)", (long long)ldc, (long long)total);
  SYG_REQUIRE(ldy >= outl[levels - 1], "idwt: ldy = %lld is smaller than the row (%lld)", (long long)ldy,
              (long long)outl[levels - 1]);
  int64_t ca, cb, w0, w1;
  const int r = idwt_resident_levels(K, outl, levels, &ca, &cb);
  idwt_work_floats(outl, levels, r, &w0, &w1);
  SYG_REQUIRE(w0 + w1 == 0 || work, "idwt: %lld samples need a workspace of syg_idwt_work_bytes",
              (long long)outl[levels - 1]);
  hipStream_t st = (hipStream_t)stream;
  float* w[2] = {(float*)work, (float*)work + B * w0};
  const int64_t ldw[2] = {w0, w1};
  const float* a = coeffs;
  int64_t lda = ldc;
  if (r >= 1) {
    IdwtK P;
    for (int i = 0; i < DWT_MAXLEV; ++i) P.K[i] = i < r ? (int32_t)K[i] : 0;
    const bool fin = r == levels;
    float* dst = fin ? y : w[(r - 1) & 1];
    const int64_t ldd = fin ? ldy : ldw[(r - 1) & 1];
    const size_t bytes = (size_t)(ca + cb) * 4;
    const int nt = block_for(K[r - 1]);
#define CALL(FF)                                                                                                  \
  {                                                                                                               \
    const int rc = reserve_dynamic_lds("idwt", (const void*)idwt_clip_kernel<FF>, bytes);                         \
    if (rc != SYG_OK) return rc;                                                                                  \
    hipLaunchKernelGGL(idwt_clip_kernel<FF>, dim3((unsigned)B), dim3(nt), bytes, st, coeffs, ldc, lens_host[0], P, r, \
                       rec_lo, rec_hi, dst, ldd, (int)ca);                                                        \
  }
    DWT_BY_F(F, CALL)
#undef CALL
    SYG_CHECK_LAUNCH("idwt (clip-resident)");
    a = dst;
    lda = ldd;
  }
  int64_t doff = lens_host[0];
  for (int i = 0; i < r; ++i) doff += K[i];
  for (int i = r; i < levels; ++i) {
    const int64_t M = K[i] - F / 2 + 1, ntiles = ceil_div(M, DTILE);
    SYG_REQUIRE(B * ntiles < 0x7fffffff, "idwt: too many tiles");
    const bool fin = i == levels - 1;
    float* dst = fin ? y : w[i & 1];
    const int64_t ldd = fin ? ldy : ldw[i & 1];
#define CALL(FF)                                                                                                    \
  hipLaunchKernelGGL(idwt_level_kernel<FF>, dim3((unsigned)(B * ntiles)), dim3(DT), 0, st, a, lda, coeffs + doff, ldc, \
                     K[i], rec_lo, rec_hi, dst, ldd, ntiles);
    DWT_BY_F(F, CALL)
#undef CALL
    SYG_CHECK_LAUNCH("idwt (streaming)");
    doff += K[i];
    a = dst;
    lda = ldd;
  }
  return SYG_OK;
}
