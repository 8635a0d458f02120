// Rhythm after the onset envelope: librosa 0.10 `feature.tempogram` (autocorrelation form), `feature.tempo` and
// `beat.beat_track`.  Parity is unpinned (librosa is not a dependency): the float64 restatement of tests/beat_ref.py is
// the contract.
//
// Tempogram (tempogram_kernel<R>): a workgroup of four waves owns a run of SYG_BEAT_SLICE_TILES tiles of TF consecutive
// frames of one clip (TF = tg_tile(win_length): what keeps the tile's result within 48 KiB).  A tile's span of the padded
// envelope (TF + win_length - 1 values, the linear ramps formed on the fly) is staged in LDS once.  A wave takes a frame:
// it writes the windowed frame f behind zeros into a buffer of its own, then lane l forms the R consecutive lags
// l R ... l R + R - 1 (R = tg_lags(win_length): the smallest served count with 64 R >= win_length, so one pass of the
// wave takes every lag): eight f[j] (the same address in every lane) and R + 7 f[j + k] make 8 R fused multiply-adds, in
// float32 over 64 values of j, then added into a float64 sum.  The order is fixed: the same call gives the same bits.
// A lane stops at the last j its lowest lag has, so the wave runs as long as lane 0: half the issue slots of the
// triangle r[k], k < win_length, are spent on lanes that have finished.  The tile's columns go through LDS so
// that the store runs along frames; the aggregate (the mean over frames, float64) is summed per lag in frame order into
// one partial row per workgroup, and tempogram_mean_kernel adds the partial rows in order.
//
// Tempo (tempo_pick_kernel): a thread per column: first argmax of log1p(1e6 a[k]) + logprior[k] in float64.
//
// Local score (ls_scale_kernel, ls_conv_kernel, ls_max_kernel): the clip's standard deviation from float64 sums, then
// the Gaussian taps of the clip's own period against the scaled envelope in float64, cut where a tap is below
// exp(-24.5) (7 standard deviations), then the clip's maximum.
//
// Beat DP (beat_dp_kernel<NT, NPT>): one wave (periods up to 383) or four (beyond) own a clip.  Thread i holds the
// transition costs of offsets i, i + NT, ... in registers; the last 2 period values of the cumulative score sit in an
// LDS ring in float64; a step is J additions, a first-argmax reduction (DPP inside a wave) and one LDS store.
//
// Beats (beat_track_kernel): the local maxima's exact median by bitwise selection on the order-preserving integer image
// of the doubles (64 counting passes), the last beat, then one thread follows the back links, trims and writes.
// No atomics anywhere.
#include <float.h>
#include <limits.h>
#include <math.h>
#include "host.h"

namespace syg {
namespace {

constexpr int BT_WIN_MAX = 2048;
constexpr int BT_PERIOD_MAX = 2047;
constexpr int BT_LOG_TABLE = 4096;
constexpr int BT_SLICE_TILES = 16;
constexpr int64_t BT_MAX_ELEMS = (int64_t)1 << 31;
constexpr int BT_DP_WAVE_PERIOD = 383;     // periods up to this: one wave a clip
constexpr int BT_LS_TILE = 1024;
constexpr int BT_LS_QMAX = 448;            // ceil(7 * 2047 / 32)

constexpr int TG_T = 256;

inline int tg_tile(int win) {
  int tf = 64;
  while (tf > 4 && (int64_t)win * tf > 12288) tf >>= 1;
  return tf;
}
inline int tg_lags(int win) {
  const int served[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32};
  for (int r : served)
    if (64 * r >= win) return r;
  return 32;
}
inline int tg_fstride(int win, int R) { return (win + R + 16 + 3) & ~3; }
inline size_t tg_lds_bytes(int win) {
  const int TF = tg_tile(win), R = tg_lags(win);
  const size_t win4 = (size_t)((win + 3) & ~3), spn4 = (size_t)((TF + win - 1 + 3) & ~3);
  return (win4 + spn4 + 4 * (size_t)tg_fstride(win, R) + (size_t)win * (TF + 1)) * sizeof(float);
}

struct TgArgs {
  const float* env; int64_t T, ld, n; int win, center, norm, TF, FS; int64_t nsl; const float* window; float* tg;
  double* part;
};

template <int R>
__global__ __launch_bounds__(TG_T) void tempogram_kernel(TgArgs A) {
  extern __shared__ float4 tg_smem[];
  const int win = A.win, TF = A.TF, TFp = TF + 1;
  float* wnd = (float*)tg_smem;
  float* span = wnd + ((win + 3) & ~3);
  float* fb = span + ((TF + win - 1 + 3) & ~3);
  float* res = fb + 4 * A.FS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t b = blockIdx.x / A.nsl, s = blockIdx.x % A.nsl;
  const float* e = A.env + b * A.ld;
  const int64_t T = A.T, n = A.n;
  const int p = A.center ? win / 2 : 0;
  for (int i = tid; i < win; i += TG_T) wnd[i] = A.window[i];
  double agg[BT_WIN_MAX / TG_T];
#pragma unroll
  for (int u = 0; u < BT_WIN_MAX / TG_T; ++u) agg[u] = 0.0;
  const int64_t f0 = s * BT_SLICE_TILES * TF, f1 = min(n, f0 + (int64_t)BT_SLICE_TILES * TF);
  const double e0 = (double)e[0], eT = (double)e[T - 1];
  float* f = fb + w * A.FS;
  const int k0 = lane * R;
  const int nj = win - k0;
  const int nblk = nj > 0 ? (nj + 7) >> 3 : 0;
  for (int j = win + lane; j < A.FS; j += 64) f[j] = 0.f;         // what a lag reads past the frame
  for (int64_t t0 = f0; t0 < f1; t0 += TF) {
    const int nf = (int)min((int64_t)TF, f1 - t0);
    __syncthreads();                             // the tile before is out of span and res
    for (int i = tid; i < nf + win - 1; i += TG_T) {
      const int64_t u = t0 + i - p;              // the envelope's index of padded sample t0 + i
      float v;
      if (u < 0) {
        v = (float)(e0 * (double)(u + p) / (double)p);
      } else if (u < T) {
        v = e[u];
      } else {
        const int64_t q = u - T;
        v = q < p ? (float)(eT * (double)(p - 1 - q) / (double)p) : 0.f;
      }
      span[i] = v;
    }
    __syncthreads();
    for (int tf = w; tf < nf; tf += 4) {
      wave_lds_sync();
      for (int j = lane; j < win; j += 64) f[j] = wnd[j] * span[tf + j];
      wave_lds_sync();
      double dacc[R];
#pragma unroll
      for (int r = 0; r < R; ++r) dacc[r] = 0.0;
      for (int c = 0; c < nblk; c += 8) {
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.f;
        const int ce = min(c + 8, nblk);
        for (int bb = c; bb < ce; ++bb) {
          const int j = bb * 8;
          float x[8], y[R + 8];
          const float4 xa = *(const float4*)(f + j), xb = *(const float4*)(f + j + 4);
          x[0] = xa.x; x[1] = xa.y; x[2] = xa.z; x[3] = xa.w; x[4] = xb.x; x[5] = xb.y; x[6] = xb.z; x[7] = xb.w;
          if constexpr (R % 4 == 0) {
#pragma unroll
            for (int q = 0; q < R / 4 + 2; ++q) {
              const float4 v = *(const float4*)(f + j + k0 + 4 * q);
              y[4 * q] = v.x; y[4 * q + 1] = v.y; y[4 * q + 2] = v.z; y[4 * q + 3] = v.w;
            }
          } else {
#pragma unroll
            for (int q = 0; q < R + 7; ++q) y[q] = f[j + k0 + q];
          }
#pragma unroll
          for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = fmaf(x[u], y[u + r], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) dacc[r] += (double)acc[r];
      }
      float rv[R];
      float m = 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        rv[r] = (float)dacc[r];
        if (k0 + r < win) m = fmaxf(m, fabsf(rv[r]));
      }
      m = wave_max(m);
      if (A.norm && m >= FLT_MIN) {
#pragma unroll
        for (int r = 0; r < R; ++r) rv[r] = rv[r] / m;
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (k0 + r < win) res[(k0 + r) * TFp + tf] = rv[r];
    }
    __syncthreads();
    if (A.tg) {
      float* o = A.tg + b * win * n + t0;
      for (int i = tid; i < win * nf; i += TG_T) {
        const int k = i / nf, tf = i - k * nf;
        o[(int64_t)k * n + tf] = res[k * TFp + tf];
      }
    }
    if (A.part) {
#pragma unroll
      for (int u = 0; u < BT_WIN_MAX / TG_T; ++u) {
        const int k = tid + u * TG_T;
        if (k < win)
          for (int tf = 0; tf < nf; ++tf) agg[u] += (double)res[k * TFp + tf];
      }
    }
  }
  if (A.part) {
#pragma unroll
    for (int u = 0; u < BT_WIN_MAX / TG_T; ++u) {
      const int k = tid + u * TG_T;
      if (k < win) A.part[(b * A.nsl + s) * win + k] = agg[u];
    }
  }
}

// a[b, k] = (sum over the slices' partial rows, in order) / n
__global__ __launch_bounds__(256) void tempogram_mean_kernel(const double* part, int64_t B, int win, int64_t nsl, int64_t n,
                                                             double* a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * win) return;
  const int64_t b = i / win;
  const int k = (int)(i - b * win);
  double s = 0.0;
  for (int64_t q = 0; q < nsl; ++q) s += part[(b * nsl + q) * win + k];
  a[i] = s / (double)n;
}

// ------------------------------------------------------------------ tempo
__global__ __launch_bounds__(256) void tempo_pick_kernel(const double* a, const float* tg, int64_t B, int win, int64_t n,
                                                         const float* metrics, const double* logprior, const double* bpms,
                                                         int32_t* kstar, double* tempo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * n) return;
  const int64_t b = i / n, t = i - b * n;
  if (!(metrics[2 * b + 1] > 0.f)) {             // an all-zero envelope: no tempo
    kstar[i] = 0;
    tempo[i] = 0.0;
    return;
  }
  double best = -INFINITY;
  int bk = 0;
  for (int k = 0; k < win; ++k) {
    const double v = a ? a[b * win + k] : (double)tg[(b * win + k) * n + t];
    const double sc = log1p(1e6 * v) + logprior[k];
    if (sc != sc) { bk = k; break; }             // numpy's argmax takes the first NaN
    if (sc > best) { best = sc; bk = k; }
  }
  kstar[i] = bk;
  tempo[i] = bpms[bk];
}

// ------------------------------------------------------------------ local score
constexpr int LS_ST = 1024;

__device__ __forceinline__ double block_sum_d(double v, double* red, int tid, int nt) {
  red[tid] = v;
  __syncthreads();
  for (int d = nt / 2; d >= 1; d >>= 1) {
    if (tid < d) red[tid] += red[tid + d];
    __syncthreads();
  }
  const double s = red[0];
  __syncthreads();
  return s;
}

// scale[b] = std(env, ddof = 1) where the envelope is divided by it, else 1
__global__ __launch_bounds__(LS_ST) void ls_scale_kernel(const float* env, int64_t T, int64_t ld, double* scale) {
  __shared__ double red[LS_ST];
  const int tid = threadIdx.x;
  const float* e = env + (int64_t)blockIdx.x * ld;
  double s = 0.0;
  for (int64_t i = tid; i < T; i += LS_ST) s += (double)e[i];
  const double mean = block_sum_d(s, red, tid, LS_ST) / (double)T;
  double q = 0.0;
  for (int64_t i = tid; i < T; i += LS_ST) {
    const double d = (double)e[i] - mean;
    q += d * d;
  }
  q = block_sum_d(q, red, tid, LS_ST);
  if (tid == 0) {
    const double sd = T >= 2 ? sqrt(q / (double)(T - 1)) : 0.0;
    scale[blockIdx.x] = (T >= 2 && isfinite(sd) && sd > 0.0) ? sd : 1.0;
  }
}

__device__ __forceinline__ bool period_served(int P) { return P >= 2 && P <= BT_PERIOD_MAX; }

__global__ __launch_bounds__(256) void ls_conv_kernel(const float* env, int64_t T, int64_t ld, const int32_t* period,
                                                      const double* scale, int64_t ntile, float* ls) {
  __shared__ double g[2 * BT_LS_QMAX + 1];
  __shared__ double x[BT_LS_TILE + 2 * BT_LS_QMAX];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / ntile, s = blockIdx.x % ntile;
  const int64_t i0 = s * BT_LS_TILE, i1 = min(T, i0 + BT_LS_TILE);
  float* o = ls + b * T;
  const int P = period[b];
  if (!period_served(P)) {
    for (int64_t i = i0 + tid; i < i1; i += 256) o[i] = 0.f;
    return;
  }
  const int Q = min(min(P, (7 * P + 31) / 32), BT_LS_QMAX);
  const float* e = env + b * ld;
  const double sd = scale[b];
  for (int q = tid; q <= 2 * Q; q += 256) {
    const double z = 32.0 * (double)(q - Q) / (double)P;
    g[q] = exp(-0.5 * (z * z));
  }
  const int nx = (int)(i1 - i0) + 2 * Q;
  for (int i = tid; i < nx; i += 256) {
    const int64_t u = i0 - Q + i;
    x[i] = (u >= 0 && u < T) ? (double)e[u] / sd : 0.0;
  }
  __syncthreads();
  for (int i = tid; i < (int)(i1 - i0); i += 256) {
    // ls[i0 + i] = sum_q g[q] e[i0 + i - q], q = -Q .. Q: x index i + Q - q
    double acc = 0.0;
    for (int q = 0; q <= 2 * Q; ++q) acc = fma(g[q], x[i + 2 * Q - q], acc);
    o[i0 + i] = (float)acc;
  }
}

__global__ __launch_bounds__(LS_ST) void ls_max_kernel(const float* ls, int64_t T, float* lsmax) {
  __shared__ float red[LS_ST / 64];
  const int tid = threadIdx.x;
  const float* r = ls + (int64_t)blockIdx.x * T;
  float m = -INFINITY;
  for (int64_t i = tid; i < T; i += LS_ST) m = fmaxf(m, r[i]);
  m = wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < LS_ST / 64; ++i) m = fmaxf(m, red[i]);
    lsmax[blockIdx.x] = m;
  }
}

// ------------------------------------------------------------------ beat DP
__device__ __forceinline__ int half_even(int P) { return (P & 1) ? ((P >> 1) + ((P >> 1) & 1)) : (P >> 1); }

constexpr int DP_CHUNK = 256;             // local scores staged at a time

struct DpArgs {
  const float* ls; const float* lsmax; const int32_t* period; int64_t T; double tightness; const double* logtab;
  int pcap, mask; double* cum; int32_t* back;
};

template <int NT, int NPT>
__global__ __launch_bounds__(NT) void beat_dp_kernel(DpArgs A) {
  extern __shared__ double dp_ring[];
  __shared__ double rv[2][NT / 64];
  __shared__ int rj[2][NT / 64];
  __shared__ float lsb[DP_CHUNK];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x, T = A.T;
  const float* l = A.ls + b * T;
  double* cum = A.cum + b * T;
  int32_t* back = A.back + b * T;
  const int P = A.period[b];
  if (P < 2 || P > A.pcap) {                     // no beats: defined outputs all the same
    for (int64_t i = tid; i < T; i += NT) { cum[i] = 0.0; back[i] = -1; }
    return;
  }
  const int J = 2 * P - half_even(P) + 1;        // offsets -2 P .. -half_even(P); J <= NT * NPT by pcap
  double tx[NPT];
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int j = tid + u * NT;
    tx[u] = 0.0;
    if (j < J) {
      const double d = A.logtab[2 * P - j - 1] - A.logtab[P - 1];
      tx[u] = -A.tightness * (d * d);
    }
  }
  const double thresh = 0.01 * (double)A.lsmax[b];
  const int mask = A.mask;
  bool first = true;
  for (int64_t c0 = 0; c0 < T; c0 += DP_CHUNK) {
    const int nc = (int)min((int64_t)DP_CHUNK, T - c0);
    __syncthreads();
    for (int i = tid; i < nc; i += NT) lsb[i] = l[c0 + i];
    __syncthreads();
    for (int ci = 0; ci < nc; ++ci) {
      const int64_t i = c0 + ci;
      double best = -INFINITY;
      int bj = INT_MAX;
#pragma unroll
      for (int u = 0; u < NPT; ++u) {
        const int j = tid + u * NT;
        if (j < J) {
          const int64_t src = i - 2 * P + j;
          const double c = tx[u] + (src >= 0 ? dp_ring[(int)(src & mask)] : 0.0);
          if (c > best) { best = c; bj = j; }
        }
      }
      wave_pick<true>(best, bj);                 // the larger value, the smaller offset among equals: numpy's first argmax
      if (NT > 64) {
        const int par = ci & 1;                  // two sets of slots: a wave may be a step ahead of its reader
        if ((tid & 63) == 0) { rv[par][tid >> 6] = best; rj[par][tid >> 6] = bj; }
        __syncthreads();
        best = rv[par][0];
        bj = rj[par][0];
#pragma unroll
        for (int q = 1; q < NT / 64; ++q) take_better<true>(best, bj, rv[par][q], rj[par][q]);
      }
      const double li = (double)lsb[ci];
      const double cs = li + best;
      int bk = -1;
      if (!(first && li < thresh)) {
        bk = (int)(i - 2 * P + bj);
        first = false;
      }
      if (tid == 0) {
        cum[i] = cs;
        back[i] = bk;
        dp_ring[(int)(i & mask)] = cs;
      }
      if (NT > 64) __syncthreads(); else wave_lds_sync();
    }
  }
}

// ------------------------------------------------------------------ beats
constexpr int BK_T = 256;

__device__ __forceinline__ unsigned long long dkey(double v) {     // order-preserving image of a double
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double dunkey(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}
__device__ __forceinline__ bool local_max(const double* c, int64_t i, int64_t T) {
  if (i == 0) return false;
  if (i == T - 1) return c[i] > c[i - 1];
  return c[i] > c[i - 1] && c[i] >= c[i + 1];
}
__device__ __forceinline__ long long block_sum_ll(long long v, long long* red, int tid) {
  red[tid] = v;
  __syncthreads();
  for (int d = BK_T / 2; d >= 1; d >>= 1) {
    if (tid < d) red[tid] += red[tid + d];
    __syncthreads();
  }
  const long long s = red[0];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(BK_T) void beat_track_kernel(const float* ls, const double* cum, const int32_t* back,
                                                          int64_t T, const int32_t* period, int trim, int32_t* beats,
                                                          int32_t* count, int32_t* last_out) {
  __shared__ long long red[BK_T];
  __shared__ unsigned long long redu[BK_T];
  __shared__ int s_cnt;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const float* l = ls + b * T;
  const double* c = cum + b * T;
  const int32_t* bl = back + b * T;
  int32_t* out = beats + b * T;
  const int P = period[b];
  long long last = -1;
  long long nlm = 0;
  if (period_served(P)) {
    long long cnt = 0;
    for (int64_t i = tid; i < T; i += BK_T) cnt += local_max(c, i, T);
    nlm = block_sum_ll(cnt, red, tid);
  }
  if (nlm > 0) {
    // the k1-th and k2-th smallest of the local maxima (0-based), k1 = (nlm - 1) / 2, k2 = nlm / 2
    long long k = (nlm - 1) / 2;
    unsigned long long prefix = 0ull;
    for (int bit = 63; bit >= 0; --bit) {
      const unsigned long long hi = bit == 63 ? 0ull : ~((2ull << bit) - 1ull);      // the bits above `bit`
      long long cz = 0;
      for (int64_t i = tid; i < T; i += BK_T)
        if (local_max(c, i, T)) {
          const unsigned long long q = dkey(c[i]);
          cz += (q & hi) == prefix && !((q >> bit) & 1ull);
        }
      cz = block_sum_ll(cz, red, tid);
      if (k >= cz) { k -= cz; prefix |= 1ull << bit; }
    }
    const double v1 = dunkey(prefix);
    double med = v1;
    if (!(nlm & 1)) {
      long long le = 0;
      unsigned long long mg = ~0ull;
      for (int64_t i = tid; i < T; i += BK_T)
        if (local_max(c, i, T)) {
          const unsigned long long q = dkey(c[i]);
          if (q <= prefix) ++le; else mg = q < mg ? q : mg;
        }
      le = block_sum_ll(le, red, tid);
      redu[tid] = mg;
      __syncthreads();
      for (int d = BK_T / 2; d >= 1; d >>= 1) {
        if (tid < d) redu[tid] = redu[tid + d] < redu[tid] ? redu[tid + d] : redu[tid];
        __syncthreads();
      }
      const double v2 = nlm / 2 < le ? v1 : dunkey(redu[0]);
      __syncthreads();
      med = __dmul_rn(__dadd_rn(v1, v2), 0.5);
    }
    long long lb = -1;
    for (int64_t i = tid; i < T; i += BK_T) {
      const double v = local_max(c, i, T) ? 2.0 * c[i] : 0.0;
      if (v > med) lb = i;                       // a thread's frames ascend
    }
    red[tid] = lb;
    __syncthreads();
    for (int d = BK_T / 2; d >= 1; d >>= 1) {
      if (tid < d) red[tid] = red[tid + d] > red[tid] ? red[tid + d] : red[tid];
      __syncthreads();
    }
    last = red[0];
    __syncthreads();
  }
  if (tid == 0) {
    int nb = 0;
    for (long long i = last; i >= 0; i = bl[i]) ++nb;
    int q = nb;
    for (long long i = last; i >= 0; i = bl[i]) out[--q] = (int32_t)i;
    int lo = 0, hi = 0;                          // the beats kept: [lo, hi)
    if (nb > 0) {
      auto sm = [&](int i) {
        const double a = i > 0 ? (double)l[out[i - 1]] : 0.0, m = (double)l[out[i]];
        const double z = i + 1 < nb ? (double)l[out[i + 1]] : 0.0;
        return __dadd_rn(__dadd_rn(__dmul_rn(0.5, a), m), __dmul_rn(0.5, z));
      };
      double th = 0.0;
      if (trim) {
        double ss = 0.0;
        for (int i = 0; i < nb; ++i) {
          const double v = sm(i);
          ss = __dadd_rn(ss, __dmul_rn(v, v));
        }
        th = __dmul_rn(0.5, sqrt(ss / (double)nb));
      }
      int vmin = -1, vmax = -1;
      for (int i = 0; i < nb; ++i)
        if (sm(i) > th) { if (vmin < 0) vmin = i; vmax = i; }
      if (vmin >= 0) { lo = vmin; hi = vmax; }   // the upper end is exclusive
    }
    for (int i = lo; i < hi; ++i) out[i - lo] = out[i];
    s_cnt = hi - lo;
    count[b] = hi - lo;
    if (last_out) last_out[b] = (int32_t)last;
  }
  __syncthreads();
  for (int64_t i = s_cnt + tid; i < T; i += BK_T) out[i] = -1;
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_beat_constants(int key) {
  switch (key) {
    case SYG_BEAT_WIN_MAX: return BT_WIN_MAX;
    case SYG_BEAT_PERIOD_MAX: return BT_PERIOD_MAX;
    case SYG_BEAT_LOG_TABLE: return BT_LOG_TABLE;
    case SYG_BEAT_SLICE_TILES: return BT_SLICE_TILES;
    case SYG_BEAT_DP_WAVE_PERIOD: return BT_DP_WAVE_PERIOD;
    case SYG_BEAT_MAX_ELEMS: return BT_MAX_ELEMS;
    default: return -1;
  }
}

extern "C" int syg_tempogram_tile(int win_length) {
  return (win_length >= 2 && win_length <= BT_WIN_MAX) ? tg_tile(win_length) : -1;
}

static int64_t tg_frames(int64_t T, int win, int center) { return center ? T : T - win + 1; }

extern "C" int64_t syg_tempogram_work_bytes(int64_t B, int64_t T, int win_length, int center) {
  if (B < 1 || T < 1 || win_length < 2 || win_length > BT_WIN_MAX) return -1;
  const int64_t n = tg_frames(T, win_length, center);
  if (n < 1 || n > BT_MAX_ELEMS || B > BT_MAX_ELEMS) return -1;
  const int64_t nsl = ceil_div(n, (int64_t)BT_SLICE_TILES * tg_tile(win_length));
  if (B > BT_MAX_ELEMS / nsl) return -1;
  return B * nsl * win_length * (int64_t)sizeof(double);
}

extern "C" int syg_tempogram_f32(const float* env, int64_t B, int64_t T, int64_t ld, int win_length, int center,
                                 const float* window, int norm, float* tg, double* agg, void* work, int64_t work_bytes,
                                 void* stream) {
  SYG_REQUIRE(env && window, "tempogram: null pointer argument (env / window)");
  SYG_REQUIRE(tg || agg, "tempogram: neither tg nor agg is asked for");
  SYG_REQUIRE(win_length >= 2 && win_length <= BT_WIN_MAX, "tempogram: win_length = %d is outside 2 .. %d", win_length,
              BT_WIN_MAX);
  SYG_REQUIRE(B >= 1 && T >= 1 && T < 0x7fffffff && ld >= T, "tempogram: bad B / T / ld");
  SYG_REQUIRE(norm == 0 || norm == 1, "tempogram: norm must be 0 (none) or 1 (inf)");
  const int64_t n = tg_frames(T, win_length, center != 0);
  SYG_REQUIRE(n >= 1, "tempogram: %lld frames are fewer than win_length = %d without centering", (long long)T, win_length);
  SYG_REQUIRE(!tg || (long double)B * win_length * (long double)n <= (long double)BT_MAX_ELEMS,
              "tempogram: the result [%lld, %d, %lld] has more than 2^31 elements", (long long)B, win_length, (long long)n);
  const int TF = tg_tile(win_length), R = tg_lags(win_length);
  const int64_t nsl = ceil_div(n, (int64_t)BT_SLICE_TILES * TF);
  SYG_REQUIRE(B * nsl < 0x7fffffff, "tempogram: too many slices");
  if (agg) {
    const int64_t wb = syg_tempogram_work_bytes(B, T, win_length, center != 0);
    SYG_REQUIRE(work && work_bytes >= wb, "tempogram: the aggregate needs a workspace of syg_tempogram_work_bytes (%lld bytes)",
                (long long)wb);
  }
  TgArgs A{env, T, ld, n, win_length, center != 0, norm, TF, tg_fstride(win_length, R), nsl, window, tg,
           agg ? (double*)work : nullptr};
  const size_t lds = tg_lds_bytes(win_length);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(B * nsl)), block(TG_T);
#define SYG_TG_CASE(RR)                                                                          \
  case RR: {                                                                                     \
    const int rc = reserve_dynamic_lds("tempogram", (const void*)tempogram_kernel<RR>, lds);     \
    if (rc != SYG_OK) return rc;                                                                 \
    hipLaunchKernelGGL(tempogram_kernel<RR>, grid, block, lds, st, A);                           \
    break;                                                                                       \
  }
  switch (R) {
    SYG_TG_CASE(1) SYG_TG_CASE(2) SYG_TG_CASE(3) SYG_TG_CASE(4) SYG_TG_CASE(6) SYG_TG_CASE(8) SYG_TG_CASE(12)
    SYG_TG_CASE(16) SYG_TG_CASE(24) SYG_TG_CASE(32)
    default: SYG_REQUIRE(false, "tempogram: no kernel for %d lags a lane", R);
  }
#undef SYG_TG_CASE
  SYG_CHECK_LAUNCH("tempogram");
  if (agg) {
    hipLaunchKernelGGL(tempogram_mean_kernel, dim3((unsigned)ceil_div(B * win_length, 256)), dim3(256), 0, st,
                       (const double*)work, B, win_length, nsl, n, agg);
    SYG_CHECK_LAUNCH("tempogram (mean)");
  }
  return SYG_OK;
}

extern "C" int64_t syg_tempo_pick_work_bytes(int64_t B) { return B >= 1 ? B * 2 * (int64_t)sizeof(float) : -1; }

extern "C" int syg_tempo_pick_f32(const double* a, const float* tg, int64_t B, int win_length, int64_t n, const float* env,
                                  int64_t T, int64_t ld, const double* logprior, const double* bpms, int32_t* kstar,
                                  double* tempo, void* work, void* stream) {
  SYG_REQUIRE((a != nullptr) != (tg != nullptr), "tempo_pick: give the aggregate a or the tempogram tg, not both");
  SYG_REQUIRE(env && logprior && bpms && kstar && tempo && work,
              "tempo_pick: null pointer argument (env / logprior / bpms / kstar / tempo / work)");
  SYG_REQUIRE(win_length >= 2 && win_length <= BT_WIN_MAX, "tempo_pick: win_length = %d is outside 2 .. %d", win_length,
              BT_WIN_MAX);
  SYG_REQUIRE(B >= 1 && n >= 1 && (a == nullptr || n == 1) && T >= 1 && ld >= T, "tempo_pick: bad B / n / T / ld");
  SYG_REQUIRE((long double)B * win_length * (long double)n <= (long double)BT_MAX_ELEMS,
              "tempo_pick: more than 2^31 elements");
  const int rc = syg_clip_metrics_f32(env, B, T, ld, (float*)work, stream);
  if (rc != SYG_OK) return rc;
  hipLaunchKernelGGL(tempo_pick_kernel, dim3((unsigned)ceil_div(B * n, 256)), dim3(256), 0, (hipStream_t)stream, a, tg, B,
                     win_length, n, (const float*)work, logprior, bpms, kstar, tempo);
  SYG_CHECK_LAUNCH("tempo_pick");
  return SYG_OK;
}

extern "C" int64_t syg_beat_local_score_work_bytes(int64_t B) { return B >= 1 ? B * (int64_t)sizeof(double) : -1; }

extern "C" int syg_beat_local_score_f32(const float* env, int64_t B, int64_t T, int64_t ld, const int32_t* period, float* ls,
                                        float* lsmax, void* work, void* stream) {
  SYG_REQUIRE(env && period && ls && lsmax && work, "beat_local_score: null pointer argument (env / period / ls / lsmax / work)");
  SYG_REQUIRE(B >= 1 && B < 0x7fffffff && T >= 1 && T < 0x7fffffff && ld >= T, "beat_local_score: bad B / T / ld");
  const int64_t ntile = ceil_div(T, BT_LS_TILE);
  SYG_REQUIRE(B * ntile < 0x7fffffff && (long double)B * (long double)T <= (long double)BT_MAX_ELEMS,
              "beat_local_score: more than 2^31 elements");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ls_scale_kernel, dim3((unsigned)B), dim3(LS_ST), 0, st, env, T, ld, (double*)work);
  SYG_CHECK_LAUNCH("beat_local_score (scale)");
  hipLaunchKernelGGL(ls_conv_kernel, dim3((unsigned)(B * ntile)), dim3(256), 0, st, env, T, ld, period, (const double*)work,
                     ntile, ls);
  SYG_CHECK_LAUNCH("beat_local_score");
  hipLaunchKernelGGL(ls_max_kernel, dim3((unsigned)B), dim3(LS_ST), 0, st, (const float*)ls, T, lsmax);
  SYG_CHECK_LAUNCH("beat_local_score (maximum)");
  return SYG_OK;
}

extern "C" int syg_beat_dp_f32(const float* ls, const float* lsmax, int64_t B, int64_t T, const int32_t* period,
                               int period_max, double tightness, const double* logtab, double* cum, int32_t* back,
                               void* stream) {
  SYG_REQUIRE(ls && lsmax && period && logtab && cum && back,
              "beat_dp: null pointer argument (ls / lsmax / period / logtab / cum / back)");
  SYG_REQUIRE(B >= 1 && B < 0x7fffffff && T >= 1 && T < 0x7fffffff && (long double)B * (long double)T <= (long double)BT_MAX_ELEMS,
              "beat_dp: bad B / T");
  SYG_REQUIRE(period_max >= 2 && period_max <= BT_PERIOD_MAX, "beat_dp: period_max = %d is outside 2 .. %d", period_max,
              BT_PERIOD_MAX);
  SYG_REQUIRE(isfinite(tightness) && tightness > 0.0, "beat_dp: tightness must be positive and finite");
  int ring = 4;
  while (ring < 2 * period_max) ring <<= 1;
  DpArgs A{ls, lsmax, period, T, tightness, logtab, period_max, ring - 1, cum, back};
  const size_t lds = (size_t)ring * sizeof(double);
  hipStream_t st = (hipStream_t)stream;
  // offsets of a row: 2 P - half_even(P) + 1 <= 1.5 P + 1.5
  if (period_max <= 84)                          // J <= 128
    hipLaunchKernelGGL((beat_dp_kernel<64, 2>), dim3((unsigned)B), dim3(64), lds, st, A);
  else if (period_max <= BT_DP_WAVE_PERIOD)      // J <= 576
    hipLaunchKernelGGL((beat_dp_kernel<64, 9>), dim3((unsigned)B), dim3(64), lds, st, A);
  else                                           // J <= 3073
    hipLaunchKernelGGL((beat_dp_kernel<256, 13>), dim3((unsigned)B), dim3(256), lds, st, A);
  SYG_CHECK_LAUNCH("beat_dp");
  return SYG_OK;
}

extern "C" int syg_beat_track_f32(const float* ls, const double* cum, const int32_t* back, int64_t B, int64_t T,
                                  const int32_t* period, int trim, int32_t* beats, int32_t* count, int32_t* last,
                                  void* stream) {
  SYG_REQUIRE(ls && cum && back && period && beats && count,
              "beat_track: null pointer argument (ls / cum / back / period / beats / count)");
  SYG_REQUIRE(B >= 1 && B < 0x7fffffff && T >= 1 && T < 0x7fffffff && (long double)B * (long double)T <= (long double)BT_MAX_ELEMS,
              "beat_track: bad B / T");
  hipLaunchKernelGGL(beat_track_kernel, dim3((unsigned)B), dim3(BK_T), 0, (hipStream_t)stream, ls, cum, back, T, period,
                     trim != 0, beats, count, last);
  SYG_CHECK_LAUNCH("beat_track");
  return SYG_OK;
}
