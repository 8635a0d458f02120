// YIN / pYIN pitch tracking: librosa 0.10 `yin` / `pyin` as called by fundamental_frequency,
// sygnals/core/audio/features.py:135-220 (and by jitter :319 / shimmer :412 through it).  The float64 restatement that
// is the contract lives in tests/pitch_ref.py; every host constant comes from sygnals_amd/_pitch.py.
//
// Frame stage (pitch_frames_kernel): one WAVE per frame of 2048 samples, persistent grid over B x T.
//   acf(tau) = sum_{j=1..W} x_j x_{j+tau} = irfft(rfft(x) rfft(x[W:0:-1]))[W + tau]: two 2048-point real transforms
//   and one inverse, each a 1024-point complex wave FFT (wave_fft.h) of the even / odd packing z[m] = x[2m] + i x[2m+1]
//   with the real-input split done in registers (the lane that owns bin k also owns 1024 - k, so the product and the
//   inverse split need no data movement); the inverse runs the forward transform on the conjugate.
//   e(tau) = sum_{j=tau+1..tau+W} x_j^2 from a float64 wave prefix sum of x^2, the CMNDF's cumulative mean from a
//   second float64 prefix sum; the CMNDF is rounded to float32 once and every later decision (parabolic shift,
//   troughs, thresholds, pitch bins) is taken on those float32 values promoted to float64 -- the tests feed the same
//   values to the restatement.  pYIN: the 100 thresholds sit on the lanes (m = lane, lane + 64); troughs are walked in
//   lag order, the Boltzmann prior of a trough is one wave sum.  Output: a compact candidate list per frame
//   (bin, prob) of stride K, its count and voiced_prob; librosa's assignment rule (larger lag wins a shared bin) and
//   the dropped bin == n_bins row are applied here.
//
// Viterbi (pyin_viterbi_kernel): one workgroup per clip, float64 scores double-buffered in LDS.  A state's predecessors
// are its band in both voicing blocks (tables of log(transition + tiny) from the host) plus the best out-of-band state,
// whose log-transition is log(tiny): that one is the first argmax of v(i) + log(tiny) over ALL states -- if it lies
// inside the band, the band entry (log T >= log(tiny)) at the same index already dominates it, so the comparison stays
// exact.  Backpointers (uint16) go to the caller's workspace; one thread backtracks.
#include <float.h>
#include "wave_fft.h"
#include "host.h"

namespace syg {
namespace {

constexpr int PW = 2;                    // waves per workgroup of the frame stage
constexpr int NF = 2048;                 // frame length (the only one offloaded)
constexpr int CM_OFF = 128;              // float offset of the CMNDF in aux (after the 64 prefix bases)
constexpr int AUX = (CM_OFF + NF) / 2;   // per-wave scratch: float64 prefix bases, then the CMNDF (float)
constexpr int NTHR = 100;                // pYIN thresholds

struct PitchLds {
  float2 sc[PW][wfft::SC_COMPLEX];       // FFT exchange; later the trough list (int)
  float2 cb[PW][1024];                   // inverse input / output (c[n] as float); later the trough probabilities
  double aux[PW][AUX];
  float2 tw2l[wfft::TW2_COMPLEX];
  float2 tw1l[wfft::TW1_COMPLEX];
  float2 t2048[8][64];                   // W_2048^k of (lane, unit j, pair d), index j * 4 + d
};

// host table layout (float64), built by sygnals_amd/_pitch.py: pyin_device_table()
//   [0, 100) thresholds linspace(0, 1, 101)[1:]   [100, 200) beta_probs   [200, 301) no_trough_prob * sum(beta[:M])
//   [301, 301 + K + 1) Boltzmann factor (1 - e^-l) / (1 - e^-l n), n = 0..K   then e^(-l pos), pos = 0..K
constexpr int PT_THR = 0, PT_BETA = 100, PT_NOTR = 200, PT_FACT = 301;

__device__ __forceinline__ double shfl_up_d(double v, int d) { return __shfl_up(v, d, 64); }

// a 64-lane Hillis-Steele: its order of additions differs from common.h's float scan (rows of 16, then the rows)
__device__ __forceinline__ double wave_excl_scan_d(double v, int lane) {
  double s = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = shfl_up_d(s, d);
    if (lane >= d) s += o;
  }
  return s - v;
}
__device__ __forceinline__ int lanes_below(uint64_t m, int lane) {
  return __popcll(m & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
}

// E = zk + conj(zm), O = -i (zk - conj(zm));  X[k] = (E + w O) / 2,  X[1024 - k] = conj(E - w O) / 2
__device__ __forceinline__ void split_fwd(float2 zk, float2 zm, float2 w, float2& xk, float2& xm) {
  const float2 E = make_float2(zk.x + zm.x, zk.y - zm.y);
  const float2 O = make_float2(zk.y + zm.y, zm.x - zk.x);
  const float2 wO = cmul(w, O);
  xk = make_float2(0.5f * (E.x + wO.x), 0.5f * (E.y + wO.y));
  xm = make_float2(0.5f * (E.x - wO.x), -0.5f * (E.y - wO.y));
}
// inverse split of the product spectrum P (Hermitian, length 2048) into the packed spectrum Zc of c[2m] + i c[2m+1]:
// Ec = (P[k] + conj(P[1024-k])) / 2, Oc = (P[k] - conj(P[1024-k])) conj(w) / 2, Zc[k] = Ec + i Oc,
// Zc[1024-k] = conj(Ec) + i conj(Oc)
__device__ __forceinline__ void split_inv(float2 pk, float2 pm, float2 w, float2& zk, float2& zm) {
  const float2 Ec = make_float2(0.5f * (pk.x + pm.x), 0.5f * (pk.y - pm.y));
  const float2 D = make_float2(0.5f * (pk.x - pm.x), 0.5f * (pk.y + pm.y));
  const float2 Oc = cmulc(D, w);
  zk = make_float2(Ec.x - Oc.y, Ec.y + Oc.x);
  zm = make_float2(Ec.x + Oc.y, -Ec.y + Oc.x);
}

struct FrameArgs {
  const float* y; int64_t L, ldy; int win, hop, center; int64_t T, nframes;
  double sr; int min_p, max_p, n_lag, mode; double trough_threshold;
  double fmin; int n_bins; const double* ptab; int K;
  float* f0; int* cand_bin; float* cand_prob; int* cand_count; float* voiced_prob; float* cmndf;
};

__device__ __forceinline__ double parabolic_shift(const float* cm, int i, int n_lag) {
  if (i <= 0 || i >= n_lag - 1) return 0.0;
  const double cl = cm[i - 1], c0 = cm[i], cr = cm[i + 1];
  const double a = cr + cl - 2.0 * c0, b = (cr - cl) / 2.0;
  return (fabs(b) >= fabs(a)) ? 0.0 : -b / a;
}

__global__ __launch_bounds__(PW * 64) void pitch_frames_kernel(FrameArgs A, const float2* __restrict__ tw) {
  __shared__ __attribute__((aligned(16))) PitchLds S;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  wfft::Lane lc;
  wfft::init_lane(lc, lane);
  wfft::init_tables(S.tw2l, S.tw1l, tw, NF, tid, PW * 64);
  for (int i = tid; i < 8 * 64; i += PW * 64) {
    const int q = i >> 6, l = i & 63;
    S.t2048[q][l] = tw[wfft::bin_of(l, q >> 2, q & 3)];
  }
  __syncthreads();
  float2* sc = S.sc[w];
  float2* cb = S.cb[w];
  float* cbf = reinterpret_cast<float*>(cb);
  int* tl = reinterpret_cast<int*>(sc);
  double* aux = S.aux[w];
  const int W = A.win, n_lag = A.n_lag;

  for (int64_t f = (int64_t)blockIdx.x * PW + w; f < A.nframes; f += (int64_t)gridDim.x * PW) {
    const int64_t b = f / A.T, t = f - b * A.T;
    const float* yr = A.y + b * A.ldy;
    const int64_t s0 = t * A.hop - (A.center ? NF / 2 : 0);
    auto xat = [&](int n) -> float {
      const int64_t s = s0 + n;
      return (s >= 0 && s < A.L) ? yr[s] : 0.f;
    };
    // ---- transforms of a = x and b = x[W:0:-1] (zero beyond W samples)
    float2 va[16], vb[16];
#pragma unroll
    for (int a = 0; a < 16; ++a) {
      const int m = 64 * a + lane;
      va[a] = make_float2(xat(2 * m), xat(2 * m + 1));
      vb[a] = make_float2(2 * m < W ? xat(W - 2 * m) : 0.f, 2 * m + 1 < W ? xat(W - 2 * m - 1) : 0.f);
    }
    float2 ak[2][4], am[2][4], bk[2][4], bm[2][4], a512, b512;
    wfft::cfft1024(va, lc, sc, S.tw1l, S.tw2l, lane, ak, am, a512);
    wfft::cfft1024(vb, lc, sc, S.tw1l, S.tw2l, lane, bk, bm, b512);
    // ---- product spectrum, inverse split, conjugate into natural order
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const float2 wk = S.t2048[4 * j + d][lane];
        float2 xa, xam, xb, xbm, zk, zm;
        split_fwd(ak[j][d], am[j][d], wk, xa, xam);
        split_fwd(bk[j][d], bm[j][d], wk, xb, xbm);
        split_inv(cmul(xa, xb), cmul(xam, xbm), wk, zk, zm);
        const int k = wfft::bin_of(lane, j, d);
        cb[k] = make_float2(zk.x, -zk.y);
        if (k != 0) cb[1024 - k] = make_float2(zm.x, -zm.y);
      }
    if (lane == 0) {
      const float2 wk = make_float2(0.f, -1.f);    // W_2048^512
      float2 xa, xam, xb, xbm, zk, zm;
      split_fwd(a512, a512, wk, xa, xam);
      split_fwd(b512, b512, wk, xb, xbm);
      split_inv(cmul(xa, xb), cmul(xam, xbm), wk, zk, zm);
      cb[512] = make_float2(zk.x, -zk.y);
    }
    wave_lds_sync();
    float2 vc[16];
#pragma unroll
    for (int a = 0; a < 16; ++a) vc[a] = cb[64 * a + lane];
    wave_lds_sync();
    float2 ck[2][4], cm_[2][4], c512;
    wfft::cfft1024(vc, lc, sc, S.tw1l, S.tw2l, lane, ck, cm_, c512);
    constexpr float INV = 1.f / 1024.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int k = wfft::bin_of(lane, j, d);
        cb[k] = make_float2(ck[j][d].x * INV, -ck[j][d].y * INV);
        if (k != 0) cb[1024 - k] = make_float2(cm_[j][d].x * INV, -cm_[j][d].y * INV);
      }
    if (lane == 0) cb[512] = make_float2(c512.x * INV, -c512.y * INV);
    wave_lds_sync();

    // ---- energies (float64): P[n] = sum_{i<n} x_i^2; lane l owns tau = 32 l .. 32 l + 31
    {
      double s = 0.0;
      for (int i = 0; i < 32; ++i) { const double v = xat(32 * lane + i); s += v * v; }
      aux[lane] = wave_excl_scan_d(s, lane);
    }
    wave_lds_sync();
    auto prefix = [&](int n) -> double {        // P[n], 0 <= n <= 2048
      const int c = n >> 5;
      double p = (c < 64) ? aux[c] : aux[63];
      if (c >= 64) { for (int i = 32 * 63; i < NF; ++i) { const double v = xat(i); p += v * v; } return p; }
      for (int i = 32 * c; i < n; ++i) { const double v = xat(i); p += v * v; }
      return p;
    };
    const double e0raw = prefix(W + 1) - prefix(1);
    const double e0 = fabs(e0raw) < 1e-6 ? 0.0 : e0raw;
    const int tau0 = 32 * lane;
    // d(tau) over this lane's 32 lags, twice: once for the cumulative-mean prefix, once (after every read of c[]) to
    // write the CMNDF over c[] -- recomputing costs a few cached loads, holding 32 float64 values costs the occupancy
    auto lane_d = [&](auto&& body) {
      if (tau0 > A.max_p) return;
      double e = prefix(tau0 + W + 1) - prefix(tau0 + 1);
#pragma unroll 1
      for (int q = 0; q < 32; ++q) {
        const int tau = tau0 + q;
        if (tau > A.max_p) break;
        const double et = fabs(e) < 1e-6 ? 0.0 : e;
        double ac = (double)cbf[W + tau];
        ac = fabs(ac) < 1e-6 ? 0.0 : ac;
        body(tau, (e0 + et) - 2.0 * ac);
        const double xa = xat(tau + W + 1), xb = xat(tau + 1);
        e = e + xa * xa - xb * xb;
      }
    };
    double csum = 0.0;
    lane_d([&](int tau, double dq) { if (tau >= 1) csum += dq; });
    double cum = wave_excl_scan_d(csum, lane);
    float* cmw = reinterpret_cast<float*>(aux) + CM_OFF;
    lane_d([&](int tau, double dq) {
      if (tau >= 1) cum += dq;
      if (tau >= A.min_p) cmw[tau - A.min_p] = (float)(dq / (cum / (double)tau + DBL_MIN));
    });
    wave_lds_sync();
    const float* cmv = cmw;
    double* pk = reinterpret_cast<double*>(cb);   // trough probabilities (c[] is no longer needed)
    if (A.cmndf)
      for (int i = lane; i < n_lag; i += 64) A.cmndf[f * n_lag + i] = cmv[i];

    // ---- troughs (localmin with edge padding; trough[0] = c[0] < c[1]), YIN's first trough under the threshold and
    // the first global minimum
    int nt = 0, first_thr = -1;
    float vmin = INFINITY;
    int imin = 0x7fffffff;
    for (int base = 0; base < n_lag; base += 64) {
      const int i = base + lane;
      bool tr = false;
      float c0 = INFINITY;
      if (i < n_lag) {
        c0 = cmv[i];
        if (i == 0) tr = c0 < cmv[1];
        else if (i == n_lag - 1) tr = c0 < cmv[i - 1];
        else tr = (c0 < cmv[i - 1]) && (c0 <= cmv[i + 1]);
        if (c0 < vmin) { vmin = c0; imin = i; }
      }
      const uint64_t m = __ballot(tr);
      if (tr) tl[nt + lanes_below(m, lane)] = i;
      nt += __popcll(m);
      if (first_thr < 0) {
        const uint64_t mt = __ballot(tr && c0 < A.trough_threshold);
        if (mt) first_thr = base + __builtin_ctzll(mt);
      }
    }
    // first index of the global minimum: wave min of value, then of index among the lanes that hold it
    imin = wave_min_i(vmin == wave_min(vmin) ? imin : 0x7fffffff);
    wave_lds_sync();

    if (A.mode == 0) {
      const int idx = first_thr >= 0 ? first_thr : imin;
      if (lane == 0) A.f0[f] = (float)(A.sr / ((double)(A.min_p + idx) + parabolic_shift(cmv, idx, n_lag)));
      continue;
    }

    // ---- pYIN: thresholds m0 = lane, m1 = lane + 64 (m1 < 100)
    const double* pt = A.ptab;
    const bool has1 = lane + 64 < NTHR;
    const double thr0 = pt[PT_THR + lane], thr1 = has1 ? pt[PT_THR + lane + 64] : -1.0;
    const double beta0 = pt[PT_BETA + lane], beta1 = has1 ? pt[PT_BETA + lane + 64] : 0.0;
    const double* fact = pt + PT_FACT;
    const double* ek = pt + PT_FACT + A.K + 1;
    int n0 = 0, n1 = 0, g = 0;
    float hg = INFINITY;
    for (int k = 0; k < nt; ++k) {
      const double h = cmv[tl[k]];
      n0 += h < thr0;
      n1 += h < thr1;
      if ((float)h < hg) { hg = (float)h; g = k; }
    }
    int p0 = 0, p1 = 0;
    for (int k = 0; k < nt; ++k) {
      const double h = cmv[tl[k]];
      double c = 0.0;
      if (h < thr0) { c += fact[n0] * ek[p0] * beta0; ++p0; }
      if (h < thr1) { c += fact[n1] * ek[p1] * beta1; ++p1; }
      double p = wave_sum_d(c);
      if (k == g) {
        const int M = __popcll(__ballot(h >= thr0)) + __popcll(__ballot(has1 && h >= thr1));
        p += pt[PT_NOTR + M];
      }
      if (lane == 0) pk[k] = p;
    }
    wave_lds_sync();
    // candidates in lag order: p > 0 and bin < n_bins (bin == n_bins is librosa's first unvoiced row, overwritten);
    // compacted in place (write position <= read position)
    int nc = 0;
    for (int base = 0; base < nt; base += 64) {
      const int k = base + lane;
      bool ok = false;
      int bin = 0;
      double p = 0.0;
      if (k < nt) {
        const int idx = tl[k];
        p = pk[k];
        const double period = (double)(A.min_p + idx) + parabolic_shift(cmv, idx, n_lag);
        const double fr = A.sr / period;
        double bi = rint(120.0 * log2(fr / A.fmin));
        bi = fmin(fmax(bi, 0.0), (double)A.n_bins);
        bin = (int)bi;
        ok = (p > 0.0) && (bin < A.n_bins);
      }
      const uint64_t m = __ballot(ok);
      wave_lds_sync();
      if (ok) { const int o = nc + lanes_below(m, lane); tl[o] = bin; pk[o] = p; }
      nc += __popcll(m);
      wave_lds_sync();
    }
    // a bin shared by consecutive candidates goes to the larger lag (librosa assigns: the last write wins)
    int nk = 0;
    double vps = 0.0;
    int* ob = A.cand_bin + f * A.K;
    float* op = A.cand_prob + f * A.K;
    for (int base = 0; base < nc; base += 64) {
      const int e = base + lane;
      const bool keep = (e < nc) && (e == nc - 1 || tl[e + 1] != tl[e]);
      const uint64_t m = __ballot(keep);
      if (keep) {
        const int o = nk + lanes_below(m, lane);
        if (o < A.K) { ob[o] = tl[e]; op[o] = (float)pk[e]; }
        vps += pk[e];
      }
      nk += __popcll(m);
    }
    vps = wave_sum_d(vps);
    if (lane == 0) {
      A.cand_count[f] = nk < A.K ? nk : A.K;
      A.voiced_prob[f] = (float)fmin(fmax(vps, 0.0), 1.0);
    }
    wave_lds_sync();
  }
}

// ------------------------------------------------------------------------------------------------ Viterbi
struct VitArgs {
  const int* cand_bin; const float* cand_prob; const int* cand_count; const float* voiced_prob;
  int64_t T; int K, n, h, R;
  const double* lstay; const double* lswitch;   // [R, 2h + 1]: log(p T[i, i + o] + tiny), o = -h .. h
  double lt0, linit_v, linit_u, fmin;
  uint16_t* ptr; float* f0; uint8_t* voiced; int* state;
};

__device__ __forceinline__ int table_row(int i, int n, int h) {
  if (n <= 2 * h + 1) return i;
  if (i < h) return i;
  if (i > n - 1 - h) return i - (n - 1) + 2 * h;
  return h;
}

// (value, index) max with the lowest index on ties, over the workgroup; red: 2 * nwaves doubles of LDS
__device__ void block_argmax(double v, int i, double* red_v, int* red_i, double& ov, int& oi) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  wave_pick<true>(v, i);
  __syncthreads();
  if (lane == 0) { red_v[wv] = v; red_i[wv] = i; }
  __syncthreads();
  v = red_v[0]; i = red_i[0];
  for (int q = 1; q < nw; ++q)
    if (red_v[q] > v || (red_v[q] == v && red_i[q] < i)) { v = red_v[q]; i = red_i[q]; }
  ov = v; oi = i;
}

__global__ __launch_bounds__(1024) void pyin_viterbi_kernel(VitArgs A) {
  extern __shared__ __attribute__((aligned(16))) double vl[];
  const int n = A.n, S2 = 2 * n, tid = threadIdx.x, nth = blockDim.x;
  double* va = vl;
  double* vb = vl + S2;
  double* lobs = vl + 2 * S2;
  double* red_v = lobs + n;
  int* red_i = reinterpret_cast<int*>(red_v + 16);
  const int64_t b = blockIdx.x;
  const int W2 = 2 * A.h + 1;

  auto emission = [&](int64_t t, double& lu) {
    const int64_t f = b * A.T + t;
    for (int j = tid; j < n; j += nth) lobs[j] = A.lt0;
    __syncthreads();
    int cnt = A.cand_count[f];
    cnt = cnt < 0 ? 0 : (cnt > A.K ? A.K : cnt);
    for (int e = tid; e < cnt; e += nth) {
      const int bin = A.cand_bin[f * A.K + e];
      if (bin >= 0 && bin < n) lobs[bin] = log((double)A.cand_prob[f * A.K + e] + DBL_MIN);
    }
    lu = log((1.0 - (double)A.voiced_prob[f]) / (double)n + DBL_MIN);
    __syncthreads();
  };

  double lu;
  emission(0, lu);
  for (int j = tid; j < S2; j += nth) va[j] = (j < n) ? lobs[j] + A.linit_v : lu + A.linit_u;
  __syncthreads();
  uint16_t* pb = A.ptr + b * A.T * (int64_t)S2;
  for (int64_t t = 1; t < A.T; ++t) {
    emission(t, lu);
    // best out-of-band predecessor: first argmax of v(i) + log(tiny) over every state
    double gv = -INFINITY;
    int gi = 0x7fffffff;
    for (int i = tid; i < S2; i += nth) {
      const double s = va[i] + A.lt0;
      if (s > gv) { gv = s; gi = i; }
    }
    block_argmax(gv, gi, red_v, red_i, gv, gi);
    const int gb = gi / n, gj = gi - gb * n;
    for (int j = tid; j < S2; j += nth) {
      const int bj = j / n, jj = j - bj * n;
      const int lo = jj - A.h < 0 ? 0 : jj - A.h, hi = jj + A.h > n - 1 ? n - 1 : jj + A.h;
      double best = -INFINITY;
      int bi = 0x7fffffff;
      for (int pbk = 0; pbk < 2; ++pbk) {
        const double* tab = (pbk == bj) ? A.lstay : A.lswitch;
        const double* vp = va + pbk * n;
        for (int ii = lo; ii <= hi; ++ii) {
          const double s = vp[ii] + tab[table_row(ii, n, A.h) * W2 + (jj - ii + A.h)];
          if (s > best) { best = s; bi = pbk * n + ii; }
        }
      }
      const bool in_band = (gj >= lo && gj <= hi);
      if (!in_band && (gv > best || (gv == best && gi < bi))) { best = gv; bi = gi; }
      vb[j] = (j < n ? lobs[j] : lu) + best;
      pb[t * S2 + j] = (uint16_t)bi;
    }
    __syncthreads();
    double* tmp = va; va = vb; vb = tmp;
  }
  double fv = -INFINITY;
  int fi = 0x7fffffff;
  for (int i = tid; i < S2; i += nth)
    if (va[i] > fv) { fv = va[i]; fi = i; }
  block_argmax(fv, fi, red_v, red_i, fv, fi);
  __syncthreads();
  if (tid == 0) {
    __threadfence_block();
    int s = fi;
    for (int64_t t = A.T - 1; t >= 0; --t) {
      const int64_t f = b * A.T + t;
      const bool v = s < n;
      if (A.state) A.state[f] = s;
      A.voiced[f] = v ? 1 : 0;
      A.f0[f] = v ? (float)(A.fmin * exp2((double)s / 120.0)) : __builtin_nanf("");
      if (t > 0) s = pb[t * S2 + s];
    }
  }
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int syg_pitch_frames_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int frame_length, int win_length,
                                    int hop, int center, int64_t T, double sr, int min_period, int max_period, int mode,
                                    double trough_threshold, double fmin, int n_bins, const double* ptab, int K,
                                    const float* twiddle, float* f0_out, int* cand_bin, float* cand_prob, int* cand_count,
                                    float* voiced_prob, float* cmndf_out, void* stream) {
  if (frame_length != NF) {
    set_error("pitch_frames: frame_length %d is not offloaded (only 2048, the length of every reference call path)",
              frame_length);
    return SYG_E_UNSUPPORTED;
  }
  SYG_REQUIRE(y && twiddle, "pitch_frames: null pointer argument (y / twiddle)");
  SYG_REQUIRE(mode == 0 || mode == 1, "pitch_frames: mode must be 0 (yin) or 1 (pyin)");
  SYG_REQUIRE(mode == 1 || f0_out, "pitch_frames: null pointer argument (f0_out)");
  SYG_REQUIRE(mode == 0 || (ptab && cand_bin && cand_prob && cand_count && voiced_prob),
              "pitch_frames: null pointer argument (pyin tables / candidate outputs)");
  SYG_REQUIRE(B >= 1 && L >= 1 && ldy >= L, "pitch_frames: bad B / L / ldy");
  SYG_REQUIRE(hop >= 1 && (center == 0 || center == 1), "pitch_frames: bad hop / center");
  SYG_REQUIRE(win_length >= 1 && win_length < NF, "pitch_frames: win_length must be in [1, 2048)");
  SYG_REQUIRE(min_period >= 1 && min_period < max_period,
              "pitch_frames: need 1 <= min_period < max_period (got %d, %d): fmin / fmax / win_length leave no lag range",
              min_period, max_period);
  SYG_REQUIRE(max_period <= NF - win_length - 1, "pitch_frames: max_period %d > frame_length - win_length - 1", max_period);
  if (const int rc = check_framing("pitch_frames", T, frames_expected(L, NF, hop, center))) return rc;
  const int n_lag = max_period - min_period + 1;
  SYG_REQUIRE(mode == 0 || (K >= (n_lag + 1) / 2 + 1 && K <= 4096), "pitch_frames: K must be >= ceil(n_lag / 2) + 1 = %d",
              (n_lag + 1) / 2 + 1);
  SYG_REQUIRE(mode == 0 || (n_bins >= 1 && n_bins < 32768 && fmin > 0.0), "pitch_frames: bad n_bins / fmin");
  SYG_REQUIRE(sr > 0.0, "pitch_frames: bad sr");
  FrameArgs A{y, L, ldy, win_length, hop, center, T, B * T, sr, min_period, max_period, n_lag, mode, trough_threshold,
              fmin, n_bins, ptab, K, f0_out, cand_bin, cand_prob, cand_count, voiced_prob, cmndf_out};
  hipLaunchKernelGGL(pitch_frames_kernel, dim3(capped_grid(ceil_div(A.nframes, PW), PITCH_FRAMES_WGS_PER_CU)), dim3(PW * 64), 0,
                     (hipStream_t)stream, A, (const float2*)twiddle);
  SYG_CHECK_LAUNCH("pitch_frames");
  return SYG_OK;
}

extern "C" int64_t syg_pyin_work_bytes(int64_t B, int64_t T, int n_bins) {
  if (B < 1 || T < 1 || n_bins < 1 || n_bins >= 32768) return -1;
  return B * T * 2 * (int64_t)n_bins * (int64_t)sizeof(uint16_t);
}

extern "C" int syg_pyin_viterbi_f32(const int* cand_bin, const float* cand_prob, const int* cand_count,
                                    const float* voiced_prob, int64_t B, int64_t T, int K, int n_bins, int half_width,
                                    const double* ltab, int n_rows, const double* lconst_host, double fmin, void* work,
                                    int64_t work_bytes, float* f0_out, uint8_t* voiced_out, int* state_out, void* stream) {
  SYG_REQUIRE(cand_bin && cand_prob && cand_count && voiced_prob && ltab && lconst_host && f0_out && voiced_out,
              "pyin_viterbi: null pointer argument");
  SYG_REQUIRE(B >= 1 && B <= 0x7fffffff && T >= 1 && K >= 1, "pyin_viterbi: bad B / T / K");
  SYG_REQUIRE(n_bins >= 1 && n_bins < 32768 && half_width >= 0 && fmin > 0.0, "pyin_viterbi: bad n_bins / half_width / fmin");
  const int R = (n_bins <= 2 * half_width + 1) ? n_bins : 2 * half_width + 1;
  SYG_REQUIRE(n_rows == R, "pyin_viterbi: the transition tables must have %d rows (got %d)", R, n_rows);
  const int64_t need = syg_pyin_work_bytes(B, T, n_bins);
  SYG_REQUIRE(work && work_bytes >= need, "pyin_viterbi: workspace of %lld bytes needed (syg_pyin_work_bytes), got %lld",
              (long long)need, (long long)work_bytes);
  const size_t lds = (size_t)(5 * n_bins) * sizeof(double) + 16 * sizeof(double) + 16 * sizeof(int);
  SYG_REQUIRE(lds <= 160 * 1024, "pyin_viterbi: n_bins %d needs %zu bytes of LDS", n_bins, lds);
  if (const int rc = reserve_dynamic_lds("pyin_viterbi", (const void*)pyin_viterbi_kernel, lds)) return rc;
  VitArgs A{cand_bin, cand_prob, cand_count, voiced_prob, T, K, n_bins, half_width, R,
            ltab, ltab + (int64_t)R * (2 * half_width + 1), lconst_host[0], lconst_host[1], lconst_host[2], fmin,
            (uint16_t*)work, f0_out, voiced_out, state_out};
  // a small batch leaves most CUs idle: give each clip more threads
  const int threads = B >= 256 ? 256 : 1024;
  hipLaunchKernelGGL(pyin_viterbi_kernel, dim3((unsigned)B), dim3(threads), lds, (hipStream_t)stream, A);
  SYG_CHECK_LAUNCH("pyin_viterbi");
  return SYG_OK;
}
