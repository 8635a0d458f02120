// Harmonic / percussive source separation: librosa 0.10 `effects.hpss` as called by harmonic_to_noise_ratio,
// sygnals/core/audio/features.py:225-316, after the STFT (syg_stft2048_c2c_f32).  The float64 restatement that is the
// contract lives in tests/hpss_ref.py.
//
// Masks (hpss_masks_kernel): a workgroup owns a tile of TT frames x FB bins of one clip.  |D| is read into two LDS
// regions: the tile's bins over TT + win_harm - 1 frames (the time halo of H) and the tile's frames over
// FB + win_perc - 1 bins (the bin halo of P), every index folded by scipy's "reflect" rule (half-sample symmetric,
// repeated), so a clip shorter than the window folds more than once.  Each median is a selection network on the
// float bits as uint32 (magnitudes are >= +0, so the integer order is the float order): Batcher's odd-even merge
// sort, comparators touching the missing top inputs dropped, and at a compile-time window only the comparators that
// reach rank k / 2 kept (dead code).  win = 31 on both axes has its own instantiation; any other pair of windows runs
// the 8 / 16 / 32 / 64-input network with +inf padding and a runtime rank.  The soft masks follow util.softmask.
//
// Inverse STFT (istft2048_kernel): one wave per segment of SEG output hops of a clip and component.  It runs the frames that touch
// the segment in order -- three before it, then its own -- through the real-split inverse on the one-wave 1024-point
// FFT (wave_fft.h; forward transform of the conjugate), windows them and overlap-adds into a four-hop LDS ring.  A hop
// is complete once its last frame is in; every output sample therefore sums its frames in frame order from zero,
// whatever the segmentation: the result is bit-identical from run to run (no atomics).  The window sum-square is
// summed in float64 in frame order, as librosa's window_sumsquare does, and rounded once.
//
// HNR rows (hnr_rows_kernel): one wave per RMS frame, frame powers of both components accumulated in float64, the
// reference's thresholds on float64 values.
#include <float.h>
#include <math.h>
#include "wave_fft.h"
#include "host.h"

namespace syg {
namespace {

constexpr int NF = 2048, NB = 1025;

// ------------------------------------------------------------------ selection networks
constexpr int next_pow2(int k) { int n = 1; while (n < k) n <<= 1; return n; }
constexpr int MAX_CMP = 600;    // Batcher's odd-even merge sort of 64 inputs has 543 comparators

template <int K>
struct OemNet {
  int a[MAX_CMP], b[MAX_CMP], n;
  constexpr OemNet() : a(), b(), n(0) {
    const int N = next_pow2(K);
    for (int p = 1; p < N; p <<= 1)
      for (int k = p; k >= 1; k >>= 1)
        for (int j = k % p; j + k < N; j += 2 * k)
          for (int i = 0; i < k && i + j + k < N; ++i)
            if ((i + j) / (2 * p) == (i + j + k) / (2 * p) && i + j + k < K) {   // top inputs (+inf) never move
              a[n] = i + j;
              b[n] = i + j + k;
              ++n;
            }
  }
};

template <int K>
__device__ __forceinline__ void oem_sort(uint32_t (&v)[K]) {
  constexpr OemNet<K> net{};
#pragma unroll
  for (int c = 0; c < net.n; ++c) {
    const uint32_t x = v[net.a[c]], y = v[net.b[c]];
    v[net.a[c]] = min(x, y);
    v[net.b[c]] = max(x, y);
  }
}

// median of a compile-time window: src[j * stride], j = 0 .. K - 1, element of rank K / 2
template <int K>
__device__ __forceinline__ uint32_t median_ct(const uint32_t* src, int stride) {
  uint32_t v[K];
#pragma unroll
  for (int j = 0; j < K; ++j) v[j] = src[j * stride];
  oem_sort<K>(v);
  return v[K / 2];
}

// runtime window 1 <= k <= N: +inf padding (0x7f800000 is above every finite magnitude) and a runtime rank
template <int N>
__device__ __forceinline__ uint32_t median_rt(const uint32_t* src, int stride, int k) {
  uint32_t v[N];
#pragma unroll
  for (int j = 0; j < N; ++j) v[j] = (j < k) ? src[min(j, k - 1) * stride] : 0x7f800000u;
  oem_sort<N>(v);
  const int r = k >> 1;
  uint32_t m = v[0];
#pragma unroll
  for (int j = 1; j < N; ++j) m = (j == r) ? v[j] : m;
  return m;
}

__device__ __forceinline__ uint32_t median_any(const uint32_t* src, int stride, int k) {
  if (k <= 8) return median_rt<8>(src, stride, k);
  if (k <= 16) return median_rt<16>(src, stride, k);
  if (k <= 32) return median_rt<32>(src, stride, k);
  return median_rt<64>(src, stride, k);
}

// scipy.ndimage "reflect": ... x1 x0 | x0 x1 ... x(n-1) | x(n-1) x(n-2) ..., period 2n
__device__ __forceinline__ int64_t reflect_idx(int64_t i, int64_t n) {
  const int64_t p = 2 * n;
  int64_t m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// |D| with the IEEE semantics of __fsqrt_rn(__fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im))), as the header states it,
// so that a host test can rebuild it bit for bit.  The products and the sum are written out under contract(off) (the
// intrinsics' bodies may be contracted into an FMA once inlined), and the square root is taken in float64 and rounded
// once, which is the correctly rounded float32 root (53 >= 2 * 24 + 2); the float32 root here compiles to the bare
// v_sqrt_f32, which is not.
__device__ __forceinline__ uint32_t mag_bits(float2 d) {
#pragma clang fp contract(off)
  const float a = d.x * d.x;
  const float b = d.y * d.y;
  return __float_as_uint((float)sqrt((double)(a + b)));
}

// util.softmask(X, X_ref, power, split_zeros) for one cell (power < 0 encodes +inf: the hard mask X > X_ref)
__device__ __forceinline__ float softmask1(float X, float Xr, float power, bool split) {
  if (power < 0.f) return X > Xr ? 1.f : 0.f;
  float Z = fmaxf(X, Xr);
  if (Z < FLT_MIN) return split ? 0.5f : 0.f;
  const float a = X / Z, r = Xr / Z;
  float m, q;
  if (power == 1.f) { m = a; q = r; }
  else if (power == 2.f) { m = a * a; q = r * r; }
  else { m = powf(a, power); q = powf(r, power); }
  return m / (m + q);
}

constexpr int TT = 16, FB = 64, MT = 256;        // tile: frames x bins, threads (4 frames per thread)
constexpr int KMAX = 63, HALO = KMAX - 1;

struct MaskArgs {
  const float2* D; int64_t B, T, ntt; int kh, kp; float power, mh, mp; int split;
  float* Mh; float* Mp; float* H; float* P;
};

template <int KH, int KP>
__global__ __launch_bounds__(MT) void hpss_masks_kernel(MaskArgs A) {
  __shared__ uint32_t sa[(TT + HALO) * FB];       // time halo: row r <-> frame t0 - kh / 2 + r, column <-> bin f0 + c
  __shared__ uint32_t sb[TT * (FB + HALO + 1)];   // bin halo: row <-> frame t0 + r, column c <-> bin f0 - kp / 2 + c
  constexpr int SBW = FB + HALO + 1;
  const int kh = KH ? KH : A.kh, kp = KP ? KP : A.kp;
  const int tid = threadIdx.x, tx = tid & (FB - 1), ty = tid >> 6;
  constexpr int nft = (NB + FB - 1) / FB;
  const int64_t blk = blockIdx.x;
  const int ft = (int)(blk % nft);
  const int64_t rest = blk / nft;
  const int64_t tt = rest % A.ntt, b = rest / A.ntt;
  const int64_t t0 = tt * TT;
  const int f0 = ft * FB;
  const float2* Db = A.D + b * A.T * NB;
  // ---- time-halo region (columns past bin 1024 are filled with a valid bin and never written out)
  const int fa = min(f0 + tx, NB - 1);
  for (int r = ty; r < TT + kh - 1; r += MT / FB) {
    const int64_t t = reflect_idx(t0 - kh / 2 + r, A.T);
    sa[r * FB + tx] = mag_bits(Db[t * NB + fa]);
  }
  // ---- bin-halo region (rows past the last frame are filled with frame T - 1 and never written out)
  for (int i = tid; i < TT * (FB + kp - 1); i += MT) {
    const int r = i / (FB + kp - 1), c = i - r * (FB + kp - 1);
    const int64_t t = min(t0 + r, A.T - 1);
    const int64_t f = reflect_idx((int64_t)f0 - kp / 2 + c, NB);
    sb[r * SBW + c] = mag_bits(Db[t * NB + f]);
  }
  __syncthreads();
  const int f = f0 + tx;
  if (f >= NB) return;
#pragma unroll
  for (int q = 0; q < TT / (MT / FB); ++q) {
    const int r = ty + q * (MT / FB);
    const int64_t t = t0 + r;
    if (t >= A.T) break;
    uint32_t hb, pb;
    if constexpr (KH > 0) hb = median_ct<KH>(sa + r * FB + tx, FB);
    else hb = median_any(sa + r * FB + tx, FB, kh);
    if constexpr (KP > 0) pb = median_ct<KP>(sb + r * SBW + tx, 1);
    else pb = median_any(sb + r * SBW + tx, 1, kp);
    const float h = __uint_as_float(hb), p = __uint_as_float(pb);
    const int64_t o = (b * A.T + t) * NB + f;
    A.Mh[o] = softmask1(h, p * A.mh, A.power, A.split);
    A.Mp[o] = softmask1(p, h * A.mp, A.power, A.split);
    if (A.H) A.H[o] = h;
    if (A.P) A.P[o] = p;
  }
}

// ------------------------------------------------------------------ inverse STFT
constexpr int IPW = 4;              // waves per workgroup: two segments x two components
constexpr int SEG = 16;             // output hops per wave
constexpr int HOP = 512;

// 62.6 KiB: two workgroups (eight waves) per CU
struct IstftLds {
  float2 sc[IPW][wfft::SC_COMPLEX];
  float ring[IPW][NF];               // four hops of one component per wave
  float2 tw2l[wfft::TW2_COMPLEX];
  float2 tw1l[wfft::TW1_COMPLEX];
  float win[NF / 2 + 1];             // synthesis window w[0 .. 1024] as float32 (periodic: w[s] = w[2048 - s])
  float wss[HOP];                    // interior window sum-square (four frames), float64 sum rounded once
};

struct IstftArgs {
  const float2* D; int64_t T, nframes, L, ldy, nseg, nwaves; const double* win;
  const float* mask[2]; float* y[2]; int ncomp;
};

__global__ __launch_bounds__(IPW * 64, 2) void istft2048_kernel(IstftArgs A, const float2* __restrict__ tw) {
  __shared__ __attribute__((aligned(16))) IstftLds S;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  wfft::Lane lc;
  wfft::init_lane(lc, lane);
  wfft::init_tables(S.tw2l, S.tw1l, tw, NF, tid, IPW * 64);
  for (int i = tid; i <= NF / 2; i += IPW * 64) S.win[i] = (float)A.win[i];
  // a position p = 512 u + i covered by four frames gets them in frame order: window indices i + 1536 ... i
  for (int i = tid; i < HOP; i += IPW * 64) {
    double ss = 0.0;
    for (int q = 3; q >= 0; --q) { const double wv = A.win[i + q * HOP]; ss += wv * wv; }
    S.wss[i] = (float)ss;
  }
  __syncthreads();
  float2* sc = S.sc[w];
  float* ring = S.ring[w];
  constexpr float INV = 1.f / 1024.f;

  // wave index -> (clip, segment, component); the components of a segment sit in neighbouring waves and share the
  // reads of D through L1 / L2
  for (int64_t wi = (int64_t)blockIdx.x * IPW + w; wi < A.nwaves; wi += (int64_t)gridDim.x * IPW) {
    const int c = (int)(wi % A.ncomp);
    const int64_t rest = wi / A.ncomp;
    const int64_t b = rest / A.nseg, sg = rest - b * A.nseg;
    const float* mask = A.mask[c];
    float* yout = A.y[c] + b * A.ldy;
    // output hops in buffer coordinates (sample n of y is buffer position n + 1024): hop 2 holds n = 0
    const int64_t hlast = (A.L - 1 + NF / 2) / HOP;
    const int64_t hs = 2 + sg * SEG, he = min(hs + SEG, hlast + 1);
    const int64_t tstart = hs - 3 > 0 ? hs - 3 : 0;
    for (int i = lane; i < NF; i += 64) ring[i] = 0.f;
    wave_lds_sync();
    const float2* Db = A.D + b * A.T * NB;
    for (int64_t t = tstart; t < he; ++t) {
      if (t < A.nframes) {
        const float2* Dt = Db + t * NB;
        const float* Mt = mask ? mask + (b * A.T + t) * NB : nullptr;
        float2 v[16];
#pragma unroll
        for (int a = 0; a < 16; ++a) {
          const int k = 64 * a + lane, km = NF / 2 - k;          // km = 1024 - k in 1 .. 1024
          float2 xk = Dt[k], xm = Dt[km];
          if (Mt) {
            const float mk = Mt[k], mm = Mt[km];
            xk = make_float2(xk.x * mk, xk.y * mk);
            xm = make_float2(xm.x * mm, xm.y * mm);
          }
          if (k == 0) { xk.y = 0.f; xm.y = 0.f; }                 // irfft ignores Im X[0], Im X[1024]
          // Zc[k] = Ec + i Oc, Ec = (X[k] + conj X[1024-k]) / 2, Oc = (X[k] - conj X[1024-k]) conj(W_2048^k) / 2
          const float2 Ec = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y));
          const float2 Dd = make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y));
          const float2 Oc = cmulc(Dd, tw[k]);
          v[a] = make_float2(Ec.x - Oc.y, -(Ec.y + Oc.x));          // conj(Zc[k]): inverse by the forward transform
        }
        float2 zk[2][4], zm[2][4], z512;
        wfft::cfft1024(v, lc, sc, S.tw1l, S.tw2l, lane, zk, zm, z512);
        // z[m] = conj(F[m]) / 1024 = x[2m] + i x[2m+1]
        const int base = (int)((t & 3) * HOP);
        auto wv = [&](int s) { return S.win[s <= NF / 2 ? s : NF - s]; };
        auto put = [&](int m, float2 F) {
          const int s = 2 * m;
          const int i0 = (base + s) & (NF - 1), i1 = (base + s + 1) & (NF - 1);
          ring[i0] += wv(s) * (F.x * INV);
          ring[i1] += wv(s + 1) * (-F.y * INV);
        };
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const int m = wfft::bin_of(lane, j, d);
            put(m, zk[j][d]);
            if (m != 0) put(NF / 2 - m, zm[j][d]);
          }
        if (lane == 0) put(512, z512);
        wave_lds_sync();
      }
      // hop t is complete: emit it if it is this segment's (a warm-up hop is only cleared), then clear its ring
      // slot, which frame t + 1 reuses for hop t + 4
      for (int i = lane; i < HOP; i += 64) {
        const int ri = (int)((t & 3) * HOP) + i;
        if (t >= hs) {
          // positions p = 512 t + i, sample n = p - 1024
          const int64_t p = t * HOP + i, n = p - NF / 2;
          const int64_t tlo = p >= NF ? (p - NF) / HOP + 1 : 0;
          const int64_t thi = min(p / HOP, A.nframes - 1);
          float wss;
          if (thi - tlo == 3) {
            wss = S.wss[i];
          } else {                           // the ends of the clip, covered by fewer frames
            double ss = 0.0;
            for (int64_t u = tlo; u <= thi; ++u) { const double x = A.win[p - u * HOP]; ss += x * x; }
            wss = (float)ss;
          }
          float v = ring[ri];
          if (wss > FLT_MIN) v = v / wss;
          if (n >= 0 && n < A.L) yout[n] = v;
        }
        ring[ri] = 0.f;
      }
      wave_lds_sync();
    }
  }
}

// ------------------------------------------------------------------ HNR rows
constexpr int HPW = 4;

struct HnrArgs {
  const float* yh; const float* yp; int64_t L, ldy; int fl, hop, center; int64_t T, nframes;
  float* hnr; float* rh; float* rp;
};

__global__ __launch_bounds__(HPW * 64) void hnr_rows_kernel(HnrArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * HPW + (threadIdx.x >> 6);
  if (f >= A.nframes) return;
  const int64_t b = f / A.T, t = f - b * A.T;
  const int64_t s0 = t * A.hop - (A.center ? A.fl / 2 : 0);
  const float* yh = A.yh + b * A.ldy;
  const float* yp = A.yp + b * A.ldy;
  double sh = 0.0, sp = 0.0;
  for (int i = lane; i < A.fl; i += 64) {
    const int64_t s = s0 + i;
    if (s >= 0 && s < A.L) {
      const double a = yh[s], c = yp[s];
      sh += a * a;
      sp += c * c;
    }
  }
  sh = wave_sum_d(sh);
  sp = wave_sum_d(sp);
  if (lane != 0) return;
  // librosa.feature.rms: sqrt(mean(x^2)); the reference squares the rms again
  const double rh = sqrt(sh / A.fl), rp = sqrt(sp / A.fl);
  const double ph = rh * rh, pp = rp * rp;
  constexpr double EPS = 1e-10;
  double v;
  if (ph > EPS && pp > EPS) v = 10.0 * log10(ph / pp);
  else if (ph > EPS) v = 80.0;
  else if (pp > EPS) v = -80.0;
  else v = NAN;
  A.hnr[f] = (float)v;
  if (A.rh) A.rh[f] = (float)rh;
  if (A.rp) A.rp[f] = (float)rp;
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int syg_hpss_masks_f32(const float* D, int64_t B, int64_t T, int win_harm, int win_perc, double power,
                                  double margin_harm, double margin_perc, float* mask_harm, float* mask_perc,
                                  float* harm_out, float* perc_out, void* stream) {
  SYG_REQUIRE(D && mask_harm && mask_perc, "hpss_masks: null pointer argument (D / mask_harm / mask_perc)");
  SYG_REQUIRE(B >= 1 && T >= 1 && B * T < ((int64_t)1 << 40) / NB, "hpss_masks: bad B / T");
  SYG_REQUIRE(win_harm >= 1 && win_harm <= KMAX && win_perc >= 1 && win_perc <= KMAX,
              "hpss_masks: median windows must be in [1, %d] (got %d, %d)", KMAX, win_harm, win_perc);
  SYG_REQUIRE(power > 0.0 && !isnan(power), "hpss_masks: power must be strictly positive");
  SYG_REQUIRE(margin_harm >= 1.0 && margin_perc >= 1.0 && isfinite(margin_harm) && isfinite(margin_perc),
              "hpss_masks: margins must be >= 1.0 and finite");
  const int64_t ntt = (T + TT - 1) / TT;
  const int64_t blocks = B * ntt * ((NB + FB - 1) / FB);
  SYG_REQUIRE(blocks < 0x7fffffff, "hpss_masks: too many tiles");
  const float pw = isinf(power) ? -1.f : (float)power;
  MaskArgs A{(const float2*)D, B, T, ntt, win_harm, win_perc, pw, (float)margin_harm, (float)margin_perc,
             margin_harm == 1.0 && margin_perc == 1.0, mask_harm, mask_perc, harm_out, perc_out};
  if (win_harm == 31 && win_perc == 31)
    hipLaunchKernelGGL((hpss_masks_kernel<31, 31>), dim3((unsigned)blocks), dim3(MT), 0, (hipStream_t)stream, A);
  else
    hipLaunchKernelGGL((hpss_masks_kernel<0, 0>), dim3((unsigned)blocks), dim3(MT), 0, (hipStream_t)stream, A);
  SYG_CHECK_LAUNCH("hpss_masks");
  return SYG_OK;
}

extern "C" int syg_istft2048_f32(const float* D, int64_t B, int64_t T, int hop, int center, int64_t length,
                                 const double* window, const float* twiddle, const float* mask_a, float* y_a,
                                 const float* mask_b, float* y_b, int64_t ldy, void* stream) {
  if (hop != HOP || center != 1) {
    set_error("istft2048: only hop 512 with center = 1 is offloaded (got hop %d, center %d)", hop, center);
    return SYG_E_UNSUPPORTED;
  }
  SYG_REQUIRE(D && window && twiddle && y_a, "istft2048: null pointer argument (D / window / twiddle / y_a)");
  SYG_REQUIRE(!mask_b == !y_b, "istft2048: mask_b and y_b go together");
  SYG_REQUIRE(!mask_b || mask_a, "istft2048: a second component needs mask_a");
  SYG_REQUIRE(B >= 1 && T >= 1 && length >= 1 && ldy >= length && B * T < ((int64_t)1 << 40) / NB,
              "istft2048: bad B / T / length / ldy");
  const int64_t padded = length + NF;
  const int64_t need = (padded + HOP - 1) / HOP;
  const int64_t nframes = T < need ? T : need;
  const int64_t hlast = (length - 1 + NF / 2) / HOP;
  const int64_t nseg = (hlast - 1 + SEG - 1) / SEG;
  const int ncomp = y_b ? 2 : 1;
  IstftArgs A{(const float2*)D, T, nframes, length, ldy, nseg, B * nseg * ncomp, window, {mask_a, mask_b}, {y_a, y_b},
              ncomp};
  hipLaunchKernelGGL(istft2048_kernel, dim3(capped_grid(ceil_div(A.nwaves, IPW), ISTFT_WGS_PER_CU)), dim3(IPW * 64), 0,
                     (hipStream_t)stream, A, (const float2*)twiddle);
  SYG_CHECK_LAUNCH("istft2048");
  return SYG_OK;
}

extern "C" int syg_hnr_rows_f32(const float* y_harm, const float* y_perc, int64_t B, int64_t L, int64_t ldy,
                                int frame_length, int hop, int center, int64_t T, float* hnr_out, float* rms_harm_out,
                                float* rms_perc_out, void* stream) {
  SYG_REQUIRE(y_harm && y_perc && hnr_out, "hnr_rows: null pointer argument (y_harm / y_perc / hnr_out)");
  SYG_REQUIRE(B >= 1 && L >= 1 && ldy >= L, "hnr_rows: bad B / L / ldy");
  SYG_REQUIRE(frame_length >= 1 && hop >= 1 && (center == 0 || center == 1), "hnr_rows: bad frame_length / hop / center");
  // (librosa.feature.rms's count on the padded signal, not frames_expected)
  if (const int rc = check_framing("hnr_rows", T, frames_padded(L, frame_length, hop, center))) return rc;
  HnrArgs A{y_harm, y_perc, L, ldy, frame_length, hop, center, T, B * T, hnr_out, rms_harm_out, rms_perc_out};
  const int64_t blocks = (A.nframes + HPW - 1) / HPW;
  SYG_REQUIRE(blocks < 0x7fffffff, "hnr_rows: too many frames");
  hipLaunchKernelGGL(hnr_rows_kernel, dim3((unsigned)blocks), dim3(HPW * 64), 0, (hipStream_t)stream, A);
  SYG_CHECK_LAUNCH("hnr_rows");
  return SYG_OK;
}
