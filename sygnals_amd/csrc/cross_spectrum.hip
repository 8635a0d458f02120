// Cross-spectral analysis of two real signals: segment-averaged cross-spectral density, the two auto-spectra and the
// magnitude-squared coherence (scipy.signal.csd / welch / coherence rules), and the device steps of generalised
// cross-correlation (GCC: spectral weighting, lag-window crop, peak picker).
//
// Fused form (syg_csd_f32): grid (nblk, B); a workgroup loops over a RUN of consecutive segments of one row pair.  Per
// segment it loads both signals' samples, removes each one's own mean / least-squares line, windows, and writes
// z[n] = x[n] + i y[n] into LDS; ONE complex transform of nfft points (block_fft) gives both spectra,
//     X[k] = (Z[k] + conj Z[N-k]) / 2,        Y[k] = (Z[k] - conj Z[N-k]) / (2i),
// and a thread accumulates Re, Im of conj(X) Y and |X|^2, |Y|^2 of its bins in float32 registers (the factors 1/2 are
// left out: the sums carry a factor 4 that the combine takes back).  The partial sums go to a workspace and are
// combined in float64 in a fixed order by two small kernels; the coherence is formed there, in float64, from the raw
// sums.  No atomics.  The split of a row's segments over workgroups depends on the segment count alone (csd_split),
// NOT on the batch: a batch equals its rows bit for bit.
//
// Rows form (syg_csd_rows_f32): the caller packs the segments as rows and transforms them with the arbitrary-length
// FFT; one kernel turns the two full spectra of a block of segments into the four products and adds them in float64
// in segment order (the roles of syg_psd_onesided_f32 and syg_col_mean_f32 of the Welch rows form).
#include "host.h"

namespace syg {
namespace {

constexpr int CSD_MAX_N = 8192;
constexpr int CSD_RUN = 16;          // segments of one workgroup, at least (the run grows once 2048 workgroups are reached)
constexpr int CSD_MAX_BLK = 2048;
constexpr int CSD_SLICE_MIN = 64;    // partial rows from which the combine's first stage is cut into slices
constexpr int CSD_SLICES = 16;
constexpr int CF_G = 16;

// run length and workgroups of a row of nseg segments
__host__ void csd_split(int64_t nseg, int& run, int& nblk) {
  int64_t r = ceil_div(nseg, CSD_MAX_BLK);
  if (r < CSD_RUN) r = CSD_RUN;
  run = (int)r;
  nblk = (int)ceil_div(nseg, r);
}
__host__ int csd_slices(int nblk) { return nblk >= CSD_SLICE_MIN ? CSD_SLICES : 1; }

struct CsdArgs {
  const float* x; const float* y; int64_t ldx, ldy;       // ldy = 0: one reference row for every x row
  int nperseg, step, nfft; int64_t nseg; int run;
  const float* win; const float2* tw; int detrend; float* partial;
};

// NT threads serve nfft <= MAXN: MAXN / NT points of either signal and (MAXN / 2) / NT + 1 bins per thread
template <int NT, int MAXN>
__global__ __launch_bounds__(NT) void csd_partial_kernel(CsdArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float red[4 * (NT / 64)];
  __shared__ float red2[2 * (NT / 64)];
  __shared__ int live[NT / 64];
  constexpr int PER = MAXN / NT, NW = NT / 64;
  constexpr int BINS = (MAXN / 2) / NT + 1;
  const int N = A.nfft, H = N >> 1, nperseg = A.nperseg;
  float2* za = reinterpret_cast<float2*>(lds);
  float2* zb = za + N;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t b = blockIdx.y;
  const float* xr = A.x + b * A.ldx;
  const float* yr = A.y + b * A.ldy;
  float are[BINS], aim[BINS], axx[BINS], ayy[BINS];
#pragma unroll
  for (int j = 0; j < BINS; ++j) { are[j] = 0.f; aim[j] = 0.f; axx[j] = 0.f; ayy[j] = 0.f; }
  const float jc = 0.5f * (float)(nperseg - 1);
  const int64_t s0 = (int64_t)blockIdx.x * A.run;
  const int64_t s1 = s0 + A.run < A.nseg ? s0 + A.run : A.nseg;
  for (int64_t sg = s0; sg < s1; ++sg) {
    const float* sx = xr + sg * (int64_t)A.step;
    const float* sy = yr + sg * (int64_t)A.step;
    float rx[PER], ry[PER];
    float sumx = 0.f, sumy = 0.f, mx = 0.f, my = 0.f;          // sums and first moments about the segment centre
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int n = tid + j * NT;
      const bool in = n < nperseg;
      rx[j] = in ? sx[n] : 0.f;
      ry[j] = in ? sy[n] : 0.f;
      sumx += rx[j]; sumy += ry[j];
      if (A.detrend == 2) { const float c = (float)n - jc; mx += c * rx[j]; my += c * ry[j]; }
    }
    // detrend as welch_partial_kernel: mean, or the least-squares line around the segment centre, each signal its own
    float meanx = 0.f, meany = 0.f, slx = 0.f, sly = 0.f;
    if (A.detrend) {
      sumx = wave_sum(sumx); sumy = wave_sum(sumy); mx = wave_sum(mx); my = wave_sum(my);
      if (lane == 0) { red[w] = sumx; red[NW + w] = sumy; red[2 * NW + w] = mx; red[3 * NW + w] = my; }
      __syncthreads();
      sumx = 0.f; sumy = 0.f; mx = 0.f; my = 0.f;
#pragma unroll
      for (int i = 0; i < NW; ++i) { sumx += red[i]; sumy += red[NW + i]; mx += red[2 * NW + i]; my += red[3 * NW + i]; }
      meanx = sumx / (float)nperseg; meany = sumy / (float)nperseg;
      if (A.detrend == 2 && nperseg > 1) {
        const double nn = (double)nperseg, den = nn * (nn * nn - 1.0) / 12.0;
        slx = (float)((double)mx / den); sly = (float)((double)my / den);
      }
      // The float32 sum of samples that sit on a DC offset loses digits that the window leaks into bins 0 and 1 (offset 3
      // on unit noise at nperseg 8192: the mean is off by 2e-7 and the coherence there by 9e-6).  The residuals sum to
      // almost nothing, so their mean is exact to float32 and corrects the first one.
      float rsx = 0.f, rsy = 0.f;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const int n = tid + j * NT;
        if (n < nperseg) {
          const float c = (float)n - jc;
          rsx += rx[j] - meanx - slx * c; rsy += ry[j] - meany - sly * c;
        }
      }
      rsx = wave_sum(rsx); rsy = wave_sum(rsy);
      if (lane == 0) { red2[w] = rsx; red2[NW + w] = rsy; }
      __syncthreads();
      rsx = 0.f; rsy = 0.f;
#pragma unroll
      for (int i = 0; i < NW; ++i) { rsx += red2[i]; rsy += red2[NW + i]; }
      meanx += rsx / (float)nperseg; meany += rsy / (float)nperseg;
    }
    // A signal whose prepared segment is all zero has a spectrum that is exactly zero, but X and Y come out of ONE
    // transform: its rounding would leave 1e-7 of the other signal in the zero one.  Such a segment adds nothing to the
    // sums the zero signal takes part in (bit 0: x is live, bit 1: y is live).
    bool nzx = false, nzy = false;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int n = tid + j * NT;
      if (n < N) {
        float2 z = make_float2(0.f, 0.f);
        if (n < nperseg) {
          const float c = (float)n - jc, wn = A.win[n];
          z.x = (rx[j] - meanx - slx * c) * wn;
          z.y = (ry[j] - meany - sly * c) * wn;
        }
        nzx |= z.x != 0.f; nzy |= z.y != 0.f;
        za[n] = z;
      }
    }
    {
      const int f = (__ballot(nzx) != 0 ? 1 : 0) | (__ballot(nzy) != 0 ? 2 : 0);
      if (lane == 0) live[w] = f;
    }
    __syncthreads();
    int fl = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) fl |= live[i];
    const float2* Z = block_fft(za, zb, N, A.tw, tid, NT);
#pragma unroll
    for (int j = 0; j < BINS; ++j) {
      const int k = tid + j * NT;
      if (k <= H) {
        const float2 zk = Z[k], zm = Z[(N - k) & (N - 1)];
        const float xr2 = zk.x + zm.x, xi2 = zk.y - zm.y;      // 2 X[k]
        const float yr2 = zk.y + zm.y, yi2 = zm.x - zk.x;      // 2 Y[k]
        if (fl == 3) {
          are[j] += fmaf(xr2, yr2, xi2 * yi2);                 // 4 Re conj(X) Y
          aim[j] += fmaf(xr2, yi2, -(xi2 * yr2));              // 4 Im conj(X) Y
        }
        if (fl & 1) axx[j] += fmaf(xr2, xr2, xi2 * xi2);
        if (fl & 2) ayy[j] += fmaf(yr2, yr2, yi2 * yi2);
      }
    }
    __syncthreads();                                           // Z, red, red2 and live are rewritten by the next segment
  }
  const int F = H + 1;
  float* po = A.partial + ((int64_t)b * gridDim.x + blockIdx.x) * 4 * (int64_t)F;
#pragma unroll
  for (int j = 0; j < BINS; ++j) {
    const int k = tid + j * NT;
    if (k <= H) { po[k] = are[j]; po[F + k] = aim[j]; po[2 * F + k] = axx[j]; po[3 * F + k] = ayy[j]; }
  }
}

// what a bin's four float64 sums become.  raw: the sums as accumulated; mul = scale / nseg (with the kernels' own factor);
// the one-sided factor 2 everywhere but DC and, for even nfft, Nyquist.  The coherence is scale-free: raw sums, float64.
struct CsdOut { float2* pxy; float* pxx; float* pyy; float* coh; };
__device__ __forceinline__ void csd_store(const CsdOut& O, int64_t b, int F, int k, int odd_nfft, double mul, double re,
                                          double im, double xx, double yy) {
  const double m = (k > 0 && (odd_nfft || k < F - 1)) ? 2.0 * mul : mul;
  const int64_t o = b * (int64_t)F + k;
  if (O.pxy) O.pxy[o] = make_float2((float)(re * m), (float)(im * m));
  if (O.pxx) O.pxx[o] = (float)(xx * m);
  if (O.pyy) O.pyy[o] = (float)(yy * m);
  if (O.coh) O.coh[o] = (float)((re * re + im * im) / (xx * yy));        // 0 / 0: NaN, as scipy.signal.coherence
}

// Combine, stage 1: grid (F / 64, B, slices); slice z adds its contiguous share of the nblk partial rows in float64:
// thread (k, g) the rows g, g + 16, ... of the slice, then the 16 sub-sums of a bin and plane in order through LDS.
__global__ __launch_bounds__(64 * CF_G) void csd_slice_kernel(const float* __restrict__ partial, int nblk, int F,
                                                               double* __restrict__ dsub) {
  __shared__ double sub[4][CF_G][64];
  const int64_t b = blockIdx.y;
  const int z = blockIdx.z, nz = gridDim.z;
  const int kx = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + kx;
  const int per = (nblk + nz - 1) / nz;
  const int j0 = z * per, j1 = (j0 + per < nblk) ? j0 + per : nblk;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (k < F)
    for (int j = j0 + g; j < j1; j += CF_G) {
      const float* p = partial + ((int64_t)b * nblk + j) * 4 * (int64_t)F + k;
#pragma unroll
      for (int q = 0; q < 4; ++q) s[q] += (double)p[(int64_t)q * F];
    }
#pragma unroll
  for (int q = 0; q < 4; ++q) sub[q][g][kx] = s[q];
  __syncthreads();
  if (g >= 4 || k >= F) return;
  double t = 0.0;                                       // thread (k, g < 4) adds plane g
#pragma unroll
  for (int i = 0; i < CF_G; ++i) t += sub[g][i][kx];
  dsub[(((int64_t)b * nz + z) * 4 + g) * F + k] = t;
}

// stage 2: the slices first to last, then the outputs
__global__ __launch_bounds__(256) void csd_final_kernel(const double* __restrict__ dsub, int nz, int F, int odd_nfft,
                                                        double mul, CsdOut O) {
  const int64_t b = blockIdx.y;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= F) return;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int z = 0; z < nz; ++z)
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] += dsub[(((int64_t)b * nz + z) * 4 + q) * F + k];
  csd_store(O, b, F, k, odd_nfft, mul, s[0], s[1], s[2], s[3]);
}

// Rows form: X, Y [rows, n] full complex spectra of `rows` consecutive segments of ONE row pair; acc [4, F] float64.
// A thread owns a bin and adds the segments in order.
__global__ __launch_bounds__(64) void csd_rows_kernel(const float2* __restrict__ X, const float2* __restrict__ Y,
                                                      int64_t rows, int64_t n, double* __restrict__ acc, int first,
                                                      int last, double mul, CsdOut O) {
  const int F = (int)(n / 2 + 1);
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= F) return;
  double re = 0.0, im = 0.0, xx = 0.0, yy = 0.0;
  if (!first) { re = acc[k]; im = acc[F + k]; xx = acc[2 * (int64_t)F + k]; yy = acc[3 * (int64_t)F + k]; }
  for (int64_t r = 0; r < rows; ++r) {
    const float2 a = X[r * n + k], c = Y[r * n + k];
    re += (double)fmaf(a.x, c.x, a.y * c.y);
    im += (double)fmaf(a.x, c.y, -(a.y * c.x));
    xx += (double)fmaf(a.x, a.x, a.y * a.y);
    yy += (double)fmaf(c.x, c.x, c.y * c.y);
  }
  acc[k] = re; acc[F + k] = im; acc[2 * (int64_t)F + k] = xx; acc[3 * (int64_t)F + k] = yy;
  if (last) csd_store(O, 0, F, k, (int)(n & 1), mul, re, im, xx, yy);
}

// ------------------------------------------------------------------------------------------------ GCC
// G[r, k] = W X[r, k] conj(Y[ry, k]) over the n TRUE bins of two plain complex transforms; W = 1, or (phat) 1 / |X conj Y|
// with W = 0 on a bin that is exactly 0.
__global__ void gcc_weight_kernel(const float2* __restrict__ X, const float2* __restrict__ Y, int64_t rows_y, int64_t n,
                                  int phat, float2* __restrict__ out) {
  const int64_t r = blockIdx.y;
  const float2* a = X + r * n;
  const float2* c = Y + (rows_y == 1 ? 0 : r) * n;
  float2* o = out + r * n;
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    float2 g = cmulc(a[k], c[k]);
    if (phat) {
      const float m = hypotf(g.x, g.y);
      g = m > 0.f ? make_float2(g.x / m, g.y / m) : make_float2(0.f, 0.f);
    }
    o[k] = g;
  }
}

// r[b, j] = Re c[b, (j - max_lag) mod n], j in [0, 2 max_lag]: the lag window of a circular correlation
__global__ void gcc_crop_kernel(const float2* __restrict__ c, int64_t n, int64_t max_lag, float* __restrict__ out) {
  const int64_t b = blockIdx.y, W = 2 * max_lag + 1;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < W; j += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = j - max_lag;
    if (t < 0) t += n;
    out[b * W + j] = c[b * n + t].x;
  }
}

// Peak picker, one wave per row of r [B, W] (row stride ldr): the first maximum; where it is interior and the parabola
// through its neighbours opens downwards, the vertex (the cepstral picker's rule, float64).  NaN samples never win.
__global__ __launch_bounds__(256) void peak_pick_kernel(const float* __restrict__ r, int64_t B, int64_t W, int64_t ldr,
                                                        int64_t lag0, double fs, double* __restrict__ delay,
                                                        int64_t* __restrict__ lag, double* __restrict__ peak) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;                                    // (whole waves leave: no barrier below)
  const float* row = r + b * ldr;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int64_t i = lane; i < W; i += 64) {
    const float v = row[i];
    if (v > best || (bi == 0x7fffffff && v == best)) { best = v; bi = (int)i; }
  }
  const float m = wave_max(best);
  const int i0 = wave_min_i(best == m ? bi : 0x7fffffff);
  if (lane != 0) return;
  if (i0 == 0x7fffffff) {                                // nothing but NaN
    delay[b] = (double)__builtin_nanf(""); lag[b] = 0; peak[b] = (double)__builtin_nanf("");
    return;
  }
  double delta = 0.0, pk = (double)m;
  if (i0 > 0 && i0 < W - 1) {
    const double a = row[i0 - 1], c = row[i0 + 1];
    const double den = a - 2.0 * (double)m + c;
    if (den < 0.0) { delta = 0.5 * (a - c) / den; pk = (double)m - 0.25 * (a - c) * delta; }
  }
  lag[b] = lag0 + i0;
  delay[b] = ((double)(lag0 + i0) + delta) / fs;
  peak[b] = pk;
}

unsigned gcc_grid_x(int64_t n, int64_t rows) {
  int64_t b = ceil_div(n, 256);
  const int64_t cap = rows >= 64 ? 64 : 4096 / (rows < 1 ? 1 : rows);
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

template <int NT, int MAXN>
int csd_launch(const CsdArgs& A, int nblk, int64_t B, hipStream_t st) {
  const size_t lds = (size_t)A.nfft * 2 * sizeof(float2);
  int rc = reserve_dynamic_lds("csd", (const void*)csd_partial_kernel<NT, MAXN>, lds);
  if (rc) return rc;
  hipLaunchKernelGGL((csd_partial_kernel<NT, MAXN>), dim3(nblk, (unsigned)B), dim3(NT), lds, st, A);
  SYG_CHECK_LAUNCH("csd_partial");
  return SYG_OK;
}

int csd_check_outputs(const char* who, const void* a, const void* b, const void* c, const void* d) {
  SYG_REQUIRE(a || b || c || d, "%s: no output asked for (pxy, pxx, pyy and coherence are all null)", who);
  return SYG_OK;
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_csd_work_bytes(int64_t B, int64_t nseg, int nfft) {
  if (B < 1 || nseg < 1 || nfft < 2) return -1;
  int run, nblk;
  csd_split(nseg, run, nblk);
  const int64_t F = nfft / 2 + 1;
  // float partial rows [B, nblk, 4, F], then (8-byte aligned) the float64 slice sums [B, slices, 4, F]
  const int64_t part = (B * nblk * 4 * F * (int64_t)sizeof(float) + 7) & ~(int64_t)7;
  return part + B * csd_slices(nblk) * 4 * F * (int64_t)sizeof(double);
}

extern "C" int syg_csd_f32(const float* x, const float* y, int64_t B, int64_t By, int64_t L, int64_t ldx, int64_t ldy,
                           int nperseg, int step, int nfft, const float* window, const float* twiddle, int detrend,
                           double scale, float* pxy_out, float* pxx_out, float* pyy_out, float* coh_out, void* work,
                           void* stream) {
  SYG_REQUIRE(x && y && window && twiddle && work, "csd: null pointer argument");
  int rc = csd_check_outputs("csd", pxy_out, pxx_out, pyy_out, coh_out);
  if (rc) return rc;
  SYG_REQUIRE(is_pow2(nfft) && nfft >= 8 && nfft <= CSD_MAX_N, "csd: nfft must be a power of two in [8, %d] (got %d)",
              CSD_MAX_N, nfft);
  SYG_REQUIRE(nperseg >= 1 && nperseg <= nfft && step >= 1 && step <= nperseg, "csd: bad nperseg/step");
  SYG_REQUIRE(B >= 1 && B <= MAX_GRID_Y && L >= nperseg && ldx >= L, "csd: bad B/L/ldx");
  SYG_REQUIRE(By == 1 || By == B, "csd: y must have one row or B = %lld rows (got %lld)", (long long)B, (long long)By);
  SYG_REQUIRE(By == 1 || ldy >= L, "csd: bad ldy");
  SYG_REQUIRE(detrend >= 0 && detrend <= 2, "csd: detrend must be 0 (none), 1 (constant) or 2 (linear)");
  const int64_t nseg = (L - (nperseg - step)) / step;
  SYG_REQUIRE(nseg >= 1, "csd: no complete segment");
  int run, nblk;
  csd_split(nseg, run, nblk);
  const int F = nfft / 2 + 1;
  hipStream_t st = (hipStream_t)stream;
  CsdArgs A{x, y, ldx, By == 1 ? 0 : ldy, nperseg, step, nfft, nseg, run, window, (const float2*)twiddle, detrend,
            (float*)work};
  if (nfft <= 512) rc = csd_launch<64, 512>(A, nblk, B, st);
  else if (nfft <= 2048) rc = csd_launch<256, 2048>(A, nblk, B, st);
  else if (nfft <= 4096) rc = csd_launch<256, 4096>(A, nblk, B, st);     // 64 KiB of LDS: two workgroups of four waves a CU
  else rc = csd_launch<512, CSD_MAX_N>(A, nblk, B, st);
  if (rc) return rc;
  const int nz = csd_slices(nblk);
  const int64_t part = (B * nblk * 4 * (int64_t)F * (int64_t)sizeof(float) + 7) & ~(int64_t)7;
  double* dsub = reinterpret_cast<double*>(reinterpret_cast<char*>(work) + part);
  hipLaunchKernelGGL(csd_slice_kernel, dim3((F + 63) / 64, (unsigned)B, nz), dim3(64 * CF_G), 0, st, (const float*)work,
                     nblk, F, dsub);
  SYG_CHECK_LAUNCH("csd_slice");
  const CsdOut O{(float2*)pxy_out, pxx_out, pyy_out, coh_out};
  hipLaunchKernelGGL(csd_final_kernel, dim3((F + 255) / 256, (unsigned)B), dim3(256), 0, st, (const double*)dsub, nz, F,
                     0, 0.25 * scale / (double)nseg, O);
  SYG_CHECK_LAUNCH("csd_final");
  return SYG_OK;
}

extern "C" int syg_csd_rows_f32(const float* X, const float* Y, int64_t rows, int64_t n, double* acc, int first,
                                int last, int64_t nseg, double scale, float* pxy_out, float* pxx_out, float* pyy_out,
                                float* coh_out, void* stream) {
  SYG_REQUIRE(X && Y && acc, "csd_rows: null pointer argument");
  SYG_REQUIRE(rows >= 1 && rows <= MAX_GRID_Y && n >= 1 && n <= ((int64_t)1 << 26), "csd_rows: bad rows / n");
  SYG_REQUIRE(nseg >= rows, "csd_rows: nseg = %lld is below the rows of this call (%lld)", (long long)nseg, (long long)rows);
  if (last) {
    int rc = csd_check_outputs("csd_rows", pxy_out, pxx_out, pyy_out, coh_out);
    if (rc) return rc;
  }
  const int64_t F = n / 2 + 1;
  const CsdOut O{(float2*)pxy_out, pxx_out, pyy_out, coh_out};
  hipLaunchKernelGGL(csd_rows_kernel, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                     (const float2*)X, (const float2*)Y, rows, n, acc, first, last, scale / (double)nseg, O);
  SYG_CHECK_LAUNCH("csd_rows");
  return SYG_OK;
}

extern "C" int syg_gcc_weight_c64(const float* X, const float* Y, int64_t rows, int64_t rows_y, int64_t n, int phat,
                                  float* out, void* stream) {
  SYG_REQUIRE(X && Y && out, "gcc_weight: null pointer argument");
  SYG_REQUIRE(rows >= 1 && rows <= MAX_GRID_Y && (rows_y == 1 || rows_y == rows), "gcc_weight: bad row counts");
  SYG_REQUIRE(n >= 1 && n <= ((int64_t)1 << 27), "gcc_weight: bad n");
  SYG_REQUIRE(phat == 0 || phat == 1, "gcc_weight: weighting must be 0 (none) or 1 (phat)");
  hipLaunchKernelGGL(gcc_weight_kernel, dim3(gcc_grid_x(n, rows), (unsigned)rows), dim3(256), 0, (hipStream_t)stream,
                     (const float2*)X, (const float2*)Y, rows_y, n, phat, (float2*)out);
  SYG_CHECK_LAUNCH("gcc_weight");
  return SYG_OK;
}

extern "C" int syg_gcc_crop_f32(const float* c, int64_t rows, int64_t n, int64_t max_lag, float* out, void* stream) {
  SYG_REQUIRE(c && out, "gcc_crop: null pointer argument");
  SYG_REQUIRE(rows >= 1 && rows <= MAX_GRID_Y && n >= 1, "gcc_crop: bad rows / n");
  SYG_REQUIRE(max_lag >= 0 && 2 * max_lag + 1 <= n, "gcc_crop: the window of 2 max_lag + 1 = %lld lags does not fit n = %lld",
              (long long)(2 * max_lag + 1), (long long)n);
  hipLaunchKernelGGL(gcc_crop_kernel, dim3(gcc_grid_x(2 * max_lag + 1, rows), (unsigned)rows), dim3(256), 0,
                     (hipStream_t)stream, (const float2*)c, n, max_lag, out);
  SYG_CHECK_LAUNCH("gcc_crop");
  return SYG_OK;
}

extern "C" int syg_peak_pick_f32(const float* r, int64_t B, int64_t W, int64_t ldr, int64_t lag0, double fs, double* delay_out,
                                 int64_t* lag_out, double* peak_out, void* stream) {
  SYG_REQUIRE(r && delay_out && lag_out && peak_out, "peak_pick: null pointer argument");
  SYG_REQUIRE(B >= 1 && W >= 1 && W < (int64_t)0x7fffffff && ldr >= W && B <= (int64_t)0x7fffffff, "peak_pick: bad B / W / ldr");
  SYG_REQUIRE(fs > 0.0 && fs <= 1.7976931348623157e308, "peak_pick: fs must be positive and finite");
  hipLaunchKernelGGL(peak_pick_kernel, dim3((unsigned)ceil_div(B, 4)), dim3(256), 0, (hipStream_t)stream, r, B, W, ldr,
                     lag0, fs, delay_out, lag_out, peak_out);
  SYG_CHECK_LAUNCH("peak_pick");
  return SYG_OK;
}
