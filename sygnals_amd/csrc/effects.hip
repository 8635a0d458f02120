// Audio effects of sygnals/core/audio/effects/: the feedback delay (delay.py:15-111, and what chorus.py computes), the
// spectral-subtraction gate of noise_reduction_spectral (utility.py:59-131) as a real mask for syg_istft2048_f32, and the
// pointwise effects (gain / mixes, tremolo.py, compression.py, mid/side widening); and add_noise of
// sygnals/core/augment/noise.py.  The float64 restatement that is the contract lives in tests/effects_ref.py (add_noise:
// tests/vocoder_ref.py).  No atomics anywhere: every result is bit-identical from run to run.
//
// Delay.  w[n] = x[n] + fb w[n - D], out[n] = dry x[n] + wet w[n - D].  The recurrence is D independent chains, one per
// residue n mod D, and neighbouring residues are neighbours in memory: a lane owns a residue and walks it in steps of D
// (delay_run_kernel), every wave access coalesced when D >= 64.  That is the whole story for a batch with a long delay
// (1024 clips, D = 11025: chains of 3 steps).  One long row, or a short delay, has few chains of L / D steps each, so a
// chain is cut into chunks of FX_CHUNK steps:
//   1. delay_ends_kernel: z[c, r] = the zero-state value of w at the end of chunk c of residue r (Horner, one read of x);
//   2. the carries s[c, r] = w at the end of chunk c - 1 obey s[c] = z[c - 1] + fb^K s[c - 1]: laid out [chunk][residue]
//      that is THIS delay again on the array z, with delay D, feedback fb^K, dry 0 and wet 1 -- the host function calls
//      itself (in place on z), so a very long chain is scanned in chunks too, level by level;
//   3. delay_run_kernel started from the carry: the plain kernel over one chunk per lane.
// The chunked form reads x twice (12 bytes per sample against 8); it is taken only where the plain form would leave
// the device mostly idle (fewer than four waves per CU) and the chains are long (>= 4 chunks).  fb = 0 is exact in both:
// every carry is then the previous sample itself and the output expression is evaluated without contraction.
//
// Gate.  Two launches: gate_profile_kernel sums |Dn|^2 over the profile's frames per bin in float64 (four frame slices
// per workgroup, combined in slice order); gate_mask_kernel is pointwise over D, lanes along the bins, four frames per
// workgroup so that one long row fills the device.
//
// add_noise.  A row's two powers are needed before its first output sample.  A row of up to AN_RESIDENT samples is one
// workgroup's: it sums while it copies y and noise into LDS and mixes from there (one launch, 12 bytes a sample).  A
// longer row takes two launches: slice sums (so that one long row still fills the device), then the mix, which adds the
// row's slices in slice order and reads y and noise again (20 bytes a sample).  syg_fx_add_noise_gen_f32 is the same mix
// on noise that is generated in registers and never stored (below, beside the kernels).
#include <float.h>
#include <math.h>
#include "host.h"
#include "rng_dev.h"

namespace syg {
namespace {

constexpr int NB = 1025;
#ifndef SYG_FX_CHUNK
#define SYG_FX_CHUNK 64              // steps of a chain per chunk; -DSYG_FX_CHUNK=n builds the variants that
#endif                               // tools/effects_bench.py --delay-only times (DESIGN.md 4.10 has the figures)
constexpr int FX_CHUNK = SYG_FX_CHUNK;
constexpr int FX_THREADS = 256;

// ------------------------------------------------------------------ delay
struct DelayArgs {
  const float* x; float* out; int64_t B, L, ldx, ldo, D, Deff, K, nch; float fb, dry, wet; const float* carry;
};

// dry x + wet w with both products rounded (no FMA): at fb = 0 a host test rebuilds the output bit for bit
__device__ __forceinline__ float delay_mix(float dry, float x, float wet, float w) {
#pragma clang fp contract(off)
  const float a = dry * x;
  const float b = wet * w;
  return a + b;
}

// lane t of a row: chunk c = t / Deff, residue r = t % Deff; steps c K .. c K + K - 1 of the chain, sample (step) D + r
__global__ __launch_bounds__(FX_THREADS) void delay_run_kernel(DelayArgs A) {
  const int64_t per_row = A.nch * A.Deff;
  const int64_t g = (int64_t)blockIdx.x * FX_THREADS + threadIdx.x;
  if (g >= A.B * per_row) return;
  const int64_t b = g / per_row, t = g - b * per_row;
  const int64_t c = t / A.Deff, r = t - c * A.Deff;
  const float* x = A.x + b * A.ldx;
  float* out = A.out + b * A.ldo;
  float wp = A.carry ? A.carry[b * per_row + t] : 0.f;      // w[n - D] of the chunk's first sample
  int64_t n = c * A.K * A.D + r;
  const int64_t span = A.K * A.D;
  const int64_t nend = (A.L - n > span) ? n + span : A.L;
  const int64_t D = A.D;
  constexpr int U = 8;                                        // loads of U steps in flight ahead of the serial chain
  for (; n + (U - 1) * D < nend; n += U * D) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = x[n + u * D];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      out[n + u * D] = delay_mix(A.dry, v[u], A.wet, wp);
      wp = fmaf(A.fb, wp, v[u]);
    }
  }
  for (; n < nend; n += D) {
    const float v = x[n];
    out[n] = delay_mix(A.dry, v, A.wet, wp);
    wp = fmaf(A.fb, wp, v);
  }
}

// z[b, c Deff + r] = sum_i fb^(K - 1 - i) x[(c K + i) D + r] over the chunk's samples inside the row (the last chunk's
// value is never used: no chunk follows it)
__global__ __launch_bounds__(FX_THREADS) void delay_ends_kernel(DelayArgs A, float* __restrict__ z) {
  const int64_t per_row = A.nch * A.Deff;
  const int64_t g = (int64_t)blockIdx.x * FX_THREADS + threadIdx.x;
  if (g >= A.B * per_row) return;
  const int64_t b = g / per_row, t = g - b * per_row;
  const int64_t c = t / A.Deff, r = t - c * A.Deff;
  const float* x = A.x + b * A.ldx;
  int64_t n = c * A.K * A.D + r;
  const int64_t span = A.K * A.D;
  const int64_t nend = (A.L - n > span) ? n + span : A.L;
  const int64_t D = A.D;
  float w = 0.f;
  constexpr int U = 8;
  for (; n + (U - 1) * D < nend; n += U * D) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = x[n + u * D];
#pragma unroll
    for (int u = 0; u < U; ++u) w = fmaf(A.fb, w, v[u]);
  }
  for (; n < nend; n += D) w = fmaf(A.fb, w, x[n]);
  z[b * per_row + t] = w;
}

// ------------------------------------------------------------------ spectral gate
constexpr int GP_SLICES = 4;         // frame slices of the profile pass (waves of a workgroup)
constexpr int GM_FRAMES = 4;         // frames per workgroup of the mask pass

// |d|^2 as __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)): no FMA, as the header states it
__device__ __forceinline__ float power_nofma(float2 d) {
#pragma clang fp contract(off)
  const float a = d.x * d.x;
  const float b = d.y * d.y;
  return a + b;
}

__global__ __launch_bounds__(64 * GP_SLICES) void gate_profile_kernel(const float2* __restrict__ Dn, int64_t Tn,
                                                                       float* __restrict__ N) {
  __shared__ double part[GP_SLICES][64];
  const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
  constexpr int ntile = (NB + 63) / 64;
  const int64_t b = blockIdx.x / ntile;
  const int k = (int)(blockIdx.x % ntile) * 64 + lane;
  double s = 0.0;
  if (k < NB) {
    const float2* p = Dn + b * Tn * NB + k;
    for (int64_t t = sl; t < Tn; t += GP_SLICES) {
      const float2 d = p[t * NB];
      s += (double)d.x * (double)d.x + (double)d.y * (double)d.y;
    }
  }
  part[sl][lane] = s;
  __syncthreads();
  if (sl == 0 && k < NB) {
    double tot = part[0][lane];
#pragma unroll
    for (int q = 1; q < GP_SLICES; ++q) tot += part[q][lane];
    N[b * NB + k] = (float)(tot / (double)Tn);
  }
}

__global__ __launch_bounds__(FX_THREADS) void gate_mask_kernel(const float2* __restrict__ D, int64_t T, int64_t nframes,
                                                                const float* __restrict__ N, float a,
                                                                float* __restrict__ G) {
  const int64_t f0 = (int64_t)blockIdx.x * GM_FRAMES;
  const int64_t b0 = f0 / T, t0 = f0 - b0 * T;               // one division per thread; the clip of frame f0 + j below
  const int64_t left = nframes - f0;
  const int ne = (int)(left < GM_FRAMES ? left : GM_FRAMES) * NB;
  const float2* Df = D + f0 * NB;
  float* Gf = G + f0 * NB;
  for (int e = threadIdx.x; e < ne; e += FX_THREADS) {
    const int j = e / NB, k = e - j * NB;
    int64_t b = b0, t = t0 + j;
    while (t >= T) { t -= T; ++b; }
    const float P = power_nofma(Df[e]);
    float g = 0.f;
    if (P > 0.f) {
      const float q = (a * N[b * NB + k]) / P;               // +inf when P is subnormal: the gain is then 0
      g = sqrtf(fmaxf(0.f, 1.f - q));
    }
    Gf[e] = g;
  }
}

// ------------------------------------------------------------------ pointwise effects
// grid: x over the samples of a row, y over the rows (a row loop past MAX_GRID_Y rows)
__global__ __launch_bounds__(FX_THREADS) void mix_kernel(const float* __restrict__ x, int64_t Lx, int64_t ldx,
                                                          const float* __restrict__ y, int64_t Ly, int64_t ldy, int64_t B,
                                                          int64_t L, float a, float bcoef, float* out, int64_t ldo) {
  const int64_t n = (int64_t)blockIdx.x * FX_THREADS + threadIdx.x;
  if (n >= L) return;
  for (int64_t r = blockIdx.y; r < B; r += gridDim.y) {
    const float xv = n < Lx ? x[r * ldx + n] : 0.f;
    float v = a * xv;
    if (y) v = fmaf(bcoef, n < Ly ? y[r * ldy + n] : 0.f, v);
    out[r * ldo + n] = v;
  }
}

constexpr int TREM_ROWS = 8;         // rows that share one evaluation of the LFO

__global__ __launch_bounds__(FX_THREADS) void tremolo_kernel(const float* x, int64_t B, int64_t L, int64_t ldx, double sr,
                                                              double w, double depth, int shape, int64_t n0, float* out,
                                                              int64_t ldo) {
  const int64_t n = (int64_t)blockIdx.x * FX_THREADS + threadIdx.x;
  if (n >= L) return;
  constexpr double PI = 3.141592653589793238462643383279502884;
  // the reference's order: ((2 pi) rate) (n / sr), every step in float64
  const double phase = w * ((double)(n0 + n) / sr);
  double lfo;
  if (shape == 0) {
    lfo = (sin(phase) + 1.0) / 2.0;
  } else if (shape == 1) {           // scipy.signal.sawtooth(phase, 0.5)
    const double tm = fmod(phase, 2.0 * PI);
    const double s = tm < 0.5 * (2.0 * PI) ? tm / (PI * 0.5) - 1.0 : (PI * 1.5 - tm) / (PI * 0.5);
    lfo = (s + 1.0) / 2.0;
  } else {                           // (sign(sin) + 1) / 2 with the exact zero mapped to 0
    lfo = sin(phase) > 0.0 ? 1.0 : 0.0;
  }
  const double m = (1.0 - depth) + lfo * depth;
  const int64_t r0 = (int64_t)blockIdx.y * TREM_ROWS;
  for (int64_t r = r0; r < B && r < r0 + TREM_ROWS; ++r) out[r * ldo + n] = (float)((double)x[r * ldx + n] * m);
}

__global__ __launch_bounds__(FX_THREADS) void compress_kernel(const float* x, int64_t B, int64_t L, int64_t ldx, double thr,
                                                               double ratio, float* out, int64_t ldo) {
  const int64_t n = (int64_t)blockIdx.x * FX_THREADS + threadIdx.x;
  if (n >= L) return;
  for (int64_t r = blockIdx.y; r < B; r += gridDim.y) {
    const float v = x[r * ldx + n];
    const double ax = fabs((double)v);
    float o = v;
    if (ax > thr) o = (float)((double)v * ((thr + (ax - thr) / ratio) / ax));
    out[r * ldo + n] = o;
  }
}

__global__ __launch_bounds__(FX_THREADS) void midside_kernel(const float* x, int64_t B, int64_t L, int64_t ldx, float width,
                                                              float* out, int64_t ldo) {
  const int64_t n = (int64_t)blockIdx.x * FX_THREADS + threadIdx.x;
  if (n >= L) return;
  for (int64_t r = blockIdx.y; r < B; r += gridDim.y) {
    const float l = x[2 * r * ldx + n], q = x[(2 * r + 1) * ldx + n];
    const float mid = (l + q) * 0.5f, side = ((l - q) * 0.5f) * width;
    out[2 * r * ldo + n] = mid + side;
    out[(2 * r + 1) * ldo + n] = mid - side;
  }
}

// ------------------------------------------------------------------ add_noise
// out = y + noise sqrt(Ps / (10^(snr / 10) Pn)) per row, Ps = mean(y^2) and Pn = mean(noise^2) in float64 (noise.py:75-99);
// a row whose Ps or Pn is below the float64 epsilon is copied.  Every sum has a fixed order: no atomics.
constexpr int AN_THREADS = 1024;           // the resident form: one workgroup a row
constexpr int64_t AN_RESIDENT = 16384;     // samples of a row it keeps in LDS between the sums and the mix (y, noise: 128 KiB)
constexpr int AN_SLICES = 64;              // most slices of a row in the two-launch form's power pass
constexpr int AN_PER_THREAD = 16;          // samples per thread of its mix pass: the row's partial sums are read once per 16
constexpr int64_t AN_SEG = (int64_t)FX_THREADS * AN_PER_THREAD;

struct NoiseArgs {
  const float* y; const float* noise; const double* snr; float* out; int64_t B, L, ldy, ldn, ldo; int S; int64_t slen; double2* part;
};

// sums of (a, c) over the workgroup, the waves' sums added in wave order; every thread gets the same pair
template <int NT>
__device__ __forceinline__ void block_sum2(double& a, double& c, double (*red)[NT / 64]) {
  a = wave_sum_d(a);
  c = wave_sum_d(c);
  __syncthreads();                           // a second call reuses `red`
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = c; }
  __syncthreads();
  a = 0.0; c = 0.0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) { a += red[0][w]; c += red[1][w]; }
}

// the reference's order: (Ps / 10^(snr / 10)) / Pn; false: the row is copied
__device__ __forceinline__ bool noise_scale(double Ps, double Pn, double snr_db, double& s) {
  constexpr double EPS = 2.220446049250313e-16;
  if (Ps < EPS || Pn < EPS) return false;
  s = sqrt((Ps / pow(10.0, snr_db / 10.0)) / Pn);
  return true;
}

__device__ __forceinline__ float noise_mix(float y, float n, double s) { return (float)((double)y + (double)n * s); }

__global__ __launch_bounds__(AN_THREADS) void noise_resident_kernel(NoiseArgs A) {
  extern __shared__ float an_rows[];         // y [L] | noise [L]
  __shared__ double red[2][AN_THREADS / 64];
  float* sy = an_rows;
  float* sn = an_rows + A.L;
  for (int64_t b = blockIdx.x; b < A.B; b += gridDim.x) {
    const float* y = A.y + b * A.ldy;
    const float* nz = A.noise + b * A.ldn;
    float* out = A.out + b * A.ldo;
    double a = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < (int)A.L; i += AN_THREADS) {    // a thread re-reads only what it wrote itself
      const float v = y[i], n = nz[i];
      sy[i] = v; sn[i] = n;
      a += (double)v * (double)v;
      c += (double)n * (double)n;
    }
    block_sum2<AN_THREADS>(a, c, red);
    double s = 0.0;
    const bool mix = noise_scale(a / (double)A.L, c / (double)A.L, A.snr[b], s);
    for (int i = threadIdx.x; i < (int)A.L; i += AN_THREADS) out[i] = mix ? noise_mix(sy[i], sn[i], s) : sy[i];
  }
}

// part[b, sl] = (sum y^2, sum noise^2) over slice sl (slen samples) of row b; grid (S, rows)
__global__ __launch_bounds__(FX_THREADS) void noise_power_kernel(NoiseArgs A) {
  __shared__ double red[2][FX_THREADS / 64];
  const int64_t n0 = (int64_t)blockIdx.x * A.slen, n1 = (A.L - n0 > A.slen) ? n0 + A.slen : A.L;
  for (int64_t b = blockIdx.y; b < A.B; b += gridDim.y) {
    const float* y = A.y + b * A.ldy;
    const float* nz = A.noise + b * A.ldn;
    double a = 0.0, c = 0.0;
    for (int64_t i = n0 + threadIdx.x; i < n1; i += FX_THREADS) {
      const float v = y[i], n = nz[i];
      a += (double)v * (double)v;
      c += (double)n * (double)n;
    }
    block_sum2<FX_THREADS>(a, c, red);
    if (threadIdx.x == 0) A.part[b * A.S + blockIdx.x] = make_double2(a, c);
  }
}

// grid (segments of AN_SEG samples, rows); the row's slices are summed in slice order by every thread (uniform loads)
__global__ __launch_bounds__(FX_THREADS) void noise_mix_kernel(NoiseArgs A) {
  const int64_t n0 = (int64_t)blockIdx.x * AN_SEG + threadIdx.x;
  for (int64_t b = blockIdx.y; b < A.B; b += gridDim.y) {
    double a = 0.0, c = 0.0;
    for (int sl = 0; sl < A.S; ++sl) { const double2 p = A.part[b * A.S + sl]; a += p.x; c += p.y; }
    double s = 0.0;
    const bool mix = noise_scale(a / (double)A.L, c / (double)A.L, A.snr[b], s);
    const float* y = A.y + b * A.ldy;
    const float* nz = A.noise + b * A.ldn;
    float* out = A.out + b * A.ldo;
#pragma unroll
    for (int j = 0; j < AN_PER_THREAD; ++j) {
      const int64_t n = n0 + (int64_t)j * FX_THREADS;
      if (n < A.L) out[n] = mix ? noise_mix(y[n], nz[n], s) : y[n];
    }
  }
}

// slices of a row in the power pass: enough workgroups to fill the device, none shorter than a mix segment
inline int noise_slices(int64_t B, int64_t L) {
  int64_t s = ceil_div(2048, B);
  if (s > AN_SLICES) s = AN_SLICES;
  const int64_t most = ceil_div(L, AN_SEG);
  return (int)(s < most ? s : most);
}

// ------------------------------------------------------------------ add_noise with the noise generated in registers
// The same arithmetic on noise[b, n] = the standard normal (seed, row first_row + b, n) of rng_dev.h, which never exists
// in memory.  A thread owns whole Philox calls (four consecutive samples).  Resident (up to AN_RESIDENT samples): y alone
// is kept in LDS, the row's noise in the threads' registers between the sums and the mix (ANG_QUADS calls a thread): one
// launch, 8 bytes a sample, every normal drawn once.  Longer rows: the power pass and the mix pass both generate (12
// bytes a sample); the power pass cuts a row into as many slices as make ANG_BLOCKS workgroups over the batch, each a
// whole number of mix segments; one wave a row then adds the slices in a fixed order and leaves the row's scale factor,
// so that no thread of the mix reads thousands of partial sums or evaluates pow.
#ifndef SYG_ANG_THREADS
#define SYG_ANG_THREADS 1024         // threads of the resident form; -DSYG_ANG_THREADS=512 builds the variant that
#endif                               // tools/noise_bench.py --shapes 2048x16384 times beside it
constexpr int ANG_THREADS = SYG_ANG_THREADS;        // (512: two workgroups a CU; measured slower)
constexpr int ANG_QUADS = (int)(AN_RESIDENT / (4 * ANG_THREADS));
constexpr int64_t ANG_BLOCKS = 2048;                // workgroups of the power pass that fill the device (8 a CU)
constexpr int ANG_SEG_QUADS = AN_PER_THREAD / 4;    // calls a thread of the two-launch form owns per segment

struct NoiseGenArgs {
  const float* y; const double* snr; float* out; int64_t B, L, ldy, ldo; int S; int64_t slen; double2* part; double2* scale;
  uint2 key; uint32_t first_row; int vy, vo;
};

// samples 4q .. 4q + 3 of a row of L: those past the end read as zero
__device__ __forceinline__ float4 load_quad(const float* __restrict__ y, int64_t q, int64_t L, int vec) {
  const int64_t n = 4 * q;
  if (vec && n + 3 < L) return *(const float4*)(y + n);
  return make_float4(n < L ? y[n] : 0.f, n + 1 < L ? y[n + 1] : 0.f, n + 2 < L ? y[n + 2] : 0.f, n + 3 < L ? y[n + 3] : 0.f);
}

__device__ __forceinline__ void store_quad(float* __restrict__ o, int64_t q, int64_t L, int vec, float4 v) {
  const int64_t n = 4 * q;
  if (vec && n + 3 < L) { *(float4*)(o + n) = v; return; }
  if (n < L) o[n] = v.x;
  if (n + 1 < L) o[n + 1] = v.y;
  if (n + 2 < L) o[n + 2] = v.z;
  if (n + 3 < L) o[n + 3] = v.w;
}

// the call's normals with those past the end of the row set to zero (they add nothing to the noise power)
__device__ __forceinline__ float4 noise_quad(uint2 key, int64_t q, uint32_t row, int64_t L) {
  float4 z = rng_normal4(key, (uint64_t)q, row);
  const int64_t n = 4 * q;
  if (n + 1 >= L) z.y = 0.f;
  if (n + 2 >= L) z.z = 0.f;
  if (n + 3 >= L) z.w = 0.f;
  return z;
}

// noise_quad fenced in by two volatile statements, which keep their order: the calls of an unrolled loop then run one
// after the other.  Interleaved by the compiler, the temporaries of four or eight Philox chains spill to scratch.
__device__ __forceinline__ float4 noise_quad_fenced(uint2 key, int64_t q, uint32_t row, int64_t L) {
  int ql = (int)q, qh = (int)(q >> 32);
  asm volatile("" : "+v"(ql), "+v"(qh));
  float4 z = noise_quad(key, (int64_t)(((uint64_t)(uint32_t)qh << 32) | (uint32_t)ql), row, L);
  asm volatile("" : "+v"(z.x), "+v"(z.y), "+v"(z.z), "+v"(z.w));
  return z;
}

__device__ __forceinline__ double quad_power(float4 v) {
  return ((double)v.x * (double)v.x + (double)v.y * (double)v.y) + ((double)v.z * (double)v.z + (double)v.w * (double)v.w);
}

__device__ __forceinline__ float4 noise_mix4(float4 y, float4 z, double s, bool mix) {
  if (!mix) return y;
  return make_float4(noise_mix(y.x, z.x, s), noise_mix(y.y, z.y, s), noise_mix(y.z, z.z, s), noise_mix(y.w, z.w, s));
}

__global__ __launch_bounds__(ANG_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void noise_gen_resident_kernel(NoiseGenArgs A) {
  constexpr int NQ = ANG_QUADS;
  extern __shared__ float4 ang_row[];        // y [4 ceil(L / 4)], the tail zero
  __shared__ double red[2][ANG_THREADS / 64];
  __shared__ double2 scale;
  float* sy = (float*)ang_row;
  const int L = (int)A.L, Lq = (L + 3) >> 2;
  for (int64_t b = blockIdx.x; b < A.B; b += gridDim.x) {
    const float* y = A.y + b * A.ldy;
    float* out = A.out + b * A.ldo;
    int tid = threadIdx.x;                                         // taken anew for every row: what is derived from it and
    asm volatile("" : "+v"(tid));                                  // hoisted out of the row loop would live in scratch
    double a = 0.0, c = 0.0;
    for (int i = tid; i < 4 * Lq; i += ANG_THREADS) {
      const float v = i < L ? y[i] : 0.f;
      sy[i] = v;
      a += (double)v * (double)v;
    }
    float4 z[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int q = tid + j * ANG_THREADS;
      z[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q < Lq) {
        z[j] = noise_quad_fenced(A.key, q, A.first_row + (uint32_t)b, L);
        c += quad_power(z[j]);
      }
    }
    block_sum2<ANG_THREADS>(a, c, red);       // (its barriers also order the stores of y before the reads below)
    if (tid == 0) {                          // one thread: pow in every wave costs as much as the wave's share of the noise
      double s0 = 0.0;
      const bool on = noise_scale(a / (double)A.L, c / (double)A.L, A.snr[b], s0);
      scale = make_double2(on ? s0 : 0.0, on ? 1.0 : 0.0);
    }
    __syncthreads();
    const double s = scale.x;
    const bool mix = scale.y != 0.0;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int q = tid + j * ANG_THREADS;
      if (q < Lq) store_quad(out, q, L, A.vo, noise_mix4(ang_row[q], z[j], s, mix));
      asm volatile("" ::: "memory");         // one call's samples after the other: no LDS read ahead across this
    }
    __syncthreads();                         // the next row overwrites y
  }
}

// part[b, sl] = (sum y^2, sum noise^2) over slice sl (slen samples, a multiple of AN_SEG) of row b; grid (S, rows)
__global__ __launch_bounds__(FX_THREADS) void noise_gen_power_kernel(NoiseGenArgs A) {
  __shared__ double red[2][FX_THREADS / 64];
  const int64_t n0 = (int64_t)blockIdx.x * A.slen, n1 = (A.L - n0 > A.slen) ? n0 + A.slen : A.L;
  for (int64_t b = blockIdx.y; b < A.B; b += gridDim.y) {
    const float* y = A.y + b * A.ldy;
    double a = 0.0, c = 0.0;
    for (int64_t q = (n0 >> 2) + threadIdx.x; 4 * q < n1; q += FX_THREADS) {
      a += quad_power(load_quad(y, q, A.L, A.vy));
      c += quad_power(noise_quad(A.key, q, A.first_row + (uint32_t)b, A.L));
    }
    block_sum2<FX_THREADS>(a, c, red);
    if (threadIdx.x == 0) A.part[b * A.S + blockIdx.x] = make_double2(a, c);
  }
}

// scale[b] = (the row's scale factor, 1), or (0, 0) for a row that is copied.  One wave a row: lane l adds its run of
// ceil(S / 64) consecutive slices in slice order, lane 0 the 64 runs in lane order (S <= 64: plain slice order).
__global__ __launch_bounds__(64) void noise_gen_scale_kernel(NoiseGenArgs A) {
  __shared__ double run[2][64];
  const int lane = threadIdx.x, per = (A.S + 63) / 64;
  for (int64_t b = blockIdx.x; b < A.B; b += gridDim.x) {
    double a = 0.0, c = 0.0;
    for (int sl = lane * per; sl < (lane + 1) * per && sl < A.S; ++sl) { const double2 p = A.part[b * A.S + sl]; a += p.x; c += p.y; }
    run[0][lane] = a;
    run[1][lane] = c;
    __syncthreads();
    if (lane == 0) {
      a = 0.0; c = 0.0;
      for (int l = 0; l < 64; ++l) { a += run[0][l]; c += run[1][l]; }
      double s = 0.0;
      const bool mix = noise_scale(a / (double)A.L, c / (double)A.L, A.snr[b], s);
      A.scale[b] = make_double2(mix ? s : 0.0, mix ? 1.0 : 0.0);
    }
    __syncthreads();
  }
}

// grid (segments of AN_SEG samples, rows); the noise is generated again
__global__ __launch_bounds__(FX_THREADS) void noise_gen_mix_kernel(NoiseGenArgs A) {
  const int64_t q0 = (int64_t)blockIdx.x * (AN_SEG / 4) + threadIdx.x;
  for (int64_t b = blockIdx.y; b < A.B; b += gridDim.y) {
    const double2 sc = A.scale[b];
    const double s = sc.x;
    const bool mix = sc.y != 0.0;
    const float* y = A.y + b * A.ldy;
    float* out = A.out + b * A.ldo;
    float4 v[ANG_SEG_QUADS];
#pragma unroll
    for (int j = 0; j < ANG_SEG_QUADS; ++j) {                    // every load in flight ahead of the generator
      const int64_t q = q0 + (int64_t)j * FX_THREADS;
      v[j] = 4 * q < A.L ? load_quad(y, q, A.L, A.vy) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < ANG_SEG_QUADS; ++j) {
      const int64_t q = q0 + (int64_t)j * FX_THREADS;
      if (4 * q < A.L) {
        const float4 z = mix ? noise_quad_fenced(A.key, q, A.first_row + (uint32_t)b, A.L) : make_float4(0.f, 0.f, 0.f, 0.f);
        store_quad(out, q, A.L, A.vo, noise_mix4(v[j], z, s, mix));
      }
    }
  }
}

// the power pass of the generating form: slices of a whole number of mix segments, ANG_BLOCKS workgroups over the batch
inline void noise_gen_slices(int64_t B, int64_t L, int& S, int64_t& slen) {
  int64_t s = ceil_div(ANG_BLOCKS, B);
  const int64_t most = ceil_div(L, AN_SEG);
  if (s > most) s = most;
  slen = ceil_div(ceil_div(L, s), AN_SEG) * AN_SEG;
  S = (int)ceil_div(L, slen);
}

int check_noise_gen_shape(int64_t B, int64_t L, int64_t first_row) {
  SYG_REQUIRE(B >= 1 && L >= 1 && L < ((int64_t)1 << 39), "fx_add_noise_gen: bad B / L");
  SYG_REQUIRE(first_row >= 0 && B <= RNG_ROW_LIMIT && first_row <= RNG_ROW_LIMIT - B,
              "fx_add_noise_gen: rows first_row .. first_row + B - 1 must lie in [0, 2^31) (got first_row = %lld, B = %lld)",
              (long long)first_row, (long long)B);
  return SYG_OK;
}

inline dim3 rows_grid(int64_t L, int64_t rows) { return dim3((unsigned)ceil_div(L, FX_THREADS), grid_rows(rows)); }

// rows [B, L] with strides: the checks every pointwise entry shares
int check_rows(const char* who, const void* x, const void* out, int64_t B, int64_t L, int64_t ldx, int64_t ldo) {
  SYG_REQUIRE(x && out, "%s: null pointer argument (x / out)", who);
  SYG_REQUIRE(B >= 1 && L >= 1 && ldx >= L && ldo >= L && L < ((int64_t)1 << 39), "%s: bad B / L / ldx / ldo", who);
  return SYG_OK;
}

// ------------------------------------------------------------------ delay: the plan both host functions share
inline int64_t delay_steps(int64_t L, int64_t D) { return ceil_div(L, D); }
inline int64_t delay_lanes(int64_t L, int64_t D) { return D < L ? D : L; }

// form: -1 the rule, 0 plain, 1 chunked (the top level of a call only; the carries below it follow the rule)
inline bool delay_chunked(int64_t B, int64_t L, int64_t D, int form, int cus) {
  if (form >= 0) return form == 1;
  return delay_steps(L, D) >= 4 * FX_CHUNK && B * delay_lanes(L, D) < (int64_t)cus * 256;
}

int64_t delay_work_floats(int64_t B, int64_t L, int64_t D, int form, int cus) {
  if (!delay_chunked(B, L, D, form, cus)) return 0;
  const int64_t nch = ceil_div(delay_steps(L, D), FX_CHUNK);
  const int64_t zl = nch * delay_lanes(L, D);
  return B * zl + delay_work_floats(B, zl, delay_lanes(L, D), -1, cus);
}

int delay_launch(const float* x, int64_t B, int64_t L, int64_t ldx, int64_t D, float fb, float dry, float wet, float* out,
                 int64_t ldo, float* work, int form, int cus, hipStream_t st) {
  const int64_t Deff = delay_lanes(L, D);
  DelayArgs A{x, out, B, L, ldx, ldo, D, Deff, delay_steps(L, D), 1, fb, dry, wet, nullptr};
  if (delay_chunked(B, L, D, form, cus)) {
    A.K = FX_CHUNK;
    A.nch = ceil_div(delay_steps(L, D), FX_CHUNK);
    const int64_t zl = A.nch * Deff;
    const int64_t blocks = ceil_div(B * zl, FX_THREADS);
    SYG_REQUIRE(blocks < 0x7fffffff, "fx_delay: too many chains");
    hipLaunchKernelGGL(delay_ends_kernel, dim3((unsigned)blocks), dim3(FX_THREADS), 0, st, A, work);
    SYG_CHECK_LAUNCH("fx_delay");
    // the carries: the same delay on z [B, zl] (chunk-major, so the delay is Deff), feedback fb^K, in place
    const float fbk = (float)pow((double)fb, (double)FX_CHUNK);
    if (const int rc = delay_launch(work, B, zl, zl, Deff, fbk, 0.f, 1.f, work, zl, work + B * zl, -1, cus, st)) return rc;
    A.carry = work;
  }
  const int64_t blocks = ceil_div(B * A.nch * Deff, FX_THREADS);
  SYG_REQUIRE(blocks < 0x7fffffff, "fx_delay: too many chains");
  hipLaunchKernelGGL(delay_run_kernel, dim3((unsigned)blocks), dim3(FX_THREADS), 0, st, A);
  SYG_CHECK_LAUNCH("fx_delay");
  return SYG_OK;
}

int check_delay_shape(int64_t B, int64_t L, int64_t D) {
  SYG_REQUIRE(B >= 1 && L >= 1 && L < ((int64_t)1 << 39) && B < ((int64_t)1 << 31), "fx_delay: bad B / L");
  SYG_REQUIRE(D >= 1 && D < ((int64_t)1 << 40), "fx_delay: delay_samples must be in [1, 2^40) (got %lld)", (long long)D);
  return SYG_OK;
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int syg_fx_delay_chunk(void) { return FX_CHUNK; }

extern "C" int64_t syg_fx_delay_work_bytes(int64_t B, int64_t L, int64_t delay_samples) {
  if (check_delay_shape(B, L, delay_samples)) return -1;
  return 4 * delay_work_floats(B, L, delay_samples, option(SYG_OPT_FX_DELAY_FORM), device_cu_count());
}

extern "C" int syg_fx_delay_f32(const float* x, int64_t B, int64_t L, int64_t ldx, int64_t delay_samples, double feedback,
                                double dry, double wet, float* out, int64_t ldo, void* work, void* stream) {
  SYG_REQUIRE(x && out, "fx_delay: null pointer argument (x / out)");
  if (const int rc = check_delay_shape(B, L, delay_samples)) return rc;
  SYG_REQUIRE(ldx >= L && ldo >= L, "fx_delay: bad ldx / ldo");
  SYG_REQUIRE(feedback >= 0.0 && feedback < 1.0, "fx_delay: feedback must be in [0, 1) (got %g)", feedback);
  SYG_REQUIRE(isfinite(dry) && isfinite(wet), "fx_delay: dry / wet must be finite");
  const float fb = (float)feedback;
  SYG_REQUIRE(fb < 1.f, "fx_delay: feedback rounds to 1 in float32");
  const int form = option(SYG_OPT_FX_DELAY_FORM), cus = device_cu_count();
  SYG_REQUIRE(work || delay_work_floats(B, L, delay_samples, form, cus) == 0,
              "fx_delay: this shape takes the chunked form and needs `work` (syg_fx_delay_work_bytes)");
  return delay_launch(x, B, L, ldx, delay_samples, fb, (float)dry, (float)wet, out, ldo, (float*)work, form, cus,
                      (hipStream_t)stream);
}

extern "C" int syg_spectral_gate_f32(const float* D, int64_t B, int64_t T, const float* Dn, int64_t Tn, double amount,
                                     float* gain, float* noise, void* stream) {
  SYG_REQUIRE(D && Dn && gain && noise, "spectral_gate: null pointer argument (D / Dn / gain / noise)");
  SYG_REQUIRE(B >= 1 && T >= 1 && Tn >= 1 && B * T < ((int64_t)1 << 40) / NB && B * Tn < ((int64_t)1 << 40) / NB,
              "spectral_gate: bad B / T / Tn");
  SYG_REQUIRE(amount >= 0.0 && isfinite(amount), "spectral_gate: reduction amount must be >= 0 and finite");
  constexpr int ntile = (NB + 63) / 64;
  SYG_REQUIRE(B * ntile < 0x7fffffff, "spectral_gate: too many clips");
  hipLaunchKernelGGL(gate_profile_kernel, dim3((unsigned)(B * ntile)), dim3(64 * GP_SLICES), 0, (hipStream_t)stream,
                     (const float2*)Dn, Tn, noise);
  SYG_CHECK_LAUNCH("spectral_gate");
  const int64_t nframes = B * T;
  hipLaunchKernelGGL(gate_mask_kernel, dim3((unsigned)ceil_div(nframes, GM_FRAMES)), dim3(FX_THREADS), 0,
                     (hipStream_t)stream, (const float2*)D, T, nframes, noise, (float)amount, gain);
  SYG_CHECK_LAUNCH("spectral_gate");
  return SYG_OK;
}

extern "C" int syg_fx_mix_f32(const float* x, int64_t Lx, int64_t ldx, const float* y, int64_t Ly, int64_t ldy, int64_t B,
                              int64_t L, double a, double b, float* out, int64_t ldo, void* stream) {
  SYG_REQUIRE(x && out, "fx_mix: null pointer argument (x / out)");
  SYG_REQUIRE(B >= 1 && L >= 1 && L < ((int64_t)1 << 39) && ldo >= L, "fx_mix: bad B / L / ldo");
  SYG_REQUIRE(Lx >= 0 && ldx >= (Lx < L ? Lx : L), "fx_mix: bad Lx / ldx");
  SYG_REQUIRE(!y || (Ly >= 0 && ldy >= (Ly < L ? Ly : L)), "fx_mix: bad Ly / ldy");
  SYG_REQUIRE(isfinite(a) && isfinite(b), "fx_mix: the coefficients must be finite");
  hipLaunchKernelGGL(mix_kernel, rows_grid(L, B), dim3(FX_THREADS), 0, (hipStream_t)stream, x, Lx, ldx, y, Ly, ldy, B, L,
                     (float)a, (float)b, out, ldo);
  SYG_CHECK_LAUNCH("fx_mix");
  return SYG_OK;
}

extern "C" int syg_fx_tremolo_f32(const float* x, int64_t B, int64_t L, int64_t ldx, double sr, double rate, double depth,
                                  int shape, int64_t n0, float* out, int64_t ldo, void* stream) {
  if (const int rc = check_rows("fx_tremolo", x, out, B, L, ldx, ldo)) return rc;
  SYG_REQUIRE(sr > 0.0 && isfinite(sr), "fx_tremolo: sr must be positive");
  SYG_REQUIRE(rate > 0.0 && isfinite(rate), "fx_tremolo: rate must be positive");
  SYG_REQUIRE(depth >= 0.0 && depth <= 1.0, "fx_tremolo: depth must be in [0, 1]");
  SYG_REQUIRE(shape >= SYG_LFO_SINE && shape <= SYG_LFO_SQUARE, "fx_tremolo: unknown LFO shape %d", shape);
  SYG_REQUIRE(n0 >= 0 && n0 < ((int64_t)1 << 52), "fx_tremolo: bad first sample index");
  const int64_t gy = ceil_div(B, TREM_ROWS);
  SYG_REQUIRE(gy <= MAX_GRID_Y, "fx_tremolo: too many rows");
  constexpr double PI = 3.141592653589793238462643383279502884;
  hipLaunchKernelGGL(tremolo_kernel, dim3((unsigned)ceil_div(L, FX_THREADS), (unsigned)gy), dim3(FX_THREADS), 0,
                     (hipStream_t)stream, x, B, L, ldx, sr, (2.0 * PI) * rate, depth, shape, n0, out, ldo);
  SYG_CHECK_LAUNCH("fx_tremolo");
  return SYG_OK;
}

extern "C" int syg_fx_compress_f32(const float* x, int64_t B, int64_t L, int64_t ldx, double threshold, double ratio,
                                   float* out, int64_t ldo, void* stream) {
  if (const int rc = check_rows("fx_compress", x, out, B, L, ldx, ldo)) return rc;
  SYG_REQUIRE(threshold >= 0.0 && isfinite(threshold), "fx_compress: threshold must be >= 0 and finite");
  SYG_REQUIRE(ratio >= 1.0, "fx_compress: ratio must be >= 1");
  hipLaunchKernelGGL(compress_kernel, rows_grid(L, B), dim3(FX_THREADS), 0, (hipStream_t)stream, x, B, L, ldx, threshold,
                     ratio, out, ldo);
  SYG_CHECK_LAUNCH("fx_compress");
  return SYG_OK;
}

extern "C" int syg_fx_midside_f32(const float* x, int64_t B, int64_t L, int64_t ldx, double width, float* out, int64_t ldo,
                                  void* stream) {
  if (const int rc = check_rows("fx_midside", x, out, B, L, ldx, ldo)) return rc;
  SYG_REQUIRE(width >= 0.0 && isfinite(width), "fx_midside: width must be >= 0 and finite");
  hipLaunchKernelGGL(midside_kernel, rows_grid(L, B), dim3(FX_THREADS), 0, (hipStream_t)stream, x, B, L, ldx, (float)width,
                     out, ldo);
  SYG_CHECK_LAUNCH("fx_midside");
  return SYG_OK;
}

extern "C" int64_t syg_fx_add_noise_resident_max(void) { return AN_RESIDENT; }

extern "C" int64_t syg_fx_add_noise_work_bytes(int64_t B, int64_t L) {
  if (B < 1 || L < 1 || L >= ((int64_t)1 << 39) || B >= ((int64_t)1 << 31)) {
    set_error("fx_add_noise: bad B / L");
    return -1;
  }
  return L <= AN_RESIDENT ? 0 : B * noise_slices(B, L) * (int64_t)sizeof(double2);
}

extern "C" int syg_fx_add_noise_f32(const float* y, int64_t B, int64_t L, int64_t ldy, const float* noise, int64_t ldn,
                                    const double* snr_db, float* out, int64_t ldo, void* work, void* stream) {
  SYG_REQUIRE(y && noise && snr_db && out, "fx_add_noise: null pointer argument (y / noise / snr_db / out)");
  SYG_REQUIRE(B >= 1 && L >= 1 && L < ((int64_t)1 << 39) && B < ((int64_t)1 << 31), "fx_add_noise: bad B / L");
  SYG_REQUIRE(ldy >= L && ldn >= L && ldo >= L, "fx_add_noise: bad ldy / ldn / ldo");
  hipStream_t st = (hipStream_t)stream;
  NoiseArgs A{y, noise, snr_db, out, B, L, ldy, ldn, ldo, 1, L, nullptr};
  if (L <= AN_RESIDENT) {
    const size_t lds = 2 * (size_t)L * sizeof(float);
    if (const int rc = reserve_dynamic_lds("fx_add_noise", (const void*)noise_resident_kernel, lds)) return rc;
    hipLaunchKernelGGL(noise_resident_kernel, dim3(capped_grid(B, NOISE_WGS_PER_CU)), dim3(AN_THREADS), lds, st, A);
    SYG_CHECK_LAUNCH("fx_add_noise");
    return SYG_OK;
  }
  SYG_REQUIRE(work, "fx_add_noise: a row past %lld samples takes two launches and needs `work` (syg_fx_add_noise_work_bytes)",
              (long long)AN_RESIDENT);
  SYG_REQUIRE(((uintptr_t)work & 15) == 0, "fx_add_noise: `work` must be 16-byte aligned");
  A.S = noise_slices(B, L);
  A.slen = ceil_div(L, A.S);
  A.part = (double2*)work;
  const unsigned gy = grid_rows(B);
  hipLaunchKernelGGL(noise_power_kernel, dim3((unsigned)A.S, gy), dim3(FX_THREADS), 0, st, A);
  SYG_CHECK_LAUNCH("fx_add_noise");
  hipLaunchKernelGGL(noise_mix_kernel, dim3((unsigned)ceil_div(L, AN_SEG), gy), dim3(FX_THREADS), 0, st, A);
  SYG_CHECK_LAUNCH("fx_add_noise");
  return SYG_OK;
}

extern "C" int64_t syg_fx_add_noise_gen_work_bytes(int64_t B, int64_t L) {
  if (check_noise_gen_shape(B, L, 0)) return -1;
  if (L <= AN_RESIDENT) return 0;
  int S; int64_t slen;
  noise_gen_slices(B, L, S, slen);
  return (B * S + B) * (int64_t)sizeof(double2);            // the slice sums, then the rows' scale factors
}

extern "C" int syg_fx_add_noise_gen_f32(const float* y, int64_t B, int64_t L, int64_t ldy, uint64_t seed, int64_t first_row,
                                        const double* snr_db, float* out, int64_t ldo, void* work, void* stream) {
  SYG_REQUIRE(y && snr_db && out, "fx_add_noise_gen: null pointer argument (y / snr_db / out)");
  if (const int rc = check_noise_gen_shape(B, L, first_row)) return rc;
  SYG_REQUIRE(ldy >= L && ldo >= L, "fx_add_noise_gen: bad ldy / ldo");
  hipStream_t st = (hipStream_t)stream;
  const int vy = ((uintptr_t)y & 15) == 0 && (ldy & 3) == 0, vo = ((uintptr_t)out & 15) == 0 && (ldo & 3) == 0;
  NoiseGenArgs A{y, snr_db, out, B, L, ldy, ldo, 1, L, nullptr, nullptr, rng_key(seed), (uint32_t)first_row, vy, vo};
  const unsigned gb = capped_grid(B, NOISE_WGS_PER_CU);
  if (L <= AN_RESIDENT) {
    const size_t lds = (size_t)ceil_div(L, 4) * sizeof(float4);
    if (const int rc = reserve_dynamic_lds("fx_add_noise_gen", (const void*)noise_gen_resident_kernel, lds)) return rc;
    hipLaunchKernelGGL(noise_gen_resident_kernel, dim3(gb), dim3(ANG_THREADS), lds, st, A);
    SYG_CHECK_LAUNCH("fx_add_noise_gen");
    return SYG_OK;
  }
  SYG_REQUIRE(work, "fx_add_noise_gen: a row past %lld samples takes three launches and needs `work` (syg_fx_add_noise_gen_work_bytes)",
              (long long)AN_RESIDENT);
  SYG_REQUIRE(((uintptr_t)work & 15) == 0, "fx_add_noise_gen: `work` must be 16-byte aligned");
  noise_gen_slices(B, L, A.S, A.slen);
  A.part = (double2*)work;
  A.scale = A.part + B * A.S;
  const unsigned gy = grid_rows(B);
  hipLaunchKernelGGL(noise_gen_power_kernel, dim3((unsigned)A.S, gy), dim3(FX_THREADS), 0, st, A);
  SYG_CHECK_LAUNCH("fx_add_noise_gen");
  hipLaunchKernelGGL(noise_gen_scale_kernel, dim3(gb), dim3(64), 0, st, A);
  SYG_CHECK_LAUNCH("fx_add_noise_gen");
  hipLaunchKernelGGL(noise_gen_mix_kernel, dim3((unsigned)ceil_div(L, AN_SEG), gy), dim3(FX_THREADS), 0, st, A);
  SYG_CHECK_LAUNCH("fx_add_noise_gen");
  return SYG_OK;
}
