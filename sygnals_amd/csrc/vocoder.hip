// Phase vocoder of librosa 0.10 (core.phase_vocoder, as effects.time_stretch calls it) between syg_stft2048_c2c_f32 and
// syg_istft2048_f32, in the product form.  librosa accumulates phase_acc += phi_advance + wrap(angle(D[c + 1]) -
// angle(D[c]) - phi_advance); modulo 2 pi the advance and the wrap cancel, so the output phasor at step t is
//     p[t] = u(D[0]) prod_{j < t} u(D[c_j + 1]) conj(u(D[c_j])),     u(z) = z / |z|,
// a complex-multiply scan: no atan2, no sincos, no accumulator that grows with t.  The float64 restatement of the angle
// form that is the contract lives in tests/vocoder_ref.py.
//
// u(z) is formed in float64 from the float32 parts (their squares neither overflow nor underflow there, 1e-30 included):
// v_rsq_f64 and two Newton steps.  u(0) = (copysign(1, re), 0): np.angle gives pi for a bin stored as -0 + 0j.  p stays in
// float64 without renormalisation: a factor is off 1 by a few 1e-16, the drift after 1e5 steps is below 1e-10.
//
// The step table (col[t] = int(step_t), alpha[t] = step_t mod 1; sygnals_amd/_tables.vocoder_steps) is the same for every
// clip and bin, so every branch on it is uniform over a wave and its loads are scalar.  A column outside [0, T) reads as
// zero: librosa pads two, and a table from elsewhere cannot make the kernel read outside D.
//
// Chain form: one lane per (clip, bin), consecutive lanes consecutive bins (a wave's load is 512 contiguous bytes), the
// lane walks t and keeps D[c + 1] when the next step's column is that one.  Chunked form, for few clips: t is cut into
// chunks of PV_CHUNK steps; pv_prod_kernel forms each chunk's product of step ratios (multiplication is associative),
// pv_scan_kernel turns them in place into the chunk-start phasors, pv_run_kernel then walks every chunk on its own.  It
// reads D twice, so it is taken only where the chain form would leave the device mostly idle.
#include <math.h>
#include "host.h"

namespace syg {
namespace {

constexpr int NB = 1025;
constexpr int PV_TILES = (NB + 63) / 64;   // waves per (clip, chunk): the last one holds bin 1024 alone
constexpr int PV_WAVES = 4;                // waves per workgroup, each with a (clip, chunk, tile) of its own
constexpr int PV_CHUNK = 32;               // steps per chunk of the chunked form

struct PvArgs {
  const float2* D; int64_t B, T; const int32_t* col; const double* alpha; int64_t Tout; float2* out;
  int64_t K, nch;                          // steps per lane and lanes per chain (chain form: K = Tout, nch = 1)
  double2* start;                          // [B, nch, NB] chunk-start phasors, or null (chain form: p0 = u(D[0]))
};

struct PvCol { double ux, uy, m; };        // unit phasor and magnitude of one element of D

__device__ __forceinline__ PvCol pv_unit(float2 z) {
  const double re = (double)z.x, im = (double)z.y;
  const double r2 = fma(re, re, im * im);
  PvCol c;
  if (r2 == 0.0) {
    c.ux = copysign(1.0, re); c.uy = 0.0; c.m = 0.0;
    return c;
  }
  double inv = __builtin_amdgcn_rsq(r2);
  inv = inv * fma(-0.5 * r2, inv * inv, 1.5);
  inv = inv * fma(-0.5 * r2, inv * inv, 1.5);
  c.ux = re * inv; c.uy = im * inv; c.m = r2 * inv;
  return c;
}

// element (c, k) of a clip whose bin-k column starts at Dk; columns outside [0, T) are zero
__device__ __forceinline__ PvCol pv_load(const float2* __restrict__ Dk, int64_t c, int64_t T) {
  return pv_unit(c >= 0 && c < T ? Dk[c * NB] : make_float2(0.f, 0.f));
}

// The walk both kernels share.  EMIT: write the outputs of steps [t0, t1); otherwise only form the product of the
// steps' ratios.  (px, py) comes in as the phasor of step t0 (EMIT) or (1, 0), and leaves advanced past step t1 - 1.
template <bool EMIT>
__device__ __forceinline__ void pv_walk(const PvArgs& A, const float2* __restrict__ Dk, float2* __restrict__ ok, int64_t t0,
                                        int64_t t1, double& px, double& py) {
  int64_t cur = INT64_MIN / 2;
  PvCol a{1.0, 0.0, 0.0}, b{1.0, 0.0, 0.0};
  double rx = 1.0, ry = 0.0;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t c = A.col[t];
    if (c != cur) {
      a = (c == cur + 1) ? b : pv_load(Dk, c, A.T);
      b = pv_load(Dk, c + 1, A.T);
      cur = c;
      rx = fma(b.ux, a.ux, b.uy * a.uy);                     // u(D[c + 1]) conj(u(D[c]))
      ry = fma(b.uy, a.ux, -(b.ux * a.uy));
    }
    if (EMIT) {
      const double al = A.alpha[t];
      const double mag = fma(al, b.m, (1.0 - al) * a.m);
      ok[t * NB] = make_float2((float)(mag * px), (float)(mag * py));
    }
    const double nx = fma(px, rx, -(py * ry)), ny = fma(px, ry, py * rx);
    px = nx; py = ny;
  }
}

// wave -> (clip b, chunk ch, bin k); false for a wave past the grid's end or a lane past bin 1024
__device__ __forceinline__ bool pv_place(const PvArgs& A, int64_t& b, int64_t& ch, int& k) {
  const int64_t w = (int64_t)blockIdx.x * PV_WAVES + (threadIdx.x >> 6);
  if (w >= A.B * A.nch * PV_TILES) return false;
  const int tile = (int)(w % PV_TILES);
  const int64_t rest = w / PV_TILES;
  b = rest / A.nch;
  ch = rest - b * A.nch;
  k = tile * 64 + (threadIdx.x & 63);
  return k < NB;
}

__global__ __launch_bounds__(64 * PV_WAVES) void pv_run_kernel(PvArgs A) {
  int64_t b, ch; int k;
  if (!pv_place(A, b, ch, k)) return;
  const float2* Dk = A.D + b * A.T * NB + k;
  const int64_t t0 = ch * A.K, t1 = (A.Tout - t0 > A.K) ? t0 + A.K : A.Tout;
  double px, py;
  if (A.start) {
    const double2 s = A.start[(b * A.nch + ch) * NB + k];
    px = s.x; py = s.y;
  } else {
    const PvCol c0 = pv_load(Dk, 0, A.T);
    px = c0.ux; py = c0.uy;
  }
  pv_walk<true>(A, Dk, A.out + b * A.Tout * NB + k, t0, t1, px, py);
}

// start[b, ch, k] <- the product of the ratios of chunk ch's steps
__global__ __launch_bounds__(64 * PV_WAVES) void pv_prod_kernel(PvArgs A) {
  int64_t b, ch; int k;
  if (!pv_place(A, b, ch, k)) return;
  const int64_t t0 = ch * A.K, t1 = (A.Tout - t0 > A.K) ? t0 + A.K : A.Tout;
  double px = 1.0, py = 0.0;
  if (ch + 1 < A.nch) pv_walk<false>(A, A.D + b * A.T * NB + k, nullptr, t0, t1, px, py);   // the last one is never used
  A.start[(b * A.nch + ch) * NB + k] = make_double2(px, py);
}

// in place: start[b, ch, k] <- u(D[b, 0, k]) prod_{j < ch} start[b, j, k]; one lane per (clip, bin)
__global__ __launch_bounds__(64 * PV_WAVES) void pv_scan_kernel(PvArgs A) {
  const int64_t w = (int64_t)blockIdx.x * PV_WAVES + (threadIdx.x >> 6);
  if (w >= A.B * PV_TILES) return;
  const int64_t b = w / PV_TILES;
  const int k = (int)(w % PV_TILES) * 64 + (threadIdx.x & 63);
  if (k >= NB) return;
  const PvCol c0 = pv_load(A.D + b * A.T * NB + k, 0, A.T);
  double px = c0.ux, py = c0.uy;
  double2* s = A.start + b * A.nch * NB + k;
  auto step = [&](int64_t ch, double2 r) {
    s[ch * NB] = make_double2(px, py);
    const double nx = fma(px, r.x, -(py * r.y)), ny = fma(px, r.y, py * r.x);
    px = nx; py = ny;
  };
  constexpr int U = 8;                     // loads of U chunks in flight ahead of the serial chain (17 waves a clip)
  int64_t ch = 0;
  for (; ch + U <= A.nch; ch += U) {
    double2 r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) r[u] = s[(ch + u) * NB];
#pragma unroll
    for (int u = 0; u < U; ++u) step(ch + u, r[u]);
  }
  for (; ch < A.nch; ++ch) step(ch, s[ch * NB]);
}

// form: -1 the rule, 0 chain, 1 chunked.  The rule: fewer than eight waves a CU in the chain form, and chains of at
// least four chunks.
inline bool pv_chunked(int64_t B, int64_t Tout, int form, int cus) {
  if (form >= 0) return form == 1;
  return Tout >= 4 * PV_CHUNK && B * PV_TILES < (int64_t)cus * 8;
}

int pv_check_shape(int64_t B, int64_t T, int64_t Tout, int form) {
  SYG_REQUIRE(B >= 1 && T >= 1 && Tout >= 1 && B * T < ((int64_t)1 << 40) / NB && B * Tout < ((int64_t)1 << 40) / NB,
              "phase_vocoder: bad B / T / T_out");
  SYG_REQUIRE(form >= -1 && form <= 1, "phase_vocoder: form must be -1 (the rule), 0 (chain) or 1 (chunked), got %d", form);
  return SYG_OK;
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int syg_phase_vocoder_chunk(void) { return PV_CHUNK; }

extern "C" int64_t syg_phase_vocoder_work_bytes(int64_t B, int64_t T_out, int form) {
  if (pv_check_shape(B, 1, T_out, form)) return -1;
  if (!pv_chunked(B, T_out, form, device_cu_count())) return 0;
  return B * ceil_div(T_out, PV_CHUNK) * NB * (int64_t)sizeof(double2);
}

extern "C" int syg_phase_vocoder_f32(const float* D, int64_t B, int64_t T, const int32_t* col, const double* alpha,
                                     int64_t T_out, float* out, void* work, int form, void* stream) {
  SYG_REQUIRE(D && col && alpha && out, "phase_vocoder: null pointer argument (D / col / alpha / out)");
  if (const int rc = pv_check_shape(B, T, T_out, form)) return rc;
  const bool chunked = pv_chunked(B, T_out, form, device_cu_count());
  SYG_REQUIRE(work || !chunked, "phase_vocoder: this shape takes the chunked form and needs `work` (syg_phase_vocoder_work_bytes)");
  SYG_REQUIRE(((uintptr_t)work & 15) == 0, "phase_vocoder: `work` must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  PvArgs A{(const float2*)D, B, T, col, alpha, T_out, (float2*)out, T_out, 1, nullptr};
  if (chunked) {
    A.K = PV_CHUNK;
    A.nch = ceil_div(T_out, PV_CHUNK);
    A.start = (double2*)work;
  }
  const int64_t blocks = ceil_div(B * A.nch * PV_TILES, PV_WAVES);
  SYG_REQUIRE(blocks < 0x7fffffff, "phase_vocoder: too many chains");
  if (chunked) {
    hipLaunchKernelGGL(pv_prod_kernel, dim3((unsigned)blocks), dim3(64 * PV_WAVES), 0, st, A);
    SYG_CHECK_LAUNCH("phase_vocoder");
    hipLaunchKernelGGL(pv_scan_kernel, dim3((unsigned)ceil_div(B * PV_TILES, PV_WAVES)), dim3(64 * PV_WAVES), 0, st, A);
    SYG_CHECK_LAUNCH("phase_vocoder");
  }
  hipLaunchKernelGGL(pv_run_kernel, dim3((unsigned)blocks), dim3(64 * PV_WAVES), 0, st, A);
  SYG_CHECK_LAUNCH("phase_vocoder");
  return SYG_OK;
}
