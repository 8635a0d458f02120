// SpecAugment (Park et al. 2019) of x [B, K, T] float32, frames fastest: a time warp, then the union of up to 16 frequency
// and 16 time masks, drawn per clip from the Philox generator (rng_dev.h).  The package's own definition; the integer /
// float64 restatement that is the contract lives in tests/specaug_ref.py, sygnals_amd/_specaug.py is the host twin.
//
// Draws.  Clip b is row r = first_row + b of stream RNG_STREAM_SPEC; item q is ONE Philox call at counter (q, 0, r, 2), of
// which words 0 and 1 are used: q = 0 the warp, 1 + i frequency mask i, 17 + j time mask j.  draw(w, n) = (w n) >> 32.
// Nothing depends on the launch shape or on where the clip lies in a batch, and there are no atomics.
//
// Shape.  The work is one read and one write per element.  A workgroup takes a tile of SPEC_TILE cells of one clip (cell
// i of a clip is row i / T, frame i % T); its first lanes make the clip's calls, one a lane, and leave the intervals in
// LDS; then the tile streams, every load of a thread issued before its first store.  Clips that lie contiguous and
// 16-byte aligned, unwarped, move as float4; everything else one float a lane, the warp with its two neighbouring reads.
// The in-place form (out = x, no warp) launches over the masks only: a workgroup per (clip, slice of the masks' cells);
// where the masks may cover the clip (their widths sum to it or more) it walks the tiles instead and stores masked cells.
// "mean": float64 chunk sums of SPEC_TILE cells of x[b, :, :T_b], cut by cell index alone and added in index order, so the
// resident form (the clip's workgroup sums the chunks itself, one launch) and the tiled form (two small launches ahead)
// give the same bits.
#include "host.h"
#include "rng_dev.h"

#pragma clang fp contract(off)

namespace syg {
namespace {

constexpr int SPEC_THREADS = 256;
constexpr int SPEC_PER = 16;                         // cells a thread moves in a tile
constexpr int SPEC_TILE = SPEC_THREADS * SPEC_PER;   // cells of a tile, and of a chunk of the "mean" sums
constexpr int SPEC_MAX_MASKS = 16;
constexpr int64_t SPEC_MAX_ELEMS = (int64_t)1 << 31;
constexpr int64_t SPEC_RESIDENT_MAX = 8192;          // the rule: clips up to this many cells take "mean" in one launch
constexpr int64_t SPEC_MAX_BLOCKS = 1 << 20;         // workgroups of a launch, at most (the rest by a grid stride)
constexpr int SPEC_SLICES_MAX = 256;                 // slices of a mask's cells in the in-place form

enum { MEAN_NONE = 0, MEAN_READ = 1, MEAN_RESIDENT = 2 };

struct SpecArgs {
  const float* x; float* out; const int64_t* lengths; const float* means; double* part;
  int64_t sxb, sxk, sob, sok, B, K, T, first_row, F, Wt, W, tiles, chunks;
  double ratio;
  uint2 key;
  int nf, nt, mean_mode, per_clip;
  float value;
};

struct ClipParams {                                  // in LDS: what the clip's calls gave
  int64_t Tb;                                        // valid frames
  int64_t c, wp;                                     // the warp: c < 0 for none
  uint32_t f0[SPEC_MAX_MASKS], f[SPEC_MAX_MASKS];    // rows [f0, f0 + f): K, T <= 2^31, so 32 bits hold every bound
  uint32_t t0[SPEC_MAX_MASKS], t[SPEC_MAX_MASKS];    // frames [t0, t0 + t)
  float value;
};

__device__ __forceinline__ int64_t draw(uint32_t w, int64_t n) { return (int64_t)(((uint64_t)w * (uint64_t)n) >> 32); }

__device__ __forceinline__ int64_t clip_frames(const int64_t* lengths, int64_t b, int64_t T) {
  if (!lengths) return T;
  const int64_t v = lengths[b];                      // the host checked it; clamped all the same: it bounds every access
  return v < 1 ? 1 : (v > T ? T : v);
}

__device__ __forceinline__ int64_t time_width_of(const SpecArgs& A, int64_t Tb) {
  const int64_t cap = (int64_t)floor(A.ratio * (double)Tb);
  return A.Wt < cap ? A.Wt : cap;
}

// item q of clip b, by one lane: q = 0 the warp, 1 .. 16 the frequency masks, 17 .. 32 the time masks
__device__ __forceinline__ void draw_item(const SpecArgs& A, ClipParams& P, int64_t b, int q, int64_t Tb) {
  const bool warp = q == 0, fm = q >= 1 && q <= SPEC_MAX_MASKS, tm = q > SPEC_MAX_MASKS && q <= 2 * SPEC_MAX_MASKS;
  const int i = fm ? q - 1 : q - 1 - SPEC_MAX_MASKS;
  if (warp && !(A.W > 0 && Tb > 2 * A.W)) { P.c = -1; P.wp = -1; return; }
  if ((fm && i >= A.nf) || (tm && i >= A.nt) || !(warp || fm || tm)) return;
  const uint4 w = philox4x32(make_uint4((uint32_t)q, 0u, (uint32_t)(A.first_row + b), (uint32_t)RNG_STREAM_SPEC), A.key);
  if (warp) {
    const int64_t c = A.W + draw(w.x, Tb - 2 * A.W);
    P.c = c;
    P.wp = c - A.W + 1 + draw(w.y, 2 * A.W);
  } else if (fm) {
    const int64_t f = draw(w.x, A.F + 1);
    P.f[i] = (uint32_t)f;
    P.f0[i] = (uint32_t)draw(w.y, A.K - f + 1);
  } else {
    const int64_t t = draw(w.x, time_width_of(A, Tb) + 1);
    P.t[i] = (uint32_t)t;
    P.t0[i] = (uint32_t)draw(w.y, Tb - t + 1);
  }
}

// float64 sum of cells [j0, j0 + n) of x[b, :, :Tb] (cell j: row j / Tb, frame j % Tb), n <= SPEC_TILE: a thread adds its
// cells 4 (tid + 256 m) + e in the order m, e ascending; a butterfly over each wave; the four waves in order.  Every
// thread returns it.  flat: cell j lies at xb[j] (the clip is contiguous over its Tb frames); vec: and xb is 16-byte
// aligned, so four cells come in one load.  The assignment of cells to threads is the same on every path: same bits.
__device__ __forceinline__ double chunk_sum(const float* xb, int64_t sxk, int64_t Tb, int64_t j0, int n, bool flat, bool vec,
                                            double* red) {
  const int tid = threadIdx.x;
  float v[SPEC_PER];
#pragma unroll
  for (int m = 0; m < SPEC_PER / 4; ++m) {
    const int base = 4 * (tid + SPEC_THREADS * m);
    if (vec && base + 4 <= n) {
      const float4 q = *reinterpret_cast<const float4*>(xb + j0 + base);
      v[4 * m] = q.x; v[4 * m + 1] = q.y; v[4 * m + 2] = q.z; v[4 * m + 3] = q.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float val = 0.f;
        if (base + e < n) {
          const uint32_t j = (uint32_t)(j0 + base + e);                // cells of a clip stay below 2^31
          if (flat) {
            val = xb[j];
          } else {
            const uint32_t k = j / (uint32_t)Tb;
            val = xb[(int64_t)k * sxk + (j - k * (uint32_t)Tb)];
          }
        }
        v[4 * m + e] = val;
      }
    }
  }
  double a = 0.0;
#pragma unroll
  for (int m = 0; m < SPEC_PER; ++m)
    if (4 * (tid + SPEC_THREADS * (m / 4)) + (m & 3) < n) a = a + (double)v[m];
  a = wave_sum_d(a);
  __syncthreads();                                   // red may still be read from the chunk before
  if ((tid & 63) == 0) red[tid >> 6] = a;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// The sum of a clip from its chunk sums, the same in both forms: thread t adds chunks t, t + 256, ... in index order
// (`mine`), then a butterfly over each wave and the four waves in order.
__device__ __forceinline__ double clip_total(double mine, double* red) {
  mine = wave_sum_d(mine);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mine;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ bool clip_flat(const SpecArgs& A, int64_t Tb) { return A.K == 1 || A.sxk == Tb; }
__device__ __forceinline__ bool clip_vec(const SpecArgs& A, int64_t b, int64_t Tb) {
  return clip_flat(A, Tb) && (((uintptr_t)(A.x + b * A.sxb)) & 15) == 0;
}

// The masks as a tile tests them.  SMALL (at most two masks of a kind, the default): the intervals sit in registers, an
// absent mask with no cells; otherwise the counts loop over LDS.
template <bool SMALL>
struct Masks {
  const ClipParams* P;
  int nf, nt;
  uint32_t Tb, f0[2], f[2], t0[2], t[2];
  __device__ __forceinline__ Masks(const ClipParams& p, int nf_, int nt_) : P(&p), nf(nf_), nt(nt_), Tb((uint32_t)p.Tb) {
    if (SMALL) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        f0[i] = i < nf ? p.f0[i] : 0u; f[i] = i < nf ? p.f[i] : 0u;
        t0[i] = i < nt ? p.t0[i] : 0u; t[i] = i < nt ? p.t[i] : 0u;
      }
    }
  }
  __device__ __forceinline__ bool hit(uint32_t k, uint32_t tt) const {
    if (tt >= Tb) return false;
    if (SMALL) return (k - f0[0] < f[0]) | (k - f0[1] < f[1]) | (tt - t0[0] < t[0]) | (tt - t0[1] < t[1]);
    bool m = false;
    for (int i = 0; i < nf; ++i) m = m || k - P->f0[i] < P->f[i];
    for (int i = 0; i < nt; ++i) m = m || tt - P->t0[i] < P->t[i];
    return m;
  }
};

// the warped clip's frame u < Tb of a row: left segment [0, c) -> wp frames, right segment [c, Tb) -> Tb - wp frames,
// each torch's linear resize with align_corners = False; the position by integer quotient and remainder (floor is exact)
__device__ __forceinline__ float warped(const float* xr, const ClipParams& P, int64_t u) {
  int64_t off = 0, n_in = P.c, n_out = P.wp;
  if (u >= P.wp) { off = P.c; n_in = P.Tb - P.c; n_out = P.Tb - P.wp; u -= P.wp; }
  int64_t q = 0;
  float w = 0.f;
  if (P.Tb <= 32768) {                               // (2u + 1) n_in < 2^31, r < 2 n_out <= 2^16: 32 bits, and exact floats
    const uint32_t a = (2u * (uint32_t)u + 1u) * (uint32_t)n_in, den = 2u * (uint32_t)n_out;
    if (a > (uint32_t)n_out) {
      const uint32_t num = a - (uint32_t)n_out, q32 = num / den;
      q = q32;
      w = (float)(num - q32 * den) / (float)den;
    }
  } else {
    const int64_t num = (2 * u + 1) * n_in - n_out, den = 2 * n_out;
    if (num > 0) {
      q = num / den;
      w = (float)((double)(num - q * den) / (double)den);
    }
  }
  const int64_t i0 = q < n_in - 1 ? q : n_in - 1, i1 = i0 + 1 < n_in - 1 ? i0 + 1 : n_in - 1;
  const float a = xr[off + i0], b = xr[off + i1];
  return a + w * (b - a);
}

// the value of the result's cell (k, t): x's, the warped clip's, or the mask's
template <bool SMALL>
__device__ __forceinline__ float cell(const float* xb, int64_t sxk, const ClipParams& P, const Masks<SMALL>& M, uint32_t k, uint32_t t) {
  if (M.hit(k, t)) return P.value;
  const float* xr = xb + (int64_t)k * sxk;
  return (P.c >= 0 && t < M.Tb) ? warped(xr, P, t) : xr[t];
}

// the clip's parameters into LDS (the block's first 33 lanes, one call a lane) and, for "mean", its value
__device__ __forceinline__ void setup_clip(const SpecArgs& A, ClipParams& P, double* red, int64_t b) {
  const int64_t Tb = clip_frames(A.lengths, b, A.T);
  __syncthreads();                                   // the clip before is done with P
  if (threadIdx.x <= 2 * SPEC_MAX_MASKS) draw_item(A, P, b, threadIdx.x, Tb);
  if (threadIdx.x == 0) { P.Tb = Tb; P.value = A.mean_mode == MEAN_READ ? A.means[b] : A.value; }
  if (A.mean_mode == MEAN_RESIDENT) {
    const int64_t cells = A.K * Tb;
    const bool flat = clip_flat(A, Tb), vec = clip_vec(A, b, Tb);
    double mine = 0.0;
    int owner = 0;                                   // chunk c is added by thread c % 256
    for (int64_t j0 = 0; j0 < cells; j0 += SPEC_TILE) {
      const double s = chunk_sum(A.x + b * A.sxb, A.sxk, Tb, j0, (int)(cells - j0 < SPEC_TILE ? cells - j0 : SPEC_TILE), flat, vec, red);
      if ((int)threadIdx.x == owner) mine = mine + s;
      owner = (owner + 1) & (SPEC_THREADS - 1);
    }
    const double total = clip_total(mine, red);
    if (threadIdx.x == 0) P.value = (float)(total / (double)cells);
  }
  __syncthreads();
}

// The copy form.  VEC: every clip lies contiguous and 16-byte aligned in x and out and no clip is warped.
// SCAN (out = x where the masks may cover the clip): the same walk over the tiles without a load, masked cells stored.
template <bool VEC, bool SMALL, bool SCAN = false>
__global__ __launch_bounds__(SPEC_THREADS) void spec_copy_kernel(SpecArgs A) {
  __shared__ ClipParams P;
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int64_t units = A.per_clip ? A.B : A.B * A.tiles, cells = A.K * A.T;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {        // uniform over the workgroup
    const int64_t b = A.per_clip ? u : u / A.tiles;
    const int64_t first = A.per_clip ? 0 : u - b * A.tiles, last = A.per_clip ? A.tiles : first + 1;
    setup_clip(A, P, red, b);
    const Masks<SMALL> M(P, A.nf, A.nt);
    const float* xb = A.x + b * A.sxb;
    float* ob = A.out + b * A.sob;
   for (int64_t tile = first; tile < last; ++tile) {
    const int64_t i0 = tile * SPEC_TILE;
    const uint32_t T = (uint32_t)A.T;
    if (VEC) {
      float4 v[SPEC_PER / 4];
      bool full[SPEC_PER / 4];
#pragma unroll
      for (int j = 0; j < SPEC_PER / 4; ++j) {
        const int64_t i = i0 + 4 * (tid + SPEC_THREADS * j);
        full[j] = i + 4 <= cells;
        if (full[j]) v[j] = *reinterpret_cast<const float4*>(xb + i);
      }
#pragma unroll
      for (int j = 0; j < SPEC_PER / 4; ++j) {
        const int64_t i = i0 + 4 * (tid + SPEC_THREADS * j);
        if (i >= cells) continue;
        uint32_t k = (uint32_t)i / T, t = (uint32_t)i - k * T;
        if (full[j]) {
          float e[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            if (M.hit(k, t)) e[a] = P.value;
            if (++t == T) { t = 0; ++k; }
          }
          *reinterpret_cast<float4*>(ob + i) = make_float4(e[0], e[1], e[2], e[3]);
        } else {                                     // the clip's last cells, fewer than four
          for (int64_t ii = i; ii < cells; ++ii) {
            ob[ii] = M.hit(k, t) ? P.value : xb[ii];
            if (++t == T) { t = 0; ++k; }
          }
        }
      }
    } else if (SCAN) {                               // four cells in a row a thread: one division for the four
#pragma unroll
      for (int j = 0; j < SPEC_PER / 4; ++j) {
        const int64_t i = i0 + 4 * (tid + SPEC_THREADS * j);
        if (i >= cells) continue;
        uint32_t k = (uint32_t)i / T, t = (uint32_t)i - k * T;
        const int n = cells - i < 4 ? (int)(cells - i) : 4;
        for (int a = 0; a < n; ++a) {
          if (M.hit(k, t)) ob[(int64_t)k * A.sok + t] = P.value;
          if (++t == T) { t = 0; ++k; }
        }
      }
    } else {
      float v[SPEC_PER];
#pragma unroll
      for (int j = 0; j < SPEC_PER; ++j) {
        const int64_t i = i0 + tid + SPEC_THREADS * j;
        if (i < cells) {
          const uint32_t k = (uint32_t)i / T, t = (uint32_t)i - k * T;
          v[j] = cell(xb, A.sxk, P, M, k, t);
        }
      }
#pragma unroll
      for (int j = 0; j < SPEC_PER; ++j) {
        const int64_t i = i0 + tid + SPEC_THREADS * j;
        if (i < cells) {
          const uint32_t k = (uint32_t)i / T, t = (uint32_t)i - k * T;
          ob[(int64_t)k * A.sok + t] = v[j];
        }
      }
    }
   }
  }
}

// The in-place form: a workgroup per (clip, slice) draws the clip's masks, one a lane, and writes its slice of the cells of
// each; nothing else is touched.
__global__ __launch_bounds__(SPEC_THREADS) void spec_inplace_kernel(SpecArgs A, int slices) {
  __shared__ ClipParams P;
  const int64_t units = A.B * slices;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t b = u / slices;
    const int slice = (int)(u - b * slices);
    const int64_t Tb = clip_frames(A.lengths, b, A.T);
    __syncthreads();
    if (threadIdx.x >= 1 && threadIdx.x <= 2 * SPEC_MAX_MASKS) draw_item(A, P, b, threadIdx.x, Tb);
    __syncthreads();
    const float value = A.mean_mode == MEAN_READ ? A.means[b] : A.value;
    float* ob = A.out + b * A.sob;
    for (int m = 0; m < A.nf + A.nt; ++m) {
      const bool fm = m < A.nf;
      const int i = fm ? m : m - A.nf;
      // rows [r0, r0 + nr) by frames [c0, c0 + nc)
      const int64_t r0 = fm ? P.f0[i] : 0, nr = fm ? P.f[i] : A.K, c0 = fm ? 0 : P.t0[i], nc = fm ? Tb : P.t[i];
      const int64_t n = nr * nc;
      for (int64_t j = (int64_t)slice * SPEC_THREADS + threadIdx.x; j < n; j += (int64_t)slices * SPEC_THREADS) {
        const uint32_t r = (uint32_t)j / (uint32_t)nc;                // n <= K T < 2^32
        ob[(r0 + r) * A.sok + c0 + ((uint32_t)j - r * (uint32_t)nc)] = value;
      }
    }
  }
}

// work: part [B][chunks] float64 (chunks = ceil(K T / SPEC_TILE)), then means [B] float32
__global__ __launch_bounds__(SPEC_THREADS) void spec_sums_kernel(SpecArgs A) {
  __shared__ double red[4];
  const int64_t units = A.B * A.chunks;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t b = u / A.chunks, ch = u - b * A.chunks;
    const int64_t Tb = clip_frames(A.lengths, b, A.T), cells = A.K * Tb, j0 = ch * SPEC_TILE;
    if (j0 >= cells) continue;                       // uniform: a shorter clip has fewer chunks
    const double s = chunk_sum(A.x + b * A.sxb, A.sxk, Tb, j0, (int)(cells - j0 < SPEC_TILE ? cells - j0 : SPEC_TILE), clip_flat(A, Tb),
                               clip_vec(A, b, Tb), red);
    if (threadIdx.x == 0) A.part[b * A.chunks + ch] = s;
  }
}

// a workgroup a clip: its chunk sums by clip_total's order
__global__ __launch_bounds__(SPEC_THREADS) void spec_means_kernel(SpecArgs A, float* means) {
  __shared__ double red[4];
  for (int64_t b = blockIdx.x; b < A.B; b += gridDim.x) {
    const int64_t cells = A.K * clip_frames(A.lengths, b, A.T), n = (cells + SPEC_TILE - 1) / SPEC_TILE;
    const double* pr = A.part + b * A.chunks;
    double mine = 0.0;
    for (int64_t c = threadIdx.x; c < n; c += SPEC_THREADS) mine = mine + pr[c];
    const double total = clip_total(mine, red);
    if (threadIdx.x == 0) means[b] = (float)(total / (double)cells);
  }
}

inline int64_t span(int64_t B, int64_t K, int64_t T, int64_t sb, int64_t sk) { return (B - 1) * sb + (K - 1) * sk + T; }
inline bool overlaps(const float* a, int64_t na, const float* b, int64_t nb) { return a < b + nb && b < a + na; }
inline unsigned grid_of(int64_t units) { return (unsigned)(units < SPEC_MAX_BLOCKS ? units : SPEC_MAX_BLOCKS); }
inline bool aligned16(const float* p, int64_t sb, int64_t B) { return ((uintptr_t)p & 15) == 0 && (B == 1 || (sb & 3) == 0); }

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_spec_augment_constants(int key) {
  switch (key) {
    case SYG_SPEC_STREAM: return RNG_STREAM_SPEC;
    case SYG_SPEC_MAX_MASKS: return SPEC_MAX_MASKS;
    case SYG_SPEC_TILE: return SPEC_TILE;
    case SYG_SPEC_RESIDENT_MAX: return SPEC_RESIDENT_MAX;
    case SYG_SPEC_MAX_ELEMS: return SPEC_MAX_ELEMS;
    default: return -1;
  }
}

extern "C" int64_t syg_spec_augment_work_bytes(int64_t B, int64_t K, int64_t T) {
  if (B < 1 || K < 1 || T < 1 || (long double)B * (long double)K * (long double)T > (long double)SPEC_MAX_ELEMS) return -1;
  return B * ceil_div(K * T, SPEC_TILE) * (int64_t)sizeof(double) + ((B + 1) / 2) * 8;
}

extern "C" int syg_spec_augment_f32(const float* x, int64_t B, int64_t K, int64_t T, int64_t sxb, int64_t sxk, float* out, int64_t sob,
                                    int64_t sok, const int64_t* lengths, uint64_t seed, int64_t first_row, int freq_masks,
                                    int64_t freq_width, int time_masks, int64_t time_width, double time_ratio, int64_t time_warp,
                                    int mean, float mask_value, int form, void* work, int64_t work_bytes, void* stream) {
  const char* who = "spec_augment";
  SYG_REQUIRE(x && out, "%s: null pointer argument (x / out)", who);
  SYG_REQUIRE(B >= 1 && K >= 1 && T >= 1, "%s: empty input (B = %lld, K = %lld, T = %lld; each must be at least 1)", who, (long long)B,
              (long long)K, (long long)T);
  const long double total = (long double)B * (long double)K * (long double)T;
  SYG_REQUIRE(total <= (long double)SPEC_MAX_ELEMS, "%s: %.0Lf elements are above 2^31 = %lld", who, total, (long long)SPEC_MAX_ELEMS);
  SYG_REQUIRE(sxb >= 0 && sxk >= 0 && (K == 1 || sxk >= T || sxk == 0), "%s: bad input strides (%lld, %lld) for T = %lld", who,
              (long long)sxb, (long long)sxk, (long long)T);
  SYG_REQUIRE(sok >= T && sob >= K * sok - (sok - T), "%s: bad output strides (%lld, %lld) for %lld rows of T = %lld", who,
              (long long)sob, (long long)sok, (long long)K, (long long)T);
  SYG_REQUIRE(freq_masks >= 0 && freq_masks <= SPEC_MAX_MASKS && time_masks >= 0 && time_masks <= SPEC_MAX_MASKS,
              "%s: freq_masks and time_masks must lie in 0 .. %d (got %d, %d)", who, SPEC_MAX_MASKS, freq_masks, time_masks);
  SYG_REQUIRE(freq_width >= 0 && freq_width <= K, "%s: freq_width must lie in [0, K = %lld] (got %lld)", who, (long long)K,
              (long long)freq_width);
  SYG_REQUIRE(time_width >= 0 && time_warp >= 0, "%s: time_width and time_warp must not be negative (got %lld, %lld)", who,
              (long long)time_width, (long long)time_warp);
  SYG_REQUIRE(time_ratio > 0.0 && time_ratio <= 1.0, "%s: time_ratio must lie in (0, 1] (got %g)", who, time_ratio);
  SYG_REQUIRE(mean == 0 || mean == 1, "%s: mean must be 0 (mask_value) or 1 (the clip's mean)", who);
  SYG_REQUIRE(mean || isfinite(mask_value), "%s: mask_value must be finite", who);
  SYG_REQUIRE(first_row >= 0 && first_row + B <= RNG_ROW_LIMIT, "%s: rows first_row .. first_row + B - 1 must lie in [0, 2^31)", who);
  SYG_REQUIRE(form >= 0 && form <= 2, "%s: form must be 0 (the rule), 1 (resident) or 2 (tiled)", who);
  const bool warp_asked = time_warp > 0;
  if (time_width > T) time_width = T;                // a mask is never wider than the clip
  if (2 * (time_warp < T ? time_warp : T) >= T) time_warp = 0;     // no clip has more than 2 W frames: none is warped
  const int64_t nx = span(B, K, T, sxb, sxk), no = span(B, K, T, sob, sok);
  const bool inplace = out == x && sob == sxb && sok == sxk;
  if (inplace)
    SYG_REQUIRE(!warp_asked, "%s: out overlaps x (with time_warp > 0 the result cannot be written onto its input)", who);
  else
    SYG_REQUIRE(!overlaps(x, nx, out, no), "%s: out overlaps x (only out = x itself with time_warp = 0 is served)", who);

  const int64_t cells = K * T;
  SpecArgs A;
  A.x = x; A.out = out; A.lengths = lengths; A.means = nullptr; A.part = nullptr;
  A.sxb = sxb; A.sxk = K == 1 ? T : sxk; A.sob = sob; A.sok = K == 1 ? T : sok; A.B = B; A.K = K; A.T = T; A.first_row = first_row;
  A.F = freq_width; A.Wt = time_width; A.W = time_warp; A.tiles = ceil_div(cells, SPEC_TILE); A.chunks = A.tiles;
  A.ratio = time_ratio; A.key = rng_key(seed); A.nf = freq_masks; A.nt = time_masks; A.mean_mode = MEAN_NONE; A.per_clip = 0; A.value = mask_value;
  const int masks = freq_masks + time_masks;
  if (inplace && masks == 0) return SYG_OK;          // nothing to write

  if (mean && masks) {
    const bool resident = !inplace && (form ? form == 1 : cells <= SPEC_RESIDENT_MAX);
    if (resident) {
      A.mean_mode = MEAN_RESIDENT;
    } else {
      SYG_REQUIRE(work && work_bytes >= syg_spec_augment_work_bytes(B, K, T), "%s: the mean needs `work` of %lld bytes", who,
                  (long long)syg_spec_augment_work_bytes(B, K, T));
      A.part = (double*)work;
      float* means = (float*)(A.part + B * A.chunks);
      hipLaunchKernelGGL(spec_sums_kernel, dim3(grid_of(B * A.chunks)), dim3(SPEC_THREADS), 0, (hipStream_t)stream, A);
      SYG_CHECK_LAUNCH(who);
      hipLaunchKernelGGL(spec_means_kernel, dim3(grid_of(B)), dim3(SPEC_THREADS), 0, (hipStream_t)stream, A, means);
      SYG_CHECK_LAUNCH(who);
      A.means = means;
      A.mean_mode = MEAN_READ;
    }
  }
  const bool small = freq_masks <= 2 && time_masks <= 2;
  if (inplace && freq_masks * freq_width * T + time_masks * time_width * K >= cells) {
    // the masks may cover the clip: walking its tiles once writes no cell twice and divides less than walking the masks
    void (*kernel)(SpecArgs) = small ? spec_copy_kernel<false, true, true> : spec_copy_kernel<false, false, true>;
    hipLaunchKernelGGL(kernel, dim3(grid_of(B * A.tiles)), dim3(SPEC_THREADS), 0, (hipStream_t)stream, A);
    SYG_CHECK_LAUNCH(who);
    return SYG_OK;
  }
  if (inplace) {
    // slices: enough workgroups for the largest mask a clip can draw, a few thousand cells each
    const int64_t big = (freq_masks ? freq_width * T : 0) > (time_masks ? time_width * K : 0) ? freq_width * T : time_width * K;
    int64_t slices = ceil_div(big > 0 ? big : 1, SPEC_TILE);
    if (slices > SPEC_SLICES_MAX) slices = SPEC_SLICES_MAX;
    hipLaunchKernelGGL(spec_inplace_kernel, dim3(grid_of(B * slices)), dim3(SPEC_THREADS), 0, (hipStream_t)stream, A, (int)slices);
    SYG_CHECK_LAUNCH(who);
    return SYG_OK;
  }
  const bool vec = time_warp == 0 && A.sxk == T && A.sok == T && aligned16(x, sxb, B) && aligned16(out, sob, B);
  // resident "mean": a workgroup a clip, which sums the clip once and walks its tiles; else a workgroup a tile
  A.per_clip = A.mean_mode == MEAN_RESIDENT;
  const unsigned grid = grid_of(A.per_clip ? B : B * A.tiles);
  void (*kernel)(SpecArgs) = vec ? (small ? spec_copy_kernel<true, true> : spec_copy_kernel<true, false>)
                                 : (small ? spec_copy_kernel<false, true> : spec_copy_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(SPEC_THREADS), 0, (hipStream_t)stream, A);
  SYG_CHECK_LAUNCH(who);
  return SYG_OK;
}
