// Loudness metering after ITU-R BS.1770 / EBU R128 and what a normaliser needs behind it (the float64 restatement that is
// the contract lives in tests/loudness_ref.py; the K-weighting design and the segment arithmetic in
// sygnals_amd/_loudness.py).  Clips are x [B, C, L] float32, unit stride along L, any stride over B and C.
//
// Segment powers.  The meter's blocks (400 ms every 100 ms, 3 s every 100 ms) are sums of 100 ms segments, segment j being
// samples [s_j, s_j+1), s_j = j fs div 10.  So the signal is read for ONE thing: sum y^2 per (clip, channel, segment), y
// the K-weighted signal, a cascade of two biquads in float64 from rest.  y never goes to memory.  The three passes are
// those of sosfilt_causal.hip over the same chunks (sosfilt_scan.h: 256 samples a chunk, a lane a chunk, 64 chunks a
// wave, tiles of 32 samples through LDS with two tiles of loads in flight):
//   pass A  every chunk from a zero state -> its zero-state end state
//   pass B  sos::scan_rows, s <- A^CS s + zs: every chunk's true initial state (in segments for rows above 256 chunks)
//   pass C  every chunk again from its true state, squaring.  fs >= 8000 makes a segment at least 800 samples, so a chunk
//           straddles at most one boundary: a lane writes two partial sums, in front of and behind its cut
//   reduce  a thread per (row, segment) adds the partial sums of the chunks that touch the segment, ascending
// Only the samples below s_n_seg (n_seg = 10 L div fs whole segments) are read: no block reaches further.  Chunk c is
// samples [256 c, 256 c + 256) of the row wherever the row lies, every sum has a fixed order and nothing is atomic: a call
// repeats its bits and a batch equals its rows.
//
// Blocks and gates.  A workgroup per clip turns the [C, n_seg] segment powers into the momentary and short-term rows
// (float32 LUFS, -inf where the power is 0), the integrated loudness (both gates in float64, wave sums of common.h, the four
// waves folded in index order) and the threshold the loudness range gates its short-term values with.  The range itself
// is picked from the SORTED short-term row by a second small kernel (the sort is the caller's: 1/4800 of the input).
//
// True peak.  max |resample_poly(x, up, 1)| without the oversampled signal: resample.hip's arithmetic at down = 1 (the
// span staged in LDS, float32 fma chain with the taps ascending, so every value is the one that kernel would have
// written), a thread running the `up` phases of one input position side by side; |y| is reduced per thread, per wave, per
// workgroup, and per clip by an integer max on the bit pattern, which has no order.
//
// Gain.  g = 10^((target - I) / 20), lowered to the peak limit, 1 where I is not finite, computed per clip on the device
// and applied by a kernel that takes the gains from that vector: nothing between measuring and scaling waits on the host.
#include "host.h"
#include "sosfilt_scan.h"
#include <math.h>
#include <string.h>

namespace syg {
namespace {

using namespace sos;

constexpr int LD_FS_MIN = 8000, LD_FS_MAX = 384000;
constexpr int LD_MOMENTARY = 4, LD_SHORT_TERM = 30;    // segments of a block
constexpr int TP_TILE = 1024, TP_THREADS = 256;        // input positions a true-peak workgroup stages at a time
constexpr int TP_TILES = 4;                            // tiles it walks before its one atomic
constexpr int TP_UP_MAX = 4, TP_KP_MAX = 64;           // phases, taps per phase at most
constexpr int GAIN_PER = 4, GAIN_THREADS = 256;
constexpr int BLK_THREADS = 256;                       // threads of the blocks-and-gates workgroup (its sums fold four waves)

struct KCoef {
  double b0[2], b1[2], b2[2], a1[2], a2[2];            // a0 = 1
};

__host__ __device__ __forceinline__ int64_t seg_start(int64_t j, int fs) { return j * fs / 10; }

// ---- pass A (MODE 0: zero state, writes end states) and pass C (MODE 1: true state, writes the partial sums)
//   init  [rows, nch, 4] true initial states (chunk 0 starts from rest);  zs  [rows, nch, 4];  part  [rows, nch, 2]
//   Le    samples of a row that are read (s_n_seg)
template <int MODE>
__global__ __launch_bounds__(64) void loud_chunk_kernel(const float* x, int64_t sb, int64_t sc, int C, int nch, int64_t Le,
                                                        int fs, KCoef P, const double* __restrict__ init,
                                                        double* __restrict__ zs, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float tile[64 * LSTR];
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.y;
  const int c0 = blockIdx.x * 64;
  const int c = c0 + lane;
  const float* inb = x + (row / C) * sb + (row % C) * sc;
  double z0[2] = {0.0, 0.0}, z1[2] = {0.0, 0.0};
  int cut = CS;                                        // first sample of the chunk that belongs to the next segment
  if (MODE == 1 && c < nch) {
    if (c > 0) {
      const double* ip = init + (row * nch + c) * 4;
      z0[0] = ip[0]; z1[0] = ip[1]; z0[1] = ip[2]; z1[1] = ip[3];
    }
    const int64_t n0 = (int64_t)c * CS;
    const int64_t e = seg_start((10 * n0 + 9) / fs + 1, fs) - n0;       // (10 n + 9) div fs: the segment of sample n
    cut = e < CS ? (int)e : CS;
  }
  auto load_tile = [&](int j0, float4 (&v)[8]) {       // 8 lanes x 16 bytes cover one chunk's 32 samples
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int ch = r * 8 + (lane >> 3), part4 = lane & 7;
      v[r] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c0 + ch < nch) {
        const int64_t i0 = (int64_t)(c0 + ch) * CS + j0 + 4 * part4;
        if (i0 + 3 < Le) {
          const f4u q = *reinterpret_cast<const f4u*>(inb + i0);
          v[r] = make_float4(q.x, q.y, q.z, q.w);
        } else {                                       // nothing behind sample Le - 1 is read
          if (i0 < Le) v[r].x = inb[i0];
          if (i0 + 1 < Le) v[r].y = inb[i0 + 1];
          if (i0 + 2 < Le) v[r].z = inb[i0 + 2];
        }
      }
    }
  };
  auto step = [&](double u) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const double yv = fma(P.b0[s], u, z0[s]);
      z0[s] = fma(P.b1[s], u, fma(-P.a1[s], yv, z1[s]));
      z1[s] = fma(P.b2[s], u, -P.a2[s] * yv);
      u = yv;
    }
    return u;
  };
  double acc = 0.0, head = 0.0;                        // head: the sum in front of the cut, once the cut is passed
  auto square = [&](double u, int j) {
    const double yv = step(u);
    if (MODE == 1) {
      const bool at = j == cut;
      head = at ? acc : head;
      acc = at ? 0.0 : acc;
      acc = fma(yv, yv, acc);
    }
  };
  float4 nxt[8], nx2[8];
  load_tile(0, nxt);
  load_tile(TS, nx2);
  for (int j0 = 0; j0 < CS; j0 += TS) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int ch = r * 8 + (lane >> 3), part4 = lane & 7;
      *reinterpret_cast<float4*>(&tile[ch * LSTR + 4 * part4]) = nxt[r];
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) nxt[r] = nx2[r];
    if (j0 + 2 * TS < CS) load_tile(j0 + 2 * TS, nx2);
    wave_lds_sync();
    const float* trow = &tile[lane * LSTR];
#pragma unroll 2
    for (int j = 0; j < TS; j += 4) {
      const float4 q = *reinterpret_cast<const float4*>(trow + j);
      square((double)q.x, j0 + j);
      square((double)q.y, j0 + j + 1);
      square((double)q.z, j0 + j + 2);
      square((double)q.w, j0 + j + 3);
    }
    wave_lds_sync();
  }
  if (c < nch) {
    if (MODE == 0) {
      double* zp = zs + (row * nch + c) * 4;
      zp[0] = z0[0]; zp[1] = z1[0]; zp[2] = z0[1]; zp[3] = z1[1];
    } else {
      double* pp = part + (row * nch + c) * 2;
      pp[0] = cut < CS ? head : acc;
      pp[1] = cut < CS ? acc : 0.0;
    }
  }
}

// ---- reduce: seg[row, j] = the partial sums of the chunks that touch segment j, chunks ascending
__global__ __launch_bounds__(256) void loud_reduce_kernel(const double* __restrict__ part, int nch, int n_seg, int fs,
                                                          int64_t rows, double* __restrict__ seg) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * n_seg) return;
  const int64_t row = i / n_seg;
  const int j = (int)(i % n_seg);
  const int64_t sj = seg_start(j, fs), sn = seg_start(j + 1, fs);
  const int c_lo = (int)(sj / CS), c_hi = (int)((sn - 1) / CS);         // c_hi < nch: s_n_seg is the last sample read
  const double* pp = part + row * nch * 2;
  double acc = 0.0;
  for (int c = c_lo; c <= c_hi; ++c) acc += pp[2 * c + ((int64_t)c * CS >= sj ? 0 : 1)];
  seg[i] = acc;
}

__device__ __forceinline__ double lufs(double z) { return z > 0.0 ? -0.691 + 10.0 * log10(z) : -INFINITY; }

// sums over a workgroup of BLK_THREADS: the wave sums of common.h, then the waves in index order
static_assert(BLK_THREADS == 256, "block_sum_* fold four waves");
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ int block_sum_i(int v, int* sh) {
  v = wave_sum_i(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const int r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return r;
}

// ---- blocks and gates: one workgroup per clip
//   seg [B, C, n_seg];  w [C];  M [B, n_m], S [B, n_s] (row strides ldm, lds), integ [B], lra_thr [B]: any may be null
__global__ __launch_bounds__(BLK_THREADS) void loud_blocks_kernel(const double* __restrict__ seg, int C, int n_seg, int fs,
                                                                  const double* __restrict__ w, float* __restrict__ M,
                                                                  int64_t ldm, float* __restrict__ S, int64_t lds,
                                                                  double* __restrict__ integ, double* __restrict__ lra_thr) {
  __shared__ double shd[BLK_THREADS / 64];
  __shared__ int shi[BLK_THREADS / 64];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const double* sp = seg + b * C * n_seg;
  auto power = [&](int j, int K) {                     // block j of K segments: channels ascending, segments ascending
    double z = 0.0;
    for (int c = 0; c < C; ++c) {
      double a = 0.0;
      for (int k = 0; k < K; ++k) a += sp[(int64_t)c * n_seg + j + k];
      z = fma(w[c], a, z);
    }
    return z / (double)(seg_start(j + K, fs) - seg_start(j, fs));
  };
  // the relative threshold: `below` LU under the power-mean of the blocks above the absolute gate (+inf: there is none)
  auto gate = [&](int K, int nb, double below, float* rowp) {
    double s1 = 0.0;
    int n1 = 0;
    for (int j = tid; j < nb; j += BLK_THREADS) {
      const double z = power(j, K), l = lufs(z);
      if (rowp) rowp[j] = (float)l;
      if (l > -70.0) { s1 += z; ++n1; }
    }
    const double sum = block_sum_d(s1, shd);
    const int cnt = block_sum_i(n1, shi);
    return cnt ? lufs(sum / cnt) - below : INFINITY;
  };
  const int n_m = n_seg >= LD_MOMENTARY ? n_seg - LD_MOMENTARY + 1 : 0;
  const int n_s = n_seg >= LD_SHORT_TERM ? n_seg - LD_SHORT_TERM + 1 : 0;
  const double gamma = gate(LD_MOMENTARY, n_m, 10.0, M ? M + b * ldm : nullptr);
  if (integ) {
    double s2 = 0.0;
    int n2 = 0;
    for (int j = tid; j < n_m; j += BLK_THREADS) {
      const double z = power(j, LD_MOMENTARY), l = lufs(z);
      if (l > -70.0 && l > gamma) { s2 += z; ++n2; }
    }
    s2 = block_sum_d(s2, shd);
    n2 = block_sum_i(n2, shi);
    if (tid == 0) integ[b] = n2 ? lufs(s2 / n2) : -INFINITY;
  }
  if (S || lra_thr) {
    const double rel = gate(LD_SHORT_TERM, n_s, 20.0, S ? S + b * lds : nullptr);
    if (tid == 0 && lra_thr) lra_thr[b] = rel > -70.0 ? rel : -70.0;
  }
}

// ---- loudness range from the ascending short-term row: the values above thr are its last n; EBU Tech 3342's two
// percentiles by nearest rank, floor((n - 1) p + 1/2) in integers
__global__ __launch_bounds__(64) void loud_lra_kernel(const float* __restrict__ S, int64_t n_s, int64_t lds,
                                                      const double* __restrict__ thr, float* __restrict__ lra) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const float* sp = S + b * lds;
  const double t = thr[b];
  int n = 0;
  for (int64_t j = lane; j < n_s; j += 64) n += (double)sp[j] > t ? 1 : 0;
  n = wave_sum_i(n);
  if (lane == 0) {
    float v = 0.f;
    if (n >= 2) {
      const int64_t lo = n_s - n, hi95 = ((int64_t)(n - 1) * 19 + 10) / 20, lo10 = ((int64_t)(n - 1) + 5) / 10;
      v = sp[lo + hi95] - sp[lo + lo10];
    }
    lra[b] = v;
  }
}

// ---- true peak: the bit pattern of max |y| per clip (over its channels), y = resample_poly(x, UP, 1) value for value.
// With t = n + n_pre_remove, output n is phase p = t mod UP of input position q = t div UP: y = sum_j tab[p][j] x~[q - j].
// A thread takes one q and runs its UP phases side by side: one LDS read of x~[q - j] feeds UP fmas, and the taps are the
// same for every lane (scalar loads).  A workgroup walks TP_TILES tiles of TP_TILE positions, staging each tile's span
// (zeros outside the row), and ends in ONE integer atomic: a clip of 2^24 samples ends in 4096 of them.
template <int UP>
__global__ __launch_bounds__(TP_THREADS) void true_peak_kernel(const float* x, int64_t sb, int64_t sc, int C, int64_t L,
                                                               int64_t npr, int Kp, const float* __restrict__ tab,
                                                               unsigned* __restrict__ peak) {
  __shared__ float xs[TP_TILE + TP_KP_MAX];
  __shared__ int wmax[TP_THREADS / 64];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.y, b = row / C;
  const float* __restrict__ xr = x + b * sb + (row % C) * sc;
  const int64_t t_lo = npr, t_hi = npr + L * UP;       // the t of the outputs that exist
  const int64_t q_lo = t_lo / UP, q_end = (t_hi - 1) / UP + 1;
  int m = 0;                                           // bits of a non-negative float order as integers; a NaN tops them
  for (int it = 0; it < TP_TILES; ++it) {
    const int64_t qt = q_lo + ((int64_t)blockIdx.x * TP_TILES + it) * TP_TILE;
    if (qt >= q_end) break;                            // (uniform)
    const int cnt = (int)(q_end - qt < TP_TILE ? q_end - qt : TP_TILE);
    if (UP == 1) {                                     // the sample peak: n_pre_remove = 0, q = n
      for (int i = tid; i < cnt; i += TP_THREADS) m = max(m, __float_as_int(fabsf(xr[qt + i])));
    } else {
      __syncthreads();                                 // the tile before has been read
      const int64_t lo = qt - (Kp - 1);
      for (int s = tid; s < cnt + Kp - 1; s += TP_THREADS) xs[s] = (lo + s >= 0 && lo + s < L) ? xr[lo + s] : 0.f;
      __syncthreads();
      for (int i = tid; i < cnt; i += TP_THREADS) {
        const float* xp = xs + i + Kp - 1;
        float acc[UP];
#pragma unroll
        for (int p = 0; p < UP; ++p) acc[p] = 0.f;
        for (int j = 0; j < Kp; ++j) {
          const float v = xp[-j];
#pragma unroll
          for (int p = 0; p < UP; ++p) acc[p] = fmaf(tab[p * Kp + j], v, acc[p]);
        }
#pragma unroll
        for (int p = 0; p < UP; ++p) {
          const int64_t t = (qt + i) * UP + p;
          if (t >= t_lo && t < t_hi) m = max(m, __float_as_int(fabsf(acc[p])));
        }
      }
    }
  }
  m = -wave_min_i(-m);
  if ((tid & 63) == 0) wmax[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) atomicMax(peak + b, (unsigned)max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3])));
}

// ---- gain of every clip, and its application
__global__ __launch_bounds__(256) void loud_gain_kernel(const double* __restrict__ integ, const float* __restrict__ tp, int64_t B,
                                                        double target, double limit_lin, double* __restrict__ gain) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const double I = integ[b];
  double g = 1.0;
  if (isfinite(I)) {
    g = pow(10.0, (target - I) / 20.0);
    if (tp && g * (double)tp[b] > limit_lin) g = limit_lin / (double)tp[b];
  }
  gain[b] = g;
}

__global__ __launch_bounds__(GAIN_THREADS) void gain_rows_kernel(const float* x, int64_t sb, int64_t sc, int C, int64_t L,
                                                                 const double* __restrict__ gain, float* y, int64_t yb,
                                                                 int64_t yc) {
  const int64_t row = blockIdx.y, b = row / C, ch = row % C;
  const float* xr = x + b * sb + ch * sc;
  float* yr = y + b * yb + ch * yc;
  const double g = gain[b];
  const int64_t i0 = ((int64_t)blockIdx.x * GAIN_THREADS + threadIdx.x) * GAIN_PER;
  if (i0 + GAIN_PER <= L) {
    const f4u q = *reinterpret_cast<const f4u*>(xr + i0);
    f4u o;
    o.x = (float)((double)q.x * g); o.y = (float)((double)q.y * g);
    o.z = (float)((double)q.z * g); o.w = (float)((double)q.w * g);
    *reinterpret_cast<f4u*>(yr + i0) = o;
  } else {
    for (int64_t i = i0; i < L; ++i) yr[i] = (float)((double)xr[i] * g);
  }
}

int64_t whole_segments(int64_t L, int fs) { return L * 10 / fs; }
int64_t chunks(int64_t n) { return (n + CS - 1) / CS; }
// clips of one launch: the grid's second dimension holds their rows
int64_t clips_per_launch(int64_t B, int64_t C) { return piece_rows(0, B, MAX_GRID_Y / C); }
// bad B / C / L / strides of a [B, C, L] input; `who` names the entry point
int check_clips(const char* who, int64_t B, int64_t C, int64_t L, int64_t sb, int64_t sc) {
  SYG_REQUIRE(B >= 1 && C >= 1 && C <= MAX_GRID_Y && L >= 1 && L < ((int64_t)1 << 40),
              "%s: bad B / C / L (B >= 1, C in [1, %lld], L in [1, 2^40); got B=%lld, C=%lld, L=%lld)", who,
              (long long)MAX_GRID_Y, (long long)B, (long long)C, (long long)L);
  SYG_REQUIRE(sb >= 0 && sc >= 0 && (C == 1 || sc >= L || sc == 0) && (B == 1 || sb >= L || sb == 0),
              "%s: bad strides (sb=%lld, sc=%lld for L=%lld: rows may repeat or lie apart, not overlap)", who, (long long)sb,
              (long long)sc, (long long)L);
  return SYG_OK;
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_loudness_constants(int key) {
  switch (key) {
    case SYG_LOUDNESS_CHUNK: return CS;
    case SYG_LOUDNESS_FS_MIN: return LD_FS_MIN;
    case SYG_LOUDNESS_FS_MAX: return LD_FS_MAX;
    case SYG_LOUDNESS_MOMENTARY: return LD_MOMENTARY;
    case SYG_LOUDNESS_SHORT_TERM: return LD_SHORT_TERM;
    case SYG_LOUDNESS_TP_TILE: return TP_TILE;
    case SYG_LOUDNESS_TP_UP_MAX: return TP_UP_MAX;
    case SYG_LOUDNESS_TP_KP_MAX: return TP_KP_MAX;
    default: set_error("loudness: unknown key %d", key); return -1;
  }
}

extern "C" int64_t syg_loudness_segments_work_bytes(int64_t B, int64_t C, int64_t L, int fs) {
  if (B < 1 || C < 1 || C > MAX_GRID_Y || L < 1 || L >= ((int64_t)1 << 40) || fs < LD_FS_MIN || fs > LD_FS_MAX) return -1;
  const int64_t n_seg = whole_segments(L, fs);
  if (n_seg == 0) return 0;
  const int64_t rows = clips_per_launch(B, C) * C, nch = chunks(seg_start(n_seg, fs));
  // per chunk: zero-state end state, true initial state (4 each), two partial sums; per segment of a long row's scan
  // (at least AHEAD chunks): its end and its start
  return rows * (nch * 10 + 2 * ((nch + AHEAD - 1) / AHEAD) * 4) * (int64_t)sizeof(double);
}

extern "C" int syg_loudness_segments_f32(const float* x, int64_t B, int64_t C, int64_t L, int64_t sb, int64_t sc, int fs,
                                         const double* sos_host, double* seg, void* work, void* stream) {
  SYG_REQUIRE(x && sos_host, "loudness_segments: null pointer argument (x, sos_host)");
  if (const int rc = check_clips("loudness_segments", B, C, L, sb, sc)) return rc;
  SYG_REQUIRE(fs >= LD_FS_MIN && fs <= LD_FS_MAX, "loudness_segments: fs=%d is not served (integer rates from %d to %d Hz)", fs,
              LD_FS_MIN, LD_FS_MAX);
  for (int s = 0; s < 2; ++s) SYG_REQUIRE(sos_host[6 * s + 3] != 0.0, "loudness_segments: a0 of section %d is zero", s);
  const int64_t n_seg = whole_segments(L, fs);
  if (n_seg == 0) return SYG_OK;                       // shorter than a segment: nothing to write
  SYG_REQUIRE(seg && work, "loudness_segments: null pointer argument (seg, work)");
  const int64_t Le = seg_start(n_seg, fs);
  SYG_REQUIRE(chunks(Le) <= (int64_t)1 << 24, "loudness_segments: L=%lld is above 2^32 samples", (long long)L);
  const int nch = (int)chunks(Le);
  KCoef P;
  double sos5[10];
  for (int s = 0; s < 2; ++s) {
    const double* c = sos_host + 6 * s;
    P.b0[s] = sos5[5 * s + 0] = c[0] / c[3];
    P.b1[s] = sos5[5 * s + 1] = c[1] / c[3];
    P.b2[s] = sos5[5 * s + 2] = c[2] / c[3];
    P.a1[s] = sos5[5 * s + 3] = c[4] / c[3];
    P.a2[s] = sos5[5 * s + 4] = c[5] / c[3];
  }
  CausalPow A, AG;
  double A1[MAXD * MAXD];
  one_step_matrix(sos5, 2, A1);
  mat_pow(A1, 4, CS, A.apow);
  const int G = scan_segment(nch), nseg = (nch + G - 1) / G;
  mat_pow(A.apow, 4, G, AG.apow);
  hipStream_t st = (hipStream_t)stream;
  const int64_t per = clips_per_launch(B, C);
  for (int64_t b0 = 0; b0 < B; b0 += per) {
    const int64_t nb = piece_rows(b0, B, per), rows = nb * C;
    const float* xb = x + b0 * sb;
    double* zs = (double*)work;                        // [rows, nch, 4]
    double* init = zs + rows * nch * 4;                // [rows, nch, 4]
    double* part = init + rows * nch * 4;              // [rows, nch, 2]
    double* ends = part + rows * nch * 2;              // [rows, nseg, 4]
    double* segs = ends + rows * nseg * 4;             // [rows, nseg, 4]
    const dim3 g((unsigned)((nch + 63) / 64), (unsigned)rows);
    hipLaunchKernelGGL((loud_chunk_kernel<0>), g, dim3(64), 0, st, xb, sb, sc, (int)C, nch, Le, fs, P, (const double*)nullptr, zs,
                       (double*)nullptr);
    scan_rows<2>(rows, nch, A, AG, zs, init, ends, segs, st);
    hipLaunchKernelGGL((loud_chunk_kernel<1>), g, dim3(64), 0, st, xb, sb, sc, (int)C, nch, Le, fs, P, (const double*)init,
                       (double*)nullptr, part);
    hipLaunchKernelGGL(loud_reduce_kernel, dim3((unsigned)ceil_div(rows * n_seg, 256)), dim3(256), 0, st, (const double*)part, nch,
                       (int)n_seg, fs, rows, seg + b0 * C * n_seg);
    SYG_CHECK_LAUNCH("loudness_segments");
  }
  return SYG_OK;
}

extern "C" int syg_loudness_blocks_f64(const double* seg, int64_t B, int64_t C, int64_t n_seg, int fs, const double* weights,
                                       float* M, int64_t ldm, float* S, int64_t lds, double* integ, double* lra_thr,
                                       void* stream) {
  SYG_REQUIRE(weights && (seg || n_seg == 0), "loudness_blocks: null pointer argument (seg, weights)");
  SYG_REQUIRE(B >= 1 && B < 0x7fffffff && C >= 1 && C <= MAX_GRID_Y && n_seg >= 0 && n_seg < ((int64_t)1 << 30),
              "loudness_blocks: bad B / C / n_seg (got B=%lld, C=%lld, n_seg=%lld)", (long long)B, (long long)C, (long long)n_seg);
  SYG_REQUIRE(fs >= LD_FS_MIN && fs <= LD_FS_MAX, "loudness_blocks: fs=%d is not served (integer rates from %d to %d Hz)", fs,
              LD_FS_MIN, LD_FS_MAX);
  const int64_t n_m = n_seg >= LD_MOMENTARY ? n_seg - LD_MOMENTARY + 1 : 0;
  const int64_t n_s = n_seg >= LD_SHORT_TERM ? n_seg - LD_SHORT_TERM + 1 : 0;
  SYG_REQUIRE((!M || ldm >= n_m) && (!S || lds >= n_s), "loudness_blocks: ldm=%lld / lds=%lld below the rows' %lld / %lld blocks",
              (long long)ldm, (long long)lds, (long long)n_m, (long long)n_s);
  hipLaunchKernelGGL(loud_blocks_kernel, dim3((unsigned)B), dim3(BLK_THREADS), 0, (hipStream_t)stream, seg, (int)C, (int)n_seg, fs,
                     weights, M, ldm, S, lds, integ, lra_thr);
  SYG_CHECK_LAUNCH("loudness_blocks");
  return SYG_OK;
}

extern "C" int syg_loudness_lra_f32(const float* s_sorted, int64_t B, int64_t n_s, int64_t lds, const double* thr, float* lra,
                                    void* stream) {
  SYG_REQUIRE(thr && lra && (s_sorted || n_s == 0), "loudness_lra: null pointer argument (s_sorted, thr, lra)");
  SYG_REQUIRE(B >= 1 && B < 0x7fffffff && n_s >= 0 && n_s < ((int64_t)1 << 30) && lds >= n_s,
              "loudness_lra: bad B / n_s / lds (got B=%lld, n_s=%lld, lds=%lld)", (long long)B, (long long)n_s, (long long)lds);
  hipLaunchKernelGGL(loud_lra_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, s_sorted, n_s, lds, thr, lra);
  SYG_CHECK_LAUNCH("loudness_lra");
  return SYG_OK;
}

extern "C" int syg_true_peak_f32(const float* x, int64_t B, int64_t C, int64_t L, int64_t sb, int64_t sc, int up,
                                 int64_t n_pre_remove, int Kp, const float* table, float* peak, void* stream) {
  SYG_REQUIRE(x && peak, "true_peak: null pointer argument (x, peak)");
  if (const int rc = check_clips("true_peak", B, C, L, sb, sc)) return rc;
  SYG_REQUIRE(up >= 1 && up <= TP_UP_MAX, "true_peak: up=%d must be in [1, %d]", up, TP_UP_MAX);
  SYG_REQUIRE(up == 1 || (table && Kp >= 1 && Kp <= TP_KP_MAX && n_pre_remove >= 0 && n_pre_remove < ((int64_t)1 << 30)),
              "true_peak: up > 1 needs the table [up, Kp], Kp in [1, %d], and n_pre_remove >= 0 (got Kp=%d)", TP_KP_MAX, Kp);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(peak, 0, (size_t)B * sizeof(float), st) != hipSuccess) {
    set_error("true_peak: cannot clear the result: %s", hipGetErrorString(hipGetLastError()));
    return SYG_E_LAUNCH;
  }
  // positions q = t div up of the outputs t = n + n_pre_remove, n < L up
  const int64_t nq = (n_pre_remove + L * up - 1) / up - n_pre_remove / up + 1;
  const int64_t gx = ceil_div(nq, (int64_t)TP_TILE * TP_TILES), per = clips_per_launch(B, C);
  SYG_REQUIRE(gx < 0x7fffffff, "true_peak: too many tiles");
  void (*k)(const float*, int64_t, int64_t, int, int64_t, int64_t, int, const float*, unsigned*) =
      up == 1 ? true_peak_kernel<1> : up == 2 ? true_peak_kernel<2> : up == 3 ? true_peak_kernel<3> : true_peak_kernel<4>;
  for (int64_t b0 = 0; b0 < B; b0 += per) {
    const int64_t nb = piece_rows(b0, B, per);
    hipLaunchKernelGGL(k, dim3((unsigned)gx, (unsigned)(nb * C)), dim3(TP_THREADS), 0, st, x + b0 * sb, sb, sc, (int)C, L,
                       up == 1 ? (int64_t)0 : n_pre_remove, Kp, table, (unsigned*)peak + b0);
    SYG_CHECK_LAUNCH("true_peak");
  }
  return SYG_OK;
}

extern "C" int syg_loudness_gain_f64(const double* integ, const float* peak, int64_t B, double target_lufs, double limit_dbtp,
                                     double* gain, void* stream) {
  SYG_REQUIRE(integ && gain, "loudness_gain: null pointer argument (integ, gain)");
  SYG_REQUIRE(B >= 1 && B < ((int64_t)1 << 38), "loudness_gain: bad B=%lld", (long long)B);
  SYG_REQUIRE(isfinite(target_lufs) && (!peak || isfinite(limit_dbtp)), "loudness_gain: target and peak limit must be finite");
  hipLaunchKernelGGL(loud_gain_kernel, dim3((unsigned)ceil_div(B, 256)), dim3(256), 0, (hipStream_t)stream, integ, peak, B,
                     target_lufs, peak ? pow(10.0, limit_dbtp / 20.0) : 0.0, gain);
  SYG_CHECK_LAUNCH("loudness_gain");
  return SYG_OK;
}

extern "C" int syg_gain_rows_f32(const float* x, int64_t B, int64_t C, int64_t L, int64_t sb, int64_t sc, const double* gain,
                                 float* y, int64_t yb, int64_t yc, void* stream) {
  SYG_REQUIRE(x && gain && y, "gain_rows: null pointer argument (x, gain, y)");
  if (const int rc = check_clips("gain_rows", B, C, L, sb, sc)) return rc;
  SYG_REQUIRE((C == 1 || yc >= L) && (B == 1 || yb >= L), "gain_rows: the result's rows overlap (yb=%lld, yc=%lld for L=%lld)",
              (long long)yb, (long long)yc, (long long)L);
  const int64_t gx = ceil_div(L, (int64_t)GAIN_THREADS * GAIN_PER), per = clips_per_launch(B, C);
  SYG_REQUIRE(gx < 0x7fffffff, "gain_rows: too many tiles");
  for (int64_t b0 = 0; b0 < B; b0 += per) {
    const int64_t nb = piece_rows(b0, B, per);
    hipLaunchKernelGGL(gain_rows_kernel, dim3((unsigned)gx, (unsigned)(nb * C)), dim3(GAIN_THREADS), 0, (hipStream_t)stream,
                       x + b0 * sb, sb, sc, (int)C, L, gain + b0, y + b0 * yb, yb, yc);
    SYG_CHECK_LAUNCH("gain_rows");
  }
  return SYG_OK;
}
