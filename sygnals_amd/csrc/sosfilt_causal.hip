// Causal SOS filtering with state in and out (scipy.signal.sosfilt(sos, x, zi=zi) semantics) for a batch of rows.
//
// The cascade is direct-form II transposed; zi / zf are scipy's (z0, z1) per section, kept on the DEVICE in float64, so
// the zf of one block is the zi of the next and a stream runs block after block without a host round trip.  Recurrences
// and states are float64, signals float32 (why: header of sosfilt.hip).
//
// One sweep of sosfilt.hip's chunked scheme (geometry and scan step shared through sosfilt_scan.h):
//   pass A  every chunk of CS samples runs from a zero state -> its zero-state end state; chunk 0 runs from zi[b], so
//           what it reports is already the true state at the start of chunk 1
//   pass B  a serial scan per row, s <- A^CS s + zs, gives every chunk its true initial state (rows of more than 256
//           chunks: in segments, three short scans instead of one long one)
//   pass C  every chunk re-runs from the true state and writes y in place order; the lane that holds sample L - 1
//           writes its state right behind that sample to zf
// A row of at most one chunk is pass C alone (its initial state is zi[b]).
//
// What differs from the zero-phase form, besides one sweep, no odd extension and no reversal: chunk c is samples
// [c CS, (c + 1) CS) of the row WHATEVER the row's address.  The zero-phase form shifts its grid by the row's
// misalignment so that every tile load is a whole 128-byte line; here that would make the place where the float64 scan
// is cut -- and with it the last bit of a float32 output -- depend on where a row happens to lie, and a batch has to
// equal its rows bit for bit.  So tile accesses are 16 bytes per lane at 4-byte alignment: whole lines for rows that
// lie on 16-byte boundaries (every row of a contiguous batch whose length is a multiple of 4), two lines per 8-lane
// segment otherwise.  A wave owns 64 consecutive chunks of one row and moves 64 x 32-sample tiles through LDS
// (lane-major rows of 36 floats) with two tiles of loads in flight; one wave per workgroup, ordering inside the wave
// replaces barriers.  No atomics, nothing waits on another workgroup: the same call gives the same bits.
//
// More than MAXS = 8 sections run as consecutive groups of at most 8 (a causal cascade composes exactly): group 0 reads
// x and writes y, every later group filters y in place, each with its own slice of zi / zf.  y may alias x: a wave
// reads a tile of its own chunks before it writes it, and no other wave touches those chunks in that launch.
#include "host.h"
#include "sosfilt_scan.h"
#include <string.h>

namespace syg {
namespace {

using namespace sos;

constexpr int MAX_SECTIONS = 32;     // sections per call: four groups of MAXS

struct CausalCoef {
  double b0[MAXS], b1[MAXS], b2[MAXS], a1[MAXS], a2[MAXS];   // a0 = 1
};

// ---- pass A (MODE 0: zero state, writes end states) and pass C (MODE 1: true state, writes y and zf)
//   zi / zf   this group's slice of the [B, n_sections, 2] states, row stride ldz doubles; either may be null
//   init      [B, nch, 2 S] true initial states (pass C of more than one chunk; chunk 0 always starts from zi)
template <int S, int MODE>
__global__ __launch_bounds__(64) void causal_chunk_kernel(const float* in, int64_t ldin, int nch, int64_t L,
                                                          CausalCoef P, const double* __restrict__ zi, int64_t ldz,
                                                          const double* __restrict__ init, double* __restrict__ zs,
                                                          float* y, int64_t ldy, double* __restrict__ zf) {
  __shared__ __attribute__((aligned(16))) float tile[64 * LSTR];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.y;
  const int c0 = blockIdx.x * 64;
  const int c = c0 + lane;
  const float* inb = in + b * ldin;
  const int c_last = (int)((L - 1) / CS), j_last = (int)((L - 1) % CS);     // where sample L - 1 lies
  double z0[S], z1[S];
#pragma unroll
  for (int s = 0; s < S; ++s) { z0[s] = 0.0; z1[s] = 0.0; }
  if (c == 0) {
    if (zi) {
      const double* ip = zi + b * ldz;
#pragma unroll
      for (int s = 0; s < S; ++s) { z0[s] = ip[2 * s]; z1[s] = ip[2 * s + 1]; }
    }
  } else if (MODE != 0 && c < nch) {
    const double* ip = init + ((int64_t)b * nch + c) * (2 * S);
#pragma unroll
    for (int s = 0; s < S; ++s) { z0[s] = ip[2 * s]; z1[s] = ip[2 * s + 1]; }
  }
  // cooperative load of one 64-chunk x 32-sample tile: 8 lanes x 16 bytes cover one chunk's 32 samples
  auto load_tile = [&](int j0, float4 (&v)[8]) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int ch = r * 8 + (lane >> 3), part = lane & 7;
      v[r] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c0 + ch < nch) {
        const int64_t i0 = (int64_t)(c0 + ch) * CS + j0 + 4 * part;
        if (i0 + 3 < L) {
          const f4u q = *reinterpret_cast<const f4u*>(inb + i0);
          v[r] = make_float4(q.x, q.y, q.z, q.w);
        } else {                                         // the row's last samples: nothing behind L - 1 is read
          if (i0 < L) v[r].x = inb[i0];
          if (i0 + 1 < L) v[r].y = inb[i0 + 1];
          if (i0 + 2 < L) v[r].z = inb[i0 + 2];
        }
      }
    }
  };
  auto step = [&](double u) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const double yv = fma(P.b0[s], u, z0[s]);
      z0[s] = fma(P.b1[s], u, fma(-P.a1[s], yv, z1[s]));
      z1[s] = fma(P.b2[s], u, -P.a2[s] * yv);
      u = yv;
    }
    return u;
  };
  float4 nxt[8], nx2[8];                 // two tiles in flight: the passes are bound by memory latency, not arithmetic
  load_tile(0, nxt);
  load_tile(TS, nx2);
  for (int j0 = 0; j0 < CS; j0 += TS) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int ch = r * 8 + (lane >> 3), part = lane & 7;
      *reinterpret_cast<float4*>(&tile[ch * LSTR + 4 * part]) = nxt[r];
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) nxt[r] = nx2[r];
    if (j0 + 2 * TS < CS) load_tile(j0 + 2 * TS, nx2);
    wave_lds_sync();
    float* row = &tile[lane * LSTR];
    // the one tile of the one wave that sample L - 1 falls into is walked sample by sample, and the lane that holds
    // that sample hands its state over right behind it (what this lane computes from there on is never stored)
    if (MODE == 1 && c0 + 64 > c_last && j0 <= j_last && j_last < j0 + TS) {   // (c0 <= c_last: c_last is the last chunk)
      for (int j = 0; j < TS; ++j) {
        row[j] = (float)step((double)row[j]);
        if (c == c_last && j0 + j == j_last && zf) {
          double* zp = zf + b * ldz;
#pragma unroll
          for (int s = 0; s < S; ++s) { zp[2 * s] = z0[s]; zp[2 * s + 1] = z1[s]; }
        }
      }
    } else {
#pragma unroll 2
      for (int j = 0; j < TS; j += 4) {
        const float4 q = *reinterpret_cast<const float4*>(row + j);
        const float o0 = (float)step((double)q.x), o1 = (float)step((double)q.y), o2 = (float)step((double)q.z),
                    o3 = (float)step((double)q.w);
        if (MODE != 0) *reinterpret_cast<float4*>(row + j) = make_float4(o0, o1, o2, o3);
      }
    }
    if (MODE != 0) {
      wave_lds_sync();
      float* yb = y + b * ldy;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int ch = r * 8 + (lane >> 3), part = lane & 7;
        if (c0 + ch < nch) {
          const float4 v = *reinterpret_cast<const float4*>(&tile[ch * LSTR + 4 * part]);
          const int64_t i0 = (int64_t)(c0 + ch) * CS + j0 + 4 * part;
          if (i0 + 3 < L) {
            f4u o; o.x = v.x; o.y = v.y; o.z = v.z; o.w = v.w;
            *reinterpret_cast<f4u*>(yb + i0) = o;
          } else {
            if (i0 < L) yb[i0] = v.x;
            if (i0 + 1 < L) yb[i0 + 1] = v.y;
            if (i0 + 2 < L) yb[i0 + 2] = v.z;
          }
        }
      }
    }
    wave_lds_sync();
  }
  if (MODE == 0 && c < nch) {
    double* zp = zs + ((int64_t)b * nch + c) * (2 * S);
#pragma unroll
    for (int s = 0; s < S; ++s) { zp[2 * s] = z0[s]; zp[2 * s + 1] = z1[s]; }
  }
}

int64_t chunks(int64_t L) { return (L + CS - 1) / CS; }

// one group of S sections over rows [0, B): `in` -> y (in may be y).  AG = A^(CS G) (two-level scan only)
template <int S>
int launch_group(const float* in, int64_t B, int64_t L, int64_t ldin, const CausalCoef& P, const CausalPow& A,
                 const CausalPow& AG, const double* zi, double* zf, int64_t ldz, float* y, int64_t ldy, void* work,
                 hipStream_t st) {
  constexpr int D = 2 * S;
  const int nch = (int)chunks(L);
  const int G = scan_segment(nch), nseg = (nch + G - 1) / G;
  const unsigned gx = (unsigned)((nch + 63) / 64);
  for (int64_t b0 = 0; b0 < B; b0 += MAX_GRID_Y) {                 // one grid dimension's worth of rows per launch
    const int64_t nb = piece_rows(b0, B, MAX_GRID_Y);
    const float* inb = in + b0 * ldin;
    float* yb = y + b0 * ldy;
    const double* zib = zi ? zi + b0 * ldz : nullptr;
    double* zfb = zf ? zf + b0 * ldz : nullptr;
    double* zs = (double*)work;                                    // [nb, nch, D]
    double* init = zs + nb * (int64_t)nch * D;                     // [nb, nch, D]
    double* ends = init + nb * (int64_t)nch * D;                   // [nb, nseg, D]
    double* segs = ends + nb * (int64_t)nseg * D;                  // [nb, nseg, D]
    const dim3 g(gx, (unsigned)nb);
    if (nch > 1) {
      hipLaunchKernelGGL((causal_chunk_kernel<S, 0>), g, dim3(64), 0, st, inb, ldin, nch, L, P, zib, ldz,
                         (const double*)nullptr, zs, (float*)nullptr, (int64_t)0, (double*)nullptr);
      scan_rows<S>(nb, nch, A, AG, zs, init, ends, segs, st);
    }
    hipLaunchKernelGGL((causal_chunk_kernel<S, 1>), g, dim3(64), 0, st, inb, ldin, nch, L, P, zib, ldz,
                       (const double*)init, (double*)nullptr, yb, ldy, zfb);
    SYG_CHECK_LAUNCH("sosfilt");
  }
  return SYG_OK;
}

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int64_t syg_sosfilt_constants(int which) {
  switch (which) {
    case 0: return CS;             // samples per chunk
    case 1: return TS;             // samples per tile
    case 2: return 64;             // chunks per wave
    case 3: return AHEAD;          // chunk states the scan keeps in flight
    case 4: return MAXS;           // sections per group
    case 5: return MAX_SECTIONS;   // sections per call
    case 6: return TWO_LEVEL;      // chunks of a row above which the scan runs in segments
    default: set_error("sosfilt: unknown key %d (0 chunk, 1 tile, 2 chunks per wave, 3 scan look-ahead, 4 sections per "
                       "group, 5 sections per call, 6 chunks above which the scan runs in segments)", which);
      return -1;
  }
}

extern "C" int64_t syg_sosfilt_work_bytes(int64_t B, int64_t L, int n_sections) {
  if (B < 1 || L < 1 || n_sections < 1 || n_sections > MAX_SECTIONS) return -1;
  const int64_t rows = grid_rows(B);                               // rows of one launch; groups and launches reuse it
  const int S = n_sections < MAXS ? n_sections : MAXS;
  const int64_t nch = chunks(L);
  // zero-state end states + true initial states per chunk, and the same two per segment of the long rows' scan (a
  // segment is at least AHEAD chunks)
  return 2 * rows * (nch + (nch + AHEAD - 1) / AHEAD) * 2 * S * (int64_t)sizeof(double);
}

extern "C" int syg_sosfilt_f32(const float* x, int64_t B, int64_t L, int64_t ldx, const double* sos_host, int n_sections,
                               const double* zi, float* y, int64_t ldy, double* zf, void* work, void* stream) {
  SYG_REQUIRE(x && y && sos_host, "sosfilt: null pointer argument (x, sos_host, y)");
  SYG_REQUIRE(n_sections >= 1 && n_sections <= MAX_SECTIONS, "sosfilt: n_sections must be in [1, %d] (got %d)",
              MAX_SECTIONS, n_sections);
  SYG_REQUIRE(L >= 1, "sosfilt: L must be at least 1 (got %lld)", (long long)L);
  SYG_REQUIRE(B >= 1 && ldx >= L && ldy >= L, "sosfilt: bad B / ldx / ldy (B=%lld, L=%lld, ldx=%lld, ldy=%lld)",
              (long long)B, (long long)L, (long long)ldx, (long long)ldy);
  SYG_REQUIRE(chunks(L) <= (int64_t)1 << 24, "sosfilt: L=%lld is above 2^32 samples", (long long)L);
  for (int s = 0; s < n_sections; ++s)
    SYG_REQUIRE(sos_host[6 * s + 3] != 0.0, "sosfilt: a0 of section %d is zero", s);
  SYG_REQUIRE(work || chunks(L) == 1, "sosfilt: rows of more than %d samples need the work buffer of syg_sosfilt_work_bytes", CS);
  hipStream_t st = (hipStream_t)stream;
  const int64_t ldz = 2 * (int64_t)n_sections;
  for (int s0 = 0; s0 < n_sections; s0 += MAXS) {
    const int S = (n_sections - s0 < MAXS) ? (n_sections - s0) : MAXS;
    CausalCoef P;
    CausalPow A, AG;
    memset(&P, 0, sizeof(P));
    double sos5[5 * MAXS];
    for (int s = 0; s < S; ++s) {
      const double* c = sos_host + 6 * (s0 + s);
      P.b0[s] = sos5[5 * s + 0] = c[0] / c[3];
      P.b1[s] = sos5[5 * s + 1] = c[1] / c[3];
      P.b2[s] = sos5[5 * s + 2] = c[2] / c[3];
      P.a1[s] = sos5[5 * s + 3] = c[4] / c[3];
      P.a2[s] = sos5[5 * s + 4] = c[5] / c[3];
    }
    double A1[MAXD * MAXD];
    one_step_matrix(sos5, S, A1);
    mat_pow(A1, 2 * S, CS, A.apow);
    const int G = scan_segment((int)chunks(L));
    mat_pow(A.apow, 2 * S, G, AG.apow);                            // A^(CS G): one step of the scan over segments
    const float* in = (s0 == 0) ? x : y;                           // later groups filter y in place
    const int64_t ldin = (s0 == 0) ? ldx : ldy;
    const double* zig = zi ? zi + 2 * s0 : nullptr;
    double* zfg = zf ? zf + 2 * s0 : nullptr;
    int rc;
    switch (S) {
      case 1: rc = launch_group<1>(in, B, L, ldin, P, A, AG, zig, zfg, ldz, y, ldy, work, st); break;
      case 2: rc = launch_group<2>(in, B, L, ldin, P, A, AG, zig, zfg, ldz, y, ldy, work, st); break;
      case 3: rc = launch_group<3>(in, B, L, ldin, P, A, AG, zig, zfg, ldz, y, ldy, work, st); break;
      case 4: rc = launch_group<4>(in, B, L, ldin, P, A, AG, zig, zfg, ldz, y, ldy, work, st); break;
      case 5: rc = launch_group<5>(in, B, L, ldin, P, A, AG, zig, zfg, ldz, y, ldy, work, st); break;
      case 6: rc = launch_group<6>(in, B, L, ldin, P, A, AG, zig, zfg, ldz, y, ldy, work, st); break;
      case 7: rc = launch_group<7>(in, B, L, ldin, P, A, AG, zig, zfg, ldz, y, ldy, work, st); break;
      default: rc = launch_group<8>(in, B, L, ldin, P, A, AG, zig, zfg, ldz, y, ldy, work, st); break;
    }
    if (rc != SYG_OK) return rc;
  }
  return SYG_OK;
}
