// Fused STFT(2048) -> power -> mel (-> dB -> DCT) kernel for gfx950 (MI355X).
//
// One persistent workgroup of W waves (W = 16: one per CU; W = 8: two) walks a contiguous chunk of tiles; a tile
// is W consecutive frames of one clip, one frame per wave.  Per tile (two barriers):
//   FFT      the tile's contiguous sample run was copied into LDS by LDS-DMA (buffer_load ... lds; the buffer
//            descriptor's range check supplies center=True's zero padding) while the previous tile was being
//            processed; each wave takes its (overlapped) frame from there, applies the analysis window (LDS copy)
//            and runs a 1024-point complex FFT held 16 points per lane (radix 16 x 16 x 4).  The two exchanges go
//            through a 4.1 KiB per-wave scratch that aliases the wave's own power row, in two half-rounds each:
//            lane-indexed planar stores (ds_write_addtid_b32) and full-wave ds_read_b64 of writer-lane pairs,
//            conflict-free under the per-instruction LDS banking, the lane pair (L, L + 32) completing each
//            other's rows with v_permlane32_swap.  Real-FFT split on mirror
//            pairs, |X|^2 stored as one skewed 1025-bin row.
//   barrier A
//   project  the W power rows are the B operand of v_mfma_f32_16x16x4_f32: the mel filterbank is stored
//            block-sparse (per 16-mel tile only its non-zero bin range), split over the waves, four k-steps per
//            16-byte load (pre-loaded behind barrier A); then the next frame is fetched LDS -> registers.
//   barrier B
//   reduce   the DMA of the tile after next is started; partial 16 x W tiles are combined in a fixed order
//            (deterministic) into mel[b, m, t] or the clip's LDS mel matrix.
// That is the matrix form of the projection.  What a launch does beyond the transform is its Mode (the enumeration and
// its table of properties, mode_traits(), stand in front of the kernel; kernel and launcher read nothing else):
//   MODE name          waves   entry point: what it does
//    0   Mel           8 | 16  syg_stft2048_mel_f32: mel by weight matrix -> mel[b, m, t]
//    1   MelRows       8 | 16  ... with stats_out / contrast_out: + per-frame statistics and contrast tail means from the
//                              same LDS rows, behind barrier B (the "row functions", row_features.h)
//    2   Complex       8       syg_stft2048_c2c_f32: complex STFT output, nothing projected
//    3   ClipMatrix    16      syg_stft2048_mfcc_f32: MODE 0 into the clip's LDS mel matrix; at a clip's last tile
//                              power_to_db + DCT-II inside the next tile's projection phase -- only MFCCs are written
//    6   ClipSeg       16      syg_stft2048_mfcc_tri_f32: MODE 3 with the projection by segment sums, one wave per row
//                              (tri_project: no weight matrix, no barrier A, no slab)
//    7   ClipSegRows   16      syg_stft2048_features_tri_f32: MODE 6 + the row functions, MFCC, statistics and contrast
//                              rows from one launch; syg_stft2048_stats_f32: the same without a table, row functions alone
//    8   TileSeg4      8 | 16  syg_stft2048_mel_tri_f32, n_segtab = 2048: the tile form of MODE 6 with a FOUR-pass table (up
//                              to 256 pieces) -- every frame's mel column straight to HBM, tiles shared out evenly over the
//                              workgroups, no clip epilogue;   9 TileSeg4Rows: + the row functions
//   10   TileSeg2      8 | 16  ... n_segtab = 1024: MODE 8 with the TWO-pass table of MODE 6;  11 TileSeg2Rows: + row functions
// Every (waves, mode) is built for the three frame load paths (LOAD 0 / 1 / 2, see fetch_frame()); MODE 6 also has the
// free-running form LOAD 3: no stage buffer, every wave prefetches its next frame from global memory under its own
// projection and the workgroup meets once per clip (syg_stft2048_mfcc_tri_freerun() says where it is used), and LOAD 4: the
// same without that barrier, a clip handed over by counters in LDS (SYG_OPT_STFT_MEET chooses between the two).
// Nothing but the input samples and the outputs touches HBM.
//
// Reference behaviour reproduced: librosa.stft (center zero padding, periodic window, rfft) -> np.abs ->
// **2 -> melspectrogram -> power_to_db(ref=np.max) -> mfcc, as called from sygnals/core/features/manager.py:184-187,
// 198, 219-223 and cepstral.py:106-115; per-frame statistics follow sygnals/core/features/frequency_domain.py:24-386.
// Index maps and LDS bank behaviour are validated by tools/wave_fft_model_v5.py.
#include "stft_host.h"
#include <stdlib.h>

// Issue priority falls as a wave advances through its frame: the SIMD's arbiter otherwise favours the oldest
// wave, which then idles at barrier A while the youngest finishes alone with nothing to hide its LDS latency.
#define SETPRIO(n) __builtin_amdgcn_s_setprio(n)
// -DSYG_DEV=1: per-phase cycle stamps (tools/timeline.py; a development build -- syg_build_variant() != 0 -- whose
// statistics output carries the counters)
#include "stft_dev.h"

// (buffer_load_dwordx2 by the compiler's own intrinsic, so that it counts the loads in its waits; the 8-byte builtin of
// this toolchain, __builtin_amdgcn_raw_buffer_load_b64, compiles to a 4-byte load)
typedef float syg_v2f __attribute__((ext_vector_type(2)));
__device__ syg_v2f syg_raw_buffer_load_v2f(__amdgpu_buffer_rsrc_t rs, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.ptr.buffer.load.v2f32");

namespace syg {
namespace {

constexpr int NFFT = 2048;
constexpr int MC = 1024;         // complex points per frame
constexpr int NBIN = 1025;
constexpr int MAXW = 16;         // waves per workgroup (8 or 16)
constexpr int P_STRIDE = 1090;   // == 2 (mod 32): conflict-free MFMA B-operand reads; rows are skewed, see ppos()
constexpr int SC_COMPLEX = 528;  // per-wave exchange scratch: 528 complex = 4224 B (16 rows of 256 B + skew)
constexpr int TW2_STRIDE = 18;   // complex entries per lane class (16 + 2 pad: distinct banks)
constexpr int TW2_FLOATS = 4 * TW2_STRIDE * 2;
constexpr int TW1_FLOATS = 15 * 64 * 2;

// Block-sparse filterbank plan for v_mfma_f32_4x4x1_16b_f32 (sygnals_amd/_tables.py: pack_mel_plan): the mel rows are
// taken in groups of four; the non-zero bin range of a group is cut into chunks of at most `steps` bins, one chunk per
// (wave, slot) -- a wave runs four slots side by side, one bin per slot and step.  The tables sit behind the packed
// weights in the same device buffer (int32, 4 x 64 entries from `table_off`, in floats):
//   [0, 64) first row POSITION ppos(bin) of slot (wave * 4 + s)   [64, 128) mel group of the slot (-1: unused)
//   [128, 192) first slot of mel group g          [192, 256) number of slots of group g
struct MelPlan {
  int steps;        // row positions per slot = MFMA steps per wave and tile (a multiple of 4, at least 28)
  int n_groups;     // mel groups of four rows
  int table_off;    // offset (in floats) of the tables inside wpacked
};
constexpr int MTAB_INTS = 256;
constexpr int SEGTAB_WORDS = 2 * 2 * 64 * 4;   // piece table of the segment-sum projection (pack_mel_segments), two passes
constexpr int SEGTAB4_WORDS = 2 * SEGTAB_WORDS; // ... four passes (MODE 8 / 9: filterbanks of up to 256 pieces, e.g. 128 bands)
constexpr int TRI4_ROW_BASE = 4;               // the four-pass tables are built with row_base = 4 (a short first piece needs room
                                               // for its lead): the projection reads from 4 words in front of the power row

struct ContrastPlan {
  int n_rows;
  int ascending;     // 1: lo[] and hi[] are non-decreasing (a band never starts below an earlier band's start)
  int lo[SYG_MAX_BANDS];
  int hi[SYG_MAX_BANDS];
  int k[SYG_MAX_BANDS];
};

typedef float v4f __attribute__((ext_vector_type(4)));

#include "row_features.h"

// MODE 3 (clip-resident MFCC): the mel tiles of a clip stay in LDS; after the clip's last tile the workgroup
// converts them to dB (per-clip max reference, top_db floor) and applies the DCT -- only MFCCs reach HBM.
struct MfccArgs {
  const float* dct;      // [n_mfcc, n_mels]
  const float* lifter;   // [n_mfcc] or null
  float* out;            // [B, n_mfcc, T]
  int n_mfcc;
  int ref_is_max;        // 1: reference = max of the clip's mel powers, 0: ref_value
  float ref_value, amin, top_db;   // top_db < 0: no floor
  int tp;                // padded frames per clip (tiles_per_clip * TILE_T): row stride of the LDS mel matrix
  int rows_per_clip;     // rows between two clips of `out` (n_mfcc, or more when the MFCCs are the head of a wider block)
};

// The two exchanges are lane-indexed (ds_write_addtid_b32: a store writes one 64-float ROW, float L from lane L, at
// M0 + an immediate offset -- no address VGPR and 2 LDS cycles for 256 B, against 6 for a ds_write_b64).  A complex
// register goes out as two planar rows (re, im); a ds_read_b64 then fetches one component of the writer lanes
// (2m, 2m + 1).  The lanes' roles are chosen so that the operands a reader needs together sit in such lane pairs, and
// the rows are spaced so that every read is conflict-free (tools/wave_fft_model_v5.py):
//   pass 1   lane l holds column b = p1col(l) = 4 a + b' with a = l & 15, b' = (l >> 4) ^ ((l >> 2) & 2)
//   exch. 1  row r, plane p at float X1_ROW r + 64 p (one 8-byte bank slot of skew per row)
//   pass 2   lane L holds (c = 8 (L >> 5) + c7, b'): rho = (L >> 1) & 7 = ((c7 & 3) << 1) | (c7 >> 2),
//            b' = 2 ((L >> 4) & 1) + (L & 1) -- the b' = 0, 1 and b' = 2, 3 of one c are lane pairs
//   exch. 2  row c' & 7, plane p at float X2_ROW (c' & 7) + 64 p (two slots of skew per row)
//   units    u = lane + 64 j: c = UNIT_C[u >> 3], c' = u & 7; each 32-lane group holds four c closed under the
//            mirror c -> 16 - c and under c -> c + 8, which is what makes exchange 2's reads conflict-free
constexpr int X1_ROW = 130;      // floats; 8 rows x 2 planes end at float 1038 <= 2 * SC_COMPLEX
constexpr int X2_ROW = 132;      // floats; ... at float 1052
static_assert(7 * X1_ROW + 128 <= 2 * SC_COMPLEX && 7 * X2_ROW + 128 <= 2 * SC_COMPLEX, "exchange rows must fit the scratch");
constexpr unsigned long long UNIT_C = 0xdb53ea62f971c840ull;   // nibble i: c of units 8 i .. 8 i + 7
__device__ __forceinline__ int p1col(int l) { return 4 * (l & 15) + ((l >> 4) ^ ((l >> 2) & 2)); }
__device__ __forceinline__ int x2rho(int c7) { return ((c7 & 3) << 1) | (c7 >> 2); }
// exchange-2 read position (float, plane 0, b' = 0) of group (c, c')
__device__ __forceinline__ int x2g(int c, int cp) { return X2_ROW * (cp & 7) + 32 * (c >> 3) + 2 * x2rho(c & 7); }

// The eight complex registers x[0..7] as 16 lane-indexed rows: x[r].x at byte ROW * 4 r, x[r].y 256 bytes behind it,
// from M0 = m0 (the LDS byte address of the scratch).  M0 is set here and clobbered: the compiler re-loads it for its
// own users (the stage buffer's LDS-DMA).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"     // (M0 is a reserved register: the clobber is what makes the
template <int ROW>                                  //  compiler set it again before its own M0 users)
__device__ __forceinline__ void addtid_rows(uint32_t m0, const float2* x) {
#define SYG_ADDTID(d, o) "ds_write_addtid_b32 %" #d " offset:%" #o "\n\t"
  asm volatile("s_mov_b32 m0, %0\n\t"
               "s_nop 0\n\t"             // (an M0 write needs one wait state before an LDS add-TID instruction reads it)
               SYG_ADDTID(1, 17) SYG_ADDTID(2, 25)
               SYG_ADDTID(3, 18) SYG_ADDTID(4, 26)
               SYG_ADDTID(5, 19) SYG_ADDTID(6, 27)
               SYG_ADDTID(7, 20) SYG_ADDTID(8, 28)
               SYG_ADDTID(9, 21) SYG_ADDTID(10, 29)
               SYG_ADDTID(11, 22) SYG_ADDTID(12, 30)
               SYG_ADDTID(13, 23) SYG_ADDTID(14, 31)
               SYG_ADDTID(15, 24) SYG_ADDTID(16, 32)
               :: "s"(m0), "v"(x[0].x), "v"(x[0].y), "v"(x[1].x), "v"(x[1].y), "v"(x[2].x), "v"(x[2].y),
                  "v"(x[3].x), "v"(x[3].y), "v"(x[4].x), "v"(x[4].y), "v"(x[5].x), "v"(x[5].y), "v"(x[6].x),
                  "v"(x[6].y), "v"(x[7].x), "v"(x[7].y),
                  "n"(0), "n"(4 * ROW), "n"(8 * ROW), "n"(12 * ROW), "n"(16 * ROW), "n"(20 * ROW), "n"(24 * ROW),
                  "n"(28 * ROW), "n"(256), "n"(4 * ROW + 256), "n"(8 * ROW + 256), "n"(12 * ROW + 256),
                  "n"(16 * ROW + 256), "n"(20 * ROW + 256), "n"(24 * ROW + 256), "n"(28 * ROW + 256)
               : "memory", "m0");
#undef SYG_ADDTID
}
#pragma clang diagnostic pop

struct LaneConst {
  float2 twb[2];     // W_2048^kb of each unit (kb = c + 16 c'); pair d uses twb * W_8^d
  float2 cA2, cA3;   // unit-0 multipliers for d = 2, 3: W_8^2, W_8^3 -- except lane 0 (see below)
  int pkb[2];        // ppos(kb): pair d of a regular unit sits at pkb + 272 d (its mirror at pmb - 272 d)
  int pmb[2];        // ppos(1024 - kb)
  int dA2, dA3;      // unit-0 position offsets for d = 2, 3 (544, 816 -- except lane 0)
  int kb[2];         // kb (complex-output mode)
  int g0[2], g1[2];  // exchange-2 read position of the primary (c' < 8) / mirror (c' >= 8) group
};

// unit u = lane + 64 j: primary group (c = UNIT_C[u >> 3], c' = u & 7), bins k = kb + 256 d; mirror group
// (16 - c, 15 - c') holds bins 1024 - k, with the c = 0 exceptions (0, 16 - c') and, for u = 0 (lane 0), the
// self-mirrored pair of groups (0,0) / (0,8) whose four pairs are the bins {0, 256, 128, 384} (+ bin 512).
// TWB: also fetch twb from the twiddle table (false: the caller keeps twb and re-makes the rest -- lane arithmetic only)
template <bool TWB = true>
__device__ __forceinline__ void init_lane_const(LaneConst& lc, int lane, const float2* __restrict__ twid) {
  constexpr float C1 = 0.92387953251128673848f, S1 = 0.38268343236508977173f, R = 0.70710678118654752440f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = (int)((uint32_t)(UNIT_C >> (32 * j)) >> (4 * (lane >> 3))) & 15, cp = lane & 7;
    int cm = 16 - c, cmp = 15 - cp;
    if (c == 0) { cm = 0; cmp = (cp == 0) ? 8 : 16 - cp; }
    lc.g0[j] = x2g(c, cp);
    lc.g1[j] = x2g(cm, cmp);
    const int kb = c + 16 * cp;
    lc.kb[j] = kb;
    lc.pkb[j] = ppos(kb);
    lc.pmb[j] = ppos(MC - kb);
    if (TWB) lc.twb[j] = twid[kb];
  }
  const bool sp = (lane == 0);
  lc.cA2 = sp ? make_float2(C1, -S1) : make_float2(0.f, -1.f);   // W_2048^128 = W_16^1   |  W_8^2
  lc.cA3 = sp ? make_float2(S1, -C1) : make_float2(-R, -R);      // W_2048^384 = W_16^3   |  W_8^3
  lc.dA2 = sp ? ppos(128) : 544;
  lc.dA3 = sp ? ppos(384) : 816;
}

// 1024-point complex forward FFT of the windowed frame + real split.  v[a] holds z[64a + p1col(lane)] on entry.
// On exit pair (j, d) holds X[k] in xs[j][d] and X[1024 - k] in xm[j][d] (k = kb_j + 256 d; lane 0 / unit 0:
// k = 0, 256, 128, 384); lane 0 also returns X[512].
// PD: priority drop (MODE 1 keeps the top level for its row functions, the transform then runs one level lower)
// X2: return 2 X instead of X (the two halvings of the real split are left out; the caller's powers are then 4 |X|^2 --
// an exact scaling that the mel-only modes take back where the mel values leave the kernel: 32 instructions per frame)
template <int PD = 0, bool X2 = false>
__device__ __forceinline__ void wave_rfft2048(float2 (&v)[16], const LaneConst& lc, float2* __restrict__ sc,
                                             const float2* __restrict__ tw1l, const float2* __restrict__ tw2l,
                                             int lane, float2 (&xs)[2][4], float2 (&xm)[2][4], float2& x512 TARGS) {
  // this lane's roles (see the maps above X1_ROW): pass-1 column, pass-2 (c7 = c & 7, b', upper half-wave)
  const int col = p1col(lane);
  const int hi = lane >> 5, rho = (lane >> 1) & 7, bp = ((lane >> 3) & 2) | (lane & 1);
  const int c7 = (rho >> 1) | ((rho & 1) << 2);
  const float* scf = reinterpret_cast<const float*>(sc);
  typedef __attribute__((address_space(3))) const float* lds_cfptr;
  const uint32_t m0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_cfptr)scf);
  // ---- pass 1: radix-16 over a (stride 64), twiddle W_1024^(b*c)
  dft16(v);
#pragma unroll
  for (int c = 1; c < 16; ++c) v[c] = cmul(v[c], tw1l[(c - 1) * 64 + col]);
  // ---- exchange 1 in two half-rounds.  Round h moves the 8 ROWS c = 8h..8h+7 (lane-indexed, 16 stores).  A pass-2
  // lane (c, b') needs the 16 operands y[c][4a + b'] of ONE row, which only one of the rounds holds: in round h the
  // lane pair (L, L + 32) shares the reading of row c7 + 8h -- L takes a = 0..7, L + 32 takes a = 8..15, four
  // ds_read_b64 per plane, each the operands a = 2i, 2i + 1 of its half (writer lanes 16 (b' ^ 2 hi) + 8 hi + 2i,
  // + 1) -- and v_permlane32_swap then hands each lane the half it is missing (L's round-1 operands <-> (L+32)'s
  // round-0 operands): full-wave stores AND full-wave loads for 16 extra VALU instructions.
  TICK(1, v[1].x);
  float2 t[16];
  {
    const float* rd = scf + X1_ROW * c7 + 8 * hi + 16 * (bp ^ (2 * hi));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      addtid_rows<X1_ROW>(m0, v + 8 * h);
      wave_lds_sync();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // (the empty asm keeps the IR load-store vectorizer from fusing the contiguous 8-byte reads of consecutive i
        // into ds_read2_b64, which runs at half the rate of ds_read_b64 and banks on 32 dwords)
        if (i > 0) asm volatile("" ::: "memory");
        const float2 re = *reinterpret_cast<const float2*>(rd + 2 * i);
        const float2 im = *reinterpret_cast<const float2*>(rd + 64 + 2 * i);
        t[8 * h + 2 * i] = make_float2(re.x, im.x);
        t[8 * h + 2 * i + 1] = make_float2(re.y, im.y);
      }
      wave_lds_sync();
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const auto sx = __builtin_amdgcn_permlane32_swap(__float_as_uint(t[i].x), __float_as_uint(t[8 + i].x), false, false);
      const auto sy = __builtin_amdgcn_permlane32_swap(__float_as_uint(t[i].y), __float_as_uint(t[8 + i].y), false, false);
      t[i] = make_float2(__uint_as_float(sx[0]), __uint_as_float(sy[0]));
      t[8 + i] = make_float2(__uint_as_float(sx[1]), __uint_as_float(sy[1]));
    }
  }
  TICK(2, t[0].x);
  // ---- pass 2: lane = (c, b'); radix-16 over a'
  SETPRIO(2 - PD > 0 ? 2 - PD : 0);
  dft16(t);
  {
    // W_64^(b'*c') from a 64-entry LDS table (4 lane classes): two twiddles per 16-byte read
    // (read through the LDS address space as one native 4-vector: a generic float4 is split into two 8-byte
    // halves and re-fused into ds_read2_b64, which costs twice the LDS cycles of ds_read_b128)
    typedef __attribute__((address_space(3))) const v4f* lds_v4;
    lds_v4 t4 = (lds_v4)(tw2l + bp * TW2_STRIDE);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const v4f tt = t4[m];
      if (m > 0) t[2 * m] = cmul(t[2 * m], make_float2(tt.x, tt.y));
      t[2 * m + 1] = cmul(t[2 * m + 1], make_float2(tt.z, tt.w));
    }
  }
  // ---- exchange 2 in two half-rounds (c' < 8, then c' >= 8); every unit's primary group has c' < 8 and its
  // mirror c' >= 8, so round 0 delivers all primaries and round 1 all mirrors.  A group's four b' are the lane
  // pairs (b' 0, 1) and (2, 3): four ds_read_b64 (two per plane).  Pass 3 = radix-4 over b'.
  TICK(3, t[1].x);
  float2 G[2][4], H[2][4];
  {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      addtid_rows<X2_ROW>(m0, t + 8 * h);
      wave_lds_sync();
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float* p = scf + (h == 0 ? lc.g0[j] : lc.g1[j]);
        const float2 r01 = *reinterpret_cast<const float2*>(p), i01 = *reinterpret_cast<const float2*>(p + 64);
        const float2 r23 = *reinterpret_cast<const float2*>(p + 16), i23 = *reinterpret_cast<const float2*>(p + 80);
        const float2 z0 = make_float2(r01.x, i01.x), z1 = make_float2(r01.y, i01.y);
        const float2 z2 = make_float2(r23.x, i23.x), z3 = make_float2(r23.y, i23.y);
        if (h == 0) bfly4(z0, z1, z2, z3, G[j][0], G[j][1], G[j][2], G[j][3]);
        else bfly4(z0, z1, z2, z3, H[j][0], H[j][1], H[j][2], H[j][3]);
      }
      wave_lds_sync();
    }
  }
  TICK(4, G[0][0].x);
  SETPRIO(1 - PD > 0 ? 1 - PD : 0);
  // ---- real split on mirror pairs
  x512 = X2 ? make_float2(2.f * G[0][2].x, -2.f * G[0][2].y)
            : make_float2(G[0][2].x, -G[0][2].y);      // X[512] = conj(Z[512]) (meaningful in lane 0 only)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    float2 zk[4] = {G[j][0], G[j][1], G[j][2], G[j][3]};
    float2 zm[4] = {H[j][3], H[j][2], H[j][1], H[j][0]};
    if (j == 0) {
      // unit 0 (lane 0) pairs the self-mirrored groups (0,0) and (0,8) differently
      const bool sp = (lane == 0);
      zk[2] = sp ? H[0][0] : zk[2];
      zk[3] = sp ? H[0][1] : zk[3];
      zm[0] = sp ? G[0][0] : zm[0];
      zm[1] = sp ? G[0][3] : zm[1];
      zm[2] = sp ? H[0][3] : zm[2];
      zm[3] = sp ? H[0][2] : zm[3];
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      // E2 = zk + conj(zm), O2 = -i (zk - conj(zm));  X[k] = (E2 + w O2)/2, X[1024-k] = conj(E2 - w O2)/2
      const float2 E = make_float2(zk[d].x + zm[d].x, zk[d].y - zm[d].y);
      const float2 O = make_float2(zk[d].y + zm[d].y, zm[d].x - zk[d].x);
      // w = twb * W_8^d (unit 0, d >= 2: twb * cA_d, which differs in lane 0 only)
      constexpr float R = 0.70710678118654752440f;
      float2 rO;
      if (d == 0) rO = O;
      else if (d == 1) rO = make_float2(R * (O.x + O.y), R * (O.y - O.x));
      else if (j == 0) rO = cmul(O, d == 2 ? lc.cA2 : lc.cA3);
      else if (d == 2) rO = make_float2(O.y, -O.x);
      else rO = make_float2(R * (O.y - O.x), -R * (O.x + O.y));
      const float2 wO = cmul(lc.twb[j], rO);
      if (X2) {
        xs[j][d] = make_float2(E.x + wO.x, E.y + wO.y);
        xm[j][d] = make_float2(E.x - wO.x, wO.y - E.y);
      } else {
        xs[j][d] = make_float2(0.5f * (E.x + wO.x), 0.5f * (E.y + wO.y));
        xm[j][d] = make_float2(0.5f * (E.x - wO.x), -0.5f * (E.y - wO.y));
      }
    }
  }
}

// Raw samples of one frame: element n = 64a + p1col(lane) of the packed complex frame covers samples s0 + 2n,
// s0 + 2n + 1; samples outside [0, L) are the zero padding of center=True.  The loads are only issued here;
// the analysis window (LDS copy) is applied by apply_window() when the frame is consumed.
//   LOAD 0 / 1: straight from global memory (scalar / 8-byte loads)
//   LOAD 2    : from the tile's staged sample run in LDS (filled by LDS-DMA, stage_tile())
//   LOAD 3    : 8-byte buffer loads through the clip's descriptor, whose range check returns the zero padding (as in
//               stage_tile()): one path for every frame.  hop, L and the clip's first sample are even, so a pair of samples
//               is inside or outside as a whole.  Each load's whole byte offset is formed in its address register, where a
//               negative one is a huge unsigned one (an immediate offset added by the hardware could bring it back in range
//               or not, depending on the width of that sum: not relied on).
template <int LOAD>
__device__ __forceinline__ void fetch_frame(float2 (&v)[16], const float* __restrict__ yb, int64_t L, int64_t s0,
                                            const float* __restrict__ stage_frame, int lane) {
  const int col = p1col(lane);
  if (LOAD == 3) {
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(yb), 0, (int)(L * 4), 0x00020000);
    const int base = ((int)s0 + 2 * col) * 4;
#pragma unroll
    for (int a = 0; a < 16; ++a) {
      int off = base + 512 * a;
      asm volatile("" : "+v"(off));
      const syg_v2f r = syg_raw_buffer_load_v2f(rs, off, 0, 0);
      v[a] = make_float2(r.x, r.y);
    }
    return;
  }
  if (LOAD == 2) {
    const float2* sf = reinterpret_cast<const float2*>(stage_frame);
#pragma unroll
    for (int a = 0; a < 16; ++a) v[a] = sf[64 * a + col];
    return;
  }
  const bool interior = (s0 >= 0) && (s0 + NFFT <= L);
  if (interior) {
#pragma unroll
    for (int a = 0; a < 16; ++a) {
      const int n = 64 * a + col;
      if (LOAD == 1) v[a] = *reinterpret_cast<const float2*>(yb + s0 + 2 * n);
      else v[a] = make_float2(yb[s0 + 2 * n], yb[s0 + 2 * n + 1]);
    }
  } else {
#pragma unroll
    for (int a = 0; a < 16; ++a) {
      const int64_t s = s0 + 2 * (64 * a + col);
      v[a].x = (s >= 0 && s < L) ? yb[s] : 0.f;
      v[a].y = (s + 1 >= 0 && s + 1 < L) ? yb[s + 1] : 0.f;
    }
  }
}

__device__ __forceinline__ void apply_window(float2 (&v)[16], const float2* __restrict__ winl, int lane) {
  const int col = p1col(lane);
#pragma unroll
  for (int a = 0; a < 16; ++a) {
    const float2 wv = winl[64 * a + col];
    v[a] = make_float2(v[a].x * wv.x, v[a].y * wv.y);
  }
}

// LDS-DMA of the sample run [s_begin, s_begin + 256 n_chunks) of one clip into the stage buffer: the buffer
// descriptor's range check returns zeros for samples before the clip (negative offsets wrap to huge unsigned
// ones) and past its end -- exactly the zero padding of center=True.  wide: 16 B per lane (needs 16-byte
// aligned runs), else 4 B per lane.
template <int WAVES>
__device__ __forceinline__ void stage_tile(const float* yb, int clip_bytes, float* stage, int s_begin, int span,
                                           bool wide, int w, int lane) {
  typedef __attribute__((address_space(3))) void* lds_ptr;
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(yb), 0, clip_bytes, 0x00020000);
  if (wide) {
    const int n = (span + 255) >> 8;
    for (int c = w; c < n; c += WAVES)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr)(stage + c * 256), 16, (s_begin + c * 256 + lane * 4) * 4,
                                               0, 0, 0);
  } else {
    const int n = (span + 63) >> 6;
    for (int c = w; c < n; c += WAVES)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr)(stage + c * 64), 4, (s_begin + c * 64 + lane) * 4, 0, 0,
                                               0);
  }
}
__device__ __forceinline__ MfccArgs uni(const MfccArgs& a) {
  MfccArgs u;
  u.dct = uni(a.dct); u.lifter = uni(a.lifter); u.out = uni(a.out); u.n_mfcc = uni(a.n_mfcc);
  u.ref_is_max = uni(a.ref_is_max); u.ref_value = uni(a.ref_value); u.amin = uni(a.amin); u.top_db = uni(a.top_db);
  u.tp = uni(a.tp); u.rows_per_clip = uni(a.rows_per_clip);
  return u;
}

// MODE 3 clip epilogue (a workgroup's chunk is whole clips): power_to_db + DCT-II (+ lifter) from the LDS mel
// matrix -- librosa.power_to_db(S, ref=np.max) (manager.py:223) -> scipy.fft.dct rows (cepstral.py:106-115).
// LDS behind the mel matrix: red[WAVES] (per-wave maxima of the clip's mel powers, written at the clip's last
// reduce), then the DCT rows [n_mfcc][n_mels] and the lifter [n_mfcc] (copied once at kernel start).
// The waves that own a 16 x 16 output tile run this in the NEXT tile's projection phase: barrier A of that tile
// orders it behind the last reduce of the clip, barrier B ahead of the next reduce that overwrites the matrix.
// The powers are converted to dB on the fly with the hardware log2: dB = 10 log10(2) (log2 x - log2 ref)
// (v_log_f32, 1 ulp: ~6e-6 dB at -100 dB; inputs are >= amin, never denormal; exactly 0 when x == ref).
// Out of line (inlined, its scalars push the tile loop's SGPRs into spills); uni() re-scalarises the arguments.
typedef __attribute__((address_space(3))) float* lds_fptr;     // (a generic pointer would make every access a flat_*)
// MODE 6 ... 11: the mel projection of ONE power row by ONE wave, by segment sums: tri_project<NPASS>() of mel_segments.h
#include "mel_segments.h"

template <int WAVES>
__device__ __noinline__ void clip_dct(int clipmel_addr, int red_addr, int dct_addr, MfccArgs mfv, int n_mels_v, int T_v, int b_v,
                                      int w_v, int lane, int stride_v = WAVES) {
  const MfccArgs mf = uni(mfv);
  const int n_mels = uni(n_mels_v), T = uni(T_v), w = uni(w_v), stride = uni(stride_v);   // output tiles w, w + stride, ...
  const int64_t b = uni(b_v);
  lds_fptr clipmel = (lds_fptr)(uintptr_t)(uint32_t)uni(clipmel_addr);
  lds_fptr red = (lds_fptr)(uintptr_t)(uint32_t)uni(red_addr);          // [WAVES] per-wave maxima of the clip
  lds_fptr dctl = (lds_fptr)(uintptr_t)(uint32_t)uni(dct_addr);         // [n_mfcc][n_mels] DCT rows, then the lifter
  lds_fptr lifl = dctl + mf.n_mfcc * n_mels;
  // clip maximum: one LDS read per lane (the WAVES per-wave maxima, one per lane of a DPP row) + row reduction
  float m = red[lane & (WAVES - 1)];
  m = fmaxf(m, dpp_f<DPP_QP_1032>(m));
  m = fmaxf(m, dpp_f<DPP_QP_2301>(m));
  m = fmaxf(m, dpp_f<DPP_ROW_HALF_MIRROR>(m));
  m = fmaxf(m, dpp_f<DPP_ROW_MIRROR>(m));
  constexpr float DB_PER_LOG2 = 3.01029995663981195f;
  const float ref = mf.ref_is_max ? m : fabsf(mf.ref_value);
  const float reflog = __builtin_amdgcn_logf(fmaxf(mf.amin, ref));
  // log_spec.max() - top_db, with log_spec monotone in the power
  const float flo = (mf.top_db >= 0.f) ? DB_PER_LOG2 * (__builtin_amdgcn_logf(fmaxf(mf.amin, m)) - reflog) - mf.top_db
                                       : -3.4e38f;
  // out[k, t] = sum_m dct[k, m] * dB[m, t]
  const int ktiles = (mf.n_mfcc + 15) >> 4, ttiles = mf.tp >> 4;
  const int f = lane & 15, g = lane >> 4;
  for (int ot = w; ot < ktiles * ttiles; ot += stride) {
    const int kt = ot / ttiles, tq = ot - kt * ttiles;
    const int krow = kt * 16 + f, tcol = tq * 16 + f;
    v4f acc = {0.f, 0.f, 0.f, 0.f};
    // four steps per round: the operand reads of a round are in flight together (this wave is on the
    // critical path to barrier B)
    for (int m0 = 0; m0 < n_mels; m0 += 16) {
      float a[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int mm = m0 + 4 * i + g;
        const bool ok = mm < n_mels;
        a[i] = (krow < mf.n_mfcc && ok) ? dctl[krow * n_mels + mm] : 0.f;
        bv[i] = ok ? clipmel[mm * mf.tp + tcol] : 1.f;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float db = fmaxf(DB_PER_LOG2 * (__builtin_amdgcn_logf(fmaxf(mf.amin, bv[i])) - reflog), flo);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], db, acc, 0, 0, 0);     // (rows past n_mels: a = 0)
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = kt * 16 + 4 * g + r;
      if (k < mf.n_mfcc && tcol < T) {
        float val = acc[r];
        if (mf.lifter) val *= lifl[k];
        mf.out[(b * mf.rows_per_clip + k) * (int64_t)T + tcol] = val;
      }
    }
  }
}

// LOAD 4 (the free-running form whose waves never meet): a clip's two hand-overs go through counters in LDS that only grow
// (the tile loop says what they count).  A wait is a poll at the lowest issue priority: load, sleep, load again.  It is
// bounded, so that a protocol error shows as NaN in the clip's output and never as a hung device: false when the bound ran out.
// HANDOVER_ROUNDS: the longest single wait at the clip barrier of the barrier form, stamped per wave over the 1024-clip
// launch (tools/timeline.py freerun), was 17.6 k cycles = 8.4 us; a round is s_sleep 8 (512 cycles) + an LDS load, >= 0.3 us
// at 2.1 GHz; 65536 rounds are >= 20 ms = 2400 x that wait, and expire within 50 ms unless a round takes 2.5 x as long.
constexpr int HANDOVER_ROUNDS = 1 << 16;
typedef __attribute__((address_space(3))) int* lds_ctr;
__device__ __forceinline__ int handover_load(lds_ctr c) {
  return __builtin_amdgcn_readfirstlane(__hip_atomic_load(c, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
}
// PRIO_BACK: the level the wave goes on at (< 0: it runs at level 0 throughout)
template <int PRIO_BACK>
__device__ __forceinline__ bool handover_wait(lds_ctr c, int target) {
  if (handover_load(c) >= target) return true;
  if (PRIO_BACK >= 0) SETPRIO(0);
  bool ok = false;
#pragma unroll 1
  for (int r = 0; r < HANDOVER_ROUNDS && !ok; ++r) {
    __builtin_amdgcn_s_sleep(8);
    ok = handover_load(c) >= target;
  }
  if (PRIO_BACK >= 0) SETPRIO(PRIO_BACK);
  return ok;
}
// one lane per wave, behind the wave's own LDS stores and reads (the LDS executes a wave's DS operations in order)
__device__ __forceinline__ void handover_add(lds_ctr c, int lane) {
  if (lane == 0) __hip_atomic_fetch_add(c, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ----------------------------------------------------------------------------------
// LOAD 0 / 1: frames read straight from global memory   LOAD 2: tiles staged in LDS by LDS-DMA (hop <= 512)
//
// LDS map (floats):  Pbuf [TILE_T][P_STRIDE] + 16   power rows; a wave's exchange scratch aliases ITS OWN row
//                                                   (the row is only written after the last scratch read, and
//                                                   nobody reads rows while an FFT phase is running)
//                    slab [WAVES][16][TILE_T]       per-wave partial mel tiles
//                    tw2l, tw1l                     twiddle tables        cpl: contrast plan
//                    winl [2048]                    analysis window
//                    stage [(WAVES-1)*512 + 2048]   the tile's contiguous sample run (LOAD 2)
// Per tile: FFT(v) -> rows | barrier A | MFMA -> slab ; fetch the next frame into v | barrier B |
//           start the DMA of the tile after next ; reduce + store [; statistics | barrier].
// The DMA therefore runs behind the reduce and the whole next FFT phase, and is drained at barrier A.
template <int WAVES, bool SLAB = true, int NPASS = 2>
struct Lds {
  static constexpr int TILE_T = WAVES;
  // (four-pass tables: 16 words in front of the first row, so that row 0's lead words are inside the allocation)
  static constexpr int O_P = (NPASS == 4) ? 16 : 0;
  static constexpr int P_FLOATS = O_P + TILE_T * P_STRIDE + 16;
  static constexpr int SLAB_FLOATS = SLAB ? WAVES * 16 * TILE_T : 0;    // (MODE 6 projects per wave: no partial tiles)
  // contrast plan + the mel plan's slot / group tables; MODE 6: the piece table of the segment-sum projection instead
  static constexpr int SEG_WORDS = NPASS * (SEGTAB_WORDS / 2);
  static constexpr int CPL_FLOATS = SLAB ? 3 * SYG_MAX_BANDS + MTAB_INTS : SEG_WORDS + 3 * SYG_MAX_BANDS;
  static constexpr int STAGE_FLOATS = (WAVES - 1) * 512 + NFFT;
  static constexpr int O_SLAB = P_FLOATS;
  static constexpr int O_TW2 = O_SLAB + SLAB_FLOATS;
  static constexpr int O_TW1 = O_TW2 + TW2_FLOATS;
  static constexpr int O_CPL = O_TW1 + TW1_FLOATS;
  static constexpr int O_WIN = O_CPL + CPL_FLOATS;
  static constexpr int O_STAGE = O_WIN + NFFT;
  static constexpr int TOTAL = O_STAGE + STAGE_FLOATS;
  static_assert(SC_COMPLEX * 2 <= P_STRIDE, "exchange scratch must fit inside a power row");
  static_assert(O_TW2 % 4 == 0 && O_WIN % 4 == 0 && O_STAGE % 4 == 0 && O_CPL % 4 == 0, "16-byte aligned LDS sections");
};

// What a launch does: one enumerator per mode (the numbers are the ones DESIGN.md, profiles/ and the tests speak of), one
// row of properties per enumerator.  A new mode is an enumerator, a row of mode_traits() and an entry point.
enum class Mode : int {    // (what each does, who launches it: the table at the top of the file)
  Mel = 0, MelRows = 1, Complex = 2, ClipMatrix = 3, ClipSeg = 6, ClipSegRows = 7,
  TileSeg4 = 8, TileSeg4Rows = 9, TileSeg2 = 10, TileSeg2Rows = 11,
};
enum class Proj { None, Matrix, Segments };   // nothing / MFMA against the packed weight matrix / tri_project per wave
constexpr bool X2_MEL = true;    // (false: no mode keeps 4 |X|^2 in its power rows)

struct ModeTraits {
  Proj proj;
  int npass;          // passes of the piece table (Segments; the other layouts are those of two passes)
  bool clip;          // the clip's mel matrix lives in LDS (whole clips per workgroup); dB + DCT epilogue at clip end
  bool rowfn;         // the per-frame row functions run
  bool complex_out;
  bool power4;        // the power rows hold 4 |X|^2: wave_rfft2048<.., X2> leaves its halvings out, the factor is taken back
                      // -- exactly, a power of two -- where mel values leave the kernel (at the store; the dB conversion of
                      // a clip works on 4 x mel with 4 x amin and 4 x ref).  The row functions need the true powers.
  bool relc;          // lane constants re-made per frame (see the tile loop)
  bool freerun;       // the 16-wave launch has the free-running form (LOAD 3)
  constexpr bool seg() const { return proj == Proj::Segments; }
  constexpr bool seg_tile() const { return seg() && !clip; }      // the tile form: mel columns to HBM, tiles shared out evenly
  constexpr bool x2() const { return X2_MEL && power4; }
  // mel matrices of a clip-resident mode: the segment form fills one while the DCT of the clip before reads the other
  constexpr int clip_matrices() const { return seg() ? 2 : 1; }
};
constexpr ModeTraits mode_traits(Mode m) {
  switch (m) {                //     proj          npass  clip   rowfn  complex power4 relc   freerun
    case Mode::Mel:          return {Proj::Matrix,   2, false, false, false, true,  false, false};
    case Mode::MelRows:      return {Proj::Matrix,   2, false, true,  false, false, false, false};
    case Mode::Complex:      return {Proj::None,     2, false, false, true,  false, false, false};
    case Mode::ClipMatrix:   return {Proj::Matrix,   2, true,  false, false, true,  false, false};
    case Mode::ClipSeg:      return {Proj::Segments, 2, true,  false, false, true,  false,  true};
    case Mode::ClipSegRows:  return {Proj::Segments, 2, true,  true,  false, false, true, false};
    case Mode::TileSeg4:     return {Proj::Segments, 4, false, false, false, true,  false, false};
    case Mode::TileSeg4Rows: return {Proj::Segments, 4, false, true,  false, false, false, false};
    case Mode::TileSeg2:     return {Proj::Segments, 2, false, false, false, true,  false, false};
    case Mode::TileSeg2Rows: return {Proj::Segments, 2, false, true,  false, false, false, false};
  }
  return {};
}
// the LDS map of a mode (the segment-sum projection has no partial tiles, so no slab)
template <int WAVES, Mode MODE>
using ModeLds = Lds<WAVES, !mode_traits(MODE).seg(), mode_traits(MODE).npass>;

template <int WAVES, int LOAD, Mode MODE>
__global__ __launch_bounds__(WAVES * 64, 4) void stft2048_kernel(
    const float* __restrict__ y, int64_t L, int64_t ldy, int hop, int pad, int64_t T, int tiles_per_clip,
    int64_t total_tiles, int tiles_per_wg, const float2* __restrict__ win2, const float2* __restrict__ twid,
    const float* __restrict__ wpacked, MelPlan plan, int n_mels, float* __restrict__ mel_out, float binhz,
    float roll_percent, float bw_p, int smask, float* __restrict__ stats_out, ContrastPlan cplan,
    float* __restrict__ contrast_out, float2* __restrict__ cout, int dma_wide, MfccArgs mf) {
  constexpr ModeTraits M = mode_traits(MODE);
  constexpr bool TRI = M.seg(), TRIMEL = M.seg_tile();   // per-wave projection by segment sums (tri_project); its tile form
  constexpr int NPASS = M.npass;
  constexpr int TRI_ROW_BASE = (NPASS == 4) ? TRI4_ROW_BASE : 0;
  typedef ModeLds<WAVES, MODE> LM;
  constexpr int SEG_WORDS = LM::SEG_WORDS;
  constexpr int NTHREADS = WAVES * 64;
  constexpr int TILE_T = WAVES;                                    // one frame per wave per tile
  constexpr bool COMPLEX_OUT = M.complex_out, ROWFN = M.rowfn, CLIPM = M.clip, X2 = M.x2();
  // free-running waves: no stage buffer; a wave holds its next frame in registers across its projection (loaded from
  // global memory) and the workgroup meets once per clip
  // LOAD 4: the same, and the workgroup never meets inside the tile loop -- a clip is handed from the waves that fill its
  // matrix to the waves that run its epilogue, and the matrix back, by counters in LDS (NOMEET)
  constexpr bool FREERUN = (LOAD >= 3), NOMEET = (LOAD == 4);
  static_assert(!FREERUN || (M.freerun && WAVES == 16 && TRI && CLIPM && !ROWFN), "LOAD 3 / 4: the free-running forms of the mode");
  constexpr int FLOAD = FREERUN ? 3 : LOAD;      // fetch_frame()'s path
#ifdef SYG_DEV_NO_RELC
  constexpr bool RELC = false;                                       // (timeline builds: round 3's form, for the before / after table)
#else
  constexpr bool RELC = M.relc;
#endif
  constexpr float MELSC = X2 ? 0.25f : 1.f;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* Pbuf = lds + LM::O_P;
  float* slab = lds + LM::O_SLAB;
  float2* tw2l = reinterpret_cast<float2*>(lds + LM::O_TW2);        // [4][18] complex
  float2* tw1l = reinterpret_cast<float2*>(lds + LM::O_TW1);        // [15][64] complex
  int* cpl = reinterpret_cast<int*>(lds + LM::O_CPL);
  int* cplc = TRI ? cpl + SEG_WORDS : cpl;           // contrast plan (MODE 6 ... 9: behind the piece table)
  float2* winl = reinterpret_cast<float2*>(lds + LM::O_WIN);
  float* stage = lds + LM::O_STAGE;
  // MODE 3: [n_mels][mf.tp], red[WAVES], dct rows, lifter -- behind the fixed map; a launch that does not stage its tiles
  // (LOAD != 2) has no stage buffer, the clip's matrix starts there (128-band matrices only fit that way)
  float* clipmel = lds + (LOAD == 2 ? LM::TOTAL : LM::O_STAGE);
  // MODE 6: two mel matrices (the DCT of a clip runs beside the first tile of the next), red[2][WAVES], dct rows, lifter
  float* tri_red = clipmel + 2 * n_mels * mf.tp;
  float* tri_dct = tri_red + 2 * WAVES;

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: keeps frame addressing on the scalar unit

  // persistent workgroup: a contiguous chunk of tiles (consecutive tiles of a clip share part of their
  // samples, so the re-reads of the frame overlap stay in this XCD's L2)
  const int64_t tile_begin = (int64_t)blockIdx.x * tiles_per_wg;
  const int64_t tile_end = (tile_begin + tiles_per_wg < total_tiles) ? tile_begin + tiles_per_wg : total_tiles;
  if (tile_begin >= tile_end) return;

  // tile -> (clip, first frame); total_tiles < 2^31 (checked on the host)
  auto clip_of = [&](int64_t tile) { return (uint32_t)tile / (uint32_t)tiles_per_clip; };
  auto t0_of = [&](int64_t tile, uint32_t cq) {
    return (int64_t)((uint32_t)tile - cq * (uint32_t)tiles_per_clip) * TILE_T;
  };
  const int span = (TILE_T - 1) * hop + NFFT;              // samples a tile touches
  auto dma = [&](int64_t tile) {
    const uint32_t cq = clip_of(tile);
    int ld = lane;
    asm volatile("" : "+v"(ld));      // (per-lane offsets are formed per refill: hoisted out of the tile loop they were spilled)
    stage_tile<WAVES>(y + (int64_t)cq * ldy, (int)(L * 4), stage, (int)(t0_of(tile, cq) * hop) - pad, span,
                      dma_wide != 0, w, ld);
  };
  if (LOAD == 2) dma(tile_begin);

  LaneConst lc;
  init_lane_const(lc, lane, twid);
  float* prow = Pbuf + w * P_STRIDE;
  float2* sc = reinterpret_cast<float2*>(prow);
  if (tid < 64) tw2l[(tid >> 4) * TW2_STRIDE + (tid & 15)] = twid[32 * (tid >> 4) * (tid & 15)];
  for (int i = tid; i < 15 * 64; i += NTHREADS) tw1l[i] = twid[2 * (i & 63) * ((i >> 6) + 1)];
  for (int i = tid; i < NFFT / 2; i += NTHREADS) winl[i] = win2[i];
  if (CLIPM) {
    if (TRI)
      for (int i = tid; i < 2 * n_mels * mf.tp; i += NTHREADS) clipmel[i] = 0.f;
    float* dctl = TRI ? tri_dct : clipmel + n_mels * mf.tp + WAVES;
    for (int i = tid; i < mf.n_mfcc * n_mels; i += NTHREADS) dctl[i] = mf.dct[i];
    if (mf.lifter != nullptr && tid < mf.n_mfcc) dctl[mf.n_mfcc * n_mels + tid] = mf.lifter[tid];
  }

  int* mtab = cpl + 3 * SYG_MAX_BANDS;              // [4][64]: slot first bin, slot group, group first slot, group slots
  if (!COMPLEX_OUT) {
    // pad words of the skewed rows, the row tails and the slack are read against zero weights: they must
    // hold finite values, so the whole buffer (and the slab behind it) is cleared once
    for (int i = tid; i < LM::P_FLOATS + LM::SLAB_FLOATS; i += NTHREADS) lds[i] = 0.f;
    if (TRI && wpacked != nullptr) {                    // (no table: statistics only, nothing is projected)
      // (word 1 of a lane's first 16 bytes: the band it stores -> that band's byte offset inside a mel matrix -- the
      // clip's LDS matrix [n_mels][tp], or (MODE 8 / 9) the clip's [n_mels][T] block of mel_out)
      const int band_bytes = (TRIMEL ? (int)T : mf.tp) * 4;
      for (int i = tid; i < SEG_WORDS; i += NTHREADS) {
        int v = reinterpret_cast<const int*>(wpacked)[i];
        if ((i & 3) == 1 && ((i >> 8) & 1) == 0 && v >= 0) v *= band_bytes;
        cpl[i] = v;
      }
    }
    if (!TRI || ROWFN) {
#pragma unroll
      for (int r = 0; r < SYG_MAX_BANDS; ++r)
        if (tid == r) { cplc[r] = cplan.lo[r]; cplc[SYG_MAX_BANDS + r] = cplan.hi[r]; cplc[2 * SYG_MAX_BANDS + r] = cplan.k[r]; }
    }
    if (!TRI)
      for (int i = tid; i < MTAB_INTS; i += NTHREADS) mtab[i] = reinterpret_cast<const int*>(wpacked)[plan.table_off + i];
  }
  if (NOMEET && tid < 8) cplc[tid] = 0;               // the hand-over counters (below)
  if (LOAD == 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  float cmax = 0.f;       // MODE 3: running maximum of the clip's mel powers produced by this thread
  int64_t pend_b = -1;    // MODE 3: clip whose dB matrix waits for its DCT
  int cur = 0;            // MODE 6: which of the two mel matrices the current clip fills
  // MODE 6: output tiles of the clip epilogue; waves without a frame in a clip's last tile; whether those waves take the
  // epilogue of the clip before (at most three output tiles each: it must stay shorter than a transform)
  bool tri_scan8 = false;
  if (TRI && wpacked != nullptr) {
    unsigned lk = 0;
#pragma unroll
    for (int p = 0; p < NPASS; ++p) lk |= (unsigned)(cpl[4 * (128 * p + lane) + 2] | cpl[4 * (128 * p + lane) + 3]);
    tri_scan8 = __builtin_amdgcn_ballot_w64((lk >> 24) != 0) != 0;
  }
  const int tri_ndct = ((mf.n_mfcc + 15) >> 4) * (mf.tp >> 4);
  const int tri_idle = (TRI && !TRIMEL) ? mf.tp - (int)T : 0;
  const bool tri_defer = TRI && !TRIMEL && tri_idle > 0 && (tri_ndct + tri_idle - 1) / (tri_idle > 0 ? tri_idle : 1) <= 3;
  const int tri_nepi = tri_defer ? tri_idle : (tri_ndct < WAVES ? tri_ndct : WAVES);   // waves that run clip_dct per clip
  // staged mode: the frame of the NEXT tile is fetched (LDS -> registers) one phase ahead, so that the stage
  // buffer can be refilled behind the FFT phase; direct modes load at the top of the tile loop
  float2 v[16];
  bool have = false;
  auto fetch = [&](int64_t tile) {
    const uint32_t cq = clip_of(tile);
    const int64_t t = t0_of(tile, cq) + w;
    have = t < T;
    int lf = lane;                    // laundered like lv below: no hoisted per-lane addresses
    asm volatile("" : "+v"(lf));
    if (have) fetch_frame<FLOAD>(v, y + (int64_t)cq * ldy, L, t * (int64_t)hop - pad, stage + w * hop, lf);
  };
  if (LOAD == 2) {
    fetch(tile_begin);
    __syncthreads();                                  // every wave holds its frame: the stage may be refilled
    if (tile_begin + 1 < tile_end) dma(tile_begin + 1);
  }
  if (FREERUN) fetch(tile_begin);
  // LOAD 4: the hand-over counters, in the words of the contrast plan (this mode has none).  They only grow; a target is
  // formed from the clip's ordinal within the workgroup (kclip), so nothing is ever reset or reused:
  //   filled[p]   + 1 by every wave that is through with a clip that fills matrix p (behind its last column store and its
  //               publish_max(); waves without a frame in the clip's last tile add too).  clip_dct of the n-th clip on p
  //               (n = 0, 1, ...) starts once filled[p] >= 16 (n + 1), wherever it runs.
  //   drained[p]  + 1 by every wave that ran clip_dct on p, behind its last read of the matrix and of red[p][].  tri_nepi
  //               waves run it per clip, so a wave may store into matrix p or red[p][w] for the n-th clip on p once
  //               drained[p] >= tri_nepi n; it checks once per clip, in front of its first projection.
  //   bad         set (never cleared) by a wave whose wait for drained[] ran out: it goes on, and every epilogue that starts
  //               from then on writes NaN (the one it did not wait for is past its check: that clip is not marked).
  // No wait is circular: what a wave of clip c + 2 waits for in drained[] is added by waves running the epilogue of clip
  // c, and those reached that epilogue by passing only waits for clips <= c (their own drained[] waits of clips <= c + 1
  // concern epilogues of clips <= c - 1, and filled[] of clip c needs every wave past clip c only).
  lds_ctr hand = (lds_ctr)cplc;
  lds_ctr filled = hand, drained = hand + 2, bad = hand + 4;
  int kclip = 0;          // LOAD 4: ordinal of the current clip within the workgroup (cur == kclip & 1)

#if SYG_DEV
  unsigned long long tacc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tprev, tmaxw[2] = {0, 0}, tw0;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tprev)::"memory");
#endif
#pragma unroll 1
  for (int64_t tile = tile_begin; tile < tile_end; ++tile) {
    const uint32_t cq = clip_of(tile);
    const int64_t b = cq;
    const int64_t t0 = t0_of(tile, cq);
    const int64_t t = t0 + w;
    if (LOAD < 2) fetch(tile);
    // MODE 1: the row functions behind barrier B are chains of dependent wave-level steps that hide their latency only
    // behind each other; a wave that is through starts its next transform, whose dense vector work would take the
    // issue slots from the waves still in their row functions (oldest wave first at equal priority) and stretch the
    // tile.  The row functions therefore run at the top level and the transform one level lower (all equal: 428 against
    // 373-390 us per 1024 clips of C4; other splits no better).  MODE 0 / 3: projection, clip epilogue and slab combine at
    // the top level, the transform one level lower (150.3 against 151.0 us for the one-launch MFCC at C2).
    constexpr int PD = 1;
    // (LOAD 4, waves that never meet: the same levels -- all equal 151.4, the transform at one constant level below
    // projection and epilogue 148.2, against 127.7 us for these: DESIGN.md section 5.0-nm)
    SETPRIO(3 - PD);
    // The filterbank operands of this wave's slots are the same for every tile but cannot stay resident (the FFT needs
    // all 128 VGPRs): the first NPRE groups of four steps are re-fetched every tile, behind pass 3 of the transform.
    constexpr int NPRE = 7;            // unconditional: every wave's segment holds >= NPRE groups (zero padded); requested
                                       // in front of barrier A (behind pass 3 already: measured, no gain -- the barrier's
                                       // wait covers the latency either way)
    const int ng = plan.steps >> 2;
    const float4* wp4w = reinterpret_cast<const float4*>(wpacked) + (int64_t)w * ng * 64;
    float4 apre[NPRE];
    if (have) {
      // the lane id is laundered through an empty asm each iteration: the LDS / global addresses derived
      // from it are then recomputed per frame (a few integer ops) instead of being hoisted out of the tile
      // loop as ~100 loop-invariant registers that would spill
      int lv = lane;
      asm volatile("" : "+v"(lv));
      // MODE 7 (row functions AND the clip epilogue: the tightest register budget): the 16 integer / constant members of
      // the lane constants are re-made per frame from the laundered lane id (about 40 integer instructions) -- kept live
      // across the out-of-line row functions they pushed a register into scratch, and a scratch reload is a memory round
      // trip that nothing hides (it sat directly behind both call sites: the fixed cost of "any real row function")
      if (RELC) init_lane_const<false>(lc, lv, twid);
      apply_window(v, winl, lv);
#if SYG_DEV
      tw0 = tacc[0];
      TICK(0, v[0].x);
      if (tacc[0] - tw0 > tmaxw[1]) tmaxw[1] = tacc[0] - tw0;
#endif
      float2 xs[2][4], xm[2][4], x512;
      wave_rfft2048<PD, X2>(v, lc, sc, tw1l, tw2l, lv, xs, xm, x512 TPASS);
      if (COMPLEX_OUT) {
        float2* o = cout + (b * T + t) * NBIN;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            int k = lc.kb[u] + 256 * d;
            if (u == 0 && d >= 2 && lane == 0) k = (d == 2) ? 128 : 384;
            o[k] = xs[u][d];
            o[MC - k] = xm[u][d];
          }
        if (lane == 0) o[512] = x512;
      } else {
        int dA2 = lc.dA2, dA3 = lc.dA3;
        // (MODE 7: the four addresses formed from these are summed per frame -- kept across the tile loop they were spilled,
        // and a spill's reload waits for every outstanding memory operation)
        if (TRI && ROWFN) asm volatile("" : "+v"(dA2), "+v"(dA3));
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const int off = (u == 0 && d == 2) ? dA2 : (u == 0 && d == 3) ? dA3 : 272 * d;
            prow[lc.pkb[u] + off] = fmaf(xs[u][d].x, xs[u][d].x, xs[u][d].y * xs[u][d].y);
            prow[lc.pmb[u] - off] = fmaf(xm[u][d].x, xm[u][d].x, xm[u][d].y * xm[u][d].y);
          }
        if (lane == 0) prow[ppos(512)] = fmaf(x512.x, x512.x, x512.y * x512.y);
      }
    } else if (!COMPLEX_OUT && !TRI) {
      for (int k = lane; k < P_STRIDE; k += 64) prow[k] = 0.f;
    }
    SETPRIO(0);
    if (COMPLEX_OUT) continue;
    if (TRI) {
      // ---- MODE 6: this wave projects its own row (no barrier A, no slab, no combine); the two barriers below only
      // hand the stage buffer over: every DMA part of the next tile has landed | X1 | fetch the next frame | X2 | refill.
      // dB + DCT of a finished clip: when the clip's last tile leaves waves without a frame (tp - T of them), THEY form
      // the output tiles of the clip BEFORE while the others transform -- the epilogue then costs nothing; otherwise the
      // first waves form them right behind the clip's last tile, beside the other waves' next transform (which fills
      // the OTHER mel matrix).  Whatever is pending when the workgroup runs out of tiles is formed behind the loop.
      SETPRIO(3);             // projection, clip epilogue and row functions at the top level
      const bool mine = (t < T);
      const bool clip_done = (t0 + TILE_T >= T);
      float* cmc = clipmel + cur * (n_mels * mf.tp);
      auto project = [&]() {
        int la = lane;
        asm volatile("" : "+v"(la)::"memory");
        wave_lds_sync();
        // (the table's band word was turned into the band's BYTE offset inside a mel matrix when the workgroup copied it)
        if (TRIMEL) {
          char* colg = reinterpret_cast<char*>(mel_out + (b * n_mels) * T + t);
          tri_project<NPASS>(prow - TRI_ROW_BASE, reinterpret_cast<const float4*>(cpl), la, tri_scan8,
                         [&](int boff, float v) { *reinterpret_cast<float*>(colg + boff) = MELSC * v; });
        } else {
          char* colb = reinterpret_cast<char*>(cmc + (int)t);
          tri_project<2>(prow, reinterpret_cast<const float4*>(cpl), la, tri_scan8, [&](int boff, float v) {
            *reinterpret_cast<float*>(colb + boff) = v;
            asm("v_max_f32_e32 %0, %0, %1" : "+v"(cmax) : "v"(v));
          });
        }
      };
      // LOAD 4: the epilogue of the workgroup's clip number k waits for all sixteen waves to be through with it; a wait
      // that ran out, or a matrix marked bad, turns the clip's output into NaN (amin and the reference: every dB value)
      auto epilogue_args = [&](lds_ctr fill, int k) {
        MfccArgs a = mf;
        const bool ok = handover_wait<3>(fill, WAVES * ((k >> 1) + 1));
        if (!ok || handover_load(bad) != 0) { a.ref_is_max = 0; a.ref_value = a.amin = __builtin_nanf(""); }
        return a;
      };
      auto publish_max = [&]() {
        const float cm = wave_max(cmax);
        cmax = 0.f;
        if (lane == 0) tri_red[cur * WAVES + w] = cm;
      };
      const bool tri_proj = wpacked != nullptr;
#if SYG_DEV
      int tdep = lane;
      TICK(5, tdep);                   // (split + row store)
#endif
      // LOAD 3: the wave's power row is stored; the loads of the frame it transforms next (of the next clip, behind a clip's
      // last tile) are issued here and land under the projection, whose ~190 vector instructions need few registers.  A wave
      // that runs clip_dct issues them behind it: the entry of an out-of-line function waits for every outstanding load.
      auto prefetch = [&]() {
        have = false;
        if (tile + 1 < tile_end) fetch(tile + 1);
      };
      const bool dct_behind = FREERUN && clip_done && !tri_defer && w < tri_ndct;   // clip_dct behind the clip barrier
      if (FREERUN && mine && !dct_behind) prefetch();
      // LOAD 4: the matrix and red[cur][w] are this clip's once the epilogue of the clip before last has left them
      if (NOMEET && t0 == 0 && kclip >= 2 && !handover_wait<3>(drained + cur, tri_nepi * (kclip >> 1)) && lane == 0)
        __hip_atomic_store(bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (mine) {
        if (tri_proj) project();
      } else if (tri_defer && pend_b >= 0) {
        float* cmp = clipmel + (cur ^ 1) * (n_mels * mf.tp);
        const MfccArgs mfe = NOMEET ? epilogue_args(filled + (cur ^ 1), kclip - 1) : mf;
        clip_dct<WAVES>((int)(uintptr_t)(lds_fptr)cmp, (int)(uintptr_t)(lds_fptr)(tri_red + (cur ^ 1) * WAVES),
                        (int)(uintptr_t)(lds_fptr)tri_dct, mfe, n_mels, (int)T, (int)pend_b, w - (WAVES - tri_idle), lane, tri_idle);
        if (NOMEET) handover_add(drained + (cur ^ 1), lane);
      }
      if (FREERUN && !mine && !dct_behind) prefetch();
      // MODE 7: statistics / contrast of this wave's own row.  Out-of-line: the entry of such a function waits for every
      // outstanding memory operation, so the results wait in lanes of three registers and are stored -- and the stage
      // refill is issued -- behind the barriers.  Statistics first (a wide contrast band may park its lists in the row's
      // low words).  WHEN a wave runs them: half of the waves of every SIMD (w & 4) right behind their projection, the
      // other half behind X2 in front of their next transform -- between two barriers every wave does the same work, but
      // one half transforms while the other half runs its chains of dependent reductions, instead of all sixteen doing
      // the same thing at the same time (all behind X2, all in front of X1 -- the first build, 832 us -- measured slower).
      // Waves w, w + 4, w + 8, w + 12 share a SIMD: two of them early, two late.
      float row_sres = 0.f;
      float2 row_pv = make_float2(0.f, 0.f);
      const bool row_early = (w >> 2) & 1;               // (8 waves: w, w + 4 share a SIMD -- one early, one late)
      auto row_compute = [&]() {
        if (stats_out != nullptr && contrast_out != nullptr) {
          const float3 f = row_features<NBIN, 0>((lds_row)prow, lane, binhz, roll_percent, bw_p, smask, (lds_iptr)cplc,
                                                     cplan.n_rows, cplan.ascending);
          row_sres = f.x; row_pv = make_float2(f.y, f.z);
        } else {
          if (stats_out != nullptr) row_sres = row_stats<NBIN, 0>((lds_row)prow, lane, binhz, roll_percent, bw_p, smask);
          if (contrast_out != nullptr)
            row_pv = row_contrast_all<0>((lds_row)prow, lane, (lds_iptr)cplc, cplan.n_rows, cplan.ascending);
        }
      };
      TICK(6, tdep);                   // projection (or the deferred clip epilogue)
      if (ROWFN && mine && row_early) {
        // (the three result registers wait in the wave's own row, dead until its next transform: live across the fetch of
        // the next frame they cost three spilled registers)
        row_compute();
        prow[lane] = row_sres; prow[64 + lane] = row_pv.x; prow[128 + lane] = row_pv.y;
      }
      if (CLIPM && clip_done) publish_max();
      TICK(7, tdep);                   // row functions of the early half
      if (NOMEET) {
        // no barrier: this wave is through with the clip (the tile loop's preamble says what the counters carry)
        if (clip_done) handover_add(filled + cur, lane);
      } else if (FREERUN) {
        // The clip barrier, the only one of the tile loop: nothing inside a clip is shared -- a wave reads its own power
        // row, writes its own column of the clip's mel matrix and keeps its own maximum.  What hangs on this barrier:
        //   - clip c's matrix and its maxima red[cur][] (publish_max above) are complete behind it: clip_dct of clip c runs
        //     behind it -- at once on the first waves, or (deferred) on the idle waves of clip c + 1's last tile, which have
        //     passed this barrier in clip c's last tile and run it IN FRONT of clip c + 1's barrier;
        //   - clip c's matrix and red[cur][] are next written in clip c + 2, that is behind clip c + 1's barrier, which a
        //     wave running clip_dct of clip c reaches only when it is through with it (both placements above);
        //   - behind the loop the pending epilogue of the last clip follows that clip's barrier (a chunk is whole clips).
        // clip_done depends on the tile alone (t0, T): every wave of the workgroup, with or without a frame, walks the
        // same tiles and so executes this barrier once per clip.
        if (clip_done) __syncthreads();
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                // X1: the clip's columns of this tile are written too
      }
#if SYG_DEV
      tw0 = tacc[8];
      TICK(8, tdep);                   // wait at X1 (free-running forms: at the clip hand-over)
      if (tacc[8] - tw0 > tmaxw[0]) tmaxw[0] = tacc[8] - tw0;
#endif
      if (LOAD == 2) {
        have = false;
        if (tile + 1 < tile_end) fetch(tile + 1);
        __syncthreads();                                // X2: every wave holds its next frame
      }
      TICK(9, tdep);                   // fetch of the next frame + wait at X2
      if (CLIPM && clip_done) {
        // (clip_dct's entry waits for outstanding memory operations, so the refill is issued behind it)
        if (tri_defer) pend_b = mf.n_mfcc > 0 ? (int64_t)b : pend_b;
        else if (w < tri_ndct) {
          const MfccArgs mfe = NOMEET ? epilogue_args(filled + cur, kclip) : mf;
          clip_dct<WAVES>((int)(uintptr_t)(lds_fptr)cmc, (int)(uintptr_t)(lds_fptr)(tri_red + cur * WAVES),
                          (int)(uintptr_t)(lds_fptr)tri_dct, mfe, n_mels, (int)T, (int)b, w, lane);
          if (NOMEET) handover_add(drained + cur, lane);
        }
        cur ^= 1;
        ++kclip;
      }
      if (dct_behind) prefetch();
      if (ROWFN && mine) {
        if (!row_early) row_compute();
        else { row_sres = prow[lane]; row_pv = make_float2(prow[64 + lane], prow[128 + lane]); }
        TICK(10, tdep);                // row functions of the late half (+ the clip epilogue where it is not deferred)
        if (contrast_out != nullptr) {
          if (lane < cplan.n_rows) {
            contrast_out[((b * 2 + 0) * cplan.n_rows + lane) * T + t] = row_pv.x;
            contrast_out[((b * 2 + 1) * cplan.n_rows + lane) * T + t] = row_pv.y;
          }
        }
#if SYG_DEV
        if (stats_out != nullptr && row_sres == 12345.678f)      // (timeline build: stats_out carries the phase counters)
#else
        if (stats_out != nullptr && lane < SYG_NSTAT && ((stats_row_mask(smask) >> lane) & 1))
#endif
          stats_out[(b * SYG_NSTAT + lane) * T + t] = row_sres;
      }
      if (LOAD == 2 && tile + 2 < tile_end) dma(tile + 2);
      TICK(11, tdep);                  // the tile's stores + the stage refill
      SETPRIO(0);
      continue;
    }
#if SYG_DEV
    int tdep = lane;
    TICK(5, tdep);
#endif
    int la = lane;                     // laundered: per-lane addresses are recomputed here, not kept across the FFT
    asm volatile("" : "+v"(la)::"memory");
    const float4* wp4 = wp4w + la;
#pragma unroll
    for (int q = 0; q < NPRE; ++q) apre[q] = wp4[q * 64];
    const int pslot = mtab[w * 4 + (la >> 4)];          // row POSITION (skewed, see ppos()) of this lane's slot
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (staged mode: the next tile's samples have landed too)
    __syncthreads();                                    // barrier A: rows complete
    TICK(6, tdep);
    if (!ROWFN) SETPRIO(3);                             // projection (+ clip epilogue) at the top level
    if (CLIPM && pend_b >= 0) {
      if (w < ((mf.n_mfcc + 15) >> 4) * (mf.tp >> 4))    // output tile w is formed by wave w
        clip_dct<WAVES>((int)(uintptr_t)(lds_fptr)clipmel, (int)(uintptr_t)(lds_fptr)(clipmel + n_mels * mf.tp),
                        (int)(uintptr_t)(lds_fptr)(clipmel + n_mels * mf.tp + WAVES), mf, n_mels, (int)T, (int)pend_b, w, lane);
      pend_b = -1;
      TICK(10, tdep);
    }

    // ---- phase 2: block-sparse mel projection on the matrix cores, v_mfma_f32_4x4x1_16b_f32: sixteen independent
    // 4 x 4 outer-product blocks per instruction.  Block b = lane >> 2 = (slot s = b >> 2, frame group h = b & 3):
    // A = four mel rows of the slot's group at the slot's current row position (lane & 3 = row), B = the power at that
    // position in the four frames 4 h + (lane & 3), D[row][frame] accumulates in four registers.  A slot walks
    // CONSECUTIVE WORDS of the skewed power rows -- the pad word after every 16 bins carries a zero weight -- so every
    // B read is one base register plus an immediate offset, all of them are in flight together, and the MFMAs then
    // issue back to back.  Only the non-zero ranges of the 4-row groups are multiplied (1221 bin-steps per tile at
    // 40 mels against 4544 for 16-row tiles).
    {
      const int fr = (4 * ((la >> 2) & 3) + (la & 3)) & (TILE_T - 1);       // frame of this lane's block column
      const float* pq = Pbuf + fr * P_STRIDE + pslot;     // 8-byte aligned: P_STRIDE and the slot positions are even
      float bq[4 * NPRE];
#pragma unroll
      for (int i = 0; i < 2 * NPRE; ++i) {                 // two positions per LDS read (half the LDS cycles of b32 reads)
        const float2 v2 = reinterpret_cast<const float2*>(pq)[i];
        bq[2 * i] = v2.x; bq[2 * i + 1] = v2.y;
      }
      // two accumulators (even / odd positions): consecutive matrix instructions do not wait for each other
      v4f acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < NPRE; ++q) {
        acc = __builtin_amdgcn_mfma_f32_4x4x1f32(apre[q].x, bq[4 * q + 0], acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_4x4x1f32(apre[q].y, bq[4 * q + 1], acc2, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_4x4x1f32(apre[q].z, bq[4 * q + 2], acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_4x4x1f32(apre[q].w, bq[4 * q + 3], acc2, 0, 0, 0);
      }
      acc += acc2;
      for (int q = NPRE; q < ng; ++q) {       // (filterbanks whose chunks are longer than 28 row positions)
        const float4 a4 = wp4[q * 64];
        const float* pb = pq + 4 * q;
        acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a4.x, pb[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a4.y, pb[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a4.z, pb[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a4.w, pb[3], acc, 0, 0, 0);
      }
      // partial sums of (slot, mel row r, frame): slab[wave][slot][r][frame]
      if (4 * ((la >> 2) & 3) + (la & 3) < TILE_T) {
        float* sl = slab + (w * 4 + (la >> 4)) * (4 * TILE_T) + fr;
#pragma unroll
        for (int r = 0; r < 4; ++r) sl[r * TILE_T] = acc[r];
      }
      TICK(7, acc[0]);
    }
    // ---- staged mode: the next tile's frame (LDS -> registers); once every wave holds its frame (barrier B)
    // the stage is refilled with the tile after next.  The statistics of MODE 1 run behind barrier B with the fetched
    // frame live in callee-saved registers (the out-of-line row functions stay inside the caller-saved ones), so that
    // mode needs no barrier of its own.
    constexpr bool FETCH_EARLY = (LOAD == 2);
    if (FETCH_EARLY) {
      have = false;
      if (tile + 1 < tile_end) fetch(tile + 1);
    }
    __syncthreads();                // barrier B: slab complete (and every wave has read its staged frame)
    TICK(8, tdep);
    const bool clip_done = CLIPM && (t0 + TILE_T >= T);
    // MODE 1 runs out-of-line row functions below: a function entry waits for EVERY outstanding memory operation
    // (s_waitcnt vmcnt(0) -- the callee cannot know the caller's counters), so nothing may be in flight when they are
    // called: the refill of the stage buffer is issued behind them and the tile's stores behind the last call.
    constexpr bool TAIL = ROWFN;
    if (!TAIL && FETCH_EARLY && tile + 2 < tile_end) dma(tile + 2);

    // ---- combine the slots of each mel group in a fixed order (ascending bins): one wave per group of four mel rows,
    // lane = (row, frame); the slots of a group are consecutive.  (MODE 1: behind the row functions -- the slab stays
    // valid until the next tile's projection -- so that their entry does not wait for these stores.)
    auto combine = [&]() {
      constexpr int GL = 4 * TILE_T;               // outputs per group and tile (64 at 16 frames)
      // group g is combined by wave (g + 6) mod WAVES.  Ten groups at 40 mels: with shift 0 the ten OLDEST waves carry
      // the combine and the six youngest -- which the arbiter already serves last -- none; shift 6 gives it to the
      // waves 6 .. 15 (148.5 vs 150.8 us for the one-launch MFCC at C2; 3: 149.1, 10: slower than 6)
      constexpr int REDSHIFT = 6;
      for (int g = (w + WAVES - REDSHIFT) % WAVES; g < plan.n_groups; g += WAVES) {
        const int first = __builtin_amdgcn_readfirstlane(mtab[128 + g]);
        const int cnt = __builtin_amdgcn_readfirstlane(mtab[192 + g]);
        int lq = lane;                    // laundered (see lv above): no hoisted per-lane addresses that would spill
        asm volatile("" : "+v"(lq));
        if (GL == 64 || lq < GL) {
          const int m = lq / TILE_T, tt = lq & (TILE_T - 1);
          const float* sp = slab + first * GL + lq;
          float sum = 0.f;
          int q = 0;
          for (; q + 4 <= cnt; q += 4) {
            const float a0 = sp[0], a1 = sp[GL], a2 = sp[2 * GL], a3 = sp[3 * GL];
            sum += a0; sum += a1; sum += a2; sum += a3;
            sp += 4 * GL;
          }
          for (; q < cnt; ++q) { sum += sp[0]; sp += GL; }
          const int mel = g * 4 + m;
          if (CLIPM) {
            if (mel < n_mels) {
              clipmel[mel * mf.tp + (int)t0 + tt] = sum;     // frames >= T hold 0 (rows were cleared)
              cmax = fmaxf(cmax, sum);                        // power is non-negative
            }
            if (!SYG_DEV && mel_out != nullptr && mel < n_mels && t0 + tt < T) mel_out[(b * n_mels + mel) * T + t0 + tt] = MELSC * sum;
          } else {
            if (mel < n_mels && t0 + tt < T) mel_out[(b * n_mels + mel) * T + t0 + tt] = MELSC * sum;
          }
        }
      }
    };
    auto publish = [&]() {
      // last tile of the clip: publish the per-wave maxima; the dB + DCT epilogue runs in the next tile's
      // projection phase (or behind the loop)
      const float cm = wave_max(cmax);
      cmax = 0.f;
      if (lane == 0) clipmel[n_mels * mf.tp + w] = cm;
      pend_b = b;
    };
    if (!TAIL) {
      combine();
      if (clip_done) publish();
    }

    TICK(9, tdep);
    // ---- phase 2b: per-frame statistics / contrast means from the same LDS rows
    if (ROWFN && (stats_out != nullptr || contrast_out != nullptr)) {
      SETPRIO(3);
      if (t < T) {
        // statistics first (a wide contrast band parks its lists in the row's low words); every result waits in a lane
        // of a register and is stored behind the last call
        float sres = 0.f, pk = 0.f, vl = 0.f;
        const bool both = stats_out != nullptr && contrast_out != nullptr;
        if (both) {
          const float3 f = row_features<NBIN, 0>((lds_row)prow, lane, binhz, roll_percent, bw_p, smask, (lds_iptr)cplc,
                                                     cplan.n_rows, cplan.ascending);
          sres = f.x; pk = f.y; vl = f.z;
        } else if (stats_out != nullptr) sres = row_stats<NBIN, 0>((lds_row)prow, lane, binhz, roll_percent, bw_p, smask);
        if (contrast_out != nullptr) {
          if (!both) {
            const float2 pv = row_contrast_all<0>((lds_row)prow, lane, (lds_iptr)cplc, cplan.n_rows, cplan.ascending);
            pk = pv.x; vl = pv.y;
          }
          if (lane < cplan.n_rows) {
            contrast_out[((b * 2 + 0) * cplan.n_rows + lane) * T + t] = pk;
            contrast_out[((b * 2 + 1) * cplan.n_rows + lane) * T + t] = vl;
          }
        }
#if SYG_DEV
        if (stats_out != nullptr && sres == 12345.678f)      // (timeline build: stats_out carries the phase counters)
#else
        if (stats_out != nullptr && lane < SYG_NSTAT && ((stats_row_mask(smask) >> lane) & 1))
#endif
          stats_out[(b * SYG_NSTAT + lane) * T + t] = sres;
      }
      // (a wave only reads and -- parking sorted lists -- overwrites ITS OWN row here; every projection that read the
      // row finished before barrier B, and the row is next written by this wave's own FFT: no barrier needed)
    }
    if (TAIL) {
      SETPRIO(0);
      TICK(11, tdep);
      combine();
      if (clip_done) publish();
      if (FETCH_EARLY && tile + 2 < tile_end) dma(tile + 2);
    }
  }
  if (TRIMEL) {
    // (no clip epilogue: the mel columns are in HBM)
  } else if (TRI) {
    // (deferred epilogue: the last clip's matrix is complete behind X1 of its last tile)
    if (pend_b >= 0 && w < tri_ndct) {
      MfccArgs mfe = mf;
      if (NOMEET) {      // (like every other epilogue: behind the sixteen increments of its clip)
        if (!handover_wait<-1>(filled + (cur ^ 1), WAVES * (((kclip - 1) >> 1) + 1)) || handover_load(bad) != 0) {
          mfe.ref_is_max = 0; mfe.ref_value = mfe.amin = __builtin_nanf("");
        }
      }
      clip_dct<WAVES>((int)(uintptr_t)(lds_fptr)(clipmel + (cur ^ 1) * (n_mels * mf.tp)),
                      (int)(uintptr_t)(lds_fptr)(tri_red + (cur ^ 1) * WAVES), (int)(uintptr_t)(lds_fptr)tri_dct, mfe, n_mels,
                      (int)T, (int)pend_b, w, lane);
    }
  } else if (CLIPM && pend_b >= 0) {
    __syncthreads();
    if (w < ((mf.n_mfcc + 15) >> 4) * (mf.tp >> 4))
      clip_dct<WAVES>((int)(uintptr_t)(lds_fptr)clipmel, (int)(uintptr_t)(lds_fptr)(clipmel + n_mels * mf.tp),
                      (int)(uintptr_t)(lds_fptr)(clipmel + n_mels * mf.tp + WAVES), mf, n_mels, (int)T, (int)pend_b, w, lane);
  }
#if SYG_DEV
  if (CLIPM && !TRI && lane < 12)
    mel_out[((int64_t)blockIdx.x * WAVES + w) * 16 + lane] = (float)tacc[lane] / (float)(tile_end - tile_begin);
  // (the free-running forms have no statistics or mel output: the counters leave through syg_dev_set_timeline()'s buffer;
  // words 12 / 13: the longest single wait at the clip hand-over / in front of the window multiply)
  if (FREERUN && mel_out != nullptr && lane < 14)
    mel_out[((int64_t)blockIdx.x * WAVES + w) * 16 + lane] =
        lane < 12 ? (float)tacc[lane] / (float)(tile_end - tile_begin) : (float)(lane == 12 ? tmaxw[0] : tmaxw[1]);
  if (ROWFN && stats_out != nullptr && lane < 12)
    stats_out[((int64_t)blockIdx.x * WAVES + w) * 16 + lane] = (float)tacc[lane] / (float)(tile_end - tile_begin);
#endif
}

// Workgroups per CU: two of 8 waves or one of 16; each takes a contiguous chunk of tiles.
// syg_set_option(SYG_OPT_RESERVED_CUS, n) leaves n CUs out of the grid.  A workgroup of these kernels fills a
// CU (16 waves x 128 VGPRs), so a kernel of another stream that needs a few CUs at the same time -- RCCL's send /
// receive workgroups while the previous batch is gathered -- either waits for a whole launch or makes this launch wait
// for it (tools/queue_bench.py: 167 -> 256 us for every second launch).  With the CUs set aside both run side by side.
void persistent_grid(int64_t total_tiles, int waves, int& wgs, int& per) {
  const int n_cu = device_cu_count();
  int use_cu = n_cu;
  const int r = option(SYG_OPT_RESERVED_CUS);
  if (r > 0 && r < n_cu) use_cu = n_cu - r;
  const int64_t slots = (int64_t)use_cu * (waves == 8 ? 2 : 1);
  int64_t p = (total_tiles + slots - 1) / slots;
  if (p < 1) p = 1;
  per = (int)p;
  wgs = (int)((total_tiles + p - 1) / p);
}

// SYG_OPT_STFT_LOAD = 0 | 1 | 2 forces the frame load path (the tests compare the three); default: staged tiles
int load_mode() {
  const int v = option(SYG_OPT_STFT_LOAD);
  return (v >= 0 && v <= 2) ? v : 2;
}

#if SYG_DEV
// timeline builds: where the free-running forms leave their per-wave counters, [workgroups][16 waves][16] floats
// (syg_dev_set_timeline(), tools/timeline.py freerun | nomeet); null: nowhere
float* g_dev_timeline = nullptr;
#endif
// Default of SYG_OPT_STFT_FREERUN = -1: on -- at C2 every run of it was faster than every run of the staged form, by several times
// the run-to-run spread
constexpr bool FREERUN_DEFAULT = true;
// Default of SYG_OPT_STFT_MEET = -1 where the free-running form runs: its waves never meet (LOAD 4) -- DESIGN.md section 5.0-nm
constexpr bool NOMEET_DEFAULT = true;
// Where the free-running form can run (syg_stft2048_mfcc_tri_freerun): 8-byte loads of sample pairs that the descriptor's
// range check takes or leaves as a whole (hop, L, ldy even, y 8-byte aligned), byte offsets inside a clip in 32 bits
bool freerun_ok(int hop, int64_t L, int64_t ldy, const float* y) {
  return hop % 2 == 0 && L % 2 == 0 && ldy % 2 == 0 && ((uintptr_t)y) % 8 == 0 && L < ((int64_t)1 << 28);
}

// LDS accounting: the fixed map of the mode (ModeLds), and behind it what a clip-resident launch adds, for the 16-wave
// forms that have one: n_mat mel matrices [n_mels][tp] (tp: padded frames per clip), each with the per-wave maxima
// red[waves] of its clip, then the DCT rows [n_mfcc][n_mels] and the lifter [n_mfcc]
constexpr int64_t LDS_LIMIT = 160 * 1024;
constexpr int64_t clip_lds_bytes(int n_mat, int n_mels, int64_t tp, int n_mfcc, int waves) {
  return (n_mat * ((int64_t)n_mels * tp + waves) + (int64_t)n_mfcc * (n_mels + 1)) * (int64_t)sizeof(float);
}
// the same from the frame count of a clip, for the mode's 16 waves
template <Mode MODE>
int64_t clip_lds_bytes(int n_mels, int64_t T, int n_mfcc) {
  return clip_lds_bytes(mode_traits(MODE).clip_matrices(), n_mels, ((T + MAXW - 1) / MAXW) * MAXW, n_mfcc, MAXW);
}
// 2: `extra` bytes fit beside the stage buffer; 1: in the stage buffer's place (the launch then loads its frames straight
// from global memory); 0: not at all.  LM: the mode's fixed map
template <class LM>
constexpr int clip_lds_fit(int64_t extra) {
  constexpr int64_t fixed = (int64_t)LM::TOTAL * sizeof(float), stage = (int64_t)LM::STAGE_FLOATS * sizeof(float);
  return fixed + extra <= LDS_LIMIT ? 2 : fixed - stage + extra <= LDS_LIMIT ? 1 : 0;
}

// What a launch reads and writes, in groups; value-initialised (LaunchArgs a = {}), an entry point sets what it uses.
//   clip: y [B, L] (row stride ldy) -> T frames per clip   mel: the filterbank's device table (packed weights + plan, or
//   the piece table) and the mel output   st: statistics / contrast rows   load: the frame load path asked for
struct ClipArgs { const float* y; int64_t B, L, ldy; int hop, center; int64_t T; const float* window; const float* twiddle; };
struct MelArgs { const float* table; MelPlan plan; int n_mels; float* mel_out; };
struct StatArgs { float binhz, roll_percent, bw_p; int smask; float* stats_out; ContrastPlan cp; float* contrast_out; };
struct LaunchArgs { ClipArgs clip; MelArgs mel; StatArgs st; float* cout; MfccArgs mf; int load; hipStream_t stream; };
// the MfccArgs of a launch without a dB + DCT epilogue
MfccArgs no_mfcc() { MfccArgs mf = {}; mf.amin = 1e-10f; mf.top_db = -1.f; return mf; }

template <int WAVES, Mode MODE>
int launch(const LaunchArgs& a) {
  constexpr ModeTraits M = mode_traits(MODE);
  typedef ModeLds<WAVES, MODE> LM;
  const ClipArgs& c = a.clip;
  MfccArgs mf = a.mf;
  const int n_mels = a.mel.n_mels;
  const int pad = c.center ? NFFT / 2 : 0;
  const int tiles = (int)((c.T + WAVES - 1) / WAVES);
  const int64_t total_tiles = c.B * tiles;
  int wgs = 0, per = 0;
  persistent_grid(total_tiles, WAVES, wgs, per);
  size_t lds = (size_t)LM::TOTAL * sizeof(float);
  int64_t clip_extra = 0;
  if (M.seg() || M.clip) mf.tp = tiles * WAVES;
  if (M.clip) {
    // whole clips per workgroup; the clip's mel matrix [n_mels][tiles * WAVES] sits behind the fixed LDS map
    persistent_grid(c.B, WAVES, wgs, per);
    per *= tiles;
    if (M.x2()) { mf.amin *= 4.f; mf.ref_value *= 4.f; }     // the clip's mel matrix holds 4 x mel (exact scaling)
    clip_extra = clip_lds_bytes(M.clip_matrices(), n_mels, mf.tp, mf.n_mfcc, WAVES);
  }
  // staged tiles (LDS-DMA) need the tile's sample run to fit the stage buffer and 32-bit byte offsets
  bool can_stage = !M.complex_out && c.hop <= 512 && c.L < ((int64_t)1 << 28);
  // a clip matrix that does not fit behind the stage buffer takes the buffer's place: frames straight from global memory
  if (M.clip && clip_lds_fit<LM>(clip_extra) < 2) can_stage = false;
  int load = a.load;
  if (load == 2 && !can_stage) load = 1;
  const bool vec2 = (c.hop % 2 == 0) && (c.ldy % 2 == 0) && (((uintptr_t)c.y) % 8 == 0);
  if (load == 1 && !vec2) load = 0;
  // the free-running form where the mode has one and its loads are possible; an explicit load path (the three are
  // compared by the tests) is kept unless the form is asked for
  if (M.freerun && WAVES == 16) {
    const int fr = option(SYG_OPT_STFT_FREERUN);
    const bool want = fr == 1 || (fr < 0 && FREERUN_DEFAULT && option(SYG_OPT_STFT_LOAD) < 0);
    if (want && freerun_ok(c.hop, c.L, c.ldy, c.y)) {
      const int meet = option(SYG_OPT_STFT_MEET);
      load = (meet == 0 || (meet < 0 && NOMEET_DEFAULT)) ? 4 : 3;
    }
  }
  if (M.clip) {       // (no stage buffer unless the tiles are staged)
    lds = lds - (load != 2 ? (size_t)LM::STAGE_FLOATS * sizeof(float) : 0) + (size_t)clip_extra;
    SYG_REQUIRE(lds <= (size_t)LDS_LIMIT, "stft2048_mfcc: the clip's mel matrix (%d x %d) does not fit the LDS left over (%zu B > %zu B); "
                "use syg_stft2048_mel_f32 + syg_logmel_dct_f32", n_mels, mf.tp, lds, (size_t)LDS_LIMIT);
  }
  const int dma_wide = (c.hop % 4 == 0) && (pad % 4 == 0) && (c.ldy % 4 == 0) && (c.L % 4 == 0) && (((uintptr_t)c.y) % 16 == 0);
  auto kern = load == 2 ? stft2048_kernel<WAVES, 2, MODE>
                        : load == 1 ? stft2048_kernel<WAVES, 1, MODE> : stft2048_kernel<WAVES, 0, MODE>;
  if constexpr (M.freerun && WAVES == 16)
    if (load >= 3) kern = load == 4 ? stft2048_kernel<WAVES, 4, MODE> : stft2048_kernel<WAVES, 3, MODE>;
  float* mel_out = a.mel.mel_out;
#if SYG_DEV
  if (load >= 3) mel_out = g_dev_timeline;      // (the free-running forms write no mel output: their counters' way out)
#endif
  const size_t cap = M.clip ? (size_t)LDS_LIMIT : (size_t)LM::TOTAL * sizeof(float);
  if (const int rc = reserve_dynamic_lds("stft2048", (const void*)kern, cap)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(WAVES * 64), lds, a.stream, c.y, c.L, c.ldy, c.hop, pad, c.T,
                     tiles, total_tiles, per, (const float2*)c.window, (const float2*)c.twiddle, a.mel.table, a.mel.plan,
                     n_mels, mel_out, a.st.binhz, a.st.roll_percent, a.st.bw_p, a.st.smask, a.st.stats_out, a.st.cp,
                     a.st.contrast_out, (float2*)a.cout, dma_wide, mf);
  SYG_CHECK_LAUNCH("stft2048");
  return SYG_OK;
}
// mel per tile (no clip residency): the mode of (projection, table passes, row functions), for 8 or 16 waves
constexpr Mode tile_mode(Proj proj, int npass, bool rows) {
  return proj == Proj::Matrix ? (rows ? Mode::MelRows : Mode::Mel)
         : npass == 4 ? (rows ? Mode::TileSeg4Rows : Mode::TileSeg4) : (rows ? Mode::TileSeg2Rows : Mode::TileSeg2);
}
template <int WAVES, Proj PROJ, int NPASS>
int launch_tile(bool rows, const LaunchArgs& a) {
  return rows ? launch<WAVES, tile_mode(PROJ, NPASS, true)>(a) : launch<WAVES, tile_mode(PROJ, NPASS, false)>(a);
}

// checks shared by the seven entry points; fills the clip group and what every launch needs beside it
int fill_clip_args(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center, int64_t T, const float* window,
                   const float* twiddle, int waves, void* stream, LaunchArgs& a) {
  if (const int rc = check_clips("stft2048", y, B, L, ldy, NFFT, hop, center, T, window, twiddle)) return rc;
  SYG_REQUIRE(B * ((T + waves - 1) / waves) < (int64_t)0x7fffffff, "stft2048: grid too large");
  a.clip = {y, B, L, ldy, hop, center, T, window, twiddle};
  a.load = load_mode(); a.stream = (hipStream_t)stream;
  return SYG_OK;
}

// statistics / contrast group of the entry points with row functions (the parameters are looked at only with stats_out)
int fill_stat_args(const char* who, float sr, float roll_percent, float bw_p, int stats_mask, float* stats_out,
                   const int32_t* cplan_host, float* contrast_out, StatArgs& st) {
  int rc = parse_contrast_plan("stft2048", NBIN, contrast_out, cplan_host, st.cp);
  if (!rc && stats_out) rc = check_stats_args(who, sr, roll_percent, bw_p, stats_mask);
  st.binhz = sr / (float)NFFT; st.roll_percent = roll_percent; st.bw_p = bw_p; st.smask = stats_mask;
  st.stats_out = stats_out; st.contrast_out = contrast_out;
  return rc;
}

int parse_mel_plan(const char* who, const int32_t* plan_host, int n_mels, MelPlan& plan) {
  // plan_host: {2 (layout version), waves, steps, n_groups, table_off}
  SYG_REQUIRE(plan_host[0] == 2, "%s: mel plan layout %d, this library needs layout 2 (sygnals_amd._tables.pack_mel_plan)",
              who, plan_host[0]);
  const int waves = plan_host[1];
  SYG_REQUIRE(waves == 8 || waves == 16, "%s: plan must be built for 8 or 16 waves (got %d)", who, waves);
  plan.steps = plan_host[2]; plan.n_groups = plan_host[3]; plan.table_off = plan_host[4];
  SYG_REQUIRE(n_mels >= 1 && plan.n_groups == (n_mels + 3) / 4 && plan.n_groups <= 64,
              "%s: plan has %d groups of four mel rows, n_mels=%d needs %d (at most 64)", who, plan.n_groups, n_mels,
              (n_mels + 3) / 4);
  SYG_REQUIRE(plan.steps >= 28 && plan.steps % 4 == 0 && plan.steps <= P_STRIDE, "%s: bad step count %d", who, plan.steps);
  SYG_REQUIRE(plan.table_off >= waves * plan.steps * 64 && plan.table_off % 4 == 0, "%s: bad table offset", who);
  static_assert(P_STRIDE % 2 == 0, "slot reads are 8-byte words");
  return SYG_OK;
}

constexpr int64_t CLIP_FRAMES_LIMIT = (int64_t)1 << 24;     // frames per clip of the forms that keep frame indices in 24 bits

}  // namespace
}  // namespace syg

using namespace syg;

extern "C" int syg_stft2048_mel_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center,
                                    int64_t T, const float* window, const float* twiddle, const float* wpacked,
                                    const int32_t* plan_host, int n_mels, float* mel_out, float sr,
                                    float roll_percent, float bw_p, int stats_mask, float* stats_out,
                                    const int32_t* cplan_host, float* contrast_out, void* stream) {
  SYG_REQUIRE(wpacked && plan_host && mel_out, "stft2048_mel: null pointer argument");
  LaunchArgs a = {};
  int rc = parse_mel_plan("stft2048_mel", plan_host, n_mels, a.mel.plan);
  if (rc) return rc;
  const int waves = plan_host[1];
  if ((rc = fill_clip_args(y, B, L, ldy, hop, center, T, window, twiddle, waves, stream, a))) return rc;
  if ((rc = fill_stat_args("stft2048_mel", sr, roll_percent, bw_p, stats_mask, stats_out, cplan_host, contrast_out, a.st))) return rc;
  if (stats_out && (rc = check_row_frames("stft2048_mel", T))) return rc;
  a.mel.table = wpacked; a.mel.n_mels = n_mels; a.mel.mel_out = mel_out;
  const bool rows = (stats_out != nullptr) || (contrast_out != nullptr);
  return waves == 8 ? launch_tile<8, Proj::Matrix, 2>(rows, a) : launch_tile<16, Proj::Matrix, 2>(rows, a);
}

// (1, the stage buffer's place: 128 bands x 94 frames; measured 186 against 196 us for the two-launch form there, 176 against
// 166 at 64 bands)
extern "C" int syg_stft2048_mfcc_fits(int n_mels, int64_t T, int n_mfcc) {
  if (n_mels < 1 || n_mels > 16 * MAXW || T < 1 || n_mfcc < 1 || n_mfcc > n_mels) return 0;
  return clip_lds_fit<ModeLds<16, Mode::ClipMatrix>>(clip_lds_bytes<Mode::ClipMatrix>(n_mels, T, n_mfcc));
}

extern "C" int syg_stft2048_mfcc_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center,
                                     int64_t T, const float* window, const float* twiddle, const float* wpacked,
                                     const int32_t* plan_host, int n_mels, const float* dct, int n_mfcc,
                                     const float* lifter, float amin, float top_db, int ref_is_max, float ref_value,
                                     float* mel_out, float* mfcc_out, void* stream) {
  SYG_REQUIRE(wpacked && plan_host && dct && mfcc_out, "stft2048_mfcc: null pointer argument");
  LaunchArgs a = {};
  int rc = parse_mel_plan("stft2048_mfcc", plan_host, n_mels, a.mel.plan);
  if (rc) return rc;
  SYG_REQUIRE(plan_host[1] == 16, "stft2048_mfcc: needs a 16-wave plan (got %d)", plan_host[1]);
  if ((rc = fill_clip_args(y, B, L, ldy, hop, center, T, window, twiddle, 16, stream, a))) return rc;
  if ((rc = fill_mfcc_args("stft2048_mfcc", "%s: need 1 <= n_mfcc <= n_mels (n_mfcc=%d n_mels=%d)", n_mels, dct, n_mfcc, n_mfcc,
                           lifter, amin, top_db, ref_is_max, ref_value, mfcc_out, T, CLIP_FRAMES_LIMIT, a.mf))) return rc;
  a.mel.table = wpacked; a.mel.n_mels = n_mels; a.mel.mel_out = mel_out; a.mf.rows_per_clip = n_mfcc;
  return launch<16, Mode::ClipMatrix>(a);
}

// syg_stft2048_mfcc_f32 for TRIANGULAR filterbanks (segtab: pack_mel_segments, [2][2][64][4] words).  Same results as the
// matrix form to rounding (both sum in float32; the affine pieces reproduce the float32 weights to 1e-7 of the largest --
// checked on the host when the table is built).  Fits: the two mel matrices have room beside the stage buffer
extern "C" int syg_stft2048_mfcc_tri_fits(int n_mels, int64_t T, int n_mfcc) {
  if (n_mels < 1 || n_mels > 127 || T < 1 || n_mfcc < 1 || n_mfcc > n_mels) return 0;
  return clip_lds_fit<ModeLds<16, Mode::ClipSeg>>(clip_lds_bytes<Mode::ClipSeg>(n_mels, T, n_mfcc)) == 2;
}

#if SYG_DEV
extern "C" void syg_dev_set_timeline(float* buf) { g_dev_timeline = buf; }
#endif
extern "C" int syg_stft2048_mfcc_tri_freerun(int hop, int64_t L, int64_t ldy, const float* y) {
  return freerun_ok(hop, L, ldy, y) ? 1 : 0;
}

extern "C" int syg_stft2048_mfcc_tri_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center,
                                         int64_t T, const float* window, const float* twiddle, const float* segtab,
                                         int n_segtab, int n_mels, const float* dct, int n_mfcc, const float* lifter,
                                         float amin, float top_db, int ref_is_max, float ref_value, float* mfcc_out,
                                         void* stream) {
  SYG_REQUIRE(segtab && dct && mfcc_out, "stft2048_mfcc_tri: null pointer argument");
  LaunchArgs a = {};
  int rc = check_segtab("stft2048_mfcc_tri", segtab, n_segtab, SEGTAB_WORDS, n_mels, 127);
  if (!rc) rc = fill_clip_args(y, B, L, ldy, hop, center, T, window, twiddle, 16, stream, a);
  if (rc) return rc;
  if ((rc = fill_mfcc_args("stft2048_mfcc_tri", "%s: need 1 <= n_mfcc <= n_mels (n_mfcc=%d n_mels=%d)", n_mels, dct, n_mfcc, n_mfcc,
                           lifter, amin, top_db, ref_is_max, ref_value, mfcc_out, T, CLIP_FRAMES_LIMIT, a.mf))) return rc;
  a.mel.table = segtab; a.mel.n_mels = n_mels; a.mf.rows_per_clip = n_mfcc;
  return launch<16, Mode::ClipSeg>(a);
}

// BASELINE config C4 from one launch, without a mel matrix in HBM and without the projection's barriers
extern "C" int syg_stft2048_features_tri_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center, int64_t T,
                                             const float* window, const float* twiddle, const float* segtab, int n_segtab,
                                             int n_mels, const float* dct, int n_mfcc, const float* lifter, float amin,
                                             float top_db, int ref_is_max, float ref_value, float sr, float roll_percent,
                                             float bw_p, int stats_mask, float* stats_out, const int32_t* cplan_host,
                                             float* contrast_out, float* mfcc_out, int mfcc_rows_per_clip, void* stream) {
  SYG_REQUIRE(segtab && dct && mfcc_out, "stft2048_features_tri: null pointer argument");
  SYG_REQUIRE(stats_out || contrast_out, "stft2048_features_tri: no statistics requested (use syg_stft2048_mfcc_tri_f32)");
  LaunchArgs a = {};
  int rc = check_segtab("stft2048_features_tri", segtab, n_segtab, SEGTAB_WORDS, n_mels, 127);
  if (!rc) rc = fill_clip_args(y, B, L, ldy, hop, center, T, window, twiddle, 16, stream, a);
  if (rc) return rc;
  if ((rc = fill_mfcc_args("stft2048_features_tri", "%s: need 1 <= n_mfcc <= n_mels and mfcc_rows_per_clip >= n_mfcc", n_mels, dct,
                           n_mfcc, mfcc_rows_per_clip, lifter, amin, top_db, ref_is_max, ref_value, mfcc_out, T, CLIP_FRAMES_LIMIT,
                           a.mf))) return rc;
  if ((rc = fill_stat_args("stft2048_features_tri", sr, roll_percent, bw_p, stats_mask, stats_out, cplan_host, contrast_out, a.st))) return rc;
  a.mel.table = segtab; a.mel.n_mels = n_mels; a.mf.rows_per_clip = mfcc_rows_per_clip;
  return launch<16, Mode::ClipSegRows>(a);
}

// The tile form: mel POWER out, syg_logmel_dct_f32 / syg_feature_block_f32 is the second launch of an MFCC; one long clip
// (BASELINE config C1) fills the chip.  Four passes: the reference's default filterbank of 128 bands (manager.py:214).
// waves = 8: two workgroups per CU, each with its own tile barriers -- they drift out of phase, so that one's transforms
// run beside the other's LDS exchanges
extern "C" int syg_stft2048_mel_tri_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center, int64_t T,
                                        const float* window, const float* twiddle, const float* segtab, int n_segtab,
                                        int n_mels, float* mel_out, float sr, float roll_percent, float bw_p, int stats_mask,
                                        float* stats_out, const int32_t* cplan_host, float* contrast_out, int waves,
                                        void* stream) {
  SYG_REQUIRE(segtab && mel_out, "stft2048_mel_tri: null pointer argument");
  // (the four-pass table, row_base 4, or the two-pass table of syg_stft2048_mfcc_tri_f32)
  int rc = check_segtab("stft2048_mel_tri", segtab, n_segtab, n_segtab == SEGTAB_WORDS ? SEGTAB_WORDS : SEGTAB4_WORDS, n_mels, 255);
  if (rc) return rc;
  SYG_REQUIRE(waves == 8 || waves == 16, "stft2048_mel_tri: waves must be 8 or 16 (got %d)", waves);
  LaunchArgs a = {};
  if ((rc = fill_clip_args(y, B, L, ldy, hop, center, T, window, twiddle, waves, stream, a))) return rc;
  SYG_REQUIRE(T * (int64_t)n_mels < ((int64_t)1 << 29), "stft2048_mel_tri: clip too long (32-bit byte offsets inside a clip's mel block)");
  const bool rows = stats_out != nullptr || contrast_out != nullptr;
  if (rows && (rc = fill_stat_args("stft2048_mel_tri", sr, roll_percent, bw_p, stats_mask, stats_out, cplan_host, contrast_out, a.st)))
    return rc;
  a.mel.table = segtab; a.mel.n_mels = n_mels; a.mel.mel_out = mel_out; a.mf = no_mfcc();
  const bool four = n_segtab == SEGTAB4_WORDS;
  if (waves == 16) return four ? launch_tile<16, Proj::Segments, 4>(rows, a) : launch_tile<16, Proj::Segments, 2>(rows, a);
  return four ? launch_tile<8, Proj::Segments, 4>(rows, a) : launch_tile<8, Proj::Segments, 2>(rows, a);
}

// syg_stft2048_features_tri_f32's mode without a filterbank: nothing is projected, no clip epilogue; the waves only meet at
// the two stage hand-over barriers.  hop <= 512 (staged tiles); other hops: syg_stft2048_mel_f32.
extern "C" int syg_stft2048_stats_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center, int64_t T,
                                      const float* window, const float* twiddle, float sr, float roll_percent, float bw_p,
                                      int stats_mask, float* stats_out, const int32_t* cplan_host, float* contrast_out,
                                      void* stream) {
  SYG_REQUIRE(stats_out || contrast_out, "stft2048_stats: no statistics requested");
  LaunchArgs a = {};
  int rc = fill_clip_args(y, B, L, ldy, hop, center, T, window, twiddle, 16, stream, a);
  if (rc) return rc;
  SYG_REQUIRE(hop <= 512 && L < ((int64_t)1 << 28), "stft2048_stats: needs hop <= 512 (staged tiles); use syg_stft2048_mel_f32");
  SYG_REQUIRE(T < CLIP_FRAMES_LIMIT, "stft2048_stats: clip too long");
  if ((rc = fill_stat_args("stft2048_stats", sr, roll_percent, bw_p, stats_mask, stats_out, cplan_host, contrast_out, a.st))) return rc;
  a.mf = no_mfcc(); a.load = 2;
  return launch<16, Mode::ClipSegRows>(a);
}

extern "C" int syg_stft2048_c2c_f32(const float* y, int64_t B, int64_t L, int64_t ldy, int hop, int center,
                                    int64_t T, const float* window, const float* twiddle, float* out,
                                    void* stream) {
  LaunchArgs a = {};
  const int rc = fill_clip_args(y, B, L, ldy, hop, center, T, window, twiddle, 8, stream, a);
  if (rc) return rc;
  SYG_REQUIRE(out, "stft2048_c2c: null output");
  a.cout = out; a.load = 1;
  return launch<8, Mode::Complex>(a);
}
