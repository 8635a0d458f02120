// The device random number generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11;
// the Random123 constants) and the standard normals drawn from it.  The float64 restatement that is the contract lives in
// tests/rng_ref.py; sygnals_amd/_rng.py is the host-side twin in integer NumPy.
//
// A sample's value depends on (seed, stream, row, n) alone: key = (seed low, seed high), counter = (q low, q high, row,
// stream) with q = n / 4; the four words of one call give samples 4q .. 4q + 3.  Nothing depends on the launch shape, on
// where a row lies in a batch, or on an atomic.  A thread that needs fewer than four samples of a call generates the
// whole call and drops the rest.
#pragma once
#include <math.h>
#include "common.h"

namespace syg {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // key increments (Weyl sequence)
constexpr int PHILOX_ROUNDS = 10;
constexpr int RNG_STREAM_NOISE = 0;        // counter word 3: noise samples
constexpr int RNG_STREAM_ROW = 1;          //                 per-row draws (a row's random SNR), host side only
constexpr int RNG_STREAM_SPEC = 2;         //                 SpecAugment's per-clip draws (spec_augment.hip)
constexpr int64_t RNG_ROW_LIMIT = (int64_t)1 << 31;

// ten rounds, the key bumped between them; per round (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))
__host__ __device__ __forceinline__ uint4 philox4x32(uint4 c, uint2 k) {
#pragma unroll
  for (int r = 0; r < PHILOX_ROUNDS; ++r) {
    const uint64_t p0 = (uint64_t)PHILOX_M0 * c.x;
    const uint64_t p1 = (uint64_t)PHILOX_M1 * c.z;
    c = make_uint4((uint32_t)(p1 >> 32) ^ c.y ^ k.x, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k.y, (uint32_t)p0);
    k.x += PHILOX_W0;
    k.y += PHILOX_W1;
  }
  return c;
}

inline uint2 rng_key(uint64_t seed) { return make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)); }

// (2 (w >> 9) + 1) 2^-24: an odd multiple of 2^-24 below 2^24 of them, exact in float32 and strictly inside (0, 1)
__device__ __forceinline__ float rng_unit(uint32_t w) { return (float)(2u * (w >> 9) + 1u) * 0x1p-24f; }

// Box-Muller on the accurate logf / sqrtf; the angle through sincospif(2 u), so that no rounded 2 pi u enters it.
// |z| <= sqrt(-2 ln 2^-24) = 5.77.
__device__ __forceinline__ void rng_box_muller(uint32_t wa, uint32_t wb, float& z0, float& z1) {
  const float r = sqrtf(-2.0f * logf(rng_unit(wa)));
  float s, c;
  sincospif(2.0f * rng_unit(wb), &s, &c);
  z0 = r * c;
  z1 = r * s;
}

// standard normals 4q .. 4q + 3 of (key, row) in the noise stream
__device__ __forceinline__ float4 rng_normal4(uint2 key, uint64_t q, uint32_t row) {
  const uint4 w = philox4x32(make_uint4((uint32_t)q, (uint32_t)(q >> 32), row, (uint32_t)RNG_STREAM_NOISE), key);
  float4 z;
  rng_box_muller(w.x, w.y, z.x, z.y);
  rng_box_muller(w.z, w.w, z.z, z.w);
  return z;
}

}  // namespace syg
