// Counter-based dropout RNG shared by every kernel that drops (rng.hip, attention.hip).
//
// Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11):
// four 32-bit counter words and two key words in, four 32-bit words out.  Plain integer C++.
//
// Draw protocol: the per-device state is two uint64 in device memory, {seed, draw}.  An op that
// drops takes ONE draw: the one-thread kernel rng_draw_kernel copies {seed, draw} into a 16-byte
// key tensor the op owns and advances draw by 1 (atomicAdd).  Every kernel of the op (forward,
// backward, mask export) reads the key from device memory, never from a host scalar, so a captured
// HIP graph takes fresh draws on every replay and forward / backward agree through the saved key.
//
// Index map (restated once on the host, multimodalreactiongeneration_amd/rng.py):
//   Philox key         (lo32(seed), hi32(seed) ^ hi32(draw))
//   flat element i     counter (lo32(i >> 2), hi32(i >> 2), 0xFFFFFFFF, lo32(draw)),  word i & 3
//   attention element  (b, head, q, k), q the global query index:
//                      counter (k >> 2, q, b * heads + head, lo32(draw)),             word k & 3
// (b * heads + head never reaches 0xFFFFFFFF, so the two families do not share counters.)
//
// Keep rule: keep iff word >= thr, thr = floor(p * 2^32) computed on the host in double and passed
// as a uint32; kept values are scaled by 1 / (1 - p) in fp32 (also passed by the host).
#pragma once
#include <cstdint>

namespace mrg {

struct Philox4 {
  uint32_t w[4];
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// the op's key as its kernels hold it: read once per thread from the 16-byte key tensor
struct DropKey {
  uint32_t k0, k1, draw_lo;
};

__device__ __forceinline__ DropKey load_drop_key(const unsigned long long* key) {
  const unsigned long long seed = key[0], draw = key[1];
  return DropKey{(uint32_t)seed, (uint32_t)(seed >> 32) ^ (uint32_t)(draw >> 32), (uint32_t)draw};
}

// the four words of flat elements 4 * i4 .. 4 * i4 + 3
__device__ __forceinline__ Philox4 flat_words(const DropKey& dk, unsigned long long i4) {
  return philox4x32_10((uint32_t)i4, (uint32_t)(i4 >> 32), 0xFFFFFFFFu, dk.draw_lo, dk.k0, dk.k1);
}

// the four words of attention elements (bh, q, 4 * k4 .. 4 * k4 + 3); bh = b * heads + head, q global
__device__ __forceinline__ Philox4 attn_words(const DropKey& dk, uint32_t bh, uint32_t q, uint32_t k4) {
  return philox4x32_10(k4, q, bh, dk.draw_lo, dk.k0, dk.k1);
}

}  // namespace mrg
