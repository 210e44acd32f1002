// The counter-based generator of the device-drawn random parameters (diffaug.hip dei2i_diffaug_draw, mask.hip dei2i_mask_draw,
// embed.hip dei2i_embed_draw, blit.hip dei2i_blit_draw, warp.hip dei2i_warp_draw): key = a seed, counter words = (call low, call high, stream word, row) -- include/dei2i_hip.h gives each user's word layout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dei2i {

struct Philox4 {
  uint32_t x0, x1, x2, x3;
};

// Philox4x32-10 (Salmon et al. 2011, Random123): ten rounds, the key bumped by the Weyl constants between rounds
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return Philox4{c0, c1, c2, c3};
}

// the grid of torch.rand: 24 bits, [0, 1)
__device__ __forceinline__ float unit_float(uint32_t x) {
#pragma clang fp contract(off)
  return (float)(x >> 8) * 0x1p-24f;
}

}  // namespace dei2i
