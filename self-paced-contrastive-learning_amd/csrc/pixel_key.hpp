// The hash key of the on-device samplers (pixel_contrast.hip: the class-balanced cell sample; cutmix.hip: the CutMix boxes):
//   key(i, seed) = fmix32(((i + 1) * 0x9E3779B1 mod 2^32) ^ seed)       (fmix32: MurmurHash3's finaliser)
// Both steps are bijections of 32-bit words: distinct indices have distinct keys.
#pragma once
#include "common.hpp"

namespace spcl {

__device__ __forceinline__ uint32_t pxs_key(uint32_t i, uint32_t seed) {
  uint32_t h = ((i + 1u) * 0x9E3779B1u) ^ seed;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

}  // namespace spcl
