// mix64.h -- the counter-based hash behind every random stream of the library (pynqs_spin_flip_rand's proposals, the
// Metropolis acceptance draws of kernels_mcmc.hip): a draw is a pure function of (seed, step, chain), no generator state.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pynqs {

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64 finaliser
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

}  // namespace pynqs
