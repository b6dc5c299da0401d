// kernels_hash.hip -- the psi hash table of a sample space: open addressing over the sorted key array's positions, with the Bloom
// filters of the fused SAMPLE_SPACE kernels appended (detcore.h: hash_find, hash_filter_bits, hash_filter2_bits, hash_string_bits).
// The reference has an optional GPU table for the same purpose (cuda_tensor.cpp:489-559).  Users: the column-major SAMPLE_SPACE
// kernels (kernels_eloc.hip), the REDUCE front end, kernels_unique.hip and the Python HashTable.
#include "detcore.h"
#include "launch.h"

namespace pynqs {

// Insert key i of the sorted key array: claim a slot by CAS on its index word, then write the key words
// (lookups only start after the build kernel has finished).
template <int LEN>
__global__ __launch_bounds__(kBlock) void hash_build_kernel(const uint64_t *__restrict__ keys, int64_t nkeys, uint64_t cap,
                                                            uint64_t *__restrict__ table, uint32_t fbits, uint32_t f2bits, uint32_t sbits) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nkeys) return;
  uint64_t q[LEN];
#pragma unroll
  for (int w = 0; w < LEN; ++w) q[w] = keys[i * LEN + w];
  constexpr int W = hash_slot_words(LEN);
  const uint64_t hq = hash_of<LEN>(q);
  uint64_t s = hq & (cap - 1);
  for (uint64_t probes = 0; probes < cap; ++probes) {
    unsigned long long *idxp = reinterpret_cast<unsigned long long *>(table + s * W + (W - 1));
    const unsigned long long old = atomicCAS(idxp, ~0ull, (unsigned long long)i);
    if (old == ~0ull) {
#pragma unroll
      for (int w = 0; w < LEN; ++w) table[s * W + w] = q[w];
      if (fbits || f2bits) {
        uint32_t z, z2, b0, b1;
        zobrist_of<LEN>(q, z, z2);
        uint32_t *filter = reinterpret_cast<uint32_t *>(table + cap * W);
        if (fbits) {
          filter_positions(z, fbits, b0, b1);
          atomicOr(filter + (b0 >> 5), 1u << (b0 & 31u));
          atomicOr(filter + (b1 >> 5), 1u << (b1 & 31u));
          filter += fbits / 32;
        }
        if (f2bits) {  // second level
          filter2_position(z2, f2bits, b0, b1);
          atomicOr(filter + b0, b1);
          filter += f2bits / 32;
        }
        if (sbits) {  // the key's alpha and beta strings
          uint32_t za, zb;
          zobrist_strings<LEN>(q, za, zb);
          filter_positions(za, sbits, b0, b1);
          atomicOr(filter + (b0 >> 5), 1u << (b0 & 31u));
          atomicOr(filter + (b1 >> 5), 1u << (b1 & 31u));
          filter += sbits / 32;
          filter_positions(zb, sbits, b0, b1);
          atomicOr(filter + (b0 >> 5), 1u << (b0 & 31u));
          atomicOr(filter + (b1 >> 5), 1u << (b1 & 31u));
        }
      }
      return;
    }
    s = (s + 1) & (cap - 1);
  }
}

template <int LEN>
__global__ __launch_bounds__(kBlock) void hash_lookup_kernel(const uint64_t *__restrict__ table, uint64_t cap,
                                                             const uint64_t *__restrict__ onv, uint64_t n,
                                                             int64_t *__restrict__ idx, uint8_t *__restrict__ mask) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint64_t q[LEN];
#pragma unroll
  for (int w = 0; w < LEN; ++w) q[w] = onv[i * LEN + w];
  const int64_t r = hash_find<LEN>(table, cap, q);
  idx[i] = r;
  mask[i] = r >= 0;
}

}  // namespace pynqs

using namespace pynqs;

extern "C" int64_t pynqs_hash_bytes(int64_t nkeys, int sorb) {
  if (nkeys < 0 || sorb < 1 || sorb > kMaxSorb) return -1;
  const int len = (sorb - 1) / 64 + 1;
  return (int64_t)(hash_capacity(nkeys) * (uint64_t)hash_slot_words(len) * 8 + hash_filter_bits(nkeys) / 8 + hash_filter2_bits(nkeys) / 8 +
                   2 * (size_t)hash_string_bits_if(nkeys) / 8);
}

extern "C" int pynqs_hash_build(const uint64_t *keys, int64_t nkeys, int sorb, void *table, void *stream) {
  pynqs::DeviceScope device_scope_(keys);
  if (nkeys < 0 || sorb < 1 || sorb > kMaxSorb) return set_error(PYNQS_EINVAL, "bad nkeys/sorb");
  if (!table || (nkeys > 0 && !keys)) return set_error(PYNQS_EINVAL, "null pointer");
  const int len = (sorb - 1) / 64 + 1;
  const uint64_t cap = hash_capacity(nkeys);
  hipStream_t st = (hipStream_t)stream;
  if ((uintptr_t)table & 15u) return set_error(PYNQS_EINVAL, "table must be 16-byte aligned");
  const size_t slot_bytes = cap * (size_t)hash_slot_words(len) * 8;
  const uint32_t fbits = hash_filter_bits(nkeys);
  if (hipMemsetAsync(table, 0xFF, slot_bytes, st) != hipSuccess) return check_launch("hash memset");
  const uint32_t f2bits = hash_filter2_bits(nkeys), sbits = hash_string_bits_if(nkeys);
  if ((fbits || f2bits) && hipMemsetAsync((char *)table + slot_bytes, 0, fbits / 8 + f2bits / 8 + 2 * (size_t)sbits / 8, st) != hipSuccess)
    return check_launch("filter memset");
  if (nkeys == 0) return PYNQS_OK;
  const uint32_t grid = (uint32_t)((nkeys + kBlock - 1) / kBlock);
  DISPATCH_LEN(len, hipLaunchKernelGGL((hash_build_kernel<LEN>), dim3(grid), dim3(kBlock), 0, st, keys, nkeys, cap, (uint64_t *)table, fbits, f2bits, sbits));
  return check_launch("hash_build");
}

extern "C" int pynqs_hash_lookup(const void *table, int64_t nkeys, const uint64_t *onv, int64_t n, int sorb, int64_t *idx,
                                 uint8_t *mask, void *stream) {
  pynqs::DeviceScope device_scope_(table);
  if (nkeys < 0 || n < 0 || sorb < 1 || sorb > kMaxSorb) return set_error(PYNQS_EINVAL, "bad nkeys/n/sorb");
  if (n == 0) return PYNQS_OK;
  if (!table || !onv || !idx || !mask) return set_error(PYNQS_EINVAL, "null pointer");
  const int len = (sorb - 1) / 64 + 1;
  const uint64_t grid = ((uint64_t)n + kBlock - 1) / kBlock;
  if (grid > 0x7fffffffull) return set_error(PYNQS_EINVAL, "n too large for one launch");
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_LEN(len, hipLaunchKernelGGL((hash_lookup_kernel<LEN>), dim3((uint32_t)grid), dim3(kBlock), 0, st, (const uint64_t *)table,
                                       hash_capacity(nkeys), onv, (uint64_t)n, idx, mask));
  return check_launch("hash_lookup");
}
