// rbm_tiles.h -- what the two fused RBM local-energy kernels (kernels_rbm.hip: real parameters; kernels_rbm_complex.hip: complex
// parameters) share because it does not depend on the number type: the cut of a walker's excitations into blocks and tiles, phase A's
// diagonal and singles, the fixed-order sum over waves, the tail of the LDS layout, and on the host the chunk rule, the workgroup size
// of the resident form, the argument checks and the launch.  FB = entries of a class's "fast" excitation table a lane owns: 4 (real,
// 4 x 4 blocks) or 2 (complex, 2 x 4 blocks); the slow side is 4 in both.
// NOT here, on purpose: the theta loops, window builders, hidden-unit loops, epilogues and window-size rules, tuned per number type;
// and the per-lane code of the tile loop (block decode, entry reads, parity, plan gather, q' row): as shared helpers it is the same
// arithmetic, but the real kernel's register allocation at the 128-VGPR line changes with it (the block decode alone: spills or
// scratch of 21 of its 30 instantiations).  What is here leaves every instantiation's registers, scratch and occupancy as they were.
#pragma once

#include "detcore.h"
#include "launch.h"
#include "plan.h"
#include "plan_dev.h"

namespace pynqs {

// How the excitations of one walker are cut into FB x 4 blocks: class k has nbf[k] x nbs[k] blocks
// (k = 0 singles x nothing, 1 alpha-alpha, 2 beta-beta, 3 alpha-beta); b[k] = cumulative block counts.
template <int FB>
struct RbmBlocks {
  uint32_t nbf[4];
  uint32_t b[4];
  uint32_t ntiles;  // tiles of 64 blocks
  MagicDiv dv[4];   // division by nbf[k]
};

template <int FB>
static inline RbmBlocks<FB> make_rbm_blocks(const SDParams &p) {
  RbmBlocks<FB> B;
  const uint32_t nf[4] = {p.d1, (uint32_t)p.noAA, (uint32_t)p.noBB, (uint32_t)p.nSa};
  const uint32_t ns[4] = {p.d1 ? 1u : 0u, (uint32_t)p.nvAA, (uint32_t)p.nvBB, (uint32_t)p.nSb};
  uint32_t acc = 0;
  for (int k = 0; k < 4; ++k) {
    B.nbf[k] = (nf[k] + FB - 1) / FB;
    B.dv[k] = make_magic(B.nbf[k]);
    acc += B.nbf[k] * ((ns[k] + 3) / 4);
    B.b[k] = acc;
  }
  B.ntiles = (acc + 63) / 64;
  return B;
}

// Both kernels' LDS starts with the walker tables; the RBM part follows 16-byte aligned (rbm_q_offset) and ends with this trailer:
// red [16 waves][nred doubles] for the sums over waves, then the counters of the tiles and of the singles' tiles (16 bytes).
// nred = 1 (real: 144 bytes) or 2 (complex: 272 bytes).
__host__ __device__ constexpr size_t rbm_trailer_bytes(int nred) { return 8 * 16 * (size_t)nred + 16; }
__host__ __device__ inline size_t rbm_q_offset(const SDParams &p) { return (lds_fixed_bytes(p) + 15) & ~(size_t)15; }

struct RbmTrailer {
  double *red;
  uint32_t *next_tile, *next_single;
};
__device__ __forceinline__ RbmTrailer rbm_trailer(unsigned char *smem, size_t lds_end, int nred) {  // lds_end = the kernel's lds_bytes_*
  double *red = reinterpret_cast<double *>(smem + lds_end - rbm_trailer_bytes(nred));
  uint32_t *counters = reinterpret_cast<uint32_t *>(red + 16 * nred);
  return RbmTrailer{red, counters, counters + 1};
}

// Phase A's jobs that do not depend on the amplitude; no barrier inside.  Only the workgroups whose chunk holds tiles of singles (and
// chunk 0, for the diagonal) need them: need_hs.  The last wave computes <x|H|x> -> hs[0] (an ordered sum of nele(nele+1)/2 terms by one
// lane: the longest serial job) while the others run the kernel's theta loop; then every wave, as it becomes free, pulls singles in
// tiles of 64 from the counter -> hs[1 + r].
template <int FB>
__device__ __forceinline__ bool rbm_needs_hs(const RbmBlocks<FB> &B, uint32_t chunk) {
  return chunk < max((B.b[0] + 63) / 64, 1u);  // (tiles of singles)
}

__device__ __forceinline__ void rbm_diagonal(bool need_hs, int lane, const SDParams &p, const PlanLayout &pl, const LdsLayout &L,
                                             const double *plan, double *hs) {
  if (need_hs) {
    const double hii = fast_diag<double>(p, pl, L, plan);
    if (lane == 0) hs[0] = hii;
  }
}

__device__ __forceinline__ void rbm_singles(bool need_hs, int lane, const SDParams &p, const PlanLayout &pl, const LdsLayout &L, int nocc,
                                            const double *plan, double *hs, uint32_t *next_single) {
  if (need_hs) {
    const uint32_t nst = (p.d1 + 63) / 64;
    for (;;) {
      uint32_t t = 0;
      if (lane == 0) t = atomicAdd(next_single, 1u);
      t = __builtin_amdgcn_readfirstlane(t);
      if (t >= nst) break;
      if (t * 64 + lane < p.d1) hs[1 + t * 64 + lane] = fast_single<double>(t * 64 + lane, p, pl, L, nocc, plan);
    }
  }
}

// Sum over the waves of a workgroup of v (a double, or a vector of doubles summed by component; each wave's lanes already hold the
// wave's sum, by __shfl_xor 32..1) in a fixed order: waves 0..nwaves-1 by thread 0, where the sum is valid.  Workgroup-uniform calls
// only (two barriers); red: the trailer's.
template <typename T>
__device__ __forceinline__ T rbm_over_waves(T v, double *red, int tid, int nwaves) {
  constexpr int N = sizeof(T) / sizeof(double);  // (red is 8-byte aligned only: by doubles)
  double c[N];
  __builtin_memcpy(c, &v, sizeof(T));
  __syncthreads();
  if ((tid & 63) == 0)
#pragma unroll
    for (int k = 0; k < N; ++k) red[N * (tid >> 6) + k] = c[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) c[k] = 0.0;
  if (tid == 0)
    for (int w = 0; w < nwaves; ++w)
#pragma unroll
      for (int k = 0; k < N; ++k) c[k] += red[N * w + k];
  __builtin_memcpy(&v, c, sizeof(T));
  return v;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
constexpr size_t kRbmMaxLds = 158 * 1024;  // of the CU's 160 KiB

// Workgroups per walker.  Few walkers: a walker's tiles are cut over several workgroups, each of which repeats the per-walker set-up
// and adds its part with an atomic; never fewer than 4 tiles per workgroup.
static inline uint32_t rbm_chunks(uint32_t ntiles, int64_t nbatch) {
  uint32_t nchunks = 1;
  if (nbatch < 1024) {
    nchunks = (uint32_t)((1024 + nbatch - 1) / nbatch);
    const uint32_t maxc = ntiles / 4 > 0 ? ntiles / 4 : 1;
    if (nchunks > maxc) nchunks = maxc;
  }
  return nchunks;
}

// Workgroup size when all of q' is resident: the one that puts the most waves on a CU (the registers allow 16; a workgroup's waves
// share its `lds` bytes), as long as the workgroup has at least two tiles per wave.  Fe2S2 (31 KiB): 256 threads, 4 workgroups per CU;
// sorb 56 with 112 hidden units (58 KiB): two workgroups per CU -> 512 threads.  blk_env (the kernel's PYNQS_*_BLOCK) overrides with
// max_threads or a half or a quarter of it.
static inline uint32_t rbm_resident_threads(size_t lds, uint32_t tiles, uint32_t max_threads, int blk_env) {
  if (blk_env > 0 && ((uint32_t)blk_env == max_threads || (uint32_t)blk_env == max_threads / 2 || (uint32_t)blk_env == max_threads / 4))
    return (uint32_t)blk_env;
  uint32_t threads = kBlock;
  size_t best = 0;
  for (uint32_t b = kBlock; b <= max_threads; b *= 2) {
    size_t waves = (160 * 1024 / (lds + 256)) * (b / 64);
    if (waves > 16) waves = 16;
    if (b > kBlock && tiles < 2 * (b / 64)) break;
    if (waves > best) { best = waves; threads = b; }
  }
  return threads;
}

// What every entry point of the two kernels works out first: the excitation tables' parameters and the layouts of the plan and of
// the RBM table (Layout / make_layout: rbm.h).  nullptr, or what is wrong with the arguments.
template <typename Layout>
struct RbmSystem {
  SDParams p;
  PlanLayout pl;
  Layout rl;
};

template <typename Layout>
static inline const char *rbm_system(int sorb, int nele, int noA, int noB, int nhidden, bool (*make_layout)(int, int, Layout *),
                                     RbmSystem<Layout> *s) {
  if (!make_sd_params(sorb, nele, noA, noB, &s->p)) return "bad sorb/noA/noB";
  if (!make_plan_layout(sorb, &s->pl)) return "plan needs an even sorb in [2, 192]";
  if (!make_layout(sorb, nhidden, &s->rl)) return "bad nhidden";
  return nullptr;
}

// the checks of a launch after rbm_system (an empty batch may come with null pointers: the caller returns PYNQS_OK for it)
static inline int rbm_batch(int64_t nbatch, int64_t max_nbatch, const void *bra, const void *plan, const void *table, const void *eloc) {
  if (nbatch < 0 || nbatch > max_nbatch) return set_error(PYNQS_EINVAL, "bad nbatch");
  if (nbatch > 0 && (!bra || !plan || !table || !eloc)) return set_error(PYNQS_EINVAL, "null pointer");
  return PYNQS_OK;
}

// grid = nbatch x nchunks workgroups; chunked launches add into eloc (out_bytes per walker) with atomics: cleared first
static inline int rbm_grid(int64_t nbatch, uint32_t nchunks, double *eloc, size_t out_bytes, hipStream_t st, uint32_t *grid) {
  const uint64_t g = (uint64_t)nbatch * nchunks;
  if (g > 0x7fffffffull) return set_error(PYNQS_EINVAL, "grid too large");
  *grid = (uint32_t)g;
  if (nchunks > 1 && hipMemsetAsync(eloc, 0, out_bytes * (size_t)nbatch, st) != hipSuccess) return check_launch("memset");
  return PYNQS_OK;
}

// launch with `lds` bytes of dynamic LDS (above 64 KiB a kernel has to be told)
template <typename Kernel, typename... Args>
static inline int rbm_launch(const char *what, Kernel kernel, uint32_t grid, uint32_t threads, size_t lds, hipStream_t st, Args... args) {
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return check_launch("hipFuncSetAttribute");
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, st, args...);
  return check_launch(what);
}

}  // namespace pynqs
