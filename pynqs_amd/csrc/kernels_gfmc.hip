// kernels_gfmc.hip -- the move of a Green's-function Monte-Carlo step (PyNQS gfmc/walker.py:260-279, sample_update):
//   beta = sum_k G[x][k];  index = first k with cumsum(G[x])[k] / beta >= u[x];  x_new = comb[x][index]
// The reference runs sum, cumsum, division, searchsorted and an advanced-index gather as five passes over the
// [n, ncomb] Green's-function matrix; here one workgroup per walker reads its row twice at most (once for the
// tile sums, then only the tile that holds the target), the row never leaves L2 in between.
//   1. every wave sums whole tiles of the row (a lane reads kPerLane consecutive values, 16-byte loads) -> LDS
//   2. the first wave scans the tile sums, finds the first tile WITH WEIGHT in which the running sum reaches u * beta,
//   3. re-reads that tile, scans it in column order and takes the first column WITH WEIGHT that reaches the target.
// The law (include/pynqs_amd.h): C_{k-1} - tau < u S <= C_k + tau with tau = m 2^-52 S, and G[index] > 0 unless index = 0.
// Every running sum compared with the target is a plain sum of the row's entries in some order (no difference of sums), so
// each is within (m - 1) 2^-53 S of its exact value.  The scans add in trees that differ from lane to lane, so across a
// zero-weight column (or an empty tile) the running sum may move by an ulp in either direction: only entries with weight
// are candidates, and where none reaches the target the last one with weight is taken, at tile level and inside the tile.
// A row of sum zero goes to index 0, and so does u = 0.
// Memory-bound: 8 B per matrix element, once.
#include "detcore.h"
#include "launch.h"

namespace pynqs {

constexpr int kGfmcMaxTiles = 1024;

__device__ __forceinline__ double wave_incl_scan(double v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// FROM_RANK: there is no comb array (the row came from the fused Green's-function kernel, pynqs_green_rbm): `comb` then holds the
// n walkers themselves and x_new is the excitation of rank index - 1 of the walker (column 0 = the walker).
template <int LEN, bool FROM_RANK>
__global__ __launch_bounds__(kBlock) void gfmc_sample_kernel(const double *__restrict__ gk, int64_t m, uint32_t tile, uint32_t ntiles,
                                                             const double *__restrict__ rnd, const uint64_t *__restrict__ comb, SDParams p,
                                                             int64_t *__restrict__ index, double *__restrict__ beta,
                                                             uint64_t *__restrict__ x_new) {
  __shared__ double tsum[kGfmcMaxTiles];
  __shared__ double s_target, s_before;
  __shared__ uint32_t s_tile;
  const int64_t walker = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double *__restrict__ row = gk + walker * m;
  // 1. tile sums: a wave per tile, lanes over consecutive columns
  for (uint32_t t = wave; t < ntiles; t += kBlock / 64) {
    const int64_t c0 = (int64_t)t * tile, c1 = min(c0 + (int64_t)tile, m);
    double acc = 0.0;
    for (int64_t c = c0 + lane; c < c1; c += 64) acc += row[c];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
    if (lane == 0) tsum[t] = acc;
  }
  __syncthreads();
  // 2. scan of the tile sums by the first wave (kGfmcMaxTiles / 64 per lane, in tile order)
  if (wave == 0) {
    constexpr int kPer = kGfmcMaxTiles / 64;
    double loc[kPer], s = 0.0;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const uint32_t t = lane * kPer + i;
      loc[i] = t < ntiles ? tsum[t] : 0.0;
      s += loc[i];
    }
    const double incl = wave_incl_scan(s, lane);
    const double total = __shfl(incl, 63);
    const double target = rnd[walker] * total;
    const double lower = __shfl_up(incl, 1);
    double before = lane ? lower : 0.0;  // sum of the tiles of the lanes in front
    // first tile with weight whose inclusive sum reaches the target (tiles in order: lanes in order, then i in order), and the
    // last tile with weight at all
    uint32_t mine = 0xffffffffu, last = 0xffffffffu;
    double mine_before = 0.0, last_before = 0.0;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const uint32_t t = lane * kPer + i;
      if (loc[i] > 0.0) {
        if (mine == 0xffffffffu && before + loc[i] >= target) { mine = t; mine_before = before; }
        last = t; last_before = before;
      }
      before += loc[i];
    }
    const uint64_t have = __ballot(mine != 0xffffffffu);
    const uint64_t any = __ballot(last != 0xffffffffu);
    // no tile reaches the target: rounding put it beyond the last partial sum -> the last tile with weight, whose scan then
    // ends on the row's last column with weight.  No tile has weight: the row's sum is zero.  A target of zero (u = 0, or
    // the product underflows) is reached by the empty sum in front of column 0 already: index 0 with or without weight
    // there, which is what the reference's searchsorted(.., right=False) gives for u = 0 on a clamped diagonal.
    const int src = have ? __ffsll((long long)have) - 1 : any ? 63 - __clzll((long long)any) : 0;
    if (lane == src) {
      s_tile = !(target > 0.0) ? 0xffffffffu : have ? mine : any ? last : 0xffffffffu;
      s_before = have ? mine_before : last_before;
      s_target = target;
    }
    if (lane == 0) beta[walker] = total;
  }
  __syncthreads();
  // 3. inside the tile, in column order: chunks of 64 columns by the first wave
  if (wave == 0) {
    const uint32_t t = s_tile;
    const double target = s_target;
    double run = s_before;
    const int64_t c0 = (int64_t)t * tile, c1 = min(c0 + (int64_t)tile, m);
    int64_t found = -1, last_pos = -1;
    if (t == 0xffffffffu) found = 0;  // a row of sum zero, or a target of zero
    for (int64_t c = c0; c < c1 && found < 0; c += 64) {
      const double v = c + lane < c1 ? row[c + lane] : 0.0;
      const double incl = wave_incl_scan(v, lane) + run;
      const uint64_t pos = __ballot(v > 0.0);
      const uint64_t hit = pos & __ballot(incl >= target);
      if (hit) found = c + __ffsll((long long)hit) - 1;
      if (pos) last_pos = c + 63 - __clzll((long long)pos);
      run = __shfl(incl, 63);
    }
    // The tile was chosen from lane-strided partial sums, the scan above adds in column order: when the two roundings
    // disagree at the tile's end the target is "just behind" the tile's last weight -> take the last column that HAS
    // weight (the tile has one: its sum is positive; never a zero-weight column, which the reference's searchsorted
    // cannot return either)
    if (found < 0) found = last_pos >= 0 ? last_pos : 0;
    if (lane == 0) index[walker] = found;
    if constexpr (FROM_RANK) {
      if (lane == 0) {
        uint64_t x[LEN];
#pragma unroll
        for (int i = 0; i < LEN; ++i) x[i] = comb[walker * LEN + i];
        if (found > 0) excite_by_rank<LEN>(x, (uint32_t)(found - 1), p);
#pragma unroll
        for (int i = 0; i < LEN; ++i) x_new[walker * LEN + i] = x[i];
      }
    } else {
      if (lane < LEN) x_new[walker * LEN + lane] = comb[(walker * m + found) * LEN + lane];
    }
  }
}

}  // namespace pynqs

using namespace pynqs;

template <bool FROM_RANK>
static int gfmc_sample_impl(const double *green, int64_t n, int64_t ncomb, const double *rand_num, const uint64_t *comb, int sorb,
                            const SDParams &p, int64_t *index, double *beta, uint64_t *x_new, void *stream) {
  pynqs::DeviceScope device_scope_(green);
  if (n < 0 || ncomb < 1 || sorb < 1 || sorb > kMaxSorb) return set_error(PYNQS_EINVAL, "bad n / ncomb / sorb");
  if (n == 0) return PYNQS_OK;
  if (!green || !rand_num || !comb || !index || !beta || !x_new) return set_error(PYNQS_EINVAL, "null pointer");
  if (n > 0x7fffffffll) return set_error(PYNQS_EINVAL, "n too large for one launch");
  // tiles of a multiple of 256 columns, at most kGfmcMaxTiles of them
  uint32_t tile = 256;
  while ((ncomb + tile - 1) / tile > kGfmcMaxTiles) tile *= 2;
  const uint32_t ntiles = (uint32_t)((ncomb + tile - 1) / tile);
  const int len = (sorb - 1) / 64 + 1;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_LEN(len, hipLaunchKernelGGL((gfmc_sample_kernel<LEN, FROM_RANK>), dim3((uint32_t)n), dim3(kBlock), 0, st, green, ncomb, tile, ntiles,
                                       rand_num, comb, p, index, beta, x_new));
  return check_launch("gfmc_sample");
}

extern "C" int pynqs_gfmc_sample(const double *green, int64_t n, int64_t ncomb, const double *rand_num, const uint64_t *comb, int sorb,
                                 int64_t *index, double *beta, uint64_t *x_new, void *stream) {
  SDParams p = {};
  return gfmc_sample_impl<false>(green, n, ncomb, rand_num, comb, sorb, p, index, beta, x_new, stream);
}

extern "C" int pynqs_gfmc_sample_rank(const double *green, int64_t n, const double *rand_num, const uint64_t *bra, int sorb, int nele,
                                      int noA, int noB, int64_t *index, double *beta, uint64_t *x_new, void *stream) {
  SDParams p;
  if (!make_sd_params(sorb, nele, noA, noB, &p)) return set_error(PYNQS_EINVAL, "bad sorb/noA/noB");
  return gfmc_sample_impl<true>(green, n, (int64_t)p.nsd + 1, rand_num, bra, sorb, p, index, beta, x_new, stream);
}

// -------------------------------------------------------------------------------------------------
// Weighted moments of the local energies for the statistics all-reduce (utils/stats/dist_stats.py:18-79):
//   out[0..3] = sum_i p_i Re x_i,  sum_i p_i Im x_i,  sum_i p_i |x_i|^2,  sum_i p_i
// in one pass and a fixed order of additions (per-lane strided sums, wave butterfly, waves, then the blocks' partial
// sums by the last block to finish): the ~10 small torch kernels this replaces cost 0.2 ms per step, a third of the
// fused sample-space step.  out has room for 4 * (kMomentBlocks + 1) doubles (the partials follow the result) and
// one counter word.
namespace pynqs {

constexpr int kMomentBlocks = 128;

// mean, var = E|O|^2 - |E O|^2 (2 - sum p), sd, se from the (all-reduced) moments: one thread instead of ten torch launches
__device__ __forceinline__ void stats_finish(const double *m, double inv_world, double counts, double *__restrict__ out) {
  const double re = m[0] * inv_world, im = m[1] * inv_world, m2 = m[2] * inv_world, ps = m[3] * inv_world;
  double var = m2 - (re * re + im * im) * (2.0 - ps);
  var = var > 0.0 ? var : 0.0;
  const double sd = sqrt(var);
  out[0] = re; out[1] = im; out[2] = var; out[3] = sd; out[4] = sd / sqrt(counts);
}

// FINISH (one rank: nothing happens between the moments and the closing arithmetic): the block that takes the last ticket also does
// stats_finish on the four sums it has just formed -- the same additions in the same order, the same closing arithmetic, one launch less.
template <bool CPLX, bool FINISH>
__global__ __launch_bounds__(kBlock) void moments_kernel(const double *__restrict__ x, const double *__restrict__ prob, int64_t n,
                                                         double *__restrict__ out, unsigned int *__restrict__ done, double inv_world,
                                                         double counts, double *__restrict__ out5) {
  __shared__ double red[4][kBlock / 64];
  __shared__ bool last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * kBlock + tid; i < n; i += (int64_t)gridDim.x * kBlock) {
    const double p = prob[i];
    const double re = CPLX ? x[2 * i] : x[i], im = CPLX ? x[2 * i + 1] : 0.0;
    s[0] += p * re; s[1] += p * im; s[2] += p * (re * re + im * im); s[3] += p;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s[k] += __shfl_xor(s[k], d);
    if (lane == 0) red[k][wave] = s[k];
  }
  __syncthreads();
  if (tid < 4) {
    double t = 0.0;
    for (int w = 0; w < kBlock / 64; ++w) t += red[tid][w];
    out[4 * (1 + blockIdx.x) + tid] = t;
  }
  __threadfence();
  __syncthreads();
  if (tid == 0) last = atomicAdd(done, 1u) == gridDim.x - 1;
  __syncthreads();
  if (last) {
    __threadfence();
    if (tid < 4) {
      double t = 0.0;
      for (unsigned b = 0; b < gridDim.x; ++b) t += out[4 * (1 + b) + tid];  // block order: reproducible
      out[tid] = t;
      if constexpr (FINISH) red[0][tid] = t;
    }
    if (tid == 0) *done = 0;  // ready for the next call
    if constexpr (FINISH) {
      __syncthreads();  // (`last` is the same for the whole block)
      if (tid == 0) stats_finish(&red[0][0], inv_world, counts, out5);
    }
  }
}

// The same sums by ONE workgroup of 1024 threads, for n <= kMomentBlocks * kBlock (every thread of the form above then holds at most one
// element): no ticket, no fence, no read-back of the partial sums.  `blocks` is the grid the form above would take; its blocks x 4 waves
// are played by the 16 waves here, eight at a time, all loads issued up front.  The 8 x 4 butterflies of such a batch are done together:
// at distance d a lane keeps one of two vectors and hands the other to its partner (the lane bit picks which), so each step halves the
// number of vectors and costs one shuffle per remaining vector -- 32 shuffles instead of 192 -- and every value is the one the plain
// butterfly gives that lane for that vector (x[l] + x[l ^ d], the same two summands).  Then the four wave sums per block in wave order
// and the blocks' sums in block order, as above: out[0..3], the partial sums behind them and out5 are the same bit for bit.
constexpr int kMomentsGroupThreads = 1024;
constexpr int kMomentsBatch = 8;  // virtual waves per wave and batch

template <bool CPLX, bool FINISH>
__global__ __launch_bounds__(kMomentsGroupThreads) void moments_onegroup_kernel(const double *__restrict__ x, const double *__restrict__ prob,
                                                                                int64_t n, int blocks, double *__restrict__ out,
                                                                                double inv_world, double counts, double *__restrict__ out5) {
  constexpr int NW = kMomentsGroupThreads / 64, VW = kBlock / 64;  // waves here; waves of a block of the form above
  __shared__ double wsum[kMomentBlocks * VW][4];
  __shared__ double part[kMomentBlocks][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = blocks * VW;
  for (int v0 = 0; v0 < V; v0 += NW * kMomentsBatch) {
    double a[4 * kMomentsBatch];  // vector 4 slot + k
    double pv[kMomentsBatch], rv[kMomentsBatch], iv[kMomentsBatch];
#pragma unroll
    for (int sl = 0; sl < kMomentsBatch; ++sl) {
      const int64_t i = (int64_t)(v0 + wave * kMomentsBatch + sl) * 64 + lane;  // (v < V or not: i < n decides)
      const bool in = i < n && v0 + wave * kMomentsBatch + sl < V;
      pv[sl] = in ? prob[i] : 0.0;
      rv[sl] = in ? (CPLX ? x[2 * i] : x[i]) : 0.0;
      iv[sl] = CPLX && in ? x[2 * i + 1] : 0.0;
    }
#pragma unroll
    for (int sl = 0; sl < kMomentsBatch; ++sl) {
      const int64_t i = (int64_t)(v0 + wave * kMomentsBatch + sl) * 64 + lane;
      double s[4] = {0.0, 0.0, 0.0, 0.0};
      if (i < n && v0 + wave * kMomentsBatch + sl < V) {
        const double p = pv[sl];
        const double re = rv[sl], im = CPLX ? iv[sl] : 0.0;
        s[0] += p * re; s[1] += p * im; s[2] += p * (re * re + im * im); s[3] += p;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) a[4 * sl + k] = s[k];
    }
    // distance 32 .. 2: the lane bit picks the vector kept
#pragma unroll
    for (int d = 32, m = 4 * kMomentsBatch; m > 1; d >>= 1, m >>= 1) {
      const bool hi = (lane & d) != 0;
#pragma unroll
      for (int j = 0; j < m / 2; ++j) {
        const double keep = hi ? a[2 * j + 1] : a[2 * j], send = hi ? a[2 * j] : a[2 * j + 1];
        a[j] = keep + __shfl_xor(send, d);
      }
    }
    static_assert(4 * kMomentsBatch == 32, "five halving steps, then distance 1");
    a[0] += __shfl_xor(a[0], 1);
    // this lane's vector: bits (32, 16) of the lane are k, bits (8, 4, 2) the slot
    const int k = ((lane >> 5) & 1) | (((lane >> 4) & 1) << 1);
    const int sl = ((lane >> 3) & 1) | (((lane >> 2) & 1) << 1) | (((lane >> 1) & 1) << 2);
    const int v = v0 + wave * kMomentsBatch + sl;
    if (!(lane & 1) && v < V) wsum[v][k] = a[0];
  }
  __syncthreads();
  if (tid < blocks * 4) {
    const int b = tid >> 2, k = tid & 3;
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < VW; ++w) t += wsum[b * VW + w][k];
    out[4 * (1 + b) + k] = t;
    part[b][k] = t;
  }
  __syncthreads();
  if (tid < 4) {
    double t = 0.0;
    for (int b = 0; b < blocks; ++b) t += part[b][tid];  // block order: reproducible
    out[tid] = t;
    if constexpr (FINISH) wsum[0][tid] = t;
  }
  if constexpr (FINISH) {
    __syncthreads();
    if (tid == 0) stats_finish(&wsum[0][0], inv_world, counts, out5);
  }
}

__global__ void stats_finish_kernel(const double *__restrict__ m, double inv_world, double counts, double *__restrict__ out) {
  stats_finish(m, inv_world, counts, out);
}

}  // namespace pynqs

extern "C" int pynqs_stats_finish(const double *moments, double inv_world, double counts, double *out5, void *stream) {
  pynqs::DeviceScope device_scope_(moments);
  if (!moments || !out5 || !(counts > 0.0)) return set_error(PYNQS_EINVAL, "bad arguments");
  hipLaunchKernelGGL(stats_finish_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, moments, inv_world, counts, out5);
  return check_launch("stats_finish");
}

extern "C" int64_t pynqs_moments_workspace(void) { return 8 * 4 * (pynqs::kMomentBlocks + 1) + 8; }

// n up to which the single-workgroup form is taken: all it can hold.  Measured (profiles/backhalf_trace.txt): 5.7 against 10.3 us per call
// at n = 8192, 9.3 against 16.4 at 16384, 16.3 against 28.7 at 32768 -- it is the faster one wherever it runs.
constexpr int64_t kMomentsOneGroupMax = (int64_t)kMomentBlocks * kBlock;

extern "C" int64_t pynqs_moments_onegroup_max(void) { return kMomentsOneGroupMax; }

static int weighted_moments_launch(const double *x, int is_complex, const double *prob, int64_t n, void *workspace, bool finish, double inv_world,
                                   double counts, double *out5, int form, void *stream) {
  pynqs::DeviceScope device_scope_(x);
  if (n < 0) return set_error(PYNQS_EINVAL, "bad n");
  if (!workspace || (n > 0 && (!x || !prob))) return set_error(PYNQS_EINVAL, "null pointer");
  if (finish && (!out5 || !(counts > 0.0))) return set_error(PYNQS_EINVAL, "bad arguments");
  if (form < PYNQS_MOMENTS_AUTO || form > PYNQS_MOMENTS_ONEGROUP || (form == PYNQS_MOMENTS_ONEGROUP && n > (int64_t)kMomentBlocks * kBlock))
    return set_error(PYNQS_EINVAL, "bad form (the single-workgroup form takes n <= 32768)");
  double *out = (double *)workspace;
  unsigned int *done = (unsigned int *)(out + 4 * (kMomentBlocks + 1));
  int64_t blocks = (n + kBlock - 1) / kBlock;
  if (blocks > kMomentBlocks) blocks = kMomentBlocks;
  if (blocks < 1) blocks = 1;
  hipStream_t st = (hipStream_t)stream;
  if (form == PYNQS_MOMENTS_ONEGROUP || (form == PYNQS_MOMENTS_AUTO && n <= kMomentsOneGroupMax)) {
#define PYNQS_MK(C, F)                                                                                                                    \
  hipLaunchKernelGGL((moments_onegroup_kernel<C, F>), dim3(1), dim3(kMomentsGroupThreads), 0, st, x, prob, n, (int)blocks, out, inv_world, \
                     counts, out5)
    if (finish) { if (is_complex) PYNQS_MK(true, true); else PYNQS_MK(false, true); }
    else { if (is_complex) PYNQS_MK(true, false); else PYNQS_MK(false, false); }
#undef PYNQS_MK
    return check_launch("weighted_moments");
  }
#define PYNQS_MK(C, F) \
  hipLaunchKernelGGL((moments_kernel<C, F>), dim3((uint32_t)blocks), dim3(kBlock), 0, st, x, prob, n, out, done, inv_world, counts, out5)
  if (finish) { if (is_complex) PYNQS_MK(true, true); else PYNQS_MK(false, true); }
  else { if (is_complex) PYNQS_MK(true, false); else PYNQS_MK(false, false); }
#undef PYNQS_MK
  return check_launch("weighted_moments");
}

extern "C" int pynqs_weighted_moments(const double *x, int is_complex, const double *prob, int64_t n, void *workspace, void *stream) {
  return weighted_moments_launch(x, is_complex, prob, n, workspace, false, 1.0, 1.0, nullptr, PYNQS_MOMENTS_AUTO, stream);
}

// pynqs_weighted_moments followed by pynqs_stats_finish in ONE launch (for one rank, where no all-reduce comes between them): the moments
// land in the workspace as before, out5 gets bit for bit what the two calls give
extern "C" int pynqs_weighted_moments_finish(const double *x, int is_complex, const double *prob, int64_t n, void *workspace, double inv_world,
                                             double counts, double *out5, void *stream) {
  return weighted_moments_launch(x, is_complex, prob, n, workspace, true, inv_world, counts, out5, PYNQS_MOMENTS_AUTO, stream);
}

// either of the two with the form chosen per call (out5 NULL: the moments alone)
extern "C" int pynqs_weighted_moments_form(const double *x, int is_complex, const double *prob, int64_t n, void *workspace, double inv_world,
                                           double counts, double *out5, int form, void *stream) {
  return weighted_moments_launch(x, is_complex, prob, n, workspace, out5 != nullptr, inv_world, counts, out5, form, stream);
}
