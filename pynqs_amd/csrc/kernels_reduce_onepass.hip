// kernels_reduce_onepass.hip -- the REDUCE front end of the local energy in ONE launch: everything between the walkers and
// the ansatz' forward (vmc/energy/eloc.py:205-324 _reduce_psi, `Func` of vmc/energy/flip.py:29-63, onv_to_tensor).
//
// Round 2 ran this as count -> host read-back -> emit (-> count_sums -> torch.multinomial -> draw) -> unique_insert ->
// unique_first -> onv_to_pm1 plus ~80 small torch kernels, and enumerated every row two or three times.  Here one workgroup
// owns a (walker, chunk) and
//   phase A  visits every column once on the tile scheduler (plan_tiles.h).  Kept columns (|H| >= eps) become records:
//            column 0, the singles and the few unpaired doubles have a FIXED slot each (they are produced by heavy tiles
//            that must not hold anybody up); the kept doubles of a tile wait in the wave's LDS scratch until the tile is
//            finished, get their place by a decoupled look-back over the tiles' counts in LDS (a wave never waits for more
//            than the COUNT of an earlier tile, which is published before anything else), and are written in tile order:
//            no atomics on the output position, no second pass, reproducible.  Sub-eps |H| are summed per tile into LDS.
//   phase B  (eps_sample > 0) scans the tile sums, draws the N uniforms of the reference's torch.multinomial over the tiles
//            (counter-based generator) and turns the per-tile draw counts into slot offsets -- all in LDS.
//   phase C  re-visits only the tiles that received draws and draws inside them (the machinery of kernels_reduce_sample.hip).
// Every record's determinant is looked up in the wave-function table (if given), else inserted into a de-duplication table;
// the winner of a slot takes the next row of the distinct list and the wave writes its +1/-1 row (the ansatz' input).
// A second, small kernel (reduce_contract_kernel) forms E_loc from the records and the amplitudes of the distinct rows.
#include "detcore.h"
#include "launch.h"
#include "plan.h"
#include "plan_dev.h"
#include "plan_tiles.h"
#include "reduce_common.h"
#include "reduce_list.h"

namespace pynqs {



// ---- phase A -------------------------------------------------------------------------------------------------------
// Wave-private LDS: the wave's quarter of the singles staging scratch doubles as the buffer of a doubles tile's kept columns
// (column, value); one word for the running count.

template <int LEN, typename T, bool SAMPLED>
struct KeepSink {
  T eps;
  uint32_t chunk, nchunks, tS;
  int64_t seg_base;
  volatile uint32_t *run;  // kept columns of the current doubles tile (wave-private LDS)
  WinnerList wl;
  uint32_t *bufc;
  T *bufh;
  volatile uint32_t *dstat;
  double *tsum;
  uint32_t *kept_total;
  const SDParams *p;
  const LdsLayout *L;
  const Walker<LEN> *wk;
  OnepassOut<T> o;
  uint32_t tile;
  double sub;

  // returns the de-duplication slot; unlisted: a new determinant whose row the caller has to allocate
  __device__ __forceinline__ int32_t record(int64_t g, uint32_t col, T h, const uint64_t (&ket)[LEN], bool &unlisted) const {
    o.rec_col[g] = (int32_t)col;
    o.rec_w[g] = h;
    if (o.rec_onv) {
#pragma unroll
      for (int i = 0; i < LEN; ++i) o.rec_onv[g * LEN + i] = ket[i];
    }
    const int32_t link = resolve_amplitude<LEN, T>(o, wl, ket, col, unlisted);
    o.rec_link[g] = link;
    return link;
  }

  // a column with a fixed slot (called from divergent code: any set of lanes)
  __device__ __forceinline__ void fixed_slot(uint32_t slot, uint32_t col, T h, const uint64_t (&ket)[LEN]) {
    const T a = fabs(h);
    if (!(a >= eps)) {
      if constexpr (SAMPLED) sub += (double)a;
      return;  // (the slot was pre-filled with -1)
    }
    bool unlisted;
    const int32_t link = record(seg_base + slot, col, h, ket, unlisted);
    if (unlisted) {  // (list full: this lane alone, inside divergent code -- rare)
      const int32_t r = atomicAdd(o.counters, 1);
      if (assign_row<LEN, T>(o, (uint32_t)link, r, ket) && o.uniq_pm1) {
        for (int j = 0; j < p->sorb; ++j) {
          const bool occ = (ket[j >> 6] >> (j & 63)) & 1ull;
          if (o.pm1_f32) reinterpret_cast<float *>(o.uniq_pm1)[(size_t)r * p->sorb + j] = occ ? 1.0f : -1.0f;
          else reinterpret_cast<double *>(o.uniq_pm1)[(size_t)r * p->sorb + j] = occ ? 1.0 : -1.0;
        }
      }
    }
  }

  __device__ __forceinline__ uint32_t advance(uint32_t total) const {
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)__ballot(1)) - 1;
    uint32_t before = 0;
    if (lane == leader) { before = *run; *run = before + total; }
    return __shfl(before, leader);
  }

  __device__ __forceinline__ void one(uint32_t col, T h, const uint64_t (&ket)[LEN]) {
    if (tile == 0) { fixed_slot(col == 0 ? 0u : 1u + (threadIdx.x & 63u), col, h, ket); return; }
    if (tile <= tS) {
      const uint32_t r0 = (chunk + (tile - 1) * nchunks) * kSinglesPerTile;
      fixed_slot(kFixedHead + (tile - 1) * kSinglesPerTile + (col - 1 - r0), col, h, ket);
      return;
    }
    const T a = fabs(h);
    const bool k = a >= eps;
    if constexpr (SAMPLED) { if (!k) sub += (double)a; }
    const uint64_t m = __ballot(k);
    if (!m) return;
    const uint32_t before = advance((uint32_t)__popcll(m));
    if (k) {
      const uint32_t at = before + __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
      bufc[at] = col;
      bufh[at] = h;
    }
  }
  __device__ __forceinline__ void two(uint32_t c0, T h0, const uint64_t (&)[LEN], uint32_t c1, T h1, const uint64_t (&)[LEN]) {
    const T a0 = fabs(h0), a1 = fabs(h1);
    const bool a = a0 >= eps, b = a1 >= eps;
    if constexpr (SAMPLED) sub += (a ? 0.0 : (double)a0) + (b ? 0.0 : (double)a1);
    const uint64_t ma = __ballot(a), mb = __ballot(b);
    if (!(ma | mb)) return;
    const uint32_t before = advance((uint32_t)(__popcll(ma) + __popcll(mb)));
    const uint64_t below = (1ull << (threadIdx.x & 63)) - 1ull;
    const uint32_t mine = before + __popcll(ma & below) + __popcll(mb & below);
    if (a) { bufc[mine] = c0; bufh[mine] = h0; }
    if (b) { bufc[mine + (a ? 1 : 0)] = c1; bufh[mine + (a ? 1 : 0)] = h1; }
  }
  __device__ __forceinline__ void pair(uint32_t col, T h0, T h1, const uint64_t (&k0)[LEN], const uint64_t (&k1)[LEN]) {
    two(col, h0, k0, col + 1, h1, k1);
  }

  // Exclusive prefix of the kept counts of the doubles tiles before tile d (decoupled look-back, one window of 64 tiles per step).
  __device__ __forceinline__ uint32_t lookback(uint32_t d, uint32_t c) const {
    const int lane = threadIdx.x & 63;
    if (d == 0 || (o.debug & 4u)) {
      if (lane == 0) dstat[d] = kStatP | c;
      return 0;
    }
    if (lane == 0) dstat[d] = kStatA | c;
    uint32_t excl = 0;
    int32_t top = (int32_t)d - 1;
    for (;;) {
      const int32_t idx = top - lane;
      const uint32_t s = idx >= 0 ? dstat[idx] : kStatP;  // below tile 0: an inclusive prefix of 0
      const uint64_t ready = __ballot(s != 0u);
      const uint64_t isP = __ballot((s & kStatP) != 0u);
      const int fp = isP ? __ffsll((long long)isP) - 1 : 64;  // nearest tile whose inclusive prefix is known
      const uint64_t need = fp >= 63 ? ~0ull : ((2ull << fp) - 1ull);
      if ((ready & need) != need) {
        __builtin_amdgcn_s_sleep(1);
        continue;
      }
      excl += op_wave_sum_shfl(lane <= fp ? (s & kStatMask) : 0u);
      if (fp < 64) break;
      top -= 64;
    }
    if (lane == 0) dstat[d] = kStatP | (excl + c);
    return excl;
  }

  __device__ __forceinline__ void flush() {  // wave-uniform
    if (tile == 0xffffffffu) return;
    const int lane = threadIdx.x & 63;
    if constexpr (SAMPLED) {
      const double s = op_wave_sum_shfl(sub);
      if (lane == 0) tsum[tile] = s;
    }
    wave_sync();
    if (tile <= tS) return;  // column 0, the singles and the unpaired doubles wrote their fixed slots themselves
    const uint32_t c = *run;
    const uint32_t excl = lookback(tile - 1 - tS, c);
    if (lane == 0 && c) atomicMax(kept_total, excl + c);
    for (uint32_t i0 = 0; i0 < c; i0 += 64) {
      const uint32_t i = i0 + lane;
      const bool act = i < c && excl + i < o.cap_d;
      bool unlisted = false;
      int32_t link = -1;
      uint64_t ket[LEN];
#pragma unroll
      for (int w = 0; w < LEN; ++w) ket[w] = 0ull;
      if (act) {
        const uint32_t col = bufc[i];
        const Excitation x = decode(col - 1, *p, *L);
        make_ket<LEN>(*wk, x, ket);
        link = record(seg_base + o.fixed + excl + i, col, bufh[i], ket, unlisted);
      }
      if (__ballot(unlisted)) allocate_now<LEN, T>(o, p->sorb, unlisted, (uint32_t)link, ket);
    }
  }
  __device__ __forceinline__ void tile_begin(uint32_t t) {
    flush();
    tile = t;
    sub = 0.0;
    if ((threadIdx.x & 63) == 0) *run = 0u;
    __builtin_amdgcn_wave_barrier();
  }
};

// ---- phase C: the draws inside a tile (same scheme as kernels_reduce_sample.hip: SampleSink) ------------------------------

template <int LEN, typename T>
struct DrawSink {
  T eps;
  DrawLds S;
  const SDParams *p;
  const LdsLayout *L;
  const Walker<LEN> *wk;
  const uint32_t *dinfo;  // LDS: slot offset << 16 | draws, per tile
  double scale;           // S_walker / N
  uint64_t key;
  int64_t sbase;          // first drawn-record slot of this walker
  OnepassOut<T> o;
  WinnerList wl;
  uint32_t tile;

  __device__ __forceinline__ void entry(uint32_t idx, uint32_t col, T h, double incl) const {
    S.prefix[idx] = incl;
    S.cs[idx] = col | (h < T(0) ? 0x80000000u : 0u);
  }
  __device__ __forceinline__ double width(T h) const {
    const T a = fabs(h);
    return a >= eps ? 0.0 : (double)a;
  }
  __device__ __forceinline__ void one(uint32_t col, T h, const uint64_t (&)[LEN]) const {
    const int lane = threadIdx.x & 63;
    uint64_t m = __ballot(1);
    const double w = width(h);
    while (m) {
      const int b = __ffsll((long long)m) - 1;
      m &= m - 1;
      if (lane == b) {
        const uint32_t idx = *S.ncols;
        const double incl = *S.run + w;
        entry(idx, col, h, incl);
        *S.ncols = idx + 1;
        *S.run = incl;
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  __device__ __forceinline__ void pair(uint32_t col, T h0, T h1, const uint64_t (&)[LEN], const uint64_t (&)[LEN]) const {
    const int lane = threadIdx.x & 63;
    const uint32_t nact = (uint32_t)__popcll(__ballot(1));
    const double w0 = width(h0), w1 = width(h1);
    const double incl = op_scan(w0 + w1, lane);
    const uint32_t base = *S.ncols;
    const double run = *S.run;
    entry(base + 2 * lane, col, h0, run + incl - w1);
    entry(base + 2 * lane + 1, col + 1, h1, run + incl);
    const double total = __shfl(incl, (int)nact - 1);
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) { *S.ncols = base + 2 * nact; *S.run = run + total; }
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ void two(uint32_t c0, T h0, const uint64_t (&)[LEN], uint32_t c1, T h1, const uint64_t (&)[LEN]) const {
    const int lane = threadIdx.x & 63;
    const double w0 = width(h0), w1 = width(h1);
    const double i0 = op_scan(w0, lane), t0 = __shfl(i0, 63);
    const double i1 = op_scan(w1, lane), t1 = __shfl(i1, 63);
    const uint32_t base = *S.ncols;
    const double run = *S.run;
    entry(base + lane, c0, h0, run + i0);
    entry(base + 64 + lane, c1, h1, run + t0 + i1);
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) { *S.ncols = base + 128; *S.run = run + t0 + t1; }
    __builtin_amdgcn_wave_barrier();
  }

  __device__ __forceinline__ void flush() {  // wave-uniform
    if (tile == 0xffffffffu) return;
    const int lane = threadIdx.x & 63;
    const uint32_t info = dinfo[tile];
    const uint32_t draws = info & 0xffffu;
    const uint32_t ncols = *S.ncols;
    const double total = *S.run;
    if (draws == 0 || ncols == 0 || !(total > 0.0)) return;
    for (uint32_t k = lane; k < draws; k += 64) {
      const uint64_t r = op_mix64(key ^ op_mix64(((uint64_t)tile << 32) | k));
      const double target = (double)(r >> 11) * 0x1.0p-53 * total;
      uint32_t lo = 0, hi = ncols;  // first idx with prefix[idx] > target
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (S.prefix[mid] > target) hi = mid; else lo = mid + 1;
      }
      if (lo >= ncols) lo = ncols - 1;
      while (lo > 0 && !(S.prefix[lo] > S.prefix[lo - 1])) --lo;  // rounding at the end: back to a column of positive width
      atomicAdd(&S.hits[lo], 1u);
    }
    __builtin_amdgcn_wave_barrier();
    int64_t pos = sbase + (info >> 16);
    for (uint32_t i0 = 0; i0 < ncols; i0 += 64) {
      const uint32_t idx = i0 + lane;
      const uint32_t hc = idx < ncols ? S.hits[idx] : 0u;
      const uint64_t m = __ballot(hc != 0u);
      bool unlisted = false;
      int32_t link = -1;
      uint64_t ket[LEN];
#pragma unroll
      for (int w = 0; w < LEN; ++w) ket[w] = 0ull;
      if (hc) {
        const uint32_t e = S.cs[idx], col = e & 0x7fffffffu;
        const int64_t at = pos + __popcll(m & ((1ull << lane) - 1ull));
        if (col == 0) {
#pragma unroll
          for (int i = 0; i < LEN; ++i) ket[i] = wk->w[i];
        } else {
          const Excitation x = decode(col - 1, *p, *L);
          make_ket<LEN>(*wk, x, ket);
        }
        o.srec_col[at] = (int32_t)col;
        const double v = scale * (double)hc;
        o.srec_w[at] = (T)((e >> 31) ? -v : v);
        if (o.srec_onv) {
#pragma unroll
          for (int i = 0; i < LEN; ++i) o.srec_onv[at * LEN + i] = ket[i];
        }
        link = resolve_amplitude<LEN, T>(o, wl, ket, col, unlisted);
        o.srec_link[at] = link;
      }
      if (__ballot(unlisted)) allocate_now<LEN, T>(o, p->sorb, unlisted, (uint32_t)link, ket);
      pos += __popcll(m);
    }
  }
  __device__ __forceinline__ bool skip_tile(uint32_t t) const { return (dinfo[t] & 0xffffu) == 0u; }
  __device__ __forceinline__ void tile_begin(uint32_t t) {
    flush();
    tile = t;
    if ((dinfo[t] & 0xffffu) == 0u) return;
    const int lane = threadIdx.x & 63;
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < kOneTileCols; i += 64) S.hits[i] = 0u;
    if (lane == 0) { *S.ncols = 0u; *S.run = 0.0; }
    __builtin_amdgcn_wave_barrier();
  }
};

// LDS after the walker tables and the staging scratch: dstat[max_tiles] | (SAMPLED) tsum[max_tiles] f64, dinfo[max_tiles], draw areas
__host__ __device__ inline size_t onepass_lds(const SDParams &p, size_t esz, uint32_t max_tiles, bool sampled, uint32_t wl_cap) {
  size_t b = (lds_bytes(p, esz) + 15) & ~(size_t)15;
  b += ((size_t)max_tiles * 4 + 15) & ~(size_t)15;
  if (sampled) {
    b += (size_t)max_tiles * 8;
    b += ((size_t)max_tiles * 4 + 15) & ~(size_t)15;
    b += (kBlock / 64) * kDrawLdsPerWave;
  }
  return b + (size_t)wl_cap * 8;
}

// entries of a workgroup's list of new determinants: what one phase can win (all its draws; a few hundred kept columns), within the
// LDS that is left
__host__ inline uint32_t winner_list_cap(int eps_sample) {
  uint32_t c = eps_sample > 256 ? (uint32_t)eps_sample : 256u;
  c = (c + 63u) & ~63u;
  return c > 2048u ? 2048u : c;
}

template <int LEN, typename T, bool SAMPLED>
__global__ __launch_bounds__(kBlock) void reduce_onepass_kernel(const uint64_t *__restrict__ bra, SDParams p, PlanLayout pl, uint32_t nchunks,
                                                                uint32_t chunk_len, uint32_t max_tiles, const T *__restrict__ plan, T eps,
                                                                uint32_t nsample, uint64_t seed, uint32_t wl_cap, OnepassOut<T> o) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ uint32_t next_tile, kept_total, wl_n;
  __shared__ int32_t wl_base;
  __shared__ uint32_t wave_run[kBlock / 64];
  __shared__ double s_part[kBlock / 64 + 1];
  __shared__ uint32_t s_parti[kBlock / 64 + 1];
  uint64_t walker;
  uint32_t chunk;
  map_workgroup(nchunks, false, walker, chunk);
  o.parent = (int32_t)walker;
  const uint64_t slot = walker * nchunks + chunk;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t seg_base = (int64_t)slot * ((int64_t)o.fixed + o.cap_d);
  if (tid == 0) { next_tile = 0; kept_total = 0; wl_n = 0; }
  unsigned char *extra = smem + ((lds_bytes(p, sizeof(T)) + 15) & ~(size_t)15);
  volatile uint32_t *dstat = reinterpret_cast<volatile uint32_t *>(extra);
  extra += ((size_t)max_tiles * 4 + 15) & ~(size_t)15;
  double *tsum = reinterpret_cast<double *>(extra);
  uint32_t *dinfo = reinterpret_cast<uint32_t *>(extra + (SAMPLED ? (size_t)max_tiles * 8 : 0));
  WinnerList wl;
  wl.n = &wl_n;
  wl.cap = wl_cap;
  wl.slot = reinterpret_cast<uint32_t *>(smem + onepass_lds(p, sizeof(T), max_tiles, SAMPLED, 0));
  wl.col = wl.slot + wl_cap;
  for (uint32_t i = tid; i < max_tiles; i += kBlock) {
    dstat[i] = 0u;
    if constexpr (SAMPLED) { tsum[i] = 0.0; dinfo[i] = 0u; }
  }
  for (uint32_t i = tid; i < o.fixed; i += kBlock) o.rec_col[seg_base + i] = -1;
  if constexpr (SAMPLED) {
    for (uint32_t i = tid; i < nsample; i += kBlock) o.srec_col[(int64_t)walker * nsample + i] = -1;
  }
  Walker<LEN> wk;
  load_walker<LEN>(bra + walker * LEN, wk);
  const LdsLayout L = carve_lds(smem, p);
  const int nocc = build_walker_tables<LEN>(wk, p, L);  // (ends with a barrier: the pre-fills above are done)

  const uint32_t tS_all = (p.d1 + kSinglesPerTile - 1) / kSinglesPerTile;
  const uint32_t tS = tS_all > chunk ? (tS_all - chunk + nchunks - 1) / nchunks : 0;
  T *quarter = reinterpret_cast<T *>(L.scratch) + wave * (kDiagTile / 4);
  {
    KeepSink<LEN, T, SAMPLED> sink;
    sink.eps = eps; sink.chunk = chunk; sink.nchunks = nchunks; sink.tS = tS; sink.seg_base = seg_base;
    sink.run = wave_run + wave; sink.wl = wl;
    sink.bufh = quarter;
    sink.bufc = reinterpret_cast<uint32_t *>(quarter + kOneTileCols);
    sink.dstat = dstat; sink.tsum = tsum; sink.kept_total = &kept_total;
    sink.p = &p; sink.L = &L; sink.wk = &wk; sink.o = o; sink.tile = 0xffffffffu; sink.sub = 0.0;
    visit_tiles<LEN, T>(p, pl, L, nocc, plan, wk, nchunks, chunk, chunk_len, 0u, &next_tile, sink);
    sink.flush();
  }
  flush_winner_list<LEN, T>(o, wl, &wl_base, p, L, wk);  // (barriers inside: phase A is over for every wave)
  if (tid == 0) {
    o.seg_count[slot] = (int32_t)kept_total;
    if (kept_total > o.cap_d) {  // (what the largest overflowing segment needed; 0 when everything fitted)
      atomicOr(reinterpret_cast<unsigned int *>(o.counters + 1), 1u);
      atomicMax(o.counters + 2, (int32_t)kept_total);
    }
  }
  if constexpr (SAMPLED) {
    // ---- phase B: inclusive scan of the tile sums (fixed order of additions), the N draws over the tiles, slot offsets ----
    const uint32_t per = (max_tiles + kBlock - 1) / kBlock;
    const uint32_t b0 = min((uint32_t)tid * per, max_tiles), b1 = min(b0 + per, max_tiles);
    double local = 0.0;
    for (uint32_t i = b0; i < b1; ++i) local += tsum[i];
    double incl = op_scan(local, lane);
    if (lane == 63) s_part[wave] = incl;
    __syncthreads();
    double before = 0.0, total = 0.0;
    for (int w = 0; w < kBlock / 64; ++w) {
      if (w < wave) before += s_part[w];
      total += s_part[w];
    }
    double run = before + incl - local;
    for (uint32_t i = b0; i < b1; ++i) { run += tsum[i]; tsum[i] = run; }
    __syncthreads();
    const double Srow = total;
    if (tid == 0 && o.row_sum) o.row_sum[walker] = Srow;
    const uint64_t key = op_mix64((o.seed_dev ? seed + *o.seed_dev : seed) ^ op_mix64(slot));
    if (Srow > 0.0) {
      for (uint32_t k = tid; k < nsample; k += kBlock) {
        const uint64_t r = op_mix64(key ^ op_mix64(0xffffffff00000000ull | k));
        const double target = (double)(r >> 11) * 0x1.0p-53 * Srow;
        uint32_t lo = 0, hi = max_tiles;
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (tsum[mid] > target) hi = mid; else lo = mid + 1;
        }
        if (lo >= max_tiles) lo = max_tiles - 1;
        while (lo > 0 && !(tsum[lo] > tsum[lo - 1])) --lo;
        atomicAdd(&dinfo[lo], 1u);
      }
    }
    __syncthreads();
    // exclusive scan of the draw counts -> offset << 16 | count
    uint32_t lsum = 0;
    for (uint32_t i = b0; i < b1; ++i) lsum += dinfo[i];
    uint32_t iscan = lsum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t ov = __shfl_up(iscan, d);
      if (lane >= d) iscan += ov;
    }
    if (lane == 63) s_parti[wave] = iscan;
    __syncthreads();
    uint32_t ibefore = 0;
    for (int w = 0; w < wave; ++w) ibefore += s_parti[w];
    uint32_t off = ibefore + iscan - lsum;
    for (uint32_t i = b0; i < b1; ++i) {
      const uint32_t c = dinfo[i];
      dinfo[i] = (off << 16) | c;
      off += c;
    }
    if (tid == 0) next_tile = 0;
    __syncthreads();
    // ---- phase C ----
    unsigned char *mine = reinterpret_cast<unsigned char *>(dinfo) + (((size_t)max_tiles * 4 + 15) & ~(size_t)15) + (size_t)wave * kDrawLdsPerWave;
    DrawLds S;
    S.prefix = reinterpret_cast<double *>(mine);
    S.run = reinterpret_cast<volatile double *>(mine + (size_t)kOneTileCols * 8);
    S.cs = reinterpret_cast<uint32_t *>(mine + (size_t)kOneTileCols * 8 + 8);
    S.hits = S.cs + kOneTileCols;
    S.ncols = reinterpret_cast<volatile uint32_t *>(S.hits + kOneTileCols);
    DrawSink<LEN, T> sink{eps, S, &p, &L, &wk, dinfo, Srow / (double)nsample, key, (int64_t)walker * nsample, o, wl, 0xffffffffu};
    visit_tiles<LEN, T>(p, pl, L, nocc, plan, wk, nchunks, chunk, chunk_len, 0u, &next_tile, sink);
    sink.flush();
    flush_winner_list<LEN, T>(o, wl, &wl_base, p, L, wk);
  }
}


// The kernels.  Eight waves per SIMD (64 VGPRs, 96 SGPRs; the 106 scalar registers the compiler would otherwise take cap the CU at SIX
// workgroups -- measured, tools/onepass_stamps.py -- whatever the LDS allows) for the forms whose LDS fits eight workgroups per CU: 8192
// walkers are 32 workgroups per CU, i.e. exactly four generations of eight.  The form that enumerates the drawn tiles a second time
// (no row cache: ~38 KB of LDS, four workgroups per CU) keeps its registers.
template <int LEN, typename T, bool SAMPLED, bool CACHED = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8)))
void reduce_onepass_list_kernel(const uint64_t *__restrict__ bra, SDParams p, PlanLayout pl, uint32_t nchunks, uint32_t chunk_len, uint32_t max_tiles,
                                const T *__restrict__ plan, T eps, uint32_t nsample, uint64_t seed, uint32_t P, OnepassOut<T> o) {
  static_assert(CACHED || !SAMPLED, "the re-enumerating form has its own kernel");
  reduce_onepass_list_body<LEN, T, SAMPLED, CACHED>(bra, p, pl, nchunks, chunk_len, max_tiles, plan, eps, nsample, seed, P, o);
}

// rows whose kept columns do not fit the list (deterministic): the list is emptied as it fills (FLUSH); ~40 KB of LDS at sorb 120, four
// workgroups per CU: no register squeeze
template <int LEN, typename T, bool SAMPLED = false, bool GTILE = false>
__global__ __launch_bounds__(kBlock) void reduce_onepass_list_flush_kernel(const uint64_t *__restrict__ bra, SDParams p, PlanLayout pl, uint32_t nchunks,
                                                                           uint32_t chunk_len, uint32_t max_tiles, const T *__restrict__ plan, T eps,
                                                                           uint32_t nsample, uint64_t seed, uint32_t P, OnepassOut<T> o) {
  reduce_onepass_list_body<LEN, T, SAMPLED, false, true, GTILE>(bra, p, pl, nchunks, chunk_len, max_tiles, plan, eps, nsample, seed, P, o);
}

template <int LEN, typename T, bool GTILE = false>
__global__ __launch_bounds__(kBlock) void reduce_onepass_list_redraw_kernel(const uint64_t *__restrict__ bra, SDParams p, PlanLayout pl, uint32_t nchunks,
                                                                            uint32_t chunk_len, uint32_t max_tiles, const T *__restrict__ plan, T eps,
                                                                            uint32_t nsample, uint64_t seed, uint32_t P, OnepassOut<T> o) {
  reduce_onepass_list_body<LEN, T, true, false, false, GTILE>(bra, p, pl, nchunks, chunk_len, max_tiles, plan, eps, nsample, seed, P, o);
}

// ---- contraction: E_loc(x) = sum_records w psi(x') / psi(x) ------------------------------------------------------------

// Which walkers a workgroup of the contraction serves (by_xcd, PYNQS_CONTRACT_BY_XCD): not group b of kBlock / 64 consecutive walkers but
// group contract_group(b, B) -- the workgroups b = j (mod 8), which share an XCD's L2 as far as the hardware has been seen to deal them,
// take a contiguous range of groups, whose rows of psi_u are neighbours (a walker's rows are contiguous, eight to a line).  A permutation
// of 0 .. B-1 for every B (the first B & 7 classes have one group more): only the speed depends on the dealing.
__host__ __device__ __forceinline__ uint32_t contract_group(uint32_t b, uint32_t B) {
  const uint32_t j = b & 7u, r = B & 7u;
  return j * (B >> 3) + (j < r ? j : r) + (b >> 3);
}

// One wave per walker.  Slots are visited in their fixed order (fixed slots, compacted doubles, drawn records; chunk by chunk),
// lane l takes slots l, l + 64, ...; the 64 partial sums meet in a butterfly: the result does not depend on anything but the
// records' positions.  psi(x) is the amplitude of the record of column 0 (kept slot 0, else among the drawn ones; 0 if it is
// nowhere -- the reference divides by zero there, too).
template <typename T, bool CPLX>
__global__ __launch_bounds__(kBlock) void reduce_contract_kernel(int64_t nbatch, uint32_t nchunks, uint32_t fixed, uint32_t cap_d,
                                                                 uint32_t nsample, const int32_t *__restrict__ rec_col,
                                                                 const T *__restrict__ rec_w, const int32_t *__restrict__ rec_link,
                                                                 const int32_t *__restrict__ seg_count, const int32_t *__restrict__ srec_col,
                                                                 const T *__restrict__ srec_w, const int32_t *__restrict__ srec_link,
                                                                 const int32_t *__restrict__ dedup_i32, int slot_i32, int row_off, uint32_t ucap,
                                                                 const double *__restrict__ psi_u, const double *__restrict__ psi_t, int divide,
                                                                 double *__restrict__ eloc, double *__restrict__ psi_x, int by_xcd) {
  const int lane = threadIdx.x & 63;
  const int64_t walker = (int64_t)(by_xcd ? contract_group(blockIdx.x, gridDim.x) : blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
  if (walker >= nbatch) return;
  double ar = 0.0, ai = 0.0, xr = 0.0, xi = 0.0;
  bool bad = false;
  auto amp = [&](int32_t link, double &re, double &im) {
    const double *src;
    int64_t at;
    if (link >= kDirectLink) {
      src = psi_u; at = link - kDirectLink;
      if ((uint32_t)at >= ucap) { bad = true; re = im = 0.0; return; }
    } else if (link >= 0) {
      if (!dedup_i32) { bad = true; re = im = 0.0; return; }  // (no de-duplication table: every link is direct)
      const int32_t row = dedup_i32[(int64_t)link * slot_i32 + row_off];
      if (row < 0 || (uint32_t)row >= ucap) { bad = true; re = im = 0.0; return; }
      src = psi_u; at = row;
    } else if (link <= -2) {
      src = psi_t; at = -2 - (int64_t)link;
    } else { bad = true; re = im = 0.0; return; }
    if constexpr (CPLX) { re = src[2 * at]; im = src[2 * at + 1]; }
    else { re = src[at]; im = 0.0; }
  };
  auto visit = [&](int32_t col, double w, int32_t link) {
    if (col < 0) return;
    double re, im;
    amp(link, re, im);
    ar += w * re; ai += w * im;
    if (col == 0) { xr = re; xi = im; }
  };
  const int64_t stride = (int64_t)fixed + cap_d;
  for (uint32_t c = 0; c < nchunks; ++c) {
    const int64_t seg = walker * nchunks + c, base = seg * stride;
    const uint32_t kept = (uint32_t)seg_count[seg];
    if (kept > cap_d) bad = true;
    const uint32_t nslots = fixed + min(kept, cap_d);
    for (uint32_t i = lane; i < nslots; i += 64) visit(rec_col[base + i], (double)rec_w[base + i], rec_link[base + i]);
  }
  for (uint32_t i = lane; i < nsample; i += 64) {
    const int64_t at = walker * nsample + i;
    visit(srec_col[at], (double)srec_w[at], srec_link[at]);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    ar += __shfl_xor(ar, d); ai += __shfl_xor(ai, d);
    xr += __shfl_xor(xr, d); xi += __shfl_xor(xi, d);  // (exactly one lane holds a non-zero psi(x))
  }
  const bool anybad = __ballot(bad) != 0;
  if (lane == 0) {
    if (anybad) { ar = ai = __builtin_nan(""); }
    if constexpr (CPLX) {
      if (divide) scaled_cdiv(ar, ai, xr, xi, ar, ai);
      eloc[2 * walker] = ar;
      eloc[2 * walker + 1] = ai;
      psi_x[2 * walker] = xr; psi_x[2 * walker + 1] = xi;
    } else {
      eloc[walker] = divide ? ar / xr : ar;
      psi_x[walker] = xr;
    }
  }
}

// The same contraction with the loads batched (PYNQS_CONTRACT_BATCHED).  The kernel above lasts as long as one wave's chain of ~20 trips
// of two dependent round trips each (records, then the amplitude through the link), and it loads weight and link of empty slots, too.
// Here a lane takes its slots l, l + 64, ... U trips at a time: the U columns (loaded one batch ahead), then weight and link of the LIVE
// slots only, then the de-duplication hop of the slot links, then the U amplitudes -- each stage's loads in flight together -- and adds
// the U products in slot order with the additions of the kernel above: eloc and psi_x are the same bit for bit, the `bad` rules too.
#ifndef PYNQS_CONTRACT_BATCH
#define PYNQS_CONTRACT_BATCH 8  // (4, 8, 16 measured: profiles/backhalf_trace.txt)
#endif
constexpr int kContractBatch = PYNQS_CONTRACT_BATCH;

// `ar += w * re` of the kernel above as the compiler contracts it there (one v_fmac_f64 per component, read off its ISA), spelled out
__device__ __forceinline__ void contract_add(double &ar, double &ai, double w, double re, double im) {
  ar = fma(w, re, ar);
  ai = fma(w, im, ai);
}

// A record is read once, by one lane; an amplitude is read by every record that links to its row (6.4 M records on 1.5 M rows on the
// flagship).  The records are loaded non-temporally, so that they pass through the L2 without taking the place of psi_u's lines.
template <typename X>
__device__ __forceinline__ X record_load(const X *p) {
  return __builtin_nontemporal_load(p);
}

template <typename T, bool CPLX, int U>
__global__ __launch_bounds__(kBlock) void reduce_contract_batched_kernel(int64_t nbatch, uint32_t nchunks, uint32_t fixed, uint32_t cap_d,
                                                                         uint32_t nsample, const int32_t *__restrict__ rec_col,
                                                                         const T *__restrict__ rec_w, const int32_t *__restrict__ rec_link,
                                                                         const int32_t *__restrict__ seg_count, const int32_t *__restrict__ srec_col,
                                                                         const T *__restrict__ srec_w, const int32_t *__restrict__ srec_link,
                                                                         const int32_t *__restrict__ dedup_i32, int slot_i32, int row_off, uint32_t ucap,
                                                                         const double *__restrict__ psi_u, const double *__restrict__ psi_t, int divide,
                                                                         double *__restrict__ eloc, double *__restrict__ psi_x, int by_xcd) {
  const uint32_t lane = threadIdx.x & 63;
  const int64_t walker = (int64_t)(by_xcd ? contract_group(blockIdx.x, gridDim.x) : blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
  if (walker >= nbatch) return;
  double ar = 0.0, ai = 0.0, xr = 0.0, xi = 0.0;
  bool bad = false;
  // count slots at colp / wp / lp: this lane's, in ascending order
  auto run = [&](const int32_t *__restrict__ colp, const T *__restrict__ wp, const int32_t *__restrict__ lp, uint32_t count) {
    int32_t coln[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = lane + 64u * u;
      coln[u] = i < count ? record_load(colp + i) : -1;
    }
    for (uint32_t i0 = lane; i0 < count; i0 += 64u * U) {
      int32_t col[U], link[U];
      T w[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        col[u] = coln[u];
        const uint32_t i = i0 + 64u * u;  // (col >= 0: i < count)
        w[u] = col[u] >= 0 ? record_load(wp + i) : T(0);
        link[u] = col[u] >= 0 ? record_load(lp + i) : -1;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {  // the next batch's columns
        const uint32_t i = i0 + 64u * (U + u);
        coln[u] = i < count ? record_load(colp + i) : -1;
      }
      // where the amplitude is: row of psi_u (>= 0), entry of psi_t (tab), or nowhere (at < 0 or at >= ucap: bad)
      int64_t at[U];
      bool tab[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t l = link[u];
        tab[u] = false;
        at[u] = -1;
        if (col[u] >= 0) {
          if (l >= kDirectLink) at[u] = l - kDirectLink;
          else if (l >= 0) { if (dedup_i32) at[u] = dedup_i32[(int64_t)l * slot_i32 + row_off]; }  // (no table: every link is direct)
          else if (l <= -2) { tab[u] = true; at[u] = -2 - (int64_t)l; }
        }
      }
      double re[U], im[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        re[u] = 0.0; im[u] = 0.0;
        if (col[u] >= 0) {
          if (tab[u]) {
            if constexpr (CPLX) { re[u] = psi_t[2 * at[u]]; im[u] = psi_t[2 * at[u] + 1]; }
            else re[u] = psi_t[at[u]];
          } else if (at[u] >= 0 && (uint64_t)at[u] < (uint64_t)ucap) {
            if constexpr (CPLX) { re[u] = psi_u[2 * at[u]]; im[u] = psi_u[2 * at[u] + 1]; }
            else re[u] = psi_u[at[u]];
          } else {
            bad = true;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (col[u] >= 0) {
          contract_add(ar, ai, (double)w[u], re[u], im[u]);
          if (col[u] == 0) { xr = re[u]; xi = im[u]; }
        }
      }
    }
  };
  const int64_t stride = (int64_t)fixed + cap_d;
  for (uint32_t c = 0; c < nchunks; ++c) {
    const int64_t seg = walker * nchunks + c, base = seg * stride;
    const uint32_t kept = (uint32_t)seg_count[seg];
    if (kept > cap_d) bad = true;
    run(rec_col + base, rec_w + base, rec_link + base, fixed + min(kept, cap_d));
  }
  if (nsample) run(srec_col + walker * nsample, srec_w + walker * nsample, srec_link + walker * nsample, nsample);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    ar += __shfl_xor(ar, d); ai += __shfl_xor(ai, d);
    xr += __shfl_xor(xr, d); xi += __shfl_xor(xi, d);  // (exactly one lane holds a non-zero psi(x))
  }
  const bool anybad = __ballot(bad) != 0;
  if (lane == 0) {
    if (anybad) { ar = ai = __builtin_nan(""); }
    if constexpr (CPLX) {
      if (divide) scaled_cdiv(ar, ai, xr, xi, ar, ai);
      eloc[2 * walker] = ar;
      eloc[2 * walker + 1] = ai;
      psi_x[2 * walker] = xr; psi_x[2 * walker + 1] = xi;
    } else {
      eloc[walker] = divide ? ar / xr : ar;
      psi_x[walker] = xr;
    }
  }
}

// the prologue of pynqs_reduce_onepass as ONE launch: the de-duplication table to "empty" (all bits set: n16 16-byte stores, grid-stride) and
// the four counter words to 0 -- instead of two memsets
__global__ __launch_bounds__(kBlock) void reduce_clear_kernel(uint4 *__restrict__ table, size_t n16, uint32_t *__restrict__ counters) {
  const uint4 ones = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n16; i += (size_t)gridDim.x * kBlock) table[i] = ones;
  if (blockIdx.x == 0 && threadIdx.x < 4) counters[threadIdx.x] = 0u;
}

}  // namespace pynqs

using namespace pynqs;

struct OnepassGeometry { uint32_t nchunks, chunk_len, max_tiles, fixed; };
static OnepassGeometry onepass_geometry(int64_t nbatch, const SDParams &p, bool sampled) {
  OnepassGeometry g;
  const uint32_t ncomb = p.nsd + 1;
  if (sampled) {  // the draws need the sums of the WHOLE row in one workgroup's LDS
    g.nchunks = 1;
    g.chunk_len = (ncomb + 255u) & ~255u;
  } else {
    plan_chunks(nbatch > 0 ? nbatch : 1, ncomb, &g.nchunks, &g.chunk_len);  // (no walkers: one walker's chunks; plan_chunks divides by the count)
  }
  g.max_tiles = max_tiles_per_chunk(p, g.nchunks, g.chunk_len);
  const uint32_t tS_all = (p.d1 + kSinglesPerTile - 1) / kSinglesPerTile;
  g.fixed = kFixedHead + ((tS_all + g.nchunks - 1) / g.nchunks) * kSinglesPerTile;
  return g;
}

static size_t onepass_static_lds(int) { return 16 + (kBlock / 64) * 4 + (kBlock / 64 + 1) * 12 + 64; }

// ---- which form a call takes: ONE decision for the launch and pynqs_reduce_onepass_plan alike (the table and the measurements: DESIGN.md 4.3)
constexpr uint32_t kLongRow = 65536;  // columns from which the look-back form is the slow one
// what a call hands the launch / what a plan offers it: io->row_cache, no io->dedup_table, io->tile_scratch (large enough), io->row_f32
struct OnepassOffer { bool row_cache, no_table, tile_scratch, row_f32; };
// form: pynqs_reduce_form; gtile: tile sums in global memory; P: list slots (look-back: slots of the winner list); lds: dynamic LDS bytes
struct OnepassDecision { int form; bool gtile; uint32_t P; size_t lds; };

// the overrides of the decision (development; DESIGN.md section 4.3 says what each value does): -1 unset
struct OnepassEnv { int list, cache, flush, row32; };
static const OnepassEnv &onepass_env() {
  auto get = [](const char *name) { const char *v = getenv(name); return v ? atoi(v) : -1; };
  static const OnepassEnv env = {get("PYNQS_OP_LIST"), get("PYNQS_OP_CACHE"), get("PYNQS_OP_FLUSH"), get("PYNQS_OP_ROW32")};
  return env;
}

// dynamic LDS of a form with P list slots (the only place that spells onepass_list_lds' flags out)
static size_t onepass_form_lds(const SDParams &p, size_t esz, uint32_t max_tiles, int eps_sample, int form, bool gtile, uint32_t P) {
  const bool sampled = eps_sample > 0;
  const uint32_t ns = (uint32_t)eps_sample;
  switch (form) {
    case PYNQS_REDUCE_LIST: return onepass_list_lds(p, esz, max_tiles, false, P, ns, false, false);
    case PYNQS_REDUCE_LIST_CACHE: return onepass_list_lds(p, esz, max_tiles, true, P, ns, true, false);
    case PYNQS_REDUCE_LIST_REDRAW: return onepass_list_lds(p, esz, max_tiles, true, P, ns, false, gtile);
    case PYNQS_REDUCE_FLUSH: return onepass_list_lds(p, esz, max_tiles, sampled, P, ns, false, gtile);
    case PYNQS_REDUCE_FLUSH_ROW32: return onepass_list_lds(p, esz, max_tiles, true, P, ns, false, gtile, false, true);
    case PYNQS_REDUCE_ROWOUT: return onepass_list_lds(p, esz, max_tiles, true, P, ns, false, false, true);
    default: return onepass_lds(p, esz, max_tiles, sampled, P);
  }
}

static OnepassDecision onepass_decide(const SDParams &p, size_t esz, const OnepassGeometry &g, uint64_t cap_doubles, int eps_sample, const OnepassOffer &o) {
  const OnepassEnv &env = onepass_env();
  constexpr size_t kLds = 160 * 1024 - 256;  // (what a list form may ask for)
  const bool sampled = eps_sample > 0, long_row = p.nsd + 1 > kLongRow;
  const uint64_t seg_cap = (uint64_t)g.fixed + cap_doubles;
  auto with = [&](int form, bool gtile, uint32_t P) { return OnepassDecision{form, gtile, P, onepass_form_lds(p, esz, g.max_tiles, eps_sample, form, gtile, P)}; };
  // sorted draws from the row's float32 copy: short rows whose kept records fit a list of as many slots as the segment has records
  if (sampled && o.row_f32 && env.list != 0 && seg_cap <= 1024 && reduce_draw_supported(p, eps_sample)) {
    const OnepassDecision d = with(PYNQS_REDUCE_ROWOUT, false, ((uint32_t)seg_cap + 1u) & ~1u);
    if (d.lds <= kLds) return d;
  }
  // a list per segment: up to 1024 slots, up to 2048 on long rows
  const bool cache = sampled && o.row_cache && env.cache != 0;
  uint32_t P = 64;
  while (P < seg_cap && P < (1u << 20)) P <<= 1;
  const OnepassDecision list = with(cache ? PYNQS_REDUCE_LIST_CACHE : sampled ? PYNQS_REDUCE_LIST_REDRAW : PYNQS_REDUCE_LIST, sampled && !cache && o.tile_scratch, P);
  const bool use_list = env.list != 0 && seg_cap <= 2048 && list.lds <= kLds && (env.list == 1 || seg_cap <= 1024 || long_row);
  // the flushing list where the records do not fit one: on long rows, without a table, or when at most a tenth of the columns can be kept
  const bool gtile_f = sampled && o.tile_scratch;
  const uint32_t flush_P = flush_list_slots((p.sorb - 1) / 64 + 1, sampled);
  const OnepassDecision flush = with(PYNQS_REDUCE_FLUSH, gtile_f, flush_P);
  const bool use_flush = !use_list && env.flush != 0 && flush.lds <= kLds &&
                         (long_row || env.flush == 1 || o.no_table || cap_doubles * 10 <= (uint64_t)g.chunk_len);
  // either gives way to the flushing form that reads the drawn tiles back from the float32 copy, where that puts more workgroups on a CU or
  // a good part of the tiles is drawn (a list that never fills is never flushed)
  if ((use_flush || (use_list && !cache && env.flush != 0)) && sampled && o.row_f32 && env.row32 != 0 && row32_fits(esz, flush_P, (uint32_t)eps_sample, gtile_f)) {
    const OnepassDecision row32 = with(PYNQS_REDUCE_FLUSH_ROW32, gtile_f, flush_P);
    const size_t wg_old = (size_t)160 * 1024 / ((use_flush ? flush.lds : list.lds) + 512), wg_new = (size_t)160 * 1024 / (row32.lds + 512);
    if (row32.lds <= kLds && (env.row32 == 1 || wg_new > wg_old || (uint64_t)eps_sample * 8 >= g.max_tiles)) return row32;
  }
  if (use_flush) return flush;
  if (use_list) return list;
  return with(PYNQS_REDUCE_LOOKBACK, false, winner_list_cap(eps_sample));
}

extern "C" int64_t pynqs_reduce_onepass_long_row(void) { return kLongRow; }

extern "C" const char *pynqs_reduce_form_name(int form) {
  static const char *const names[] = {"?", "lookback", "list", "list_cache", "list_redraw", "flush", "flush_row32", "rowout"};
  return names[form >= PYNQS_REDUCE_LOOKBACK && form <= PYNQS_REDUCE_ROWOUT ? form : 0];
}

// the system and the sizes every host entry point of the front end takes
static bool onepass_arguments(int64_t nbatch, int64_t sorb, int64_t nele, int64_t noA, int64_t noB, int64_t dtype, int64_t eps_sample, SDParams *p) {
  PlanLayout pl;
  for (int64_t v : {sorb, nele, noA, noB})
    if (v < 0 || v > 1024) return false;
  return make_sd_params((int)sorb, (int)nele, (int)noA, (int)noB, p) && make_plan_layout((int)sorb, &pl) && nbatch >= 0 && nbatch <= 0x7fffffffll &&
         eps_sample >= 0 && eps_sample <= 65535 && (dtype == PYNQS_F32 || dtype == PYNQS_F64);
}

extern "C" int pynqs_reduce_onepass_plan(const pynqs_reduce_plan_request *r, pynqs_reduce_plan *out) {
  SDParams p;
  if (!r || !out) return set_error(PYNQS_EINVAL, "null pointer");
  if (!onepass_arguments(r->nbatch, r->sorb, r->nele, r->noA, r->noB, r->dtype, r->eps_sample, &p) || r->cap_doubles < 0 || r->dedup_slots < 0)
    return set_error(PYNQS_EINVAL, "bad sorb/noA/noB (even sorb in [2, 192]) / nbatch / eps_sample (at most 65535 draws) / dtype / capacities");
  const int eps_sample = (int)r->eps_sample, len = ((int)r->sorb - 1) / 64 + 1;
  const bool sampled = eps_sample > 0;
  const int64_t n = r->nbatch, ncomb = (int64_t)p.nsd + 1;
  const size_t esz = r->dtype == PYNQS_F64 ? 8 : 4;
  const OnepassGeometry g = onepass_geometry(n, p, sampled);
  *out = pynqs_reduce_plan{};
  out->segments = n * (int64_t)g.nchunks;
  out->nchunks = g.nchunks; out->chunk_len = g.chunk_len; out->max_tiles = g.max_tiles; out->fixed = g.fixed;
  out->table_bytes = r->dedup_slots * dedup_slot_words(len) * 8; out->long_row = ncomb > kLongRow;
  // serves: a coarser test than onepass_decide(), as it always was (float64 integrals, 2048 slots, any cap_doubles): the look-back form fits,
  // or (draws on long rows) the flushing form with its tile sums in global memory does
  const bool lookback = onepass_form_lds(p, 8, g.max_tiles, eps_sample, PYNQS_REDUCE_LOOKBACK, false, winner_list_cap(eps_sample)) + onepass_static_lds(len) <= 160 * 1024;
  const bool flushing = sampled && out->long_row &&
                        onepass_form_lds(p, 8, g.max_tiles, eps_sample, PYNQS_REDUCE_FLUSH, true, 2048) + 256 + onepass_static_lds(len) <= 160 * 1024;
  out->serves = lookback || flushing;
  auto decide = [&](bool row_cache, bool tile_scratch, bool row_f32) {
    return onepass_decide(p, esz, g, (uint64_t)r->cap_doubles, eps_sample, OnepassOffer{row_cache, !r->with_table, tile_scratch, row_f32});
  };
  // what to offer.  First the float32 row copy, where a call that gets it would use it (the flushing form is asked with the tile scratch it
  // would also get); then the row cache, where the draws are dense in the row; then, on long rows, the tile scratch
  const bool tiles_row = sampled && ncomb > (r->tile_scratch_min_row < 0 ? (int64_t)kLongRow : r->tile_scratch_min_row);
  if (sampled && r->allow_row_f32)
    out->row_f32_form = decide(false, false, true).form == PYNQS_REDUCE_ROWOUT ? 1 : decide(false, tiles_row, true).form == PYNQS_REDUCE_FLUSH_ROW32 ? 2 : 0;
  const int64_t row_f32 = n * (int64_t)draw_row_stride((uint32_t)ncomb);
  if (out->row_f32_form == 1 || (out->row_f32_form == 2 && 4 * row_f32 <= r->row_f32_max_bytes)) out->row_f32_elements = row_f32 > 1 ? row_f32 : 1;
  if (!out->row_f32_elements && sampled && r->allow_row_cache && (int64_t)eps_sample * 64 >= ncomb && n * ncomb * (int64_t)esz <= r->row_cache_max_bytes)
    out->row_cache_elements = n * ncomb > 1 ? n * ncomb : 1;
  if (tiles_row && !out->row_cache_elements && (!out->row_f32_elements || out->row_f32_form == 2))
    out->tile_scratch_bytes = n * (int64_t)tile_scratch_stride(g.max_tiles);
  const OnepassDecision d = decide(out->row_cache_elements > 0, out->tile_scratch_bytes > 0, out->row_f32_elements > 0);
  out->form = d.form; out->tile_sums_global = d.gtile; out->list_slots = d.P; out->lds_bytes = (int64_t)d.lds;
  return PYNQS_OK;
}

extern "C" int pynqs_reduce_onepass_list_capacity(int64_t nbatch, int sorb, int nele, int noA, int noB, int dtype, int eps_sample,
                                                  int with_row_cache, int without_table, int64_t *cap_doubles) {
  SDParams p;
  if (!cap_doubles) return set_error(PYNQS_EINVAL, "null pointer");
  if (!onepass_arguments(nbatch, sorb, nele, noA, noB, dtype, eps_sample, &p)) return set_error(PYNQS_EINVAL, "bad sorb/noA/noB (even sorb in [2, 192]) / nbatch / eps_sample / dtype");
  const OnepassGeometry g = onepass_geometry(nbatch, p, eps_sample > 0);
  auto listed = [&](uint64_t cap) {
    // (with draws and no row cache the caller is expected to pass io->tile_scratch)
    const OnepassDecision d = onepass_decide(p, dtype == PYNQS_F64 ? 8 : 4, g, cap, eps_sample,
                                             OnepassOffer{with_row_cache != 0, without_table != 0, eps_sample > 0 && with_row_cache == 0, false});
    return d.form != PYNQS_REDUCE_LOOKBACK && d.lds + onepass_static_lds(0) <= 160 * 1024;
  };
  *cap_doubles = -1;
  // (the forms are monotonic in the capacity: LIST up to a limit, then possibly the flushing form up to another, or without one)
  if (listed((uint64_t)1 << 29)) { *cap_doubles = ((int64_t)1 << 30) - 1; return PYNQS_OK; }
  for (uint32_t seg = 2048; seg >= 128 && seg >= g.fixed; seg >>= 1)
    if (listed(seg - g.fixed)) { *cap_doubles = (int64_t)(seg - g.fixed); break; }
  if ((int64_t)(g.chunk_len / 10) > *cap_doubles && listed(g.chunk_len / 10)) *cap_doubles = g.chunk_len / 10;
  return PYNQS_OK;
}

// the kernels of this file by form (the two with the float32 row copy have launchers of their own: kernels_reduce_rowout.hip); the cases stand
// in the order in which the kernels have always been instantiated, which keeps the device code the same file byte for byte
template <int LEN, typename TT, bool SM>
static auto onepass_kernel(const OnepassDecision &d) -> decltype(&reduce_onepass_kernel<LEN, TT, SM>) {
  switch (d.form) {
    case PYNQS_REDUCE_FLUSH: return d.gtile ? reduce_onepass_list_flush_kernel<LEN, TT, SM, SM> : reduce_onepass_list_flush_kernel<LEN, TT, SM, false>;
    case PYNQS_REDUCE_LIST_REDRAW: return d.gtile ? reduce_onepass_list_redraw_kernel<LEN, TT, true> : reduce_onepass_list_redraw_kernel<LEN, TT, false>;
    case PYNQS_REDUCE_LIST: return reduce_onepass_list_kernel<LEN, TT, false, false>;
    case PYNQS_REDUCE_LIST_CACHE: return reduce_onepass_list_kernel<LEN, TT, SM, SM>;
    default: return reduce_onepass_kernel<LEN, TT, SM>;
  }
}

extern "C" int pynqs_reduce_onepass(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan, int dtype,
                                    double eps, int eps_sample, uint64_t seed, const pynqs_reduce_io *io, void *stream) {
  return pynqs_reduce_onepass_form(bra, nbatch, sorb, nele, noA, noB, plan, dtype, eps, eps_sample, seed, io, PYNQS_ROWOUT_TILEWISE, stream);
}

extern "C" int pynqs_reduce_onepass_form(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan, int dtype,
                                         double eps, int eps_sample, uint64_t seed, const pynqs_reduce_io *io, int rowout_form, void *stream) {
  pynqs::DeviceScope device_scope_(bra);
  if (rowout_form != PYNQS_ROWOUT_TILEWISE && rowout_form != PYNQS_ROWOUT_PER_COLUMN) return set_error(PYNQS_EINVAL, "bad form");
  SDParams p;
  PlanLayout pl;
  if (!make_sd_params(sorb, nele, noA, noB, &p) || !make_plan_layout(sorb, &pl)) return set_error(PYNQS_EINVAL, "bad sorb/noA/noB (even sorb in [2, 192])");
  if (nbatch < 0 || nbatch > 0x7fffffffll || (dtype != PYNQS_F32 && dtype != PYNQS_F64)) return set_error(PYNQS_EINVAL, "bad nbatch/dtype");
  if (eps_sample < 0 || eps_sample > 65535) return set_error(PYNQS_EINVAL, "eps_sample must be in [0, 65535]");
  if (!io) return set_error(PYNQS_EINVAL, "null pointer");
  const bool sampled = eps_sample > 0;
  if (!io->counters || !io->uniq_onv || !io->rec_col || !io->rec_w || !io->rec_link || !io->seg_count ||
      (sampled && (!io->srec_col || !io->srec_w || !io->srec_link)))
    return set_error(PYNQS_EINVAL, "null pointer");
  if (io->cap_unique < 1 || io->cap_unique >= (1ll << 30) || io->cap_doubles < 0 || io->cap_doubles >= (1ll << 30) ||
      (io->dedup_table && (io->dedup_slots < 64 || (io->dedup_slots & (io->dedup_slots - 1)) || io->dedup_slots > (1ll << 30) ||
                           2 * io->cap_unique > io->dedup_slots)))
    return set_error(PYNQS_EINVAL, "bad capacities (dedup_slots: power of two >= 2 * cap_unique)");
  if (io->pm1_dtype != PYNQS_F32 && io->pm1_dtype != PYNQS_F64) return set_error(PYNQS_EINVAL, "bad pm1_dtype");
  if (io->lut_table && io->lut_nkeys < 0) return set_error(PYNQS_EINVAL, "bad lut_nkeys");
  hipStream_t st = (hipStream_t)stream;
  const int len = (sorb - 1) / 64 + 1;
  // the form, from the buffers given; a caller that planned (io->form) is held to its plan before anything is enqueued
  const OnepassGeometry g = onepass_geometry(nbatch, p, sampled);
  const bool have_tiles = io->tile_scratch != nullptr && io->tile_scratch_bytes >= (int64_t)((size_t)nbatch * tile_scratch_stride(g.max_tiles));
  const OnepassDecision d = onepass_decide(p, dtype == PYNQS_F64 ? 8 : 4, g, (uint64_t)io->cap_doubles, eps_sample,
                                           OnepassOffer{io->row_cache != nullptr, io->dedup_table == nullptr, have_tiles, io->row_f32 != nullptr});
  if (io->form != 0 && nbatch > 0 && io->form != d.form) return set_error(PYNQS_EINVAL, "plan and buffers disagree");
  // one clear kernel instead of two memsets (Fe2S2, 64 MB table: no slower than the runtime's fill of the table alone, and one launch
  // less); PYNQS_REDUCE_CLEAR_KERNEL=0 brings the memsets back
  static const bool clear_kernel = !(getenv("PYNQS_REDUCE_CLEAR_KERNEL") && atoi(getenv("PYNQS_REDUCE_CLEAR_KERNEL")) == 0);
  const size_t table_bytes = io->dedup_table ? (size_t)io->dedup_slots * dedup_slot_words(len) * 8 : 0;
  if (clear_kernel && table_bytes && table_bytes % 16 == 0 && ((uintptr_t)io->dedup_table & 15) == 0 && ((uintptr_t)io->counters & 3) == 0) {
    const size_t n16 = table_bytes / 16;
    size_t blocks = (n16 + (size_t)kBlock * 8 - 1) / ((size_t)kBlock * 8);  // 8 stores per thread, up to 8 workgroups per CU
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(reduce_clear_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, st, (uint4 *)io->dedup_table, n16, (uint32_t *)io->counters);
  } else {
    if (hipMemsetAsync(io->counters, 0, 16, st) != hipSuccess) return check_launch("memset");
    if (table_bytes && hipMemsetAsync(io->dedup_table, 0xFF, table_bytes, st) != hipSuccess) return check_launch("memset");
  }
  if (nbatch == 0) return PYNQS_OK;
  if (!bra || !plan) return set_error(PYNQS_EINVAL, "null pointer");
  const uint64_t grid = (uint64_t)nbatch * g.nchunks;
  if (grid > 0x7fffffffull) return set_error(PYNQS_EINVAL, "grid too large");
  if (grid * ((uint64_t)g.fixed + (uint64_t)io->cap_doubles) > 0x7fffffffull * 16ull) return set_error(PYNQS_EINVAL, "record arrays too large");
  if (d.lds + onepass_static_lds(len) > 160 * 1024) return set_error(PYNQS_EINVAL, "row too long for the fused form (LDS): use the multi-pass entry points");
  if (!io->dedup_table && d.form == PYNQS_REDUCE_LOOKBACK)
    return set_error(PYNQS_EINVAL, "no de-duplication table: only the LIST forms run without one (cap_doubles <= pynqs_reduce_onepass_list_capacity)");
  static const bool verbose = getenv("PYNQS_OP_VERBOSE") != nullptr;
  if (verbose)
    fprintf(stderr, "pynqs_reduce_onepass: form %s%s, LDS %zu bytes per workgroup (walker tables %zu, max_tiles %u, list P %u), %u chunk(s) per walker\n",
            pynqs_reduce_form_name(d.form), d.gtile ? " (tile sums in global memory)" : "", d.lds, (size_t)lds_fixed_bytes(p), g.max_tiles, d.P, g.nchunks);
  // eloc.py:257-264: with draws and eps <= 0 nothing is kept (every column can be drawn); without draws |H| >= eps as it stands
  const double eps_eff = (sampled && !(eps > 0.0)) ? __builtin_inf() : eps;
  switch (d.form) {
    case PYNQS_REDUCE_ROWOUT:
      return launch_reduce_rowout(bra, nbatch, p, pl, g.chunk_len, g.max_tiles, plan, dtype, eps_eff, eps_sample, seed, d.P, d.lds, io, g.fixed, rowout_form, st);
    case PYNQS_REDUCE_FLUSH_ROW32:
      return launch_reduce_flush_row32(bra, nbatch, p, pl, g.chunk_len, g.max_tiles, plan, dtype, eps_eff, eps_sample, seed, d.P, d.lds, io, g.fixed, d.gtile, st);
    default: break;  // PYNQS_REDUCE_LOOKBACK, _LIST, _LIST_CACHE, _LIST_REDRAW, _FLUSH: the kernels of this file, onepass_kernel()
  }
#define PYNQS_OP_LAUNCH(TT, SM)                                                                                                      \
  do {                                                                                                                               \
    auto kfn = onepass_kernel<LEN, TT, SM>(d);                                                                                       \
    if (d.lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize,    \
                                                 (int)d.lds) != hipSuccess)                                                          \
      return check_launch("hipFuncSetAttribute");                                                                                   \
    hipLaunchKernelGGL(kfn, dim3((uint32_t)grid), dim3(kBlock), d.lds, st, bra, p, pl, g.nchunks, g.chunk_len, g.max_tiles, (const TT *)plan, \
                       (TT)eps_eff, (uint32_t)eps_sample, seed, d.P, make_out<TT>(io, len, g.fixed, d.gtile ? g.max_tiles : 0u));    \
  } while (0)
  DISPATCH_LEN(len, {
    if (dtype == PYNQS_F64) { if (sampled) PYNQS_OP_LAUNCH(double, true); else PYNQS_OP_LAUNCH(double, false); }
    else { if (sampled) PYNQS_OP_LAUNCH(float, true); else PYNQS_OP_LAUNCH(float, false); }
  });
#undef PYNQS_OP_LAUNCH
  return check_launch("reduce_onepass");
}

extern "C" int pynqs_reduce_contract_form(int64_t nbatch, int sorb, int nele, int noA, int noB, int dtype, int eps_sample,
                                          const pynqs_reduce_io *io, const double *psi_unique, const double *psi_table, int psi_is_complex,
                                          int divide, double *eloc, double *psi_x, int form, void *stream) {
  pynqs::DeviceScope device_scope_(eloc);
  SDParams p;
  if (!make_sd_params(sorb, nele, noA, noB, &p)) return set_error(PYNQS_EINVAL, "bad sorb/noA/noB");
  if (nbatch < 0 || nbatch > 0x7fffffffll || (dtype != PYNQS_F32 && dtype != PYNQS_F64) || eps_sample < 0 || eps_sample > 65535)
    return set_error(PYNQS_EINVAL, "bad nbatch/dtype/eps_sample");
  const int by_xcd = (form & PYNQS_CONTRACT_BY_XCD) != 0;
  form &= ~PYNQS_CONTRACT_BY_XCD;
  if (form != PYNQS_CONTRACT_BATCHED && form != PYNQS_CONTRACT_SERIAL) return set_error(PYNQS_EINVAL, "bad form");
  if (nbatch == 0) return PYNQS_OK;
  if (!io || !io->rec_col || !io->rec_w || !io->rec_link || !io->seg_count || !psi_unique || !eloc || !psi_x ||
      (eps_sample > 0 && (!io->srec_col || !io->srec_w || !io->srec_link)) || (io->lut_table && !psi_table))
    return set_error(PYNQS_EINVAL, "null pointer");
  const OnepassGeometry g = onepass_geometry(nbatch, p, eps_sample > 0);
  const uint32_t nchunks = g.nchunks, fixed = g.fixed;
  const int len = (sorb - 1) / 64 + 1;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t grid = (uint32_t)((nbatch + kBlock / 64 - 1) / (kBlock / 64));
#define PYNQS_CT_ARGS(TT)                                                                                                           \
  dim3(grid), dim3(kBlock), 0, st, nbatch, nchunks, fixed, (uint32_t)io->cap_doubles, (uint32_t)eps_sample, io->rec_col,            \
      (const TT *)io->rec_w, io->rec_link, io->seg_count, io->srec_col, (const TT *)io->srec_w, io->srec_link,                      \
      (const int32_t *)io->dedup_table, dedup_slot_words(len) * 2, dedup_row_offset(len), (uint32_t)io->cap_unique, psi_unique,     \
      psi_table, divide, eloc, psi_x, by_xcd
#define PYNQS_CT_LAUNCH(TT, CX)                                                                             \
  do {                                                                                                      \
    if (form == PYNQS_CONTRACT_SERIAL) hipLaunchKernelGGL((reduce_contract_kernel<TT, CX>), PYNQS_CT_ARGS(TT)); \
    else hipLaunchKernelGGL((reduce_contract_batched_kernel<TT, CX, kContractBatch>), PYNQS_CT_ARGS(TT));   \
  } while (0)
  if (dtype == PYNQS_F64) { if (psi_is_complex) PYNQS_CT_LAUNCH(double, true); else PYNQS_CT_LAUNCH(double, false); }
  else { if (psi_is_complex) PYNQS_CT_LAUNCH(float, true); else PYNQS_CT_LAUNCH(float, false); }
#undef PYNQS_CT_LAUNCH
#undef PYNQS_CT_ARGS
  return check_launch("reduce_contract");
}

extern "C" int64_t pynqs_reduce_contract_group(int64_t b, int64_t B) {
  if (b < 0 || b >= B || B > 0xffffffffll) return -1;
  return (int64_t)pynqs::contract_group((uint32_t)b, (uint32_t)B);
}

extern "C" int pynqs_reduce_contract(int64_t nbatch, int sorb, int nele, int noA, int noB, int dtype, int eps_sample,
                                     const pynqs_reduce_io *io, const double *psi_unique, const double *psi_table, int psi_is_complex,
                                     int divide, double *eloc, double *psi_x, void *stream) {
  return pynqs_reduce_contract_form(nbatch, sorb, nele, noA, noB, dtype, eps_sample, io, psi_unique, psi_table, psi_is_complex, divide, eloc,
                                    psi_x, PYNQS_CONTRACT_BATCHED | PYNQS_CONTRACT_BY_XCD, stream);
}

#ifdef PYNQS_OP_STAMPS
extern "C" int pynqs_debug_stamps(unsigned long long *out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(pynqs::g_stamps), sizeof(unsigned long long) * 8192 * 16);
}
#endif
