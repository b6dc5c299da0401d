// kernels_rdm.hip -- one- and two-body reduced density matrices in the integrals' own packed layouts (include/pynqs_amd.h, "reduced
// density matrices"): the transpose of detcore.h's element().  element() gathers integrals into <x|H|x'>; here w_x sign psi(x')/psi(x) is
// scattered back onto the slots those integrals were read from, so that dot(h1e, rdm1) + dot(h2e, rdm2) = sum_x w_x Re E_loc(x) for ANY
// integrals.
//
//   pynqs_rdm_scatter : any ansatz.  One workgroup per walker (build_walker_tables + decode), the ratio row [ncomb] of the walker is read
//       once, every contribution is one f64 global atomic add.  Not bit-reproducible (the order of the atomics is not fixed).
//   pynqs_rdm_rbm     : real RBM, the loop turned inside out.  A workgroup OWNS one side of an excitation -- a pair of orbitals (same
//       spin, or one alpha and one beta) or, for the singles, one orbital -- and its lane items own the other side.  The owner is the
//       PARTICLE side (empty in the walker) when the shells are more than half full, so that few walkers qualify per workgroup and most
//       lane items (hole pairs) are live, and the hole side otherwise.  The workgroup compacts the walkers that qualify (in walker
//       order), and per walker stages, for theta' = theta shifted by the owner's orbitals,
//           a_h = 1 / (1 + exp(-2 theta'_h)),  b_h = 1 / (1 + exp(2 theta'_h))        (formed directly: no cancellation when saturated)
//       in LDS; an item with the orbitals Q then has
//           psi(x') / psi(x) = [prod_h cosh theta'_h / cosh theta_h * visible(owner)] * c_Q * prod_h (b_h + a_h g_h(Q)),
//           g_h(Q) = prod_{o in Q} exp(-+4 W_ho),   c_Q = exp(+-2 sum_{o in Q} (sum_h W_ho - a_o)),
//       one fma and one multiplication per item and hidden unit plus the product of the two table rows (exp(-+4W) of the RBM table, copied
//       into LDS).  Signs are bit tests on the walker's prefix-parity masks.  Every item adds its walkers in walker order into a register;
//       the results go to directed tables [particle side][hole side] in the workspace, and a last kernel forms every packed slot from
//       them (slot (ij, kl) = table[ij][kl] + table[kl][ij]): no float atomics, every sum in a fixed order, two calls give the same bits.
//       The singles' spectator terms (rdm2[(h,k),(q,k)] for every occupied k) are added by the item that owns (h, q) into its own LDS row.
//   pynqs_rdm_jrbm    : Jastrow-RBM, the same kernel (JASTROW).  With S = M + M^T (zero diagonal, the Jastrow table) and r_o = sum_j S_oj x_j
//       the ratio gains exp(Delta), Delta = -2 sum_{i in F} x_i r_i + 4 sum_{i<j in F} S_ij x_i x_j over the flipped orbitals F.  In a
//       qualifying walker every owner orbital has x = xo and every live item orbital x = xl = -xo, so every pair term is a constant of
//       the workgroup: + 4 S_o0o1 joins the owner's visible term, 4 S_l0l1 - 4 (S_o0l0 + S_o0l1 + S_o1l0 + S_o1l1) (singles: - 4 S_ol) the
//       exponent of the lane constant.  Per walker -2 xo (r_o0 + r_o1) joins the owner's exponent and e_o = exp(-2 xl r_o) is staged for
//       every orbital next to a_h, b_h (published by the same barrier); an item multiplies by e_l0 e_l1.  r [n][sorb] comes from
//       rdm_r_kernel (one fma chain per walker and orbital) in the workspace.  M = 0: every added term is +-0 and every added factor 1,
//       the bits of pynqs_rdm_rbm.
#include "detcore.h"
#include "launch.h"
#include "rbm.h"

namespace pynqs {

constexpr int kRdmMaxItems = 8;    // lane items per thread of the fused kernel: K * K <= 8 * 256
constexpr int kRdmMaxHidden = 512; // two hidden units per thread in the staging step
constexpr size_t kRdmMaxLds = 64 * 1024;

template <int LEN>
__device__ __forceinline__ bool rdm_valid_walker(const uint64_t (&w)[LEN], int sorb, int noA, int noB) {
  int a = 0, b = 0;
  bool ok = true;
#pragma unroll
  for (int i = 0; i < LEN; ++i) {
    a += __popcll(w[i] & 0x5555555555555555ull);
    b += __popcll(w[i] & 0xAAAAAAAAAAAAAAAAull);
    const int lo = sorb - 64 * i;  // orbitals of this word below sorb
    if (lo < 64) ok = ok && (lo <= 0 ? w[i] == 0ull : (w[i] >> lo) == 0ull);
  }
  return ok && a == noA && b == noB;
}

// ---- scatter path -----------------------------------------------------------------------------------------------------------------------
template <int LEN, bool CPLX>
__global__ __launch_bounds__(kBlock) void rdm_scatter_kernel(const uint64_t *__restrict__ bra, const double *__restrict__ w,
                                                             const double *__restrict__ ratio, SDParams p, double *__restrict__ rdm1,
                                                             double *__restrict__ rdm2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint64_t walker = blockIdx.x;
  const int tid = threadIdx.x;
  Walker<LEN> wk;
  load_walker<LEN>(bra + walker * LEN, wk);
  if (!rdm_valid_walker<LEN>(wk.w, p.sorb, p.noA, p.noB)) return;  // (workgroup-uniform) the tables below index by noA / noB
  const LdsLayout L = carve_lds(smem, p);
  const int nocc = build_walker_tables<LEN>(wk, p, L);
  const double wx = w[walker];
  const double *__restrict__ row = ratio + walker * (uint64_t)(p.nsd + 1) * (CPLX ? 2 : 1);
  // x' = x: +w on rdm1[p,p] and on the diagonal pair slots
  const int nterms = nocc * (nocc + 1) / 2;
  for (int t = tid; t < nterms; t += kBlock) {
    int a = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (a * (a + 1) / 2 > t) --a;
    while ((a + 1) * (a + 2) / 2 <= t) ++a;
    const int pos = t - a * (a + 1) / 2;
    const uint32_t pa = L.occa[a];
    if (pos == 0) {
      unsafeAtomicAdd(rdm1 + (size_t)pa * p.sorb + pa, wx);
    } else {
      const uint32_t pr = pair_index(pa, L.occa[pos - 1]);  // occa ascends: pa is the larger
      unsafeAtomicAdd(rdm2 + tri_index(pr, pr), wx);
    }
  }
  for (uint32_t r = tid; r < p.nsd; r += kBlock) {
    const Excitation e = decode(r, p, L);
    double v = wx * row[(size_t)(1 + r) * (CPLX ? 2 : 1)];  // the real part
    if (e.par) v = -v;
    if (e.is_double) {
      unsafeAtomicAdd(rdm2 + tri_index(pair_index(e.h0, e.h1), pair_index(e.q0, e.q1)), v);
    } else {
      const int h = e.h0, q = e.q0;
      unsafeAtomicAdd(rdm1 + (size_t)q * p.sorb + h, v);
      for (int t = 0; t < nocc; ++t) {
        const int k = L.occv[t];
        if (k == h) continue;
        const uint32_t ij = h > k ? pair_index(h, k) : pair_index(k, h);
        const uint32_t kl = q > k ? pair_index(q, k) : pair_index(k, q);
        unsafeAtomicAdd(rdm2 + tri_index(ij, kl), ((h > k) != (q > k)) ? -v : v);
      }
    }
  }
}

// ---- fused path -------------------------------------------------------------------------------------------------------------------------
// The walkers are cut into slices (whole multiples of kBlock walkers; a function of the sizes alone, so that the order of every sum is
// fixed): a workgroup serves one owner and one slice, and a serial chain of a few microseconds per qualifying walker is what it spends
// its time on -- without slices Fe2S2 x 8192 walkers has 780 + 40 such chains of 500 to 2000 walkers.  Every slice has tables of its
// own; the last kernel adds them in slice order.
// workspace (doubles): theta [n][H] | Dg [nslS][sorb][sorb] | T [nslS][sorb][sorb][sorb + 1] | Daa, Dbb [nslD][npS][npS] | Dab [nslD][K K][K K]
// (pynqs_rdm_jrbm: | r [n][sorb] behind them, RdmJastrow::offR)
struct RdmLayout {
  int sorb, K, H, Hq, npS, owner_empty, noA, noB;
  int nslD, nslS;      // slices of the pair kernel / of the singles and diagonal kernels
  int64_t lenD, lenS;  // walkers per slice
  int64_t szDg, szT, szD[3];
  int64_t offTheta, offDg, offT, offD[3], total;  // doubles
  int64_t offE4, offWt, offVb;                    // into the RBM table: exp(-+4W) (the sign the lane side needs), W^T, a
};

static inline bool make_rdm_layout(int64_t n, int sorb, int noA, int noB, int H, RdmLayout *r) {
  RbmLayout rl;
  if (sorb < 2 || (sorb & 1) || sorb > kMaxSorb || n < 0 || !make_rbm_layout(sorb, H, &rl)) return false;
  const int K = sorb / 2;
  if (noA < 0 || noB < 0 || noA > K || noB > K) return false;
  r->sorb = sorb; r->K = K; r->H = H; r->Hq = rl.Hq; r->npS = K * (K - 1) / 2; r->noA = noA; r->noB = noB;
  r->owner_empty = (noA + noB) > K ? 1 : 0;  // more than half full: the particle side owns
  // lane side = holes (occupied, flipped to empty: theta changes by -2W per orbital, g = exp(-4W)) when the owner is the particle side
  r->offE4 = r->owner_empty ? rl.offE4m : rl.offE4p;
  r->offWt = rl.offWt; r->offVb = rl.offVb;
  int64_t o = 0;
  r->offTheta = o; o += n * H;
  r->szDg = (int64_t)sorb * sorb; r->szT = (int64_t)sorb * sorb * (sorb + 1);
  r->szD[0] = r->szD[1] = (int64_t)r->npS * r->npS; r->szD[2] = (int64_t)K * K * K * K;
  // slices: enough workgroups to fill the chip several times over (256 CUs x 5 resident workgroups), tables within 16 M doubles each
  const int64_t chunks = n > 0 ? (n + kBlock - 1) / kBlock : 1;
  auto slices = [&](int64_t owners, int64_t per_slice, int64_t want, int *nsl, int64_t *len) {
    int64_t s = (want + owners - 1) / owners;
    const int64_t cap = ((int64_t)16 << 20) / (per_slice > 0 ? per_slice : 1);
    if (s > cap) s = cap;
    if (s > chunks) s = chunks;
    if (s < 1) s = 1;
    const int64_t per = (chunks + s - 1) / s;  // chunks per slice
    *len = per * kBlock;
    *nsl = (int)((chunks + per - 1) / per);
  };
  slices(2 * (int64_t)r->npS + (int64_t)K * K, 2 * r->szD[0] + r->szD[2], 4096, &r->nslD, &r->lenD);
  slices(sorb, r->szT + r->szDg, 2048, &r->nslS, &r->lenS);
  r->offDg = o; o += r->nslS * r->szDg;
  r->offT = o; o += r->nslS * r->szT;
  for (int c = 0; c < 3; ++c) { r->offD[c] = o; o += r->nslD * r->szD[c]; }
  r->total = o;
  return true;
}

__host__ __device__ inline size_t rdm_lds_bytes(const RdmLayout &r, bool singles, bool jastrow = false) {
  // G [sorb][Hq] | ab [2 buffers][2][H] | red [2 buffers][kBlock / 64] | cs [sorb] | (singles) Ts [K][sorb] | list [kBlock] u32 | wcnt [kBlock / 64] u32
  // | (jastrow) ev [2 buffers][sorb]
  return 8 * ((size_t)r.sorb * r.Hq + 4 * (size_t)r.H + 2 * (kBlock / 64) + r.sorb + (singles ? (size_t)r.K * r.sorb : 0)) + 4 * (kBlock + kBlock / 64) +
         (jastrow ? 16 * (size_t)r.sorb : 0);
}

// what the JASTROW flavour of rdm_rbm_kernel reads beside the RBM table: the Jastrow table (rbm.h) and where r [n][sorb] lies in the workspace
struct RdmJastrow {
  const double *tab;
  int64_t offS, offR;  // doubles: S in the table, r in the workspace
};

// theta[i][h] = b_h + sum_o W_ho x_o: one fma chain over the orbitals in ascending order
template <int LEN>
__global__ __launch_bounds__(kBlock) void rdm_theta_kernel(const uint64_t *__restrict__ bra, int64_t n, RdmLayout r,
                                                           const double *__restrict__ rbm, int64_t offHb, double *__restrict__ ws) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= n * r.H) return;
  const int64_t i = g / r.H;
  const int h = (int)(g - i * r.H);
  uint64_t x[LEN];
#pragma unroll
  for (int k = 0; k < LEN; ++k) x[k] = bra[i * LEN + k];
  double th = rbm[offHb + h];
  for (int o = 0; o < r.sorb; ++o) th = fma(bit_of<LEN>(x, o) ? 1.0 : -1.0, rbm[r.offWt + (int64_t)o * r.Hq + h], th);
  ws[r.offTheta + g] = th;
}

// r[i][o] = sum_j S_oj x_j: one fma chain over the orbitals in ascending order from 0 (S_oo = 0)
template <int LEN>
__global__ __launch_bounds__(kBlock) void rdm_r_kernel(const uint64_t *__restrict__ bra, int64_t n, int sorb, RdmJastrow jz, double *__restrict__ ws) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= n * sorb) return;
  const int64_t i = g / sorb;
  const int o = (int)(g - i * sorb);
  uint64_t x[LEN];
#pragma unroll
  for (int k = 0; k < LEN; ++k) x[k] = bra[i * LEN + k];
  const double *__restrict__ row = jz.tab + jz.offS + (int64_t)o * sorb;
  double acc = 0.0;
  for (int j = 0; j < sorb; ++j) acc = fma(bit_of<LEN>(x, j) ? 1.0 : -1.0, row[j], acc);
  ws[jz.offR + g] = acc;
}

// Dg[slice][p][q] = sum_x w_x n_p(x) n_q(x), the slice's walkers in order: one workgroup per (p, slice), one thread per q
template <int LEN>
__global__ __launch_bounds__(kBlock) void rdm_diag_kernel(const uint64_t *__restrict__ bra, int64_t n, const double *__restrict__ w,
                                                          RdmLayout r, double *__restrict__ ws) {
  const int p = blockIdx.x % r.sorb, q = threadIdx.x;
  const int64_t slice = blockIdx.x / r.sorb, i0 = slice * r.lenS, i1 = i0 + r.lenS < n ? i0 + r.lenS : n;
  double acc = 0.0;
  for (int64_t i = i0; i < i1; ++i) {
    uint64_t x[LEN];
#pragma unroll
    for (int k = 0; k < LEN; ++k) x[k] = bra[i * LEN + k];
    if (!rdm_valid_walker<LEN>(x, r.sorb, r.noA, r.noB)) continue;
    if (q < r.sorb && bit_of<LEN>(x, p) && bit_of<LEN>(x, q)) acc += w[i];
  }
  if (q < r.sorb) ws[r.offDg + slice * r.szDg + (int64_t)p * r.sorb + q] = acc;
}

// the walker's words (every lane holds the same values) -> scalar registers and prefix-parity masks: load_walker without the load
template <int LEN>
__device__ __forceinline__ void rdm_make_walker(const uint64_t (&x)[LEN], Walker<LEN> &wk) {
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < LEN; ++i) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x[i]);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(x[i] >> 32));
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    wk.w[i] = v;
    const uint64_t pp = prefix_parity_excl(v);
    wk.pm[i] = carry ? ~pp : pp;
    carry ^= (uint32_t)__popcll(v) & 1u;
  }
}

// class 0 / 1: alpha-alpha / beta-beta pairs, 2: alpha-beta pairs (block = owner pair); SINGLES: block = owner orbital; JASTROW: the
// Jastrow-RBM (jz is not read otherwise)
template <int LEN, bool SINGLES, bool JASTROW>
__global__ __launch_bounds__(kBlock) void rdm_rbm_kernel(const uint64_t *__restrict__ bra, int64_t n, const double *__restrict__ w,
                                                         RdmLayout r, const double *__restrict__ rbm, double *__restrict__ ws, RdmJastrow jz) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *G = reinterpret_cast<double *>(smem);
  double *ab = G + (size_t)r.sorb * r.Hq;   // [2][2][H]: a_h, b_h, double-buffered over the walkers
  double *red = ab + 4 * r.H;               // [2][kBlock / 64]: the waves' shares of ln(owner factor)
  double *cs = red + 2 * (kBlock / 64);
  double *Ts = cs + r.sorb;
  uint32_t *list = reinterpret_cast<uint32_t *>(Ts + (SINGLES ? (size_t)r.K * r.sorb : 0));
  uint32_t *wcnt = list + kBlock;
  double *ev = reinterpret_cast<double *>(wcnt + kBlock / 64);  // (JASTROW) [2][sorb]: e_o = exp(-2 xl r_o), double-buffered as ab
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sorb = r.sorb, K = r.K, H = r.H, Hq = r.Hq;
  const bool oe = r.owner_empty != 0;
  // ---- the owner
  int cls, o0, o1, nitems;
  uint32_t owner_rank;
  const uint32_t nown = SINGLES ? (uint32_t)sorb : 2u * (uint32_t)r.npS + (uint32_t)(K * K);
  const int64_t slice = blockIdx.x / nown, slen = SINGLES ? r.lenS : r.lenD;
  const int64_t n0 = slice * slen, n1 = n0 + slen < n ? n0 + slen : n;
  if constexpr (SINGLES) {
    owner_rank = blockIdx.x % nown;
    cls = owner_rank & 1;  // spin
    o0 = o1 = (int)owner_rank;
    nitems = K;
  } else {
    uint32_t b = blockIdx.x % nown;
    if (b < 2u * r.npS) {
      cls = b >= (uint32_t)r.npS;
      owner_rank = b - cls * r.npS;
      int hi, lo;
      pair_unrank((int)owner_rank, hi, lo);
      o0 = 2 * hi + cls; o1 = 2 * lo + cls;
      nitems = r.npS;
    } else {
      cls = 2;
      owner_rank = b - 2u * r.npS;
      o0 = 2 * (int)(owner_rank / K); o1 = 2 * (int)(owner_rank % K) + 1;  // (alpha, beta)
      nitems = K * K;
    }
  }
  // ---- tables: g rows, column sums of W
  for (int e = tid; e < sorb * Hq; e += kBlock) G[e] = rbm[r.offE4 + e];
  for (int o = tid; o < sorb; o += kBlock) {
    double s = 0.0;
    for (int h = 0; h < H; ++h) s += rbm[r.offWt + (int64_t)o * Hq + h];
    cs[o] = s;
  }
  if constexpr (SINGLES)
    for (int e = tid; e < K * sorb; e += kBlock) Ts[e] = 0.0;
  // owner's shift of theta for this thread's hidden units: theta' = theta - 2 x_o W_ho summed over the owner's orbitals
  const double xo = oe ? -1.0 : 1.0;  // x_o of the owner's orbitals in a qualifying walker
  double dth[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int h = tid + s * kBlock;
    dth[s] = 0.0;
    if (h < H) {
      const double ws0 = rbm[r.offWt + (int64_t)o0 * Hq + h];
      const double wsum = SINGLES ? ws0 : ws0 + rbm[r.offWt + (int64_t)o1 * Hq + h];
      dth[s] = -2.0 * xo * wsum;
    }
  }
  double vis_owner = -2.0 * xo * (SINGLES ? rbm[r.offVb + o0] : rbm[r.offVb + o0] + rbm[r.offVb + o1]);
  const double *__restrict__ Sj = jz.tab + jz.offS;  // (JASTROW) S [sorb][sorb]
  // the orbital whose e_o this thread stages: from the last thread down, the waves that stage no hidden unit when H is small
  const int oj = kBlock - 1 - tid;
  if constexpr (JASTROW && !SINGLES) vis_owner += 4.0 * Sj[(int64_t)o0 * sorb + o1];  // the owner pair: x_o0 x_o1 = 1
  __syncthreads();
  // ---- this thread's items: orbitals l0 (> l1 within a same-spin pair; alpha, beta in class 2), constant c_Q, running sum
  int l0[kRdmMaxItems], l1[kRdmMaxItems];
  double lc[kRdmMaxItems], acc[kRdmMaxItems];
  const double xl = -xo;  // x_o of the lane side's orbitals
#pragma unroll
  for (int j = 0; j < kRdmMaxItems; ++j) {
    const int it = tid + j * kBlock;
    l0[j] = l1[j] = 0; lc[j] = 0.0; acc[j] = 0.0;
    if (it < nitems) {
      if constexpr (SINGLES) {
        l0[j] = l1[j] = 2 * it + cls;
        double lnc = 2.0 * xl * (cs[l0[j]] - rbm[r.offVb + l0[j]]);
        // the pair terms of the flip formula that involve the item are constants of the workgroup: x_o x_l = -1
        if constexpr (JASTROW) lnc += -4.0 * Sj[(int64_t)o0 * sorb + l0[j]];
        lc[j] = exp(lnc);
      } else {
        if (cls < 2) {
          int hi, lo;
          pair_unrank(it, hi, lo);
          l0[j] = 2 * hi + cls; l1[j] = 2 * lo + cls;
        } else {
          l0[j] = 2 * (it / K); l1[j] = 2 * (it % K) + 1;
        }
        double lnc = 2.0 * xl * ((cs[l0[j]] + cs[l1[j]]) - (rbm[r.offVb + l0[j]] + rbm[r.offVb + l1[j]]));
        if constexpr (JASTROW) {
          // + 4 S within the item pair, - 4 S for each of the four crossed owner-item pairs
          const int64_t r0 = (int64_t)o0 * sorb, r1 = (int64_t)o1 * sorb;
          lnc += 4.0 * Sj[(int64_t)l0[j] * sorb + l1[j]] - 4.0 * (((Sj[r0 + l0[j]] + Sj[r0 + l1[j]]) + Sj[r1 + l0[j]]) + Sj[r1 + l1[j]]);
        }
        lc[j] = exp(lnc);
      }
    }
  }
  // ---- the walkers, kBlock at a time: compact those whose owner orbitals are all empty (oe) / all occupied, in walker order
  uint32_t parity = 0;  // which ab / red buffer the next walker takes
  for (int64_t base = n0; base < n1; base += kBlock) {
    bool take = false;
    {
      const int64_t i = base + tid;
      if (i < n1) {
        uint64_t x[LEN];
#pragma unroll
        for (int k = 0; k < LEN; ++k) x[k] = bra[i * LEN + k];
        const uint32_t want = oe ? 0u : 1u;
        take = rdm_valid_walker<LEN>(x, sorb, r.noA, r.noB) && bit_of<LEN>(x, o0) == want && bit_of<LEN>(x, o1) == want;
      }
    }
    const uint64_t m = __ballot(take);
    __syncthreads();  // the previous chunk's list has been consumed
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, cnt = 0;
#pragma unroll
    for (int v = 0; v < kBlock / 64; ++v) {
      const uint32_t c = wcnt[v];
      if (v < wave) before += c;
      cnt += c;
    }
    if (take) list[before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)tid;
    __syncthreads();
    // the next walker's words, weight and theta are requested while the current one is worked on
    uint64_t xn[LEN];
    double thn[2], wn = 0.0;
    [[maybe_unused]] double ron = 0.0, rln = 0.0;  // (JASTROW) r of the owner's orbitals (summed), r of this thread's orbital oj
    auto request = [&](uint32_t t) {
      const int64_t i = base + list[t];
#pragma unroll
      for (int k = 0; k < LEN; ++k) xn[k] = bra[i * LEN + k];
      wn = w[i];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int h = tid + s * kBlock;
        thn[s] = h < H ? ws[r.offTheta + i * H + h] : 0.0;
      }
      if constexpr (JASTROW) {
        const double *__restrict__ ri = ws + jz.offR + i * sorb;
        ron = SINGLES ? ri[o0] : ri[o0] + ri[o1];
        rln = oj < sorb ? ri[oj] : 0.0;
      }
    };
    if (cnt) request(0);
    for (uint32_t t = 0; t < cnt; ++t) {
      Walker<LEN> wk;
      rdm_make_walker<LEN>(xn, wk);
      const double wi = wn, th0 = thn[0], th1 = thn[1];
      [[maybe_unused]] const double ro = ron, rl = rln;
      if (t + 1 < cnt) request(t + 1);
      double *__restrict__ abp = ab + (size_t)parity * 2 * H;
      double *__restrict__ redp = red + parity * (kBlock / 64);
      [[maybe_unused]] double *__restrict__ evp = ev + (size_t)parity * sorb;
      parity ^= 1u;
      // stage a_h, b_h of theta' and the owner's factor  prod_h cosh theta'_h / cosh theta_h
      double lnf = 0.0;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int h = tid + s * kBlock;
        if (h < H) {
          const double th = s ? th1 : th0, d = dth[s], tp = th + d;
          const double sg = th < 0.0 ? -1.0 : 1.0;
          abp[h] = 1.0 / (1.0 + exp(-2.0 * tp));
          abp[H + h] = 1.0 / (1.0 + exp(2.0 * tp));
          // ln(cosh(theta + d) / cosh theta) = s d + log1p(exp(-2 s theta')) - log1p(exp(-2 |theta|)),  s = sign theta
          lnf += fma(sg, d, log1p(exp(-2.0 * sg * tp)) - log1p(exp(-2.0 * fabs(th))));
        }
      }
      if constexpr (JASTROW)
        if (oj < sorb) evp[oj] = exp(-2.0 * xl * rl);  // (an orbital that is not on the lane side in this walker: any value, read by no live item)
      // fixed order: a butterfly over the lanes (the same bits in every lane), then the waves in turn
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) lnf += __shfl_xor(lnf, d);
      if (lane == 0) redp[wave] = lnf;
      // ONE barrier per walker: it publishes this walker's buffers; the other pair of buffers is rewritten only after the next
      // walker's barrier, which no wave reaches before it has finished this walker's items
      __syncthreads();
      double lnsum = 0.0;
#pragma unroll
      for (int v = 0; v < kBlock / 64; ++v) lnsum += redp[v];
      double lnown = lnsum + vis_owner;
      if constexpr (JASTROW) lnown += -2.0 * xo * ro;
      const double cw = wi * exp(lnown);
      const uint32_t lane_occ = oe ? 1u : 0u;
#pragma unroll
      for (int j = 0; j < kRdmMaxItems; ++j) {
        const int it = tid + j * kBlock;
        if (it >= nitems) break;
        const int a0 = l0[j], a1 = l1[j];
        if (bit_of<LEN>(wk.w, a0) != lane_occ || bit_of<LEN>(wk.w, a1) != lane_occ) continue;
        const double *__restrict__ g0 = G + (size_t)a0 * Hq;
        const double *__restrict__ g1 = G + (size_t)a1 * Hq;
        double prod = 1.0;
        for (int h = 0; h < H; ++h) {
          const double g = SINGLES ? g0[h] : g0[h] * g1[h];
          prod *= fma(abp[h], g, abp[H + h]);
        }
        double v = (cw * lc[j]) * prod;
        if constexpr (JASTROW) v *= SINGLES ? evp[a0] : evp[a0] * evp[a1];
        uint32_t par;
        if constexpr (SINGLES) {
          const int hh = oe ? a0 : o0, qq = oe ? o0 : a0;
          par = bit_of<LEN>(wk.pm, hh) ^ bit_of<LEN>(wk.pm, qq) ^ (uint32_t)(hh < qq);
          if (par) v = -v;
          acc[j] += v;
          // spectators: every occupied k other than the hole, into this item's own row (no other thread touches it)
          double *__restrict__ trow = Ts + (size_t)it * sorb;
#pragma unroll
          for (int wd = 0; wd < LEN; ++wd)
            for (uint64_t bits = wk.w[wd]; bits; bits &= bits - 1) {
              const int k = 64 * wd + __builtin_ctzll(bits);
              if (k != hh) trow[k] += v;
            }
        } else {
          // holes h0 > h1 (or alpha, beta), particles q0 > q1
          const int h0 = oe ? a0 : o0, h1 = oe ? a1 : o1, q0 = oe ? o0 : a0, q1 = oe ? o1 : a1;
          par = bit_of<LEN>(wk.pm, h0) ^ bit_of<LEN>(wk.pm, h1) ^ bit_of<LEN>(wk.pm, q0) ^ bit_of<LEN>(wk.pm, q1) ^ 1u;
          if (cls < 2) par ^= (uint32_t)(h0 < q0) ^ (uint32_t)(h1 < q0) ^ (uint32_t)(h0 < q1) ^ (uint32_t)(h1 < q1);
          else par ^= (uint32_t)(h0 < q0) ^ (uint32_t)(h1 < q1) ^ (uint32_t)(h0 < q1) ^ (uint32_t)(h1 < q0);  // (ha, hb), (qa, qb): detcore.h decode
          if (par) v = -v;
          acc[j] += v;
        }
      }
    }
  }
  // ---- results: directed tables [particle side][hole side]
#pragma unroll
  for (int j = 0; j < kRdmMaxItems; ++j) {
    const int it = tid + j * kBlock;
    if (it >= nitems) break;
    if constexpr (SINGLES) {
      const int part = oe ? o0 : l0[j], hole = oe ? l0[j] : o0;
      double *__restrict__ out = ws + r.offT + slice * r.szT + ((int64_t)part * sorb + hole) * (sorb + 1);
      if (part != hole) {
        for (int k = 0; k < sorb; ++k) out[k] = Ts[(size_t)it * sorb + k];
        out[sorb] = acc[j];
      }
    } else {
      const int64_t np = cls < 2 ? r.npS : (int64_t)K * K;
      const int64_t at = oe ? (int64_t)owner_rank * np + it : (int64_t)it * np + owner_rank;
      ws[r.offD[cls] + slice * r.szD[cls] + at] = acc[j];
    }
  }
}

// every entry of rdm1 and every packed slot of rdm2 from the tables, one thread each
__global__ __launch_bounds__(kBlock) void rdm_fold_kernel(RdmLayout r, const double *__restrict__ ws, double *__restrict__ rdm1,
                                                          double *__restrict__ rdm2, int64_t nslots) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int sorb = r.sorb, K = r.K;
  // the slices' tables in slice order
  auto sumS = [&](int64_t off, int64_t sz, int nsl, int64_t at) {
    double v = 0.0;
    for (int sl = 0; sl < nsl; ++sl) v += ws[off + sl * sz + at];
    return v;
  };
  auto Tsum = [&](int part, int hole, int k) { return sumS(r.offT, r.szT, r.nslS, ((int64_t)part * sorb + hole) * (sorb + 1) + k); };
  if (g < (int64_t)sorb * sorb) {
    const int q = (int)(g / sorb), h = (int)(g - (int64_t)q * sorb);
    double v = 0.0;
    if (q == h) v = sumS(r.offDg, r.szDg, r.nslS, (int64_t)h * sorb + h);
    else if (((q ^ h) & 1) == 0) v = Tsum(q, h, sorb);
    rdm1[g] = v;
  }
  if (g >= nslots) return;
  // g = P (P + 1) / 2 + Q, P >= Q
  int64_t P = (int64_t)((sqrt(8.0 * (double)g + 1.0) - 1.0) * 0.5);
  while (P * (P + 1) / 2 > g) --P;
  while ((P + 1) * (P + 2) / 2 <= g) ++P;
  const int64_t Q = g - P * (P + 1) / 2;
  int i, j, k, l;
  pair_unrank((int)P, i, j);
  pair_unrank((int)Q, k, l);
  double v = 0.0;
  if (P == Q) {
    v = sumS(r.offDg, r.szDg, r.nslS, (int64_t)i * sorb + j);
  } else if (i != k && i != l && j != k && j != l) {
    const bool sameP = ((i ^ j) & 1) == 0, sameQ = ((k ^ l) & 1) == 0;
    if (sameP && sameQ && ((i ^ k) & 1) == 0) {
      const int c = i & 1;
      const int64_t a = (int64_t)(i >> 1) * ((i >> 1) - 1) / 2 + (j >> 1), b = (int64_t)(k >> 1) * ((k >> 1) - 1) / 2 + (l >> 1);
      v = sumS(r.offD[c], r.szD[c], r.nslD, a * r.npS + b) + sumS(r.offD[c], r.szD[c], r.nslD, b * r.npS + a);
    } else if (!sameP && !sameQ) {
      const int ia = (i & 1) ? j : i, ib = (i & 1) ? i : j, ka = (k & 1) ? l : k, kb = (k & 1) ? k : l;
      const int64_t a = (int64_t)(ia >> 1) * K + (ib >> 1), b = (int64_t)(ka >> 1) * K + (kb >> 1), np = (int64_t)K * K;
      v = sumS(r.offD[2], r.szD[2], r.nslD, a * np + b) + sumS(r.offD[2], r.szD[2], r.nslD, b * np + a);
    }
  } else {
    // one shared orbital s: pair P = (h, s), pair Q = (q, s); the singles h -> q and q -> h, spectator s
    const int s = (i == k || i == l) ? i : j, h = (s == i) ? j : i, q = (s == k) ? l : k;
    if (((h ^ q) & 1) == 0) {
      const double t = Tsum(q, h, s) + Tsum(h, q, s);
      v = ((h > s) != (q > s)) ? -t : t;
    }
  }
  rdm2[g] = v;
}

}  // namespace pynqs

// =================================================================================================
using namespace pynqs;

extern "C" int pynqs_rdm_scatter(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const double *w,
                                 const double *ratio, int is_complex, double *rdm1, double *rdm2, void *stream) {
  pynqs::DeviceScope device_scope_(rdm1);
  SDParams p;
  if (!make_sd_params(sorb, nele, noA, noB, &p) || nele != noA + noB) return set_error(PYNQS_EINVAL, "rdm_scatter: bad sorb/nele/noA/noB");
  if (nbatch < 0 || nbatch > 0x7fffffffll) return set_error(PYNQS_EINVAL, "rdm_scatter: bad nbatch");
  if (nbatch == 0) return PYNQS_OK;
  if (!bra || !w || !ratio || !rdm1 || !rdm2) return set_error(PYNQS_EINVAL, "null pointer");
  const size_t lds = lds_bytes(p, 0);
  if (lds > kRdmMaxLds) return set_error(PYNQS_EINVAL, "rdm_scatter: the walker tables of this system do not fit the LDS");
  const int len = (sorb - 1) / 64 + 1;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_LEN(len, {
    if (is_complex) hipLaunchKernelGGL((rdm_scatter_kernel<LEN, true>), dim3((uint32_t)nbatch), dim3(kBlock), lds, st, bra, w, ratio, p, rdm1, rdm2);
    else hipLaunchKernelGGL((rdm_scatter_kernel<LEN, false>), dim3((uint32_t)nbatch), dim3(kBlock), lds, st, bra, w, ratio, p, rdm1, rdm2);
  });
  return check_launch("rdm_scatter");
}

extern "C" int pynqs_rdm_rbm_supported(int sorb, int nele, int noA, int noB, int nhidden) {
  RdmLayout r;
  if (nele != noA + noB || !make_rdm_layout(0, sorb, noA, noB, nhidden, &r)) return 0;
  if (nhidden > kRdmMaxHidden || sorb > kBlock || r.K * r.K > kRdmMaxItems * kBlock) return 0;
  return rdm_lds_bytes(r, true) <= kRdmMaxLds ? 1 : 0;
}

extern "C" int64_t pynqs_rdm_rbm_workspace(int64_t nbatch, int sorb, int nhidden) {
  RdmLayout r;
  if (!make_rdm_layout(nbatch, sorb, 0, 0, nhidden, &r)) return -1;
  return r.total * 8;
}

// pynqs_rdm_rbm (jastrow_table null) and pynqs_rdm_jrbm: the same launches, the JASTROW flavour of the owner kernel and rdm_r_kernel before it
static int rdm_fused_launch(const char *what, const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const double *w,
                            const void *rbm_table, const void *jastrow_table, int nhidden, void *workspace, double *rdm1, double *rdm2,
                            void *stream) {
  const bool jastrow = jastrow_table != nullptr;
  if (nbatch < 0 || nbatch > 0x7fffffffll) return set_error(PYNQS_EINVAL, jastrow ? "rdm_jrbm: bad nbatch" : "rdm_rbm: bad nbatch");
  RdmLayout r;
  RbmLayout rl;
  make_rdm_layout(nbatch, sorb, noA, noB, nhidden, &r);
  make_rbm_layout(sorb, nhidden, &rl);
  RdmJastrow jz = {nullptr, 0, 0};
  if (jastrow) {
    JastrowLayout jl;
    make_jastrow_layout(sorb, &jl);
    jz.tab = (const double *)jastrow_table; jz.offS = jl.offS; jz.offR = r.total;
  }
  hipStream_t st = (hipStream_t)stream;
  double *ws = (double *)workspace;
  const double *rbm = (const double *)rbm_table;
  // (the last kernel reads only entries that some workgroup has written -- every (owner, item, slice) writes its sum, zero included --
  // so the tables need no clearing; without walkers nothing is launched to write them)
  if (nbatch == 0 && hipMemsetAsync(ws, 0, (size_t)r.total * 8, st) != hipSuccess) return check_launch(what);
  const int len = (sorb - 1) / 64 + 1;
  const int64_t nth = nbatch * nhidden, nr = nbatch * sorb;
  if ((nth + kBlock - 1) / kBlock > 0x7fffffffll) return set_error(PYNQS_EINVAL, jastrow ? "rdm_jrbm: too many walkers for one call" : "rdm_rbm: too many walkers for one call");
  const uint32_t nowners = 2u * (uint32_t)r.npS + (uint32_t)(r.K * r.K);
  const size_t ldsD = rdm_lds_bytes(r, false, jastrow), ldsS = rdm_lds_bytes(r, true, jastrow);
  DISPATCH_LEN(len, {
    if (nth > 0) {
      hipLaunchKernelGGL((rdm_theta_kernel<LEN>), dim3((uint32_t)((nth + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, bra, nbatch, r, rbm, rl.offHb, ws);
      hipLaunchKernelGGL((rdm_diag_kernel<LEN>), dim3((uint32_t)(sorb * r.nslS)), dim3(kBlock), 0, st, bra, nbatch, w, r, ws);
      if (jastrow) {
        hipLaunchKernelGGL((rdm_r_kernel<LEN>), dim3((uint32_t)((nr + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, bra, nbatch, sorb, jz, ws);
        hipLaunchKernelGGL((rdm_rbm_kernel<LEN, false, true>), dim3(nowners * (uint32_t)r.nslD), dim3(kBlock), ldsD, st, bra, nbatch, w, r, rbm, ws, jz);
        hipLaunchKernelGGL((rdm_rbm_kernel<LEN, true, true>), dim3((uint32_t)(sorb * r.nslS)), dim3(kBlock), ldsS, st, bra, nbatch, w, r, rbm, ws, jz);
      } else {
        hipLaunchKernelGGL((rdm_rbm_kernel<LEN, false, false>), dim3(nowners * (uint32_t)r.nslD), dim3(kBlock), ldsD, st, bra, nbatch, w, r, rbm, ws, jz);
        hipLaunchKernelGGL((rdm_rbm_kernel<LEN, true, false>), dim3((uint32_t)(sorb * r.nslS)), dim3(kBlock), ldsS, st, bra, nbatch, w, r, rbm, ws, jz);
      }
    }
  });
  const int64_t pair = (int64_t)sorb * (sorb - 1) / 2, nslots = pair * (pair + 1) / 2;
  const int64_t nfold = nslots > (int64_t)sorb * sorb ? nslots : (int64_t)sorb * sorb;
  hipLaunchKernelGGL(rdm_fold_kernel, dim3((uint32_t)((nfold + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, r, ws, rdm1, rdm2, nslots);
  return check_launch(what);
}

extern "C" int pynqs_rdm_rbm(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const double *w,
                             const void *rbm_table, int nhidden, void *workspace, double *rdm1, double *rdm2, void *stream) {
  pynqs::DeviceScope device_scope_(rdm1);
  if (!pynqs_rdm_rbm_supported(sorb, nele, noA, noB, nhidden)) return set_error(PYNQS_EINVAL, "rdm_rbm: sizes not served by the fused kernel");
  if (!rbm_table || !workspace || !rdm1 || !rdm2 || (nbatch > 0 && (!bra || !w))) return set_error(PYNQS_EINVAL, "null pointer");
  return rdm_fused_launch("rdm_rbm", bra, nbatch, sorb, nele, noA, noB, w, rbm_table, nullptr, nhidden, workspace, rdm1, rdm2, stream);
}

extern "C" int pynqs_rdm_jrbm_supported(int sorb, int nele, int noA, int noB, int nhidden) {
  RdmLayout r;
  JastrowLayout jl;
  if (!pynqs_rdm_rbm_supported(sorb, nele, noA, noB, nhidden) || !make_jastrow_layout(sorb, &jl)) return 0;
  make_rdm_layout(0, sorb, noA, noB, nhidden, &r);
  return rdm_lds_bytes(r, true, true) <= kRdmMaxLds ? 1 : 0;
}

extern "C" int64_t pynqs_rdm_jrbm_workspace(int64_t nbatch, int sorb, int nhidden) {
  RdmLayout r;
  if (!make_rdm_layout(nbatch, sorb, 0, 0, nhidden, &r)) return -1;
  return (r.total + nbatch * sorb) * 8;  // r [n][sorb] behind pynqs_rdm_rbm's
}

extern "C" int pynqs_rdm_jrbm(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const double *w,
                              const void *rbm_table, const void *jastrow_table, int nhidden, void *workspace, double *rdm1, double *rdm2,
                              void *stream) {
  pynqs::DeviceScope device_scope_(rdm1);
  if (!pynqs_rdm_jrbm_supported(sorb, nele, noA, noB, nhidden)) return set_error(PYNQS_EINVAL, "rdm_jrbm: sizes not served by the fused kernel");
  if (!rbm_table || !jastrow_table || !workspace || !rdm1 || !rdm2 || (nbatch > 0 && (!bra || !w))) return set_error(PYNQS_EINVAL, "null pointer");
  return rdm_fused_launch("rdm_jrbm", bra, nbatch, sorb, nele, noA, noB, w, rbm_table, jastrow_table, nhidden, workspace, rdm1, rdm2, stream);
}
