// kernels_rbm.hip -- SIMPLE local energy (vmc/energy/eloc.py:121-203, _simple) with the amplitude ratio of a real
// RBM (vmc/ansatz/rbm/rbm.py:186-211) evaluated on chip: nothing of size nbatch x ncomb ever reaches HBM.
//
//   E_loc(x) = sum_x' <x|H|x'> psi(x') / psi(x),     psi(x) = exp(a.x) prod_h 2 cosh(theta_h(x))
//
// An excitation flips 2 or 4 orbitals F (occupied x_o = +1 -> -1, empty -1 -> +1): theta'_h = theta_h - delta_h,
// delta_h = 2 sum_{o in F} W[h][o] x_o.  With s_h = sign(theta_h), rho_h = exp(-2|theta_h|), m_h = 1/(1+rho_h):
//   cosh(theta_h - delta_h) / cosh(theta_h) = exp(-s_h delta_h) * (m_h + m_h rho_h * prod_{o in F} q_h(o)),
//   q_h(o) = exp(4 s_h W[h][o] x_o)
// (no overflow for any theta; the reference's psi(x')/psi(x) of two products over-/underflows first), so
//   psi(x')/psi(x) = prod_{o in F} C(o) * prod_h (m_h + n_h prod_{o in F} q_h(o)),
//   C(o) = exp(-2 x_o (a_o + sum_h s_h W[h][o])),  n_h = m_h rho_h.
// Every excitation multiplies four rows (a single: its two orbitals and a dummy row twice), so the rows kept in
// LDS are q'_h(o) = (m_h rho_h)^(1/4) q_h(o) and a factor is m_h + prod_{o in F} q'_h(o).
// Per walker the workgroup builds q'[o][h] in LDS (one read of exp(+-4W) per element, no transcendental in the
// inner loop) and C(o); then every lane owns a 4 x 4 block of excitations -- 4 entries of a class's "fast"
// excitation table x 4 entries of its "slow" table (hole pairs x particle pairs, alpha singles x beta singles:
// detcore.h) -- and runs over the hidden units with 16 running products in registers:
//   per hidden unit and lane: 16 LDS reads, 8 multiplications for the 8 pair products, 16 x (fma + mul).
// The cut into blocks and tiles, phase A's diagonal and singles, the sums over waves, the tail of the LDS layout and the host-side
// launch rules are shared with the complex-parameter kernel (kernels_rbm_complex.hip): rbm_tiles.h.
// The kernel is bound by the f64 vector rate (84 % busy), not by HBM.  When sorb x
// num_hidden does not fit the LDS the WINDOWED variant streams q' through it (see eloc_rbm_kernel).
// Matrix elements come from the integral plan exactly as in kernels_plan.hip.
//
// FLAVOUR selects the reference's other amplitudes that share the hidden-unit product (rbm.py:199-211):
//   kRbmReal  psi = exp(a.x)  prod_h 2cosh(theta_h)
//   kRbmTanh  psi = tanh(a.x) prod_h 2cosh(theta_h)            -- C(o) without a_o; tanh(a.x') = 1 - 2 / (exp(2 a.x') + 1) with
//             exp(2 a.x') = exp(2 a.x) prod_{o in F} exp(-4 x_o a_o): table products and one division per column
//   kRbmPhase psi = exp(i (a.x + sum_h ln 2cosh(theta_h)))     -- "pRBM": the phase difference of x' and x IS the logarithm of the
//             real flavour's ratio, so psi(x')/psi(x) = exp(i ln t) with t from the same running products; E_loc is complex
// ("cos" and "complex" need complex running products: they take the module path.)
//
// GREEN: the fixed-node Green's-function row of a GFMC step (gfmc/walker.py:167-235, _calculate_green_kernel) from the same
// pass, for the real-valued flavours: with r_k = psi(x'_k)/psi(x) and h_k = <x|H|x'_k>, a move k >= 1 keeps the sign when
// h_k r_k < 0 (the reference's cos(phase difference + gamma) < 0) and then has weight g_k = -h_k r_k; the others add to the
// sign-flip potential v_sf = sum h_k r_k on the diagonal: g_0 = max(0, Lambda - h_0 - v_sf).  The row is written in the
// reference's column order (column = 1 + rank, excitation.cpp:43-109 incl. the `idx % noAA` rotation); E_loc is unchanged.
//
// JASTROW (real flavour, resident form): psi(x) = exp(a.x + x^T M x) prod_h 2cosh(theta_h), the two-body Jastrow factor of
// vmc/ansatz/rbm/rbm_other.py (class Jastrow) multiplied onto the RBM.  With S = M + M^T (zero diagonal; the Jastrow table of rbm.h) and
// r_o = sum_j S_oj x_j, flipping the orbitals F changes x^T M x by  -2 sum_{o in F} x_o r_o + 4 sum_{i<j in F} S_ij x_i x_j:
//   the first term joins C(o) = exp(-2 x_o (a_o + r_o + sum_h s_h W[h][o])): nothing new per column, no LDS;
//   the second is a product of pair factors exp(4 S_ij x_i x_j) = E4p[i][j] where the walker's x_i = x_j, else E4m[i][j]: one for a
//   single, six for a double, read in the tile epilogue and multiplied onto the running products: a lane's 4 x 4 block takes 4 + 4
//   loads for the pairs inside its fast and slow entries and 64 for the crossed pairs, 4.5 loads and 6 products per column.  They come
//   from a per-walker triangle P[i > j] = exp(4 S_ij x_i x_j) in LDS behind the trailer (4 sorb (sorb - 1) bytes, built from the table
//   next to C(o); `pairs_in_lds`) where three workgroups still fit a CU with it, else from the table itself (L2-resident, 16 sorb^2
//   bytes).  Fe2S2, 8192 walkers: 0.97-1.13 ms from LDS, 1.00-1.17 ms from L2, pynqs_eloc_rbm 0.77 ms in the same run.
// tr M scales psi(x) only.  Every statement of it stands under `if constexpr (JASTROW)`.
//
// GREEN and JASTROW together (pynqs_green_jrbm): the pair factors join the running products in the tile epilogue BEFORE add_column, so
// the row, v_sf and the diagonal see the full ratio.
//
// The arguments mean the same in all 57 instantiations: `green`, `lambda`, `clamped` are the row's (nullptr, 0, nullptr without GREEN),
// `jastrow` is the Jastrow table (nullptr without JASTROW), `pairs_in_lds` the home of the walker's pair factors, `chunks` the workgroups
// per walker (1 with GREEN: the row finishes its diagonal in the kernel).
//
// SIGNED (no GREEN form): every column's matrix element times sigma_k = eta_m(x'_k) eta_m(x), eta_m(y) = (-1)^(doubly occupied spatial
// orbitals of y): the second pass of the spin-flip-projected local energy (vmc/energy/flip.py, _simple_flip; pynqs_eloc_rbm_flip /
// pynqs_eloc_jrbm_flip below, formula in include/pynqs_amd.h), run on the spin-mirrored table W[h][o ^ 1], a[o ^ 1] (M[i ^ 1][j ^ 1]), whose
// amplitude is psi(flip y).  Flipping orbital o changes the number of doubly occupied spatial orbitals by the walker's bit at o ^ 1, so
// sigma_k = (-1)^pi_k with pi_k = XOR_{o in F} occ(o ^ 1) XOR #(spatial orbitals with both spin orbitals in F): two 4-bit masks per lane in
// the tile epilogue, XORed into the doubles' fermionic parity and applied to the staged singles where they are consumed; x' = x has +1.
// Every statement of it stands under `if constexpr (SIGNED)`; the other instantiations' registers are what they were.
#include <string.h>

#include "rbm.h"
#include "rbm_math.h"
#include "rbm_tiles.h"

namespace pynqs {

// W[H][sorb], hb[H], vb[sorb] (row-major, the reference's parameter shapes) -> RBM table (rbm.h)
__global__ __launch_bounds__(kBlock) void rbm_table_kernel(const double *__restrict__ W, const double *__restrict__ hb,
                                                           const double *__restrict__ vb, RbmLayout rl, double *__restrict__ tab) {
  const int64_t row = (int64_t)rl.sorb * rl.Hq;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < row) {
    const int o = (int)(i / rl.Hq), h = (int)(i - (int64_t)o * rl.Hq);
    const double w = h < rl.H ? W[(int64_t)h * rl.sorb + o] : 0.0;
    tab[rl.offWt + i] = w;
    tab[rl.offE4p + i] = exp(4.0 * w);
    tab[rl.offE4m + i] = exp(-4.0 * w);
  }
  if (i < rl.Hq) tab[rl.offHb + i] = i < rl.H ? hb[i] : 0.0;
  if (i < rl.total - rl.offVb) tab[rl.offVb + i] = (vb && i < rl.sorb) ? vb[i] : 0.0;
}

constexpr int kRbmFB = 4;   // a lane owns 4 x 4 excitations (rbm_tiles.h)
constexpr int kRbmRed = 1;  // doubles per wave in the LDS trailer

// LDS after the walker tables (16-byte aligned): [q / staging][mn][sh][Cq][hs]
//   q   [sorb + 1][hw+1] row r(o) = o/2 for alpha, sorb/2 + o/2 for beta orbitals (a wave mostly reads rows of one
//                       spin: consecutive rows -> different bank pairs); row `sorb` belongs to the dummy orbital
//                       (the partner of a single); hw hidden units at a time (all of them in the fast kernel)
//   mn  [2][Hq]         m_h, then (m_h rho_h)^(1/4) (1, 0 in the padding)
//   sh  [Hq]            s_h
//   Cq  [sorb + 2]      C(o) by orbital, 1 for the dummy orbital `sorb`
//   hs  [d1 + 2]        <x|H|x>, then the singles
// then rowaddr and the trailer (rbm_tiles.h)
__device__ __forceinline__ uint32_t rbm_row(uint32_t o, uint32_t K) { return (o >> 1) + ((o & 1u) ? K : 0u); }
typedef __attribute__((address_space(3))) const double lds_cdouble;  // read through a 32-bit LDS address

struct RbmLds {
  double *q, *mn, *sh, *Cq, *Aq, *hs;  // Aq [sorb + 2]: exp(-4 x_o a_o) (tanh flavour: exp(2 a.x') = exp(2 a.x) prod over the flipped orbitals)
  uint32_t *rowaddr;  // [sorb + 2]: LDS byte address of an orbital's q row (the dummy's at index sorb)
};

// `hw` = hidden units resident in LDS at a time: rl.Hloop (all of them, the fast kernel) or a multiple of 8 (the
// windowed kernel for sorb x num_hidden beyond the LDS); row stride hw + 1 doubles (odd: see rbm.h)
__host__ __device__ inline size_t rbm_region_bytes(const SDParams &p, uint32_t hw) {
  return (((size_t)(p.sorb + 1) * (hw + 1) * 8) + 15) & ~(size_t)15;
}

__host__ __device__ inline size_t lds_bytes_rbm(const SDParams &p, const RbmLayout &rl, uint32_t hw) {
  return rbm_q_offset(p) + rbm_region_bytes(p, hw) +
         8 * (3 * (size_t)rl.Hq + 2 * (size_t)(p.sorb + 2) + (size_t)(p.d1 + 2)) + 4 * (((size_t)p.sorb + 2 + 3) & ~(size_t)3) + rbm_trailer_bytes(kRbmRed);
}

// WINDOWED = false: all hidden units of q' live in LDS, waves pull tiles from a counter (the fast kernel).
// WINDOWED = true : sorb x num_hidden does not fit: the workgroup streams q' through LDS `hw` hidden units at a time;
//                   in every round each wave holds the 16 x 64 running products of ONE tile in registers across the
//                   windows (two barriers per window).
enum : int { kRbmReal = 0, kRbmTanh = 1, kRbmPhase = 2 };

template <int LEN, bool WINDOWED, int FLAVOUR, bool GREEN, bool JASTROW = false, bool SIGNED = false>
__global__ __launch_bounds__(1024, 4) void eloc_rbm_kernel(const uint64_t *__restrict__ bra, SDParams p, PlanLayout pl, RbmLayout rl,
                                                          RbmBlocks<kRbmFB> B, uint32_t chunks, uint32_t hw, const double *__restrict__ plan,
                                                          const double *__restrict__ rbm, double *__restrict__ eloc,
                                                          double *__restrict__ psi, double lambda, double *__restrict__ green,
                                                          uint8_t *__restrict__ clamped, const double *__restrict__ jastrow, bool pairs_in_lds) {
  static_assert(!GREEN || FLAVOUR != kRbmPhase, "the fixed-node row needs a real-valued amplitude");
  static_assert(!JASTROW || (FLAVOUR == kRbmReal && !WINDOWED), "the Jastrow factor: real flavour, resident form");
  static_assert(!SIGNED || !GREEN, "the signed sum is the second pass of the spin-flip-projected energy: no row");
  // `chunks` = workgroups per walker; 1 whenever GREEN.  Only the row with the Jastrow factor takes the 1 at compile time: a run-time count
  // costs that form 6-9 spilled SGPRs, a compile-time 1 in every GREEN form costs <3, true, 0, true> 14 spilled VGPRs
  // (profiles/eloc_rbm_args_resource_usage.txt).
  // `pairs_in_lds` is a `bool`, read where it is used, by measurement too: as a `uint32_t`, in another place of the list, or taken into a
  // local at the top, the JASTROW forms compile with fewer spills and pynqs_eloc_jrbm runs 1-1.4 % slower (same file).
  const uint32_t nchunks = (GREEN && JASTROW) ? 1u : chunks;
  // no static __shared__ here: with the dynamic region at LDS address 0 the row offsets below are the addresses and
  // the ds_read immediates carry the rest (a static in front costs one v_add per read)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const RbmTrailer T = rbm_trailer(smem, lds_bytes_rbm(p, rl, hw), kRbmRed);
  const uint64_t wg = blockIdx.x;
  const uint64_t walker = wg / nchunks;
  const uint32_t chunk = (uint32_t)(wg - walker * nchunks);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nthreads = blockDim.x, nwaves = nthreads >> 6;  // 3 or 4 waves: whichever divides the walker's tiles better
  if (tid == 0) { *T.next_tile = 0; *T.next_single = 0; }
  Walker<LEN> wk;
  load_walker<LEN>(bra + walker * LEN, wk);
  const LdsLayout L = carve_lds(smem, p);
  const int nocc = build_walker_tables<LEN>(wk, p, L);
  const int sorb = p.sorb, H = rl.H, Hq = rl.Hq;
  const uint32_t K = (uint32_t)sorb >> 1;
  RbmLds R;
  {
    // (plain offsets from the LDS array: a pointer that went through an integer cast is no longer known to be LDS
    // and its loads become flat_load with full waits)
    R.q = reinterpret_cast<double *>(smem + rbm_q_offset(p));
    R.mn = reinterpret_cast<double *>(smem + rbm_q_offset(p) + rbm_region_bytes(p, hw));
    R.sh = R.mn + 2 * Hq;
    R.Cq = R.sh + Hq;
    R.Aq = R.Cq + (sorb + 2);
    R.hs = R.Aq + (sorb + 2);
    R.rowaddr = reinterpret_cast<uint32_t *>(R.hs + (p.d1 + 2));
  }
#if defined(PYNQS_RBM_STOP) && PYNQS_RBM_STOP == 1
  if (tid == 0) eloc[walker] = (double)nocc;
  return;
#endif
  // ---- phase A, no barrier inside: three independent jobs on different waves -----------------------------------
  //   last wave  : <x|H|x> (ordered sum of nele(nele+1)/2 terms by one lane: the longest serial job)
  //   other waves: theta_h -> m_h, n_h, s_h (and ln psi(x)), then the singles' matrix elements in tiles of 16
  // The singles / diagonal are staged in wave-private quarters of the region q will occupy afterwards.
  const bool need_hs = rbm_needs_hs(B, chunk);
  const double *__restrict__ Wt = rbm + rl.offWt;
  double lnpsi = 0.0;
  [[maybe_unused]] double xsx = 0.0;  // JASTROW: this thread's share of sum_{i<j} S_ij x_i x_j = sum_o x_o r_o / 2, summed apart from lnpsi
  const int kThetaThreads = nthreads - 64;
  if (wave == nwaves - 1) {
    rbm_diagonal(need_hs, lane, p, pl, L, plan, R.hs);
  } else {
    for (int h = tid; h < Hq; h += kThetaThreads) {
      double m = 1.0, n = 0.0, s = 1.0;
      if (h < H) {
        double th = rbm[rl.offHb + h];
#pragma unroll 16
        for (int o = 0; o < sorb; ++o) {  // independent loads: 16 in flight per round trip (L2 latency ~0.6 us)
          const double w = Wt[(size_t)o * Hq + h];
          th += bit_of<LEN>(wk.w, o) ? w : -w;
        }
        const double a = fabs(th), rho = exp(-2.0 * a), lc = a + log1p(rho);  // lc = ln 2cosh(theta)
        m = 1.0 / (1.0 + rho);
        n = exp(-0.25 * (a + lc));  // (m rho)^(1/4): every excitation multiplies four rows (singles: two + dummy twice)
        s = th >= 0.0 ? 1.0 : -1.0;
        lnpsi += lc;
      }
      R.mn[h] = m; R.mn[Hq + h] = n; R.sh[h] = s;
    }
  }
  rbm_singles(need_hs, lane, p, pl, L, nocc, plan, R.hs, T.next_single);  // every wave, as it becomes free
  __syncthreads();
#if defined(PYNQS_RBM_STOP) && PYNQS_RBM_STOP == 2
  if (tid == 0) eloc[walker] = R.hs[0];
  return;
#endif
  // ---- phase B: q'[o][h] = (m_h rho_h)^(1/4) exp(4 s_h x_o W[h][o]) for the hidden units [h0, h0 + hw) into LDS, a wave
  // per row, and (with_sum) sum_h s_h W[h][o] -> Cq[o].  kRowBatch rows x 2 columns per lane are requested together:
  // an un-batched loop pays one L2 round trip per row.
  constexpr int kRowBatch = 4;
  const double *__restrict__ E4 = rbm + rl.offE4p;
  const uint32_t dE4 = (uint32_t)(rl.offE4m - rl.offE4p), uHq = (uint32_t)Hq, stride = hw + 1;
  auto build_window = [&](uint32_t h0, bool with_sum) {
    bool pos[2];   // s_h > 0 for this lane's two columns
    double fq[2];  // (m_h rho_h)^(1/4), 0 in the padding
    double sgn[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const uint32_t j = lane + 64 * c, h = h0 + j;
      const bool in = j < hw && h < (uint32_t)H;
      sgn[c] = in ? R.sh[h] : 0.0;
      pos[c] = sgn[c] > 0.0;
      fq[c] = in ? R.mn[Hq + h] : 0.0;
    }
    for (int o0 = wave; o0 <= sorb; o0 += nwaves * kRowBatch) {
      double e4[kRowBatch][2], wv[kRowBatch][2];
#pragma unroll
      for (int b = 0; b < kRowBatch; ++b) {
        const int o = o0 + b * nwaves;
        const bool occ = o < sorb && bit_of<LEN>(wk.w, o);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const uint32_t j = lane + 64 * c, h = h0 + j, idx = (uint32_t)o * uHq + h;
          e4[b][c] = 1.0; wv[b][c] = 0.0;
          if (o < sorb && j < hw && h < (uint32_t)H) {
            e4[b][c] = E4[idx + (pos[c] == occ ? 0u : dE4)];
            if (with_sum) wv[b][c] = Wt[idx];
          }
        }
      }
#pragma unroll
      for (int b = 0; b < kRowBatch; ++b) {
        const int o = o0 + b * nwaves;
        if (o > sorb) break;  // wave-uniform
        const bool occ = o < sorb && bit_of<LEN>(wk.w, o);
        const uint32_t rowq = (o < sorb ? rbm_row(o, K) : (uint32_t)sorb) * stride;
        double S = sgn[0] * wv[b][0] + sgn[1] * wv[b][1];
#pragma unroll
        for (int c = 0; c < 2; ++c)
          if (lane + 64 * c < stride) R.q[rowq + lane + 64 * c] = e4[b][c] * fq[c];
        for (uint32_t j = lane + 128; j < stride; j += 64) {  // windows wider than 128 hidden units: the rest of the row
          const uint32_t h = h0 + j;
          double v = 0.0;
          if (j < hw && h < (uint32_t)H) {
            const double s2 = R.sh[h];
            v = R.mn[Hq + h];
            if (o < sorb) {
              const uint32_t idx = (uint32_t)o * uHq + h;
              v *= E4[idx + ((s2 > 0.0) == occ ? 0u : dE4)];
              if (with_sum) S += s2 * Wt[idx];
            }
          }
          R.q[rowq + j] = v;
        }
        if (with_sum) {
#pragma unroll
          for (int d = 32; d > 0; d >>= 1) S += __shfl_xor(S, d);
          if (lane == 0) R.Cq[o] = S;  // sum_h s_h W[h][o]; turned into C(o) below, all orbitals at once
        }
      }
    }
  };
  if constexpr (!WINDOWED) {
    build_window(0u, true);
  } else {
    // sum_h s_h W[h][o] over ALL hidden units, a wave per orbital (the windows are built inside the rounds below)
    for (int o = wave; o <= sorb; o += nwaves) {
      double S = 0.0;
      if (o < sorb)
        for (int h = lane; h < H; h += 64) S += R.sh[h] * Wt[(uint32_t)o * uHq + h];
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) S += __shfl_xor(S, d);
      if (lane == 0) R.Cq[o] = S;
    }
  }
  __syncthreads();
  const uint32_t qbase = __builtin_amdgcn_groupstaticsize() + (uint32_t)rbm_q_offset(p), rowB = stride * 8u;
  for (int o = tid; o <= sorb; o += nthreads) {
    R.rowaddr[o] = qbase + (o < sorb ? rbm_row(o, K) : (uint32_t)sorb) * rowB;
    double c = 1.0, da = 1.0;
    if (o < sorb) {
      const double x = bit_of<LEN>(wk.w, o) ? 1.0 : -1.0, a = rbm[rl.offVb + o];
      if constexpr (FLAVOUR == kRbmTanh) {
        c = exp(-2.0 * x * R.Cq[o]);
        da = exp(-4.0 * x * a);
      } else if constexpr (JASTROW) {
        // r_o = sum_j S_jo x_j (S is symmetric: column o, so that consecutive lanes read consecutive words; S_oo = 0), 16 loads in flight
        const double *__restrict__ S = jastrow;
        double r = 0.0;
#pragma unroll 16
        for (int j = 0; j < sorb; ++j) {
          const double s = S[(uint32_t)j * (uint32_t)sorb + (uint32_t)o];
          r += bit_of<LEN>(wk.w, j) ? s : -s;
        }
        c = exp(-2.0 * x * ((a + r) + R.Cq[o]));
        lnpsi += x * a;
        xsx += 0.5 * x * r;
      } else {
        c = exp(-2.0 * x * (a + R.Cq[o]));
        lnpsi += x * a;
      }
    }
    R.Cq[o] = c;
    if constexpr (FLAVOUR == kRbmTanh) R.Aq[o] = da;
  }
  if constexpr (JASTROW) {
    // the walker's pair factors in LDS (pairs_in_lds), behind the kernel's own layout (where they are is worked out again at each use:
    // nothing of it lives across the hidden-unit loop)
    // (one and two words only: at three the triangle is 66 KiB and more and never chosen, and the branch alone costs that
    // instantiation a spill inside the hidden-unit loop)
    double *jP = reinterpret_cast<double *>(smem + lds_bytes_rbm(p, rl, hw));
    if (LEN < 3 && pairs_in_lds) {  // P[a (a - 1) / 2 + b] = exp(4 S_ab x_a x_b), b < a: a wave per row, consecutive lanes read consecutive words
      const uint32_t n2 = (uint32_t)jastrow_pairs(sorb);
      for (int a = 1 + wave; a < sorb; a += nwaves) {
        const uint32_t xa = bit_of<LEN>(wk.w, a);
        for (int b = lane; b < a; b += 64)
          jP[(uint32_t)(a * (a - 1) / 2 + b)] = jastrow[(bit_of<LEN>(wk.w, b) == xa ? n2 : 2u * n2) + (uint32_t)a * (uint32_t)sorb + (uint32_t)b];
      }
    }
  }
  double ax = 0.0, e2ax = 1.0, inv_tanh_ax = 1.0;  // tanh flavour: a.x (wave-uniform: scalar loads), exp(2 a.x), 1 / tanh(a.x)
  if constexpr (FLAVOUR == kRbmTanh) {
    for (int o = 0; o < sorb; ++o) {
      const double a = rbm[rl.offVb + o];
      ax += bit_of<LEN>(wk.w, o) ? a : -a;
    }
    e2ax = exp(2.0 * ax);
    inv_tanh_ax = 1.0 / tanh(ax);
  }
  __syncthreads();
#if defined(PYNQS_RBM_STOP) && PYNQS_RBM_STOP == 3
  if (tid == 0) eloc[walker] = R.hs[0] + R.Cq[0] + R.q[5];
  return;
#endif

  // ---- tiles of 64 blocks: pulled by the waves from an LDS counter, or (WINDOWED) one per wave and round ------------
  const double *__restrict__ Vss = plan + pl.offVss;
  const double *__restrict__ Vab = plan + pl.offVab;
  const uint32_t my_tiles = B.ntiles > chunk ? (B.ntiles - chunk + nchunks - 1) / nchunks : 0;
  const uint32_t nrounds = (my_tiles + nwaves - 1) / nwaves;  // WINDOWED only
  double esum = 0.0, esum_im = 0.0;  // GREEN: esum_im collects the sign-flip potential
  double *__restrict__ grow = GREEN ? green + (size_t)walker * (p.nsd + 1) : nullptr;
  // one column's contribution: h = <x|H|x'>, t = the real flavour's psi(x')/psi(x) (for tanh: without the visible factor),
  // da = exp(2 (a.x' - a.x)), col = the reference's column of x' (GREEN)
  // (branch-free but for the GREEN store: a branch per column keeps the 16 divisions / logarithms of a block from overlapping --
  // the phase flavour ran 1.70 ms with `if (ok) add_column(...)`, 1.12 ms without)
  auto add_column = [&](bool ok, double h, double t, double da, uint32_t col) {
    if constexpr (FLAVOUR == kRbmReal || FLAVOUR == kRbmTanh) {
      double r = t;
      if constexpr (FLAVOUR == kRbmTanh) r = t * ((1.0 - 2.0 / fma(e2ax, da, 1.0)) * inv_tanh_ax);  // tanh(a.x'): exp(2 a.x') = inf -> 1, 0 -> -1
      const double hr = ok ? h * r : 0.0;
      esum += hr;
      if constexpr (GREEN) {
        const bool keeps_sign = (r < 0.0) != (h < 0.0);
        if (ok) grow[col] = keeps_sign ? -hr : 0.0;
        esum_im += keeps_sign ? 0.0 : hr;
      }
    } else {
      double sn, cs;
      sincos_mod(log(ok ? t : 1.0), sn, cs);
      esum += (ok ? h : 0.0) * cs;
      esum_im += (ok ? h : 0.0) * sn;
    }
  };
  for (uint32_t round = 0;; ++round) {
    uint32_t lt = 0;
    if constexpr (WINDOWED) {
      if (round >= nrounds) break;       // workgroup-uniform: the windows below contain barriers
      lt = round * nwaves + wave;        // >= my_tiles: a wave without a tile still helps to build the windows
    } else {
      if (lane == 0) lt = atomicAdd(T.next_tile, 1u);
      lt = __builtin_amdgcn_readfirstlane(lt);
      if (lt >= my_tiles) break;
    }
    const uint32_t id = lt < my_tiles ? (chunk + lt * nchunks) * 64u + (uint32_t)lane : 0xffffffffu;
    // class and block of this lane
    int cls = 4;
    uint32_t bid = 0, nbf = 1, offF = 0, offS = 0, nF = 1, nS = 1;
    MagicDiv dv = B.dv[0];
    if (id < B.b[0]) { cls = 0; bid = id; nbf = B.nbf[0]; offF = p.offSa; nF = p.d1; }
    else if (id < B.b[1]) { cls = 1; bid = id - B.b[0]; nbf = B.nbf[1]; dv = B.dv[1]; offF = p.offHPa; offS = p.offPPa; nF = p.noAA; nS = p.nvAA; }
    else if (id < B.b[2]) { cls = 2; bid = id - B.b[1]; nbf = B.nbf[2]; dv = B.dv[2]; offF = p.offHPb; offS = p.offPPb; nF = p.noBB; nS = p.nvBB; }
    else if (id < B.b[3]) { cls = 3; bid = id - B.b[2]; nbf = B.nbf[3]; dv = B.dv[3]; offF = p.offSa; offS = p.offSb; nF = p.nSa; nS = p.nSb; }
    const uint32_t bs = mdiv(bid, dv), bf = bid - bs * nbf;
    const bool real_fast = cls < 4, real_slow = cls >= 1 && cls < 4;
    // the 4 + 4 table entries of this lane's block; re-read where needed rather than kept in registers over the
    // hidden-unit loop (the kernel sits at the 128-VGPR line)
    auto entries = [&](uint32_t (&ef)[4], uint32_t (&es)[4]) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ef[i] = real_fast ? L.tab[offF + min(4 * bf + i, nF - 1)] : 0u;
        es[i] = real_slow ? L.tab[offS + min(4 * bs + i, nS - 1)] : 0u;
      }
    };
    double acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 1.0;
    // One hidden unit per sub-step: 16 ds_read_b64 (2 LDS cycles each, 256 B/clk) feed 8 + 32 f64 operations
    // (the rows carry (m_h rho_h)^(1/4), so the product of an excitation's four rows is n_h prod q).
    // Eight sub-steps share one update of the row addresses (immediate offsets); the empty asm keeps the compiler
    // from fusing the loads of neighbouring hidden units into ds_read2_b64 (half the LDS rate) or into 16-byte
    // loads (twice the registers: the kernel must stay below 128 VGPRs for 4 waves per SIMD).
    auto hidden_units = [&](uint32_t h0, uint32_t count) {
      // the q' rows of the 8 entries' orbitals as 32-bit LDS addresses (the dynamic region starts at the static
      // size; an array of generic pointers loses the address space and its loads become flat_load)
      uint32_t rb[16];
      {
        uint32_t ef[4], es[4];
        entries(ef, es);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          rb[2 * i] = R.rowaddr[real_fast ? (ef[i] & 0xff) : (uint32_t)sorb];
          rb[2 * i + 1] = R.rowaddr[real_fast ? ((ef[i] >> 8) & 0xff) : (uint32_t)sorb];
          rb[8 + 2 * i] = R.rowaddr[real_slow ? (es[i] & 0xff) : (uint32_t)sorb];
          rb[8 + 2 * i + 1] = R.rowaddr[real_slow ? ((es[i] >> 8) & 0xff) : (uint32_t)sorb];
        }
      }
      for (uint32_t h = 0; h < count; h += 8) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          double v[16];
#pragma unroll
          for (int k = 0; k < 16; ++k) v[k] = *reinterpret_cast<lds_cdouble *>(rb[k] + 8 * c);
          const double m = R.mn[h0 + h + c];
          double gf[4], gs[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            gf[i] = v[2 * i] * v[2 * i + 1];
            gs[i] = v[8 + 2 * i] * v[8 + 2 * i + 1];
          }
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[4 * i + j] *= fma(gf[i], gs[j], m);
          asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) rb[k] += 64;
      }
    };
    if constexpr (WINDOWED) {
      for (uint32_t h0 = 0; h0 < (uint32_t)rl.Hloop; h0 += hw) {
        __syncthreads();  // the previous window has been consumed by every wave
        build_window(h0, false);
        __syncthreads();
        hidden_units(h0, min(hw, (uint32_t)rl.Hloop - h0));
      }
    } else {
      hidden_units(0u, (uint32_t)rl.Hloop);
    }
    // matrix elements, prefactors, sum
    if (cls < 4) {
      uint32_t ef[4], es[4];
      entries(ef, es);
      double cf[4], cs[4], af[4], as[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        cf[i] = R.Cq[ef[i] & 0xff] * R.Cq[(ef[i] >> 8) & 0xff];
        cs[i] = cls == 0 ? 1.0 : R.Cq[es[i] & 0xff] * R.Cq[(es[i] >> 8) & 0xff];
        af[i] = as[i] = 1.0;
        if constexpr (FLAVOUR == kRbmTanh) {
          af[i] = R.Aq[ef[i] & 0xff] * R.Aq[(ef[i] >> 8) & 0xff];
          as[i] = cls == 0 ? 1.0 : R.Aq[es[i] & 0xff] * R.Aq[(es[i] >> 8) & 0xff];
        }
      }
      // SIGNED: sigma_k = (-1)^pi_k, pi_k = XOR over the flipped orbitals o of the walker's bit at the spin partner o ^ 1, XOR the number
      // of spatial orbitals with both spin orbitals flipped.  An entry's two orbitals have one spin, so only a fast and a slow orbital of
      // the alpha-beta class can be partners.  Bit i of sgf / sgs: the XOR over fast entry i's / slow entry i's two orbitals.
      [[maybe_unused]] uint32_t sgf = 0, sgs = 0;
      if constexpr (SIGNED) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          sgf |= (bit_of<LEN>(wk.w, (int)((ef[i] & 0xff) ^ 1u)) ^ bit_of<LEN>(wk.w, (int)(((ef[i] >> 8) & 0xff) ^ 1u))) << i;
          sgs |= (bit_of<LEN>(wk.w, (int)((es[i] & 0xff) ^ 1u)) ^ bit_of<LEN>(wk.w, (int)(((es[i] >> 8) & 0xff) ^ 1u))) << i;
        }
      }
      if constexpr (JASTROW) {
        // exp(4 S_ab x_a x_b) of two flipped orbitals, from the walker's triangle in LDS or from the table; the sign x_a x_b from the
        // walker's bits (hole-hole and particle-particle pairs +, hole-particle pairs -, whichever class and entry they come from).  The
        // pair factors join the running products before the matrix elements are gathered: one fast entry at a time (its own pair and
        // its 2 x 8 pairs with the slow entries' orbitals: 17 loads in flight), so that the 72 loads of a block never hold more
        // registers than the hidden-unit loop leaves free.
        auto join_pairs = [&](auto pair_factor) {  // pair_factor(a, b, ka, kb): a != b; ka, kb: the orbitals' bits in occ
          if (cls == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[4 * i] *= pair_factor(ef[i] & 0xff, (ef[i] >> 8) & 0xff, 2 * i, 2 * i + 1);
          } else {
            double js[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) js[j] = pair_factor(es[j] & 0xff, (es[j] >> 8) & 0xff, 8 + 2 * j, 9 + 2 * j);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const uint32_t a0 = ef[i] & 0xff, a1 = (ef[i] >> 8) & 0xff;
              const double jf = pair_factor(a0, a1, 2 * i, 2 * i + 1);
              double u[8];  // the two pairs of a0, a1 with each orbital of the slow entries
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const uint32_t b0 = es[j] & 0xff, b1 = (es[j] >> 8) & 0xff;
                u[2 * j] = pair_factor(a0, b0, 2 * i, 8 + 2 * j) * pair_factor(a1, b0, 2 * i + 1, 8 + 2 * j);
                u[2 * j + 1] = pair_factor(a0, b1, 2 * i, 9 + 2 * j) * pair_factor(a1, b1, 2 * i + 1, 9 + 2 * j);
              }
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[4 * i + j] *= (jf * js[j]) * (u[2 * j] * u[2 * j + 1]);
              asm volatile("" ::: "memory");
            }
          }
        };
        if (LEN < 3 && pairs_in_lds) {  // (workgroup-uniform)
          const double *jP = reinterpret_cast<const double *>(smem + lds_bytes_rbm(p, rl, hw));
          join_pairs([&](uint32_t a, uint32_t b, int, int) {
            const uint32_t hi = max(a, b), lo = min(a, b);
            return jP[((hi * (hi - 1u)) >> 1) + lo];
          });
        } else {
          uint32_t occ = 0;  // the walker's bits of the 16 orbitals: bit 2 i + k of entry ef[i], bit 8 + 2 j + k of es[j] (k = 0: the low byte)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            occ |= bit_of<LEN>(wk.w, (int)(ef[i] & 0xff)) << (2 * i) | bit_of<LEN>(wk.w, (int)((ef[i] >> 8) & 0xff)) << (2 * i + 1);
            occ |= bit_of<LEN>(wk.w, (int)(es[i] & 0xff)) << (8 + 2 * i) | bit_of<LEN>(wk.w, (int)((es[i] >> 8) & 0xff)) << (9 + 2 * i);
          }
          const uint32_t n2 = (uint32_t)jastrow_pairs(sorb);
          join_pairs([&](uint32_t a, uint32_t b, int ka, int kb) {
            return jastrow[((((occ >> ka) ^ (occ >> kb)) & 1u) ? 2u * n2 : n2) + a * (uint32_t)sorb + b];
          });
        }
      }
      if (cls == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t f = 4 * bf + i;
          if constexpr (SIGNED) add_column(f < nF, ((sgf >> i) & 1u) ? -R.hs[1 + min(f, nF - 1)] : R.hs[1 + min(f, nF - 1)], acc[4 * i] * cf[i], af[i], 1u + f);
          else add_column(f < nF, R.hs[1 + min(f, nF - 1)], acc[4 * i] * cf[i], af[i], 1u + f);
        }
      } else {
        const bool opp = cls == 3;
        const double *__restrict__ V = opp ? Vab : Vss + (size_t)(cls - 1) * pl.NP * pl.NP;
        const uint32_t mul = opp ? (uint32_t)(pl.K * pl.K) : (uint32_t)pl.NP;
        const uint32_t mask = opp ? 0x7fffu : 0x1fffu;
        double hv[16];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) hv[4 * i + j] = V[((es[j] >> 17) & mask) * mul + ((ef[i] >> 17) & mask)];
        // GREEN: column of (fast f, slow s) = 1 + class base + s * nF + u, u = f - rot (mod nF) for the same-spin classes
        const uint32_t cbase = 1u + (cls == 1 ? p.d1 : (cls == 2 ? p.d2 : p.d3));
        const uint32_t rot = cls == 1 ? (uint32_t)p.rotA : (cls == 2 ? (uint32_t)p.rotB : 0u);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int a0 = ef[i] & 0xff, a1 = (ef[i] >> 8) & 0xff;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int b0 = es[j] & 0xff, b1 = (es[j] >> 8) & 0xff;
            uint32_t par = ((ef[i] ^ es[j]) >> 16) & 1u;  // as plan_dev.h: finish_double
            if (opp) par ^= (uint32_t)(a0 < b1) ^ (uint32_t)(b0 < a1) ^ 1u;
            else par ^= (uint32_t)(a0 < b0) ^ (uint32_t)(a1 < b0) ^ (uint32_t)(a0 < b1) ^ (uint32_t)(a1 < b1);
            if constexpr (SIGNED)
              par ^= (((sgf >> i) ^ (sgs >> j)) & 1u) ^ (uint32_t)((a0 ^ 1) == b0) ^ (uint32_t)((a0 ^ 1) == b1) ^ (uint32_t)((a1 ^ 1) == b0) ^
                     (uint32_t)((a1 ^ 1) == b1);
            const bool ok = 4 * bf + i < nF && 4 * bs + j < nS;
            const double t = (acc[4 * i + j] * cf[i]) * cs[j];
            uint32_t col = 0;
            if constexpr (GREEN) {
              const uint32_t f = 4 * bf + i;
              col = cbase + (4 * bs + j) * nF + (f >= rot ? f - rot : f + nF - rot);
            }
            if constexpr (FLAVOUR == kRbmPhase) {
              // branch-free first pass: the phase ln t and the signed matrix element in place (0 for the padding columns of the block)
              acc[4 * i + j] = log(ok ? t : 1.0);
              hv[4 * i + j] = ok ? (par ? -hv[4 * i + j] : hv[4 * i + j]) : 0.0;
            } else {
              add_column(ok, par ? -hv[4 * i + j] : hv[4 * i + j], t, af[i] * as[j], col);
            }
          }
        }
        if constexpr (FLAVOUR == kRbmPhase) {
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            // (not the library's sincos: its large-argument path costs code and registers on each of the 16 columns, and the
            // argument, the logarithm of an amplitude ratio, is moderate: |x| < 1e5)
            double sn, cs;
            sincos_mod(acc[k], sn, cs);
            esum += hv[k] * cs;
            esum_im += hv[k] * sn;
          }
        }
      }
    }
  }
  if (chunk == 0 && tid == 0) esum += R.hs[0];  // x' = x
  // fixed-order reductions: lanes, then waves (rbm_over_waves: valid in thread 0).  kRbmPhase: eloc / psi hold (re, im) pairs
  constexpr int kOut = FLAVOUR == kRbmPhase ? 2 : 1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    esum += __shfl_xor(esum, o);
    lnpsi += __shfl_xor(lnpsi, o);
    if constexpr (FLAVOUR == kRbmPhase || GREEN) esum_im += __shfl_xor(esum_im, o);
  }
  const double e_re = rbm_over_waves(esum, T.red, tid, nwaves);
  if (tid == 0) {
    if (nchunks == 1) eloc[kOut * walker] = e_re;
    else atomicAdd(eloc + kOut * walker, e_re);
  }
  if constexpr (GREEN) {  // (launched with one workgroup per walker)
    const double v_sf = rbm_over_waves(esum_im, T.red, tid, nwaves);
    if (tid == 0) {
      const double k0 = lambda - (R.hs[0] + v_sf);
      grow[0] = k0 < 0.0 ? 0.0 : k0;
      clamped[walker] = k0 < 0.0 ? 1 : 0;
    }
  }
  if constexpr (FLAVOUR == kRbmPhase) {
    const double e_im = rbm_over_waves(esum_im, T.red, tid, nwaves);
    if (tid == 0) {
      if (nchunks == 1) eloc[2 * walker + 1] = e_im;
      else atomicAdd(eloc + 2 * walker + 1, e_im);
    }
  }
  if (psi != nullptr && chunk == 0) {  // workgroup-uniform
    const double s = rbm_over_waves(lnpsi, T.red, tid, nwaves);
    [[maybe_unused]] double xmx = 0.0;
    if constexpr (JASTROW) {  // x^T M x = tr M + sum_{i<j} S_ij x_i x_j, the sum apart from lnpsi: at most sorb - 1 of its additions round
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) xsx += __shfl_xor(xsx, o);
      xmx = rbm_over_waves(xsx, T.red, tid, nwaves) + jastrow[3 * jastrow_pairs(sorb)];
    }
    if (tid == 0) {
      if constexpr (JASTROW) psi[walker] = exp(s + xmx);
      else if constexpr (FLAVOUR == kRbmReal) psi[walker] = exp(s);
      else if constexpr (FLAVOUR == kRbmTanh) psi[walker] = tanh(ax) * exp(s);
      else sincos(s, &psi[2 * walker + 1], &psi[2 * walker]);
    }
  }
}

}  // namespace pynqs

// =================================================================================================
using namespace pynqs;

static int rbm_block_env() {  // PYNQS_RBM_BLOCK, read once
  static const int blk_env = getenv("PYNQS_RBM_BLOCK") ? atoi(getenv("PYNQS_RBM_BLOCK")) : 0;
  return blk_env;
}

// Shape of the windowed kernel (sorb x num_hidden does not fit in LDS), by the number of tiles a walker's row has:
// many tiles -> ONE workgroup of 1024 threads per CU around a 136 KiB window (16 waves share it, half as many windows
// and barriers: sorb 120, 240 hidden units, 1024 walkers: 70.3 ms with 256 threads and 64 KiB, 41.6 with 512 and 64 KiB,
// 32.6 with 1024 and 136 KiB); fewer tiles than waves would idle -> 512 or 256 threads, two workgroups per CU around
// 64 KiB windows.  PYNQS_RBM_BLOCK / PYNQS_RBM_WINDOW_KB override.
struct RbmShape {
  uint32_t threads;
  size_t window_lds;
};
static RbmShape rbm_windowed_shape(uint32_t ntiles) {
  const int blk_env = rbm_block_env();
  static const int win_env = getenv("PYNQS_RBM_WINDOW_KB") ? atoi(getenv("PYNQS_RBM_WINDOW_KB")) : 0;
  RbmShape s;
  s.threads = (blk_env == 256 || blk_env == 512 || blk_env == 1024) ? (uint32_t)blk_env : (ntiles >= 64 ? 1024u : (ntiles >= 24 ? 512u : 256u));
  s.window_lds = (size_t)(win_env > 0 ? win_env : (s.threads == 1024 ? 136 : 64)) * 1024;
  if (s.window_lds > kRbmMaxLds) s.window_lds = kRbmMaxLds;
  return s;
}

// whether all hidden units of q' fit the LDS: the resident form (the only one with the Jastrow factor: pynqs_eloc_jrbm_supported)
static bool rbm_resident(const SDParams &p, const RbmLayout &rl) { return lds_bytes_rbm(p, rl, (uint32_t)rl.Hloop) <= kRbmMaxLds; }

// hidden units resident in LDS: all of them (rl.Hloop) when that fits, else the largest multiple of 8 that keeps the
// workgroup within window_lds (at least 8); 0 if not even that fits
static uint32_t rbm_window(const SDParams &p, const RbmLayout &rl, size_t window_lds) {
  if (rbm_resident(p, rl)) return (uint32_t)rl.Hloop;
  const size_t other = lds_bytes_rbm(p, rl, 0u) - rbm_region_bytes(p, 0u);
  for (uint32_t hw = 256; hw >= 8; hw -= 8)
    if (other + rbm_region_bytes(p, hw) <= (hw > 8 ? window_lds : kRbmMaxLds)) return hw;
  return 0;
}

// JASTROW: the walker's pair factors as a triangle in LDS behind the kernel's own layout (4 sorb (sorb - 1) bytes) as long as three
// workgroups still fit a CU (or as many as fitted without it, if fewer), else read from the table in L2.  Fe2S2: 35 + 6.1 KiB, three
// workgroups per CU instead of four (12 of the 16 waves the registers allow).  PYNQS_JRBM_PAIRS=lds / l2 (read at every call) forces
// one of them where it fits.
static size_t jrbm_pairs_bytes(const SDParams &p) { return 8 * ((size_t)p.sorb * (size_t)(p.sorb - 1) / 2); }
static bool jrbm_pairs_in_lds(const SDParams &p, const RbmLayout &rl) {
  const char *env = getenv("PYNQS_JRBM_PAIRS");
  const size_t base = lds_bytes_rbm(p, rl, (uint32_t)rl.Hloop), with = base + jrbm_pairs_bytes(p);
  if (p.sorb > 128 || with > kRbmMaxLds || (env && !strcmp(env, "l2"))) return false;  // (the kernel has the LDS form for one and two words)
  if (env && !strcmp(env, "lds")) return true;
  const size_t per_cu = 160 * 1024 / (base + 256), per_cu_with = 160 * 1024 / (with + 256);
  return per_cu_with >= (per_cu < 3 ? per_cu : 3);
}

// A launch of eloc_rbm_kernel on nbatch walkers, worked out here and nowhere else: the launcher launches it and the host entries
// (pynqs_eloc_rbm_form, pynqs_eloc_jrbm_form, pynqs_eloc_rbm_geometry) report it.
struct RbmLaunch {
  uint32_t nchunks;   // workgroups per walker (rbm_chunks)
  uint32_t hw;        // hidden units resident in LDS
  bool windowed;      // hw < all of them: the windowed kernel, in rbm_windowed_shape's shape
  bool pairs_in_lds;  // JASTROW: the walker's pair factors behind the kernel's own LDS layout
  size_t lds;         // bytes of dynamic LDS
  uint32_t threads;
  uint64_t grid;
};
// false where the launch is not served: the walker tables leave no LDS for the RBM rows, or, with the Jastrow factor (resident form
// only), sorb x num_hidden is beyond the LDS
static bool rbm_launch_form(const RbmSystem<RbmLayout> &s, int64_t nbatch, bool green, bool jastrow, RbmLaunch *f) {
  const uint32_t ntiles = make_rbm_blocks<kRbmFB>(s.p).ntiles;
  f->nchunks = green ? 1 : rbm_chunks(ntiles, nbatch);  // (the Green's-function row finishes its diagonal in the kernel: one workgroup per walker)
  const RbmShape shape = rbm_windowed_shape(ntiles / f->nchunks);
  f->hw = rbm_window(s.p, s.rl, shape.window_lds);
  f->windowed = !rbm_resident(s.p, s.rl);
  if (f->hw == 0 || (jastrow && f->windowed)) return false;
  f->pairs_in_lds = jastrow && jrbm_pairs_in_lds(s.p, s.rl);
  f->lds = lds_bytes_rbm(s.p, s.rl, f->hw) + (f->pairs_in_lds ? jrbm_pairs_bytes(s.p) : 0);
  // (3-wave workgroups divide Fe2S2's 9 tiles evenly but leave only 12 waves per CU -- LDS allows 4 workgroups --
  // and were 8 % slower at 80 hidden units; the kernel itself runs with any multiple of 64 threads >= 128)
  f->threads = f->windowed ? shape.threads : rbm_resident_threads(f->lds, ntiles / f->nchunks, 1024, rbm_block_env());
  f->grid = (uint64_t)nbatch * f->nchunks;
  return true;
}

// the same from an entry point's arguments; the form as the _form entries report it: bit 0 = windowed, bit 1 = chunked, bit 2 = pairs in LDS
static bool rbm_launch_query(int64_t nbatch, int sorb, int nele, int noA, int noB, int nhidden, bool green, bool jastrow, RbmLaunch *f) {
  RbmSystem<RbmLayout> s;
  return nbatch >= 1 && !rbm_system(sorb, nele, noA, noB, nhidden, make_rbm_layout, &s) && rbm_launch_form(s, nbatch, green, jastrow, f);
}
static int rbm_form_bits(const RbmLaunch &f) { return (f.windowed ? 1 : 0) | (f.nchunks > 1 ? 2 : 0) | (f.pairs_in_lds ? 4 : 0); }

extern "C" int pynqs_eloc_rbm_form(int64_t nbatch, int sorb, int nele, int noA, int noB, int nhidden, int green) {
  RbmLaunch f;
  return rbm_launch_query(nbatch, sorb, nele, noA, noB, nhidden, green != 0, false, &f) ? rbm_form_bits(f) : -1;
}

extern "C" int pynqs_eloc_jrbm_form(int64_t nbatch, int sorb, int nele, int noA, int noB, int nhidden) {
  RbmLaunch f;
  return rbm_launch_query(nbatch, sorb, nele, noA, noB, nhidden, false, true, &f) ? rbm_form_bits(f) : -1;
}

extern "C" int pynqs_eloc_rbm_geometry(int64_t nbatch, int sorb, int nele, int noA, int noB, int nhidden, int green, int jastrow, int64_t *out6) {
  RbmLaunch f;
  if (!out6 || nbatch > 0x7fffffffll || !rbm_launch_query(nbatch, sorb, nele, noA, noB, nhidden, green != 0, jastrow != 0, &f)) return -1;
  out6[0] = (int64_t)f.grid, out6[1] = f.threads, out6[2] = (int64_t)f.lds, out6[3] = f.hw, out6[4] = f.nchunks, out6[5] = f.pairs_in_lds ? 1 : 0;
  return 0;
}

extern "C" int64_t pynqs_rbm_table_bytes(int sorb, int nhidden) {
  RbmLayout rl;
  if (!make_rbm_layout(sorb, nhidden, &rl)) return -1;
  return rl.total * 8;
}

extern "C" int pynqs_eloc_rbm_supported(int sorb, int nele, int noA, int noB, int nhidden) {
  RbmSystem<RbmLayout> s;
  if (rbm_system(sorb, nele, noA, noB, nhidden, make_rbm_layout, &s)) return 0;
  return rbm_window(s.p, s.rl, kRbmMaxLds) > 0 ? 1 : 0;
}

extern "C" int pynqs_rbm_table_build(const double *weights, const double *hidden_bias, const double *visible_bias, int sorb,
                                     int nhidden, void *table, void *stream) {
  pynqs::DeviceScope device_scope_(weights);
  RbmLayout rl;
  if (!make_rbm_layout(sorb, nhidden, &rl)) return set_error(PYNQS_EINVAL, "bad sorb / nhidden");
  if (!weights || !hidden_bias || !table) return set_error(PYNQS_EINVAL, "null pointer");
  const int64_t n = (int64_t)rl.sorb * rl.Hq;
  const uint32_t grid = (uint32_t)((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(rbm_table_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, weights, hidden_bias, visible_bias, rl,
                     (double *)table);
  return check_launch("rbm_table_build");
}

extern "C" int pynqs_eloc_jrbm_supported(int sorb, int nele, int noA, int noB, int nhidden) {  // the resident form only
  RbmSystem<RbmLayout> s;
  if (rbm_system(sorb, nele, noA, noB, nhidden, make_rbm_layout, &s)) return 0;
  return rbm_resident(s.p, s.rl) ? 1 : 0;
}

// ---- the one launcher of eloc_rbm_kernel.  RbmCall: an entry point's pointers and scalars; RbmMode: which amplitude and which sums.
struct RbmCall {  // (in the order of the entry points' own arguments)
  const uint64_t *bra;
  int64_t nbatch;
  int sorb, nele, noA, noB;
  const void *plan, *rbm_table, *jastrow_table;  // jastrow_table: read with kRbmJastrow only
  int nhidden;
  double *eloc, *psi;
  void *stream;
  double lambda = 0.0;  // the row's three, read with kRbmGreen only
  double *green = nullptr;
  uint8_t *clamped = nullptr;
};
enum : unsigned { kRbmSigned = 1, kRbmGreen = 2, kRbmJastrow = 4 };
struct RbmMode {
  int flavour;    // PYNQS_RBM_REAL / _TANH / _PHASE (the kernel's kRbmReal / kRbmTanh / kRbmPhase)
  unsigned what;  // kRbmSigned: every column times sigma_k; kRbmGreen: the fixed-node row; kRbmJastrow: the two-body factor
};

// The 57 instantiations: three word counts x (resident, windowed) x (three flavours plain and SIGNED, two real-valued ones with GREEN),
// and three word counts x (plain, SIGNED, GREEN) with JASTROW (real flavour, resident).  nullptr for every other combination.
using RbmKernel = decltype(&eloc_rbm_kernel<1, false, kRbmReal, false>);
template <int LEN, bool WINDOWED, int FLAVOUR>
static RbmKernel rbm_kernel_of(unsigned what) {
  constexpr bool kCanJastrow = FLAVOUR == kRbmReal && !WINDOWED, kCanGreen = FLAVOUR != kRbmPhase;
  switch (what) {
    case 0: return eloc_rbm_kernel<LEN, WINDOWED, FLAVOUR, false>;
    case kRbmSigned: return eloc_rbm_kernel<LEN, WINDOWED, FLAVOUR, false, false, true>;
    case kRbmGreen: if constexpr (kCanGreen) return eloc_rbm_kernel<LEN, WINDOWED, FLAVOUR, true>; break;
    case kRbmJastrow: if constexpr (kCanJastrow) return eloc_rbm_kernel<LEN, false, kRbmReal, false, true>; break;
    case kRbmJastrow | kRbmSigned: if constexpr (kCanJastrow) return eloc_rbm_kernel<LEN, false, kRbmReal, false, true, true>; break;
    case kRbmJastrow | kRbmGreen: if constexpr (kCanJastrow) return eloc_rbm_kernel<LEN, false, kRbmReal, true, true>; break;
  }
  return nullptr;
}
template <int LEN, bool WINDOWED>
static RbmKernel rbm_kernel_of(const RbmMode &m) {
  return m.flavour == PYNQS_RBM_REAL   ? rbm_kernel_of<LEN, WINDOWED, kRbmReal>(m.what)
         : m.flavour == PYNQS_RBM_TANH ? rbm_kernel_of<LEN, WINDOWED, kRbmTanh>(m.what)
                                       : rbm_kernel_of<LEN, WINDOWED, kRbmPhase>(m.what);
}
static RbmKernel rbm_kernel(int len, bool windowed, const RbmMode &m) {
  DISPATCH_LEN(len, return windowed ? rbm_kernel_of<LEN, true>(m) : rbm_kernel_of<LEN, false>(m));
  return nullptr;
}

static int eloc_rbm_launch(const RbmCall &c, const RbmMode &m) {
  pynqs::DeviceScope device_scope_(c.bra);
  const bool green = m.what & kRbmGreen, jastrow = m.what & kRbmJastrow;
  if (m.flavour < PYNQS_RBM_REAL || m.flavour > PYNQS_RBM_PHASE) return set_error(PYNQS_EINVAL, "unknown RBM flavour");
  if (green && (m.flavour == PYNQS_RBM_PHASE || !c.green || !c.clamped))
    return set_error(PYNQS_EINVAL, "the Green's-function row needs a real-valued flavour, green and clamped");
  RbmSystem<RbmLayout> sys;
  if (const char *bad = rbm_system(c.sorb, c.nele, c.noA, c.noB, c.nhidden, make_rbm_layout, &sys)) return set_error(PYNQS_EINVAL, bad);
  if (const int rc = rbm_batch(c.nbatch, 0x7fffffffll, c.bra, c.plan, c.rbm_table, c.eloc)) return rc;
  if (c.nbatch == 0) return PYNQS_OK;
  if (jastrow && !c.jastrow_table) return set_error(PYNQS_EINVAL, "null pointer");
  RbmLaunch f;
  if (!rbm_launch_form(sys, c.nbatch, green, jastrow, &f))
    return set_error(PYNQS_EINVAL, "eloc_rbm: no LDS for the RBM rows of this system (pynqs_eloc_rbm_supported / pynqs_eloc_jrbm_supported)");
  const RbmKernel kernel = rbm_kernel((c.sorb - 1) / 64 + 1, f.windowed, m);
  if (!kernel) return set_error(PYNQS_EINVAL, "eloc_rbm: no kernel for this flavour and mode");
  hipStream_t st = (hipStream_t)c.stream;
  uint32_t checked;  // (rbm_grid: f.grid within the range of a launch, and eloc cleared for a chunked one)
  if (const int rc = rbm_grid(c.nbatch, f.nchunks, c.eloc, m.flavour == PYNQS_RBM_PHASE ? 16 : 8, st, &checked)) return rc;
  const auto &[p, pl, rl] = sys;
  return rbm_launch("eloc_rbm", kernel, (uint32_t)f.grid, f.threads, f.lds, st, c.bra, p, pl, rl, make_rbm_blocks<kRbmFB>(p), f.nchunks, f.hw,
                    (const double *)c.plan, (const double *)c.rbm_table, c.eloc, c.psi, green ? c.lambda : 0.0, green ? c.green : nullptr,
                    green ? c.clamped : nullptr, jastrow ? (const double *)c.jastrow_table : nullptr, f.pairs_in_lds);
}

extern "C" int pynqs_eloc_rbm_flavour(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                                      const void *rbm_table, int nhidden, int flavour, double *eloc, double *psi, void *stream) {
  return eloc_rbm_launch({bra, nbatch, sorb, nele, noA, noB, plan, rbm_table, nullptr, nhidden, eloc, psi, stream}, {flavour, 0});
}

extern "C" int pynqs_eloc_rbm(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                              const void *rbm_table, int nhidden, double *eloc, double *psi, void *stream) {
  return eloc_rbm_launch({bra, nbatch, sorb, nele, noA, noB, plan, rbm_table, nullptr, nhidden, eloc, psi, stream}, {PYNQS_RBM_REAL, 0});
}

extern "C" int pynqs_eloc_rbm_signed(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                                     const void *rbm_table, int nhidden, int flavour, double *eloc, double *psi, void *stream) {
  return eloc_rbm_launch({bra, nbatch, sorb, nele, noA, noB, plan, rbm_table, nullptr, nhidden, eloc, psi, stream}, {flavour, kRbmSigned});
}

extern "C" int pynqs_green_rbm(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                               const void *rbm_table, int nhidden, int flavour, double lambda, double *eloc, double *psi, double *green,
                               uint8_t *clamped, void *stream) {
  return eloc_rbm_launch({bra, nbatch, sorb, nele, noA, noB, plan, rbm_table, nullptr, nhidden, eloc, psi, stream, lambda, green, clamped},
                         {flavour, kRbmGreen});
}

// ---- the same with the two-body Jastrow factor exp(x^T M x) on the real RBM (JASTROW): the resident form only; the LDS (plus the
// walker's triangle), the cut into chunks and the workgroup size are those of pynqs_eloc_rbm
extern "C" int pynqs_eloc_jrbm(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                               const void *rbm_table, const void *jastrow_table, int nhidden, double *eloc, double *psi, void *stream) {
  return eloc_rbm_launch({bra, nbatch, sorb, nele, noA, noB, plan, rbm_table, jastrow_table, nhidden, eloc, psi, stream}, {PYNQS_RBM_REAL, kRbmJastrow});
}

extern "C" int pynqs_eloc_jrbm_signed(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                                      const void *rbm_table, const void *jastrow_table, int nhidden, double *eloc, double *psi, void *stream) {
  return eloc_rbm_launch({bra, nbatch, sorb, nele, noA, noB, plan, rbm_table, jastrow_table, nhidden, eloc, psi, stream},
                         {PYNQS_RBM_REAL, kRbmJastrow | kRbmSigned});
}

// The fixed-node Green's row with the Jastrow factor (GREEN and JASTROW): pynqs_green_rbm's row for pynqs_eloc_jrbm's amplitude, one
// workgroup per walker.  A missing table and a system that is not served are refused for an empty batch too, which the launcher
// (empty batch: PYNQS_OK before it looks at the form) does not do: hence the check here, by the launcher's own rule (rbm_resident).
extern "C" int pynqs_green_jrbm(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                                const void *rbm_table, const void *jastrow_table, int nhidden, double lambda, double *eloc, double *psi,
                                double *green, uint8_t *clamped, void *stream) {
  if (!jastrow_table || !pynqs_eloc_jrbm_supported(sorb, nele, noA, noB, nhidden))
    return set_error(PYNQS_EINVAL, "green_jrbm: null pointer, or sorb x nhidden beyond the LDS (pynqs_eloc_jrbm_supported)");
  return eloc_rbm_launch({bra, nbatch, sorb, nele, noA, noB, plan, rbm_table, jastrow_table, nhidden, eloc, psi, stream, lambda, green, clamped},
                         {PYNQS_RBM_REAL, kRbmJastrow | kRbmGreen});
}

// ---- the spin-flip-projected local energy (vmc/energy/flip.py, _simple_flip; formula and mirrored-table convention: include/pynqs_amd.h):
//   E_proj = [E + eta eta_m(x) R Em] / extra_norm^2,  E: the plain pass, Em: the SIGNED pass on the mirrored table, R = psim(x) / psi(x).
// One thread per walker; eloc holds E on entry and E_proj on return.  PHASE: (re, im) pairs, R and the product in complex arithmetic.
namespace pynqs {
template <bool PHASE>
__global__ __launch_bounds__(kBlock) void flip_combine_kernel(const uint64_t *__restrict__ bra, int64_t n, int len, double eta, double extra_norm,
                                                              const double *__restrict__ extra_norm_dev, const double *__restrict__ psi,
                                                              const double *__restrict__ em, const double *__restrict__ psim,
                                                              double *__restrict__ eloc) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t docc = 0;  // doubly occupied spatial orbitals: bits 2k and 2k + 1 of a word
  for (int w = 0; w < len; ++w) {
    const uint64_t v = bra[i * len + w];
    docc += (uint32_t)__popcll(v & (v >> 1) & 0x5555555555555555ull);
  }
  const double nrm = extra_norm_dev ? *extra_norm_dev : extra_norm;
  const double c = (docc & 1u) ? -eta : eta, n2 = nrm * nrm;
  if constexpr (PHASE) {
    const double pr = psi[2 * i], pi = psi[2 * i + 1], qr = psim[2 * i], qi = psim[2 * i + 1], d = pr * pr + pi * pi;
    const double rr = (qr * pr + qi * pi) / d, ri = (qi * pr - qr * pi) / d;  // R = psim conj(psi) / |psi|^2
    const double er = em[2 * i], ei = em[2 * i + 1];
    eloc[2 * i] = (eloc[2 * i] + c * (rr * er - ri * ei)) / n2;
    eloc[2 * i + 1] = (eloc[2 * i + 1] + c * (rr * ei + ri * er)) / n2;
  } else {
    eloc[i] = (eloc[i] + c * ((psim[i] / psi[i]) * em[i])) / n2;
  }
}
}  // namespace pynqs

static int flip_combine(const uint64_t *bra, int64_t nbatch, int sorb, bool phase, double eta, double extra_norm, const double *extra_norm_dev,
                        const double *psi, const double *work, double *eloc, void *stream) {
  const int len = (sorb - 1) / 64 + 1;
  const int64_t k = phase ? 2 : 1;
  const uint32_t grid = (uint32_t)((nbatch + kBlock - 1) / kBlock);
  hipLaunchKernelGGL((phase ? flip_combine_kernel<true> : flip_combine_kernel<false>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, bra, nbatch,
                     len, eta, extra_norm, extra_norm_dev, psi, work, work + k * nbatch, eloc);
  return check_launch("flip_combine");
}

// both flip entries: the plain pass, the SIGNED pass on the mirrored tables into work (Em, behind it psim), then the combine
static int eloc_flip(const RbmCall &c, RbmMode m, const void *rbm_table_mirror, const void *jastrow_table_mirror, double eta, double extra_norm,
                     const double *extra_norm_dev, double *work) {
  const bool jastrow = m.what & kRbmJastrow;
  if (c.nbatch > 0 && (!rbm_table_mirror || (jastrow && !jastrow_table_mirror) || !c.psi || !work)) return set_error(PYNQS_EINVAL, "null pointer");
  if (int rc = eloc_rbm_launch(c, m)) return rc;
  if (c.nbatch == 0) return PYNQS_OK;
  const int64_t k = m.flavour == PYNQS_RBM_PHASE ? 2 : 1;
  RbmCall mirror = c;
  mirror.rbm_table = rbm_table_mirror, mirror.jastrow_table = jastrow_table_mirror, mirror.eloc = work, mirror.psi = work + k * c.nbatch;
  m.what |= kRbmSigned;
  if (int rc = eloc_rbm_launch(mirror, m)) return rc;
  pynqs::DeviceScope device_scope_(c.bra);
  return flip_combine(c.bra, c.nbatch, c.sorb, k == 2, eta, extra_norm, extra_norm_dev, c.psi, work, c.eloc, c.stream);
}

extern "C" int pynqs_eloc_rbm_flip_supported(int sorb, int nele, int noA, int noB, int nhidden) {
  return pynqs_eloc_rbm_supported(sorb, nele, noA, noB, nhidden);
}

extern "C" int pynqs_eloc_rbm_flip_form(int64_t nbatch, int sorb, int nele, int noA, int noB, int nhidden) {
  return pynqs_eloc_rbm_form(nbatch, sorb, nele, noA, noB, nhidden, 0);
}

extern "C" int pynqs_eloc_rbm_flip(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                                   const void *rbm_table, const void *rbm_table_mirror, int nhidden, int flavour, double eta, double extra_norm,
                                   const double *extra_norm_dev, double *eloc, double *psi, double *work, void *stream) {
  return eloc_flip({bra, nbatch, sorb, nele, noA, noB, plan, rbm_table, nullptr, nhidden, eloc, psi, stream}, {flavour, 0}, rbm_table_mirror, nullptr,
                   eta, extra_norm, extra_norm_dev, work);
}

extern "C" int pynqs_eloc_jrbm_flip_supported(int sorb, int nele, int noA, int noB, int nhidden) {
  return pynqs_eloc_jrbm_supported(sorb, nele, noA, noB, nhidden);
}

extern "C" int pynqs_eloc_jrbm_flip_form(int64_t nbatch, int sorb, int nele, int noA, int noB, int nhidden) {
  return pynqs_eloc_jrbm_form(nbatch, sorb, nele, noA, noB, nhidden);
}

extern "C" int pynqs_eloc_jrbm_flip(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                                    const void *rbm_table, const void *jastrow_table, const void *rbm_table_mirror,
                                    const void *jastrow_table_mirror, int nhidden, double eta, double extra_norm, const double *extra_norm_dev,
                                    double *eloc, double *psi, double *work, void *stream) {
  return eloc_flip({bra, nbatch, sorb, nele, noA, noB, plan, rbm_table, jastrow_table, nhidden, eloc, psi, stream}, {PYNQS_RBM_REAL, kRbmJastrow},
                   rbm_table_mirror, jastrow_table_mirror, eta, extra_norm, extra_norm_dev, work);
}
