// kernels_mcmc.hip -- many-chain Metropolis sampling (PyNQS' Sampler.MCMC, vmc/sample.py:480-569, one chain in a Python loop there):
//   pynqs_mcmc_rbm    : the fused kernel for RBM amplitudes; every chain runs `nsteps` steps inside one launch
//   pynqs_mcmc_jrbm   : the same for the real RBM times the Jastrow factor exp(x^T M x) (pynqs_amd.rbm.JastrowRBM; JAS of mcmc_rbm_kernel)
//   pynqs_mcmc_accept : one accept / reject step of any ansatz, from proposals of pynqs_spin_flip_rand and their psi
// All follow the rule written out in include/pynqs_amd.h; with equal psi they make the same decisions (the fused kernel's ratio is
// exp(2 (ln|psi'| - ln|psi|)), the generic one |psi'|^2 / |psi|^2: equal to rounding).
//
// The fused kernel.  G lanes (a power of two, G * kMcmcSlots >= H) own one chain; lane g holds the hidden units h = g + G j, j < 8, as
//   theta_h (complex: re, im)  and  q_h = exp(-2 s_h theta_h),  s_h = sign(Re theta_h),  |q_h| = exp(-2 |Re theta_h|) <= 1,
// so that 2cosh(theta_h) = exp(s_h theta_h) (1 + q_h) and  ln|psi| = Re a.x + sum_h (|Re theta_h| + ln|1 + q_h|)  (tanh: ln|tanh a.x|
// instead of a.x).  A move flips orbitals F (2 or 4): theta'_h = theta_h + sum_{o in F} 2 x'_o W_ho and
//   q'_h = q_h prod_{o in F} exp(-4 s_h x'_o W_ho)            (the table's E4m / E4p entries: no exponential),
//   if the sign of Re theta_h changed (decided on theta, which is tracked too):  q'_h <- 1 / q'_h  (= exp(-2 s'_h theta'_h) again; deciding
//   on |q'_h| > 1 instead would let rounding flip the branch where Re theta_h = 0 exactly, as for rbm_type "cos"),
//   if |q'_h| < 1e-290 (|Re theta'_h| > ~333): q'_h from theta'_h by exp (+ sincos), flushed to 0 below 1e-290: the product would sink
//   into the subnormals and lose its digits; and if |q'_h| > 1 (the product of a flushed q_h = 0 after a sign change is 1 / 0 = inf;
//   otherwise only rounding at Re theta'_h ~ 0, or exp(+-4 W) overflowed in the table),
// and ln|psi'| - ln|psi| = Re a.(x' - x) + sum_h (|Re theta'_h| - |Re theta_h|) + ln prod_h |1 + q'_h| / |1 + q_h| -- per lane a product of
// at most 8 ratios in [1/2, 2] (real) and one logarithm, then a butterfly over the G lanes.  No quantity leaves the range of a double for
// any |Re theta_h| (the state is never exp(+-theta)).  The state is recomputed from the parameters at the start of every launch
// (theta = b + W x, sorb fma per hidden unit), so that the rounding of the updates cannot drift over a run.
// tanh keeps the hidden part sum_h ln|2cosh theta_h| (always finite) apart from ln|tanh a.x| (-inf where a.x = 0) and forms ln|psi| of an
// accepted state from the two, so that leaving a state of amplitude zero gives the new state's own ln|psi| (not -inf + inf).
// The parameter table is copied into LDS when it fits 64 KB (Fe2S2 with 40 real hidden units: 39 KB), else read from the L2.
// The proposal is computed by every lane of the group (the same hash, the same excite_by_rank), so the group needs no exchange for it;
// the butterfly leaves the same sum in every lane (each stage adds the same two numbers), so the lanes take the same decision.
#include "detcore.h"
#include "launch.h"
#include "mix64.h"
#include "rbm.h"
#include "rbm_math.h"

namespace pynqs {

constexpr int kMcmcSlots = 8;      // hidden units per lane
constexpr int kMcmcMaxGroup = 64;  // lanes per chain at most: nhidden <= 512
constexpr double kMcmcTiny = 1e-290;

__device__ __forceinline__ uint32_t mcmc_r0(uint64_t seed, uint64_t t, uint64_t c, uint32_t nsd) {
  const uint64_t h = mix64(mix64(seed) ^ mix64((t << 32) + c));  // = pynqs_spin_flip_rand's draw (offset (t << 32) + chain_base)
  return (uint32_t)__umul64hi(h, (uint64_t)nsd + 1);
}

__device__ __forceinline__ double mcmc_uniform(uint64_t seed, uint64_t t, uint64_t c) {
  const uint64_t h = mix64(mix64(seed ^ PYNQS_MCMC_ACCEPT_KEY) ^ mix64((t << 32) + c));
  return ((double)(h >> 11) + 0.5) * 0x1p-53;
}

__device__ __forceinline__ double group_sum(double v, int G) {
  for (int d = 1; d < G; d <<= 1) v += __shfl_xor(v, d);
  return v;
}

// ln|2cosh theta| from (|Re theta|, q)
template <bool CPLX>
__device__ __forceinline__ double lncosh_of(double ar, double qr, double qi) {
  if constexpr (CPLX) return ar + 0.5 * log(fma(qi, qi, (1.0 + qr) * (1.0 + qr)));
  else return ar + log1p(qr);
}

// q = exp(-2 s theta) from theta directly, s = sign(Re theta); 0 where |q| < kMcmcTiny (no digits are lost to the subnormals)
template <bool CPLX>
__device__ __forceinline__ void q_of(double tr, double ti, double &qr, double &qi) {
  double m = exp(-2.0 * fabs(tr));
  m = m >= kMcmcTiny ? m : 0.0;
  if constexpr (CPLX) {
    double sn, cs;
    sincos_mod(-2.0 * (tr < 0.0 ? -ti : ti), sn, cs);
    qr = m * cs; qi = m * sn;
  } else {
    qr = m; qi = 0.0;
  }
}

struct McmcTable {
  const double *tab;
  int H, stride;                              // row stride in elements (real: doubles, complex: (re, im) pairs)
  int64_t offWt, offE4p, offE4m, offHb, offVb;  // in elements
  int64_t total;                              // table size in doubles
  const double *jas;                          // the Jastrow table (pynqs_mcmc_jrbm only)
};

constexpr int64_t kMcmcLdsBytes = 64 * 1024;

// where the chain kernel reads S, the first block of the Jastrow table (rbm.h): no Jastrow factor; from the table in the L2; from LDS,
// behind the RBM table (both within kMcmcLdsBytes)
constexpr int kJasNone = 0, kJasL2 = 1, kJasLds = 2;

// JAS != kJasNone: the real flavour times the Jastrow factor exp(x^T M x) (pynqs_mcmc_jrbm; T.jas = the Jastrow table).  Every Jastrow
// statement is under if constexpr, so the instantiations without it compile to what they were.  With S = M + M^T without its diagonal,
//   ln|psi_J(x)| = tr M + sum_{i<j} S_ij x_i x_j   (at the start of a launch: lane g sums the rows i = g (mod G), the butterfly that
//                                                   sums the hidden units' ln 2cosh sums these shares too)
//   ln|psi_J(x')| - ln|psi_J(x)| = -2 sum_{i in F} x_i r_i + 4 sum_{i<j in F} S_ij x_i x_j,   r_i = sum_j S_ij x_j,
// r_i formed at every step from the state before the move: lane g sums the orbitals j = g (mod G) of the <= 4 rows and adds its share
// to the value it hands the hidden units' butterfly (no second butterfly; every lane ends with the same bits); the pair term (<= 6
// products) is added by every lane after it.  Nothing of the Jastrow factor is carried from step to step but ln|psi| itself.
template <int LEN, int FLAVOUR, bool IN_LDS, int JAS = kJasNone>
__global__ __launch_bounds__(kBlock) void mcmc_rbm_kernel(uint64_t *__restrict__ states, int64_t nchains, SDParams p, McmcTable T, int G,
                                                          uint64_t seed, uint64_t chain_base, uint64_t t0, int nsteps, int every,
                                                          uint64_t *__restrict__ rec, int64_t *__restrict__ nacc, double *__restrict__ lnpsi_out) {
  static_assert(JAS == kJasNone || FLAVOUR == PYNQS_RBM_REAL, "the Jastrow factor multiplies the real flavour only");
  static_assert(JAS != kJasLds || IN_LDS, "S joins the RBM table in LDS, never alone");
  constexpr bool CPLX = FLAVOUR == PYNQS_RBM_COMPLEX;
  constexpr bool HIDDEN = FLAVOUR != PYNQS_RBM_PHASE;  // (pRBM: |psi| = 1, every proposal is accepted)
  constexpr int C = CPLX ? 2 : 1;
  constexpr int J = kMcmcSlots;
  extern __shared__ __attribute__((aligned(16))) double lds_tab[];
  if constexpr (IN_LDS) {
    for (int64_t k = threadIdx.x; k < T.total; k += kBlock) lds_tab[k] = T.tab[k];
    if constexpr (JAS == kJasLds)
      for (int64_t k = threadIdx.x; k < jastrow_pairs(p.sorb); k += kBlock) lds_tab[T.total + k] = T.jas[k];
    __syncthreads();
  }
  const double *__restrict__ tab = IN_LDS ? lds_tab : T.tab;
  const double *__restrict__ S = JAS == kJasLds ? lds_tab + T.total : T.jas;  // [sorb][sorb] (JAS != kJasNone)
  const int64_t gt = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t i = gt / G;
  const int g = (int)(gt - i * G);
  if (i >= nchains) return;  // (whole groups: G divides kBlock)
  const uint64_t c = chain_base + (uint64_t)i;
  const int sorb = p.sorb, H = T.H;
  uint64_t x[LEN];
#pragma unroll
  for (int w = 0; w < LEN; ++w) x[w] = states[i * LEN + w];

  // ---- the chain's state from scratch
  double thr[J], thi[J], qr[J], qi[J];
  double ax = 0.0, lnh = 0.0, lnpsi = 0.0;  // lnh: the hidden part of ln|psi| (tanh only)
  if constexpr (HIDDEN) {
    double part = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int h = g + G * j;
      thr[j] = thi[j] = qr[j] = qi[j] = 0.0;
      if (h < H) {
        double tr = tab[(T.offHb + h) * C], ti = CPLX ? tab[(T.offHb + h) * C + 1] : 0.0;
        for (int o = 0; o < sorb; ++o) {
          const double xo = pm1_of<LEN>(x, o);
          const int64_t e = (T.offWt + (int64_t)o * T.stride + h) * C;
          tr = fma(xo, tab[e], tr);
          if constexpr (CPLX) ti = fma(xo, tab[e + 1], ti);
        }
        thr[j] = tr; thi[j] = ti;
        q_of<CPLX>(tr, ti, qr[j], qi[j]);
        part += lncosh_of<CPLX>(fabs(tr), qr[j], qi[j]);
      }
    }
    for (int o = 0; o < sorb; ++o) ax = fma(pm1_of<LEN>(x, o), tab[(T.offVb + o) * C], ax);
    if constexpr (JAS != kJasNone) {
      for (int a = g; a < sorb; a += G) {
        double r = 0.0;
        for (int b = a + 1; b < sorb; ++b) r = fma(S[a * sorb + b], pm1_of<LEN>(x, b), r);
        part = fma(pm1_of<LEN>(x, a), r, part);
      }
    }
    lnh = group_sum(part, G);
    lnpsi = lnh + (FLAVOUR == PYNQS_RBM_TANH ? log(fabs(tanh(ax))) : ax);
    if constexpr (JAS != kJasNone) lnpsi += T.jas[3 * jastrow_pairs(sorb)];  // tr M (JastrowLayout::offTr)
  }

  int64_t accepted = 0;
  for (int k = 0; k < nsteps; ++k) {
    const uint64_t t = t0 + (uint64_t)k;
    uint64_t xn[LEN];
#pragma unroll
    for (int w = 0; w < LEN; ++w) xn[w] = x[w];
    const uint32_t r0 = mcmc_r0(seed, t, c, p.nsd);
    if (r0 != 0) excite_by_rank<LEN>(xn, r0 - 1, p);
    bool accept = true;
    if constexpr (HIDDEN) {
      // the flipped orbitals and their new values (at most 4; unused slots have sign 0 and contribute nothing)
      int fo[4] = {0, 0, 0, 0};
      double fs[4] = {0.0, 0.0, 0.0, 0.0};
      int nf = 0;
#pragma unroll
      for (int w = 0; w < LEN; ++w) {
        uint64_t d = x[w] ^ xn[w];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (d && nf < 4) {
            const int b = __builtin_ctzll(d);
            d &= d - 1;
            const int o = 64 * w + b;
            const double s = ((xn[w] >> b) & 1ull) ? 1.0 : -1.0;
#pragma unroll
            for (int f = 0; f < 4; ++f)  // (selected, not indexed: the arrays stay in registers)
              if (f == nf) { fo[f] = o; fs[f] = s; }
            ++nf;
          }
        }
      }
      double nthr[J], nthi[J], nqr[J], nqi[J];
      double lsum = 0.0, pn = 1.0, po = 1.0;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int h = g + G * j;
        nthr[j] = thr[j]; nthi[j] = thi[j]; nqr[j] = qr[j]; nqi[j] = qi[j];
        if (h < H) {
          const double sh = thr[j] < 0.0 ? -1.0 : 1.0;
          double dr = 0.0, di = 0.0, fr = 1.0, fi = 0.0;
#pragma unroll
          for (int f = 0; f < 4; ++f) {
            if (f < nf) {
              const int64_t e = (int64_t)fo[f] * T.stride + h;
              const int64_t ew = (T.offWt + e) * C, ee = ((sh * fs[f] > 0.0 ? T.offE4m : T.offE4p) + e) * C;
              dr = fma(2.0 * fs[f], tab[ew], dr);
              if constexpr (CPLX) {
                di = fma(2.0 * fs[f], tab[ew + 1], di);
                const double er = tab[ee], ei = tab[ee + 1];
                const double nr = fma(-fi, ei, fr * er);
                fi = fma(fr, ei, fi * er);
                fr = nr;
              } else {
                fr *= tab[ee];
              }
            }
          }
          const double tr = thr[j] + dr, ti = thi[j] + di;
          double ur, ui;
          if constexpr (CPLX) {
            ur = fma(-qi[j], fi, qr[j] * fr);
            ui = fma(qr[j], fi, qi[j] * fr);
            const double n2 = fma(ui, ui, ur * ur);
            if ((tr < 0.0) != (thr[j] < 0.0)) { ur = ur / n2; ui = -ui / n2; }  // 1 / q
          } else {
            ui = 0.0;
            ur = qr[j] * fr;
            // (after a sign change |q fr| >= 1, so without this inverse the |q'| <= 1 test below would recompute q' by exp: dropping
            //  it changes only the speed, and only the complex inverse above is load-bearing)
            if ((tr < 0.0) != (thr[j] < 0.0)) ur = 1.0 / ur;
          }
          const double mq = fmax(fabs(ur), fabs(ui));
          if (!(mq >= kMcmcTiny && mq <= 1.0)) q_of<CPLX>(tr, ti, ur, ui);
          lsum += fabs(tr) - fabs(thr[j]);
          if constexpr (CPLX) {
            pn *= fma(ui, ui, (1.0 + ur) * (1.0 + ur));
            po *= fma(qi[j], qi[j], (1.0 + qr[j]) * (1.0 + qr[j]));
          } else {
            pn *= 1.0 + ur;
            po *= 1.0 + qr[j];
          }
          nthr[j] = tr; nthi[j] = ti; nqr[j] = ur; nqi[j] = ui;
        }
      }
      double share = fma(CPLX ? 0.5 : 1.0, log(pn / po), lsum);
      if constexpr (JAS != kJasNone) {
        // -2 sum_{i in F} x_i r_i = sum_f 2 fs[f] r_f (fs is the NEW value -x_i), this lane's orbitals of r_f
        double r[4] = {0.0, 0.0, 0.0, 0.0};
        for (int b = g; b < sorb; b += G) {
          const double xb = pm1_of<LEN>(x, b);
#pragma unroll
          for (int f = 0; f < 4; ++f)
            if (f < nf) r[f] = fma(S[fo[f] * sorb + b], xb, r[f]);
        }
        double jl = 0.0;
#pragma unroll
        for (int f = 0; f < 4; ++f) jl = fma(2.0 * fs[f], r[f], jl);
        share += jl;
      }
      const double dh = group_sum(share, G);
      double dax = 0.0;
#pragma unroll
      for (int f = 0; f < 4; ++f)
        if (f < nf) dax = fma(2.0 * fs[f], tab[(T.offVb + fo[f]) * C], dax);
      const double axn = ax + dax;
      const double lvn = FLAVOUR == PYNQS_RBM_TANH ? log(fabs(tanh(axn))) : 0.0;  // (-inf: x' has amplitude zero)
      double dl = dh + (FLAVOUR == PYNQS_RBM_TANH ? lvn - log(fabs(tanh(ax))) : dax);
      if constexpr (JAS != kJasNone) {
        // + 4 sum_{i<j in F} S_ij x_i x_j (x_i x_j = fs_i fs_j); the same loads and products in every lane of the group
        double pr = 0.0;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
#pragma unroll
          for (int f2 = f + 1; f2 < 4; ++f2)
            if (f2 < nf) pr = fma(fs[f] * fs[f2], S[fo[f] * sorb + fo[f2]], pr);
        }
        dl = fma(4.0, pr, dl);
      }
      // u <= |psi'|^2 / |psi|^2, and every proposal from a state of amplitude zero (then dl is +inf or nan)
      accept = !(lnpsi > -INFINITY) || mcmc_uniform(seed, t, c) <= exp(2.0 * dl);
      if (accept) {
#pragma unroll
        for (int j = 0; j < J; ++j) { thr[j] = nthr[j]; thi[j] = nthi[j]; qr[j] = nqr[j]; qi[j] = nqi[j]; }
        ax = axn;
        if constexpr (FLAVOUR == PYNQS_RBM_TANH) {
          lnh += dh;
          lnpsi = lnh + lvn;
        } else {
          lnpsi += dl;
        }
      }
    }
    if (accept) {
#pragma unroll
      for (int w = 0; w < LEN; ++w) x[w] = xn[w];
      ++accepted;
    }
    if (rec && (k + 1) % every == 0) {
      uint64_t *r = rec + ((int64_t)((k + 1) / every - 1) * nchains + i) * LEN;
#pragma unroll
      for (int w = 0; w < LEN; ++w)
        if (g == w % G) r[w] = x[w];
    }
  }
  if (g != 0) return;
#pragma unroll
  for (int w = 0; w < LEN; ++w) states[i * LEN + w] = x[w];
  if (nacc) nacc[i] += accepted;
  if (lnpsi_out) lnpsi_out[i] = lnpsi;
}

// the generic step: psi given by the caller (any ansatz), the proposals by pynqs_spin_flip_rand at the same (seed, t, chain_base)
template <int LEN, bool CPLX>
__global__ __launch_bounds__(kBlock) void mcmc_accept_kernel(uint64_t *__restrict__ states, double *__restrict__ psi,
                                                             const uint64_t *__restrict__ prop, const double *__restrict__ psi_prop, int64_t n,
                                                             uint64_t seed, uint64_t chain_base, uint64_t t, uint64_t *__restrict__ rec,
                                                             int64_t *__restrict__ nacc) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  constexpr int C = CPLX ? 2 : 1;
  double pr = psi_prop[i * C], pi = CPLX ? psi_prop[i * C + 1] : 0.0;
  double cr = psi[i * C], ci = CPLX ? psi[i * C + 1] : 0.0;
  // |psi'|^2 / |psi|^2 with both amplitudes scaled by the same power of two (exact; the larger part of psi to [1/2, 1)), so that no square
  // under- or overflows where it could decide (the squares of the unscaled values give 0 / 0 below ~1e-162, inf / inf above ~1e154);
  // non-finite amplitudes as include/pynqs_amd.h says
  bool accept;
  if (!(isfinite(pr) && isfinite(pi))) {
    accept = false;
  } else if (!(isfinite(cr) && isfinite(ci)) || (cr == 0.0 && ci == 0.0)) {
    accept = true;
  } else {
    int e;
    frexp(fmax(fabs(cr), fabs(ci)), &e);
    pr = ldexp(pr, -e); pi = ldexp(pi, -e); cr = ldexp(cr, -e); ci = ldexp(ci, -e);
    const double a = CPLX ? pr * pr + pi * pi : pr * pr, b = CPLX ? cr * cr + ci * ci : cr * cr;
    accept = mcmc_uniform(seed, t, chain_base + (uint64_t)i) <= a / b;
  }
  uint64_t x[LEN];
#pragma unroll
  for (int w = 0; w < LEN; ++w) x[w] = accept ? prop[i * LEN + w] : states[i * LEN + w];
  if (accept) {
#pragma unroll
    for (int w = 0; w < LEN; ++w) states[i * LEN + w] = x[w];
    psi[i * C] = psi_prop[i * C];
    if (CPLX) psi[i * C + 1] = psi_prop[i * C + 1];
    if (nacc) nacc[i] += 1;
  }
  if (rec) {
#pragma unroll
    for (int w = 0; w < LEN; ++w) rec[i * LEN + w] = x[w];
  }
}

// lanes per chain for nhidden hidden units (0: unsupported)
static int mcmc_group(int nhidden) {
  int G = 1;
  while (G * kMcmcSlots < nhidden) G *= 2;
  return G <= kMcmcMaxGroup ? G : 0;
}

}  // namespace pynqs

using namespace pynqs;

extern "C" int pynqs_mcmc_rbm_supported(int sorb, int nhidden, int flavour) {
  if (sorb < 1 || sorb > kMaxSorb || nhidden < 1 || mcmc_group(nhidden) == 0) return 0;
  if (flavour == PYNQS_RBM_COMPLEX) {
    CrbmLayout cl;
    return make_crbm_layout(sorb, nhidden, &cl) ? 1 : 0;
  }
  RbmLayout rl;
  return (flavour == PYNQS_RBM_REAL || flavour == PYNQS_RBM_TANH || flavour == PYNQS_RBM_PHASE) && make_rbm_layout(sorb, nhidden, &rl) ? 1 : 0;
}

extern "C" int pynqs_mcmc_rbm(uint64_t *states, int64_t nchains, int sorb, int noA, int noB, const void *table, int nhidden, int flavour,
                              uint64_t seed, uint64_t chain_base, uint64_t t0, int nsteps, int every, uint64_t *records, int64_t *n_accept,
                              double *lnpsi, void *stream) {
  pynqs::DeviceScope device_scope_(states);
  SDParams p;
  if (!make_sd_params(sorb, noA + noB, noA, noB, &p)) return set_error(PYNQS_EINVAL, "mcmc_rbm: bad sorb/noA/noB");
  if (!pynqs_mcmc_rbm_supported(sorb, nhidden, flavour)) return set_error(PYNQS_EINVAL, "mcmc_rbm: unsupported flavour / nhidden / sorb");
  if (nchains < 0 || nsteps < 0 || every < 1) return set_error(PYNQS_EINVAL, "mcmc_rbm: bad nchains/nsteps/every");
  if (chain_base + (uint64_t)nchains > (1ull << 32)) return set_error(PYNQS_EINVAL, "mcmc_rbm: chain indices must stay below 2^32");
  if (nchains == 0) return PYNQS_OK;
  if (!states || !table) return set_error(PYNQS_EINVAL, "null pointer");
  McmcTable T;
  T.tab = (const double *)table;
  T.jas = nullptr;
  T.H = nhidden;
  if (flavour == PYNQS_RBM_COMPLEX) {
    CrbmLayout cl;
    make_crbm_layout(sorb, nhidden, &cl);
    T.stride = cl.Hs; T.offWt = cl.offWt; T.offE4p = cl.offE4p; T.offE4m = cl.offE4m; T.offHb = cl.offHb; T.offVb = cl.offVb;
    T.total = 2 * cl.total;
  } else {
    RbmLayout rl;
    make_rbm_layout(sorb, nhidden, &rl);
    T.stride = rl.Hq; T.offWt = rl.offWt; T.offE4p = rl.offE4p; T.offE4m = rl.offE4m; T.offHb = rl.offHb; T.offVb = rl.offVb;
    T.total = rl.total;
  }
  const int G = mcmc_group(nhidden);
  const uint64_t grid = ((uint64_t)nchains * G + kBlock - 1) / kBlock;
  if (grid > 0x7fffffffull) return set_error(PYNQS_EINVAL, "nchains too large for one launch");
  const int len = (sorb - 1) / 64 + 1;
  hipStream_t st = (hipStream_t)stream;
  const bool in_lds = flavour != PYNQS_RBM_PHASE && T.total * 8 <= kMcmcLdsBytes;  // (pRBM reads no table)
  const size_t lds = in_lds ? (size_t)T.total * 8 : 0;
#define PYNQS_MC(F)                                                                                                                     \
  do {                                                                                                                                  \
    if (in_lds)                                                                                                                         \
      hipLaunchKernelGGL((mcmc_rbm_kernel<LEN, F, true>), dim3((uint32_t)grid), dim3(kBlock), lds, st, states, nchains, p, T, G, seed,   \
                         chain_base, t0, nsteps, every, records, n_accept, lnpsi);                                                      \
    else                                                                                                                                \
      hipLaunchKernelGGL((mcmc_rbm_kernel<LEN, F, false>), dim3((uint32_t)grid), dim3(kBlock), 0, st, states, nchains, p, T, G, seed,   \
                         chain_base, t0, nsteps, every, records, n_accept, lnpsi);                                                      \
  } while (0)
  DISPATCH_LEN(len, {
    switch (flavour) {
      case PYNQS_RBM_REAL: PYNQS_MC(PYNQS_RBM_REAL); break;
      case PYNQS_RBM_TANH: PYNQS_MC(PYNQS_RBM_TANH); break;
      case PYNQS_RBM_PHASE: PYNQS_MC(PYNQS_RBM_PHASE); break;
      default: PYNQS_MC(PYNQS_RBM_COMPLEX); break;
    }
  });
#undef PYNQS_MC
  return check_launch("mcmc_rbm");
}

// bit 0: the RBM table in LDS, bit 1: S too (both within kMcmcLdsBytes); the shape alone decides
static int mcmc_jrbm_form(int sorb, const RbmLayout &rl) {
  if (rl.total * 8 > kMcmcLdsBytes) return 0;
  return (rl.total + jastrow_pairs(sorb)) * 8 <= kMcmcLdsBytes ? 3 : 1;
}

extern "C" int pynqs_mcmc_jrbm_supported(int sorb, int nhidden) {
  JastrowLayout jl;
  return pynqs_mcmc_rbm_supported(sorb, nhidden, PYNQS_RBM_REAL) && make_jastrow_layout(sorb, &jl) ? 1 : 0;
}

extern "C" int pynqs_mcmc_jrbm_form(int sorb, int nhidden) {
  if (!pynqs_mcmc_jrbm_supported(sorb, nhidden)) return -1;
  RbmLayout rl;
  make_rbm_layout(sorb, nhidden, &rl);
  return mcmc_jrbm_form(sorb, rl);
}

extern "C" int pynqs_mcmc_jrbm(uint64_t *states, int64_t nchains, int sorb, int noA, int noB, const void *rbm_table,
                               const void *jastrow_table, int nhidden, uint64_t seed, uint64_t chain_base, uint64_t t0, int nsteps,
                               int every, uint64_t *records, int64_t *n_accept, double *lnpsi, void *stream) {
  pynqs::DeviceScope device_scope_(states);
  SDParams p;
  if (!make_sd_params(sorb, noA + noB, noA, noB, &p)) return set_error(PYNQS_EINVAL, "mcmc_jrbm: bad sorb/noA/noB");
  if (!pynqs_mcmc_jrbm_supported(sorb, nhidden)) return set_error(PYNQS_EINVAL, "mcmc_jrbm: unsupported nhidden / sorb");
  if (nchains < 0 || nsteps < 0 || every < 1) return set_error(PYNQS_EINVAL, "mcmc_jrbm: bad nchains/nsteps/every");
  if (chain_base + (uint64_t)nchains > (1ull << 32)) return set_error(PYNQS_EINVAL, "mcmc_jrbm: chain indices must stay below 2^32");
  if (nchains == 0) return PYNQS_OK;
  if (!states || !rbm_table || !jastrow_table) return set_error(PYNQS_EINVAL, "null pointer");
  RbmLayout rl;
  make_rbm_layout(sorb, nhidden, &rl);
  McmcTable T;
  T.tab = (const double *)rbm_table;
  T.jas = (const double *)jastrow_table;
  T.H = nhidden;
  T.stride = rl.Hq; T.offWt = rl.offWt; T.offE4p = rl.offE4p; T.offE4m = rl.offE4m; T.offHb = rl.offHb; T.offVb = rl.offVb;
  T.total = rl.total;
  const int G = mcmc_group(nhidden);
  const uint64_t grid = ((uint64_t)nchains * G + kBlock - 1) / kBlock;
  if (grid > 0x7fffffffull) return set_error(PYNQS_EINVAL, "nchains too large for one launch");
  const int len = (sorb - 1) / 64 + 1;
  hipStream_t st = (hipStream_t)stream;
  const int form = mcmc_jrbm_form(sorb, rl);
  const size_t lds = form == 3 ? (size_t)(T.total + jastrow_pairs(sorb)) * 8 : form == 1 ? (size_t)T.total * 8 : 0;
#define PYNQS_MCJ(JAS, IN_LDS)                                                                                                          \
  hipLaunchKernelGGL((mcmc_rbm_kernel<LEN, PYNQS_RBM_REAL, IN_LDS, JAS>), dim3((uint32_t)grid), dim3(kBlock), lds, st, states, nchains, \
                     p, T, G, seed, chain_base, t0, nsteps, every, records, n_accept, lnpsi)
  DISPATCH_LEN(len, {
    if (form == 3) PYNQS_MCJ(kJasLds, true);
    else if (form == 1) PYNQS_MCJ(kJasL2, true);
    else PYNQS_MCJ(kJasL2, false);
  });
#undef PYNQS_MCJ
  return check_launch("mcmc_jrbm");
}

extern "C" int pynqs_mcmc_accept(uint64_t *states, double *psi, const uint64_t *proposals, const double *psi_proposals, int64_t nchains,
                                 int sorb, int is_complex, uint64_t seed, uint64_t chain_base, uint64_t t, uint64_t *record_row,
                                 int64_t *n_accept, void *stream) {
  pynqs::DeviceScope device_scope_(states);
  if (sorb < 1 || sorb > kMaxSorb || nchains < 0) return set_error(PYNQS_EINVAL, "mcmc_accept: bad sorb/nchains");
  if (chain_base + (uint64_t)nchains > (1ull << 32)) return set_error(PYNQS_EINVAL, "mcmc_accept: chain indices must stay below 2^32");
  if (nchains == 0) return PYNQS_OK;
  if (!states || !psi || !proposals || !psi_proposals) return set_error(PYNQS_EINVAL, "null pointer");
  const uint64_t grid = ((uint64_t)nchains + kBlock - 1) / kBlock;
  if (grid > 0x7fffffffull) return set_error(PYNQS_EINVAL, "nchains too large for one launch");
  const int len = (sorb - 1) / 64 + 1;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_LEN(len, {
    if (is_complex)
      hipLaunchKernelGGL((mcmc_accept_kernel<LEN, true>), dim3((uint32_t)grid), dim3(kBlock), 0, st, states, psi, proposals, psi_proposals,
                         nchains, seed, chain_base, t, record_row, n_accept);
    else
      hipLaunchKernelGGL((mcmc_accept_kernel<LEN, false>), dim3((uint32_t)grid), dim3(kBlock), 0, st, states, psi, proposals, psi_proposals,
                         nchains, seed, chain_base, t, record_row, n_accept);
  });
  return check_launch("mcmc_accept");
}
