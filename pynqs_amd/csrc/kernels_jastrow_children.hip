// kernels_jastrow_children.hip -- the two-body Jastrow factor exp(x'^T M x') on the DISTINCT x' of a REDUCE front end, each from its parent
// walker, multiplied onto the RBM amplitudes that pynqs_rbm_forward_children has written (kernels_rbm_forward.hip is not involved beyond
// that: this file never sees the hidden layer).  With S = M + M^T without its diagonal (the Jastrow table of rbm.h),
//     x^T M x = tr M + 1/2 sum_o x_o r_o,   r_o = sum_j S_oj x_j,
// and for x' = x with the orbitals F flipped (|F| <= 4)
//     Delta = x'^T M x' - x^T M x = -2 sum_{i in F} x_i r_i + 4 sum_{i<j in F} S_ij x_i x_j          (x: the PARENT's +-1 values).
//   pynqs_jastrow_children_prepare : per parent p, table[p][o] = r_o (o < sorb) and table[p][sorb] = q0 = tr M + 1/2 sum_o x_o r_o
//     kernel 1: a thread per (parent, orbital): one fma chain over j ascending from 0 (the chain of rdm_r_kernel, kernels_rdm.hip)
//     kernel 2: a thread per parent: one fma chain over o ascending from 0, then fma(0.5, sum, tr M).  No atomics: two calls give the same bits.
//   pynqs_jastrow_children_apply   : psi[r] *= exp(q0[p] + Delta_r), p = parent[r], F from onv[r] XOR walkers[p]; ONE THREAD PER ROW, the grid
//     is NOT capped (ceil(n / 256) workgroups, no stride loop: nothing to ask a geometry entry for).  onv, parent and psi are read with
//     consecutive lanes on consecutive rows; the parent's words, at most four r_i, q0 and at most six S_ij are gathers served by the L2
//     (nwalkers x (sorb + 1) doubles: 2.7 MB for 8192 walkers of 40 orbitals; S: sorb^2 doubles).  The exponent is one sum
//     (lin = sum x_i r_i and pair = sum S_ij x_i x_j as fma chains in ascending flip order, Delta = fma(-2, lin, 4 pair), q0 + Delta) and one
//     exp per row.  No flip: lin = pair = 0, Delta = 0 exactly and psi *= exp(q0).
//     A STRANGER -- parent outside [0, nwalkers), or more than four orbitals differ from the named parent -- gets its exponent from scratch on
//     its own bits: tr M + sum_i x'_i (sum_{j>i} S_ij x'_j).  Never truncated to four flips, never clamped to walker 0.
//     Bits of onv[r] at and above sorb are ignored (they cannot index past a table).  Rows at and past min(*count_dev, n) are neither read
//     nor written.  A row whose psi is 0, inf or nan is left as it is (inf x exp(..) = 0 would otherwise make a nan of an inf).
#include "detcore.h"
#include "launch.h"
#include "rbm.h"

namespace pynqs {

// r[p][o] = sum_j S_oj x_j: one fma chain over the orbitals in ascending order from 0 (S_oo = 0); row stride sorb + 1
template <int LEN>
__global__ __launch_bounds__(kBlock) void jastrow_children_r_kernel(const uint64_t *__restrict__ walkers, int64_t nw, int sorb,
                                                                    const double *__restrict__ S, double *__restrict__ tab) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= nw * sorb) return;
  const int64_t p = g / sorb;
  const int o = (int)(g - p * sorb);
  uint64_t x[LEN];
#pragma unroll
  for (int k = 0; k < LEN; ++k) x[k] = walkers[p * LEN + k];
  const double *__restrict__ row = S + (int64_t)o * sorb;
  double acc = 0.0;
  for (int j = 0; j < sorb; ++j) acc = fma(bit_of<LEN>(x, j) ? 1.0 : -1.0, row[j], acc);
  tab[p * (sorb + 1) + o] = acc;
}

// q0[p] = tr M + 1/2 sum_o x_o r_o: one fma chain over the orbitals in ascending order from 0
template <int LEN>
__global__ __launch_bounds__(kBlock) void jastrow_children_q0_kernel(const uint64_t *__restrict__ walkers, int64_t nw, int sorb,
                                                                     const double *__restrict__ tr, double *__restrict__ tab) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= nw) return;
  uint64_t x[LEN];
#pragma unroll
  for (int k = 0; k < LEN; ++k) x[k] = walkers[p * LEN + k];
  double *__restrict__ row = tab + p * (sorb + 1);
  double acc = 0.0;
  for (int o = 0; o < sorb; ++o) acc = fma(bit_of<LEN>(x, o) ? 1.0 : -1.0, row[o], acc);
  row[sorb] = fma(0.5, acc, tr[0]);
}

template <int LEN>
__global__ __launch_bounds__(kBlock) void jastrow_children_apply_kernel(const uint64_t *__restrict__ onv, int64_t n, const int32_t *__restrict__ count_dev,
                                                                        const int32_t *__restrict__ parent, const uint64_t *__restrict__ walkers,
                                                                        int64_t nw, const double *__restrict__ tab, const double *__restrict__ S,
                                                                        const double *__restrict__ tr, int sorb, double *__restrict__ psi) {
  int64_t cnt = n;
  if (count_dev) cnt = min((int64_t)max(*count_dev, 0), n);
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= cnt) return;
  const double v = psi[i];
  uint64_t x[LEN], d[LEN], w[LEN];
#pragma unroll
  for (int k = 0; k < LEN; ++k) x[k] = onv[i * LEN + k];
  const int top = sorb - 64 * (LEN - 1);  // orbitals of the last word (1 .. 64)
  x[LEN - 1] &= top >= 64 ? ~0ull : ((1ull << top) - 1ull);
  const int64_t p = parent[i];
  bool stranger = p < 0 || p >= nw;
  int nflip = 0;
  if (!stranger) {
#pragma unroll
    for (int k = 0; k < LEN; ++k) {
      w[k] = walkers[p * LEN + k];
      d[k] = x[k] ^ w[k];
    }
    d[LEN - 1] &= top >= 64 ? ~0ull : ((1ull << top) - 1ull);  // (a parent's bits above sorb do not make flips either)
#pragma unroll
    for (int k = 0; k < LEN; ++k) nflip += __popcll(d[k]);
    stranger = nflip > 4;
  }
  double e;
  if (!stranger) {
    const double *__restrict__ row = tab + p * (sorb + 1);
    // the flipped orbitals in ascending order; an empty slot: orbital 0 with x = 0 (its terms are +-0)
    int f[4];
    double xs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int o = -1;
#pragma unroll
      for (int q = LEN - 1; q >= 0; --q)
        if (d[q]) o = 64 * q + __ffsll((long long)d[q]) - 1;
#pragma unroll
      for (int q = 0; q < LEN; ++q)
        if (o >= 0 && (o >> 6) == q) d[q] &= d[q] - 1ull;
      xs[k] = o < 0 ? 0.0 : (bit_of<LEN>(w, o) ? 1.0 : -1.0);
      f[k] = o < 0 ? 0 : o;
    }
    double lin = 0.0, pair = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) lin = fma(xs[k], row[f[k]], lin);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = a + 1; b < 4; ++b) pair = fma(xs[a] * xs[b], S[(int64_t)f[a] * sorb + f[b]], pair);
    e = row[sorb] + fma(-2.0, lin, 4.0 * pair);
  } else {
    double acc = 0.0;
    for (int a = 0; a < sorb; ++a) {
      const double *__restrict__ srow = S + (int64_t)a * sorb;
      double r = 0.0;
      for (int b = a + 1; b < sorb; ++b) r = fma(bit_of<LEN>(x, b) ? 1.0 : -1.0, srow[b], r);
      acc = fma(bit_of<LEN>(x, a) ? 1.0 : -1.0, r, acc);
    }
    e = acc + tr[0];
  }
  if (v != 0.0 && isfinite(v)) psi[i] = v * exp(e);
}

}  // namespace pynqs

using namespace pynqs;

extern "C" int64_t pynqs_jastrow_children_table_bytes(int64_t nwalkers, int sorb) {
  if (nwalkers < 0 || nwalkers > 0x7fffffffll || sorb < 1 || sorb > kMaxSorb) return -1;
  return nwalkers * (sorb + 1) * 8;
}

extern "C" int pynqs_jastrow_children_prepare(const uint64_t *walkers, int64_t nwalkers, int sorb, const void *jastrow_table, void *table,
                                              void *stream) {
  pynqs::DeviceScope device_scope_(walkers);
  JastrowLayout jl;
  if (nwalkers < 0 || nwalkers > 0x7fffffffll || !make_jastrow_layout(sorb, &jl)) return set_error(PYNQS_EINVAL, "jastrow_children_prepare: bad nwalkers/sorb");
  if (!jastrow_table || (nwalkers > 0 && (!walkers || !table))) return set_error(PYNQS_EINVAL, "null pointer");
  if (nwalkers == 0) return PYNQS_OK;
  const double *jt = (const double *)jastrow_table;
  const int len = (sorb - 1) / 64 + 1;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t g1 = (uint32_t)((nwalkers * sorb + kBlock - 1) / kBlock), g2 = (uint32_t)((nwalkers + kBlock - 1) / kBlock);
  DISPATCH_LEN(len, {
    hipLaunchKernelGGL((jastrow_children_r_kernel<LEN>), dim3(g1), dim3(kBlock), 0, st, walkers, nwalkers, sorb, jt + jl.offS, (double *)table);
    hipLaunchKernelGGL((jastrow_children_q0_kernel<LEN>), dim3(g2), dim3(kBlock), 0, st, walkers, nwalkers, sorb, jt + jl.offTr, (double *)table);
  });
  return check_launch("jastrow_children_prepare");
}

extern "C" int pynqs_jastrow_children_apply(const uint64_t *onv, int64_t n, const int32_t *count_dev, const int32_t *parent,
                                            const uint64_t *walkers, int64_t nwalkers, const void *table, const void *jastrow_table, int sorb,
                                            double *psi, void *stream) {
  pynqs::DeviceScope device_scope_(onv);
  JastrowLayout jl;
  if (n < 0 || n > 0x7fffffffll * kBlock || nwalkers < 0 || nwalkers > 0x7fffffffll || !make_jastrow_layout(sorb, &jl))
    return set_error(PYNQS_EINVAL, "jastrow_children_apply: bad n/nwalkers/sorb");
  if (!jastrow_table || (n > 0 && (!onv || !parent || !psi)) || (nwalkers > 0 && (!walkers || !table))) return set_error(PYNQS_EINVAL, "null pointer");
  if (n == 0) return PYNQS_OK;
  const double *jt = (const double *)jastrow_table;
  const int len = (sorb - 1) / 64 + 1;
  const uint32_t grid = (uint32_t)((n + kBlock - 1) / kBlock);
  DISPATCH_LEN(len, {
    hipLaunchKernelGGL((jastrow_children_apply_kernel<LEN>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, onv, n, count_dev, parent, walkers,
                       nwalkers, (const double *)table, jt + jl.offS, jt + jl.offTr, sorb, psi);
  });
  return check_launch("jastrow_children_apply");
}
