// kernels_jastrow.hip -- the two-body Jastrow factor exp(x^T M x) that multiplies a real RBM (vmc/ansatz/rbm/rbm_other.py, class Jastrow,
// prod_dim = 1; the product of vmc/ansatz/hybrid/multi.py), outside the local-energy kernel (kernels_rbm.hip, JASTROW):
//   pynqs_jastrow_table_build : M [sorb][sorb] -> the Jastrow table of rbm.h (S = M + M^T without its diagonal, exp(+-4 S), tr M)
//   pynqs_jastrow_grad        : the energy-gradient estimator of kernels_rbm_grad.hip for M.  d ln psi / d M_ij = x_i x_j, so
//                                   grad_M[i][j] = 2 sum_n f_n x_i(n) x_j(n),   f_n = p_n (E_loc,n - <E> c_n),
//                               and the Jastrow part of the loss, 2 sum_n f_n x_n^T M x_n; straight from the packed bits.
//   kernel 1: a workgroup takes 64 walkers: their words and f_n go to LDS, then the 256 threads share out the sorb^2 outputs and each
//             adds its 64 terms +- f_n in turn (the sign from two bits); the first 64 threads form x^T M x of a walker each (rows summed
//             one by one, M_ij wave-uniform) and thread 0 adds the 64 shares of the loss in turn.  Partial sums go to the workspace.
//   kernel 2: one thread per output adds the workgroups' partial sums in their order.  No atomics: two calls give the same bits.
#include "detcore.h"
#include "launch.h"
#include "rbm.h"
#include "rbm_math.h"

namespace pynqs {

__global__ __launch_bounds__(kBlock) void jastrow_table_kernel(const double *__restrict__ M, JastrowLayout jl, double *__restrict__ tab) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t n2 = jastrow_pairs(jl.sorb);
  if (k < n2) {
    const int i = (int)(k / jl.sorb), j = (int)(k - (int64_t)i * jl.sorb);
    const double s = i == j ? 0.0 : M[k] + M[(int64_t)j * jl.sorb + i];
    tab[jl.offS + k] = s;
    tab[jl.offE4p + k] = exp(4.0 * s);
    tab[jl.offE4m + k] = exp(-4.0 * s);
  }
  if (k == 0) {
    double tr = 0.0;
    for (int i = 0; i < jl.sorb; ++i) tr += M[(int64_t)i * jl.sorb + i];
    tab[jl.offTr] = tr;
    if (jl.total > jl.offTr + 1) tab[jl.offTr + 1] = 0.0;
  }
}

constexpr int kJGradWalkers = 64;  // per workgroup

template <int LEN>
__global__ __launch_bounds__(kBlock) void jastrow_grad_partial_kernel(const uint64_t *__restrict__ onv, int64_t n, int sorb,
                                                                      const double *__restrict__ M, const double *__restrict__ prob,
                                                                      const double *__restrict__ eloc, const double *__restrict__ e_total,
                                                                      const double *__restrict__ pw, double *__restrict__ partial) {
  __shared__ uint64_t xs[kJGradWalkers][LEN];
  __shared__ double fs[kJGradWalkers];  // f_w (0 past the end), then 2 f_w x_w^T M x_w
  const int tid = threadIdx.x;
  const int64_t n2 = jastrow_pairs(sorb);
  double *__restrict__ out = partial + (int64_t)blockIdx.x * (n2 + 1);
  uint64_t ket[LEN];
  double f = 0.0;
  if (tid < kJGradWalkers) {
    const int64_t i = (int64_t)blockIdx.x * kJGradWalkers + tid;
    const int64_t row = i < n ? i : n - 1;
#pragma unroll
    for (int k = 0; k < LEN; ++k) xs[tid][k] = ket[k] = onv[row * LEN + k];
    if (i < n) f = prob[i] * fma(-e_total[0], pw ? pw[i] : 1.0, eloc[i]);  // (fused: E - <E> c is rounded once, relative to itself)
    fs[tid] = f;
  }
  __syncthreads();
  for (int k = tid; k < n2; k += kBlock) {
    const int a = k / sorb, b = k - a * sorb;
    double g = 0.0;
#pragma unroll 8
    for (int v = 0; v < kJGradWalkers; ++v) {
      const bool same = ((xs[v][a >> 6] >> (a & 63)) & 1ull) == ((xs[v][b >> 6] >> (b & 63)) & 1ull);
      const double fv = fs[v];
      g += same ? fv : -fv;
    }
    out[k] = g;
  }
  __syncthreads();  // fs is read above and rewritten below
  if (tid < kJGradWalkers) {  // (one wave: every lane walks M, the loads are wave-uniform)
    double xmx = 0.0;
    for (int a = 0; a < sorb; ++a) {
      double r = 0.0;
      for (int b = 0; b < sorb; ++b) r = fma(pm1_of<LEN>(ket, b), M[(size_t)a * sorb + b], r);
      xmx = fma(pm1_of<LEN>(ket, a), r, xmx);
    }
    fs[tid] = 2.0 * (f * xmx);
  }
  __syncthreads();
  if (tid == 0) {
    double l = 0.0;
    for (int v = 0; v < kJGradWalkers; ++v) l += fs[v];
    out[n2] = l;
  }
}

// grad_M[k] = 2 x (the workgroups' partial sums in their order); loss = the sum of their shares
__global__ __launch_bounds__(kBlock) void jastrow_grad_reduce_kernel(const double *__restrict__ partial, int64_t ngroups, int sorb,
                                                                     double *__restrict__ grad, double *__restrict__ loss) {
  const int64_t n2 = jastrow_pairs(sorb);
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k > n2) return;
  double s = 0.0;
  constexpr int RU = 8;  // loads in flight (the additions keep their order)
  for (int64_t g0 = 0; g0 < ngroups; g0 += RU) {
    double v[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) v[u] = g0 + u < ngroups ? partial[(g0 + u) * (n2 + 1) + k] : 0.0;
#pragma unroll
    for (int u = 0; u < RU; ++u) s += v[u];
  }
  if (k < n2) grad[k] = 2.0 * s;
  else if (loss) loss[0] = s;
}

}  // namespace pynqs

using namespace pynqs;

extern "C" int64_t pynqs_jastrow_table_bytes(int sorb) {
  JastrowLayout jl;
  if (!make_jastrow_layout(sorb, &jl)) return -1;
  return jl.total * 8;
}

extern "C" int pynqs_jastrow_table_build(const double *jastrow, int sorb, void *table, void *stream) {
  pynqs::DeviceScope device_scope_(jastrow);
  JastrowLayout jl;
  if (!make_jastrow_layout(sorb, &jl)) return set_error(PYNQS_EINVAL, "bad sorb");
  if (!jastrow || !table) return set_error(PYNQS_EINVAL, "null pointer");
  const uint32_t grid = (uint32_t)((jastrow_pairs(sorb) + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(jastrow_table_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, jastrow, jl, (double *)table);
  return check_launch("jastrow_table_build");
}

extern "C" int64_t pynqs_jastrow_grad_workspace(int64_t n, int sorb) {
  if (n < 0 || sorb < 1 || sorb > kMaxSorb) return -1;
  const int64_t groups = (n + kJGradWalkers - 1) / kJGradWalkers;
  return groups * (jastrow_pairs(sorb) + 1) * 8;
}

extern "C" int pynqs_jastrow_grad(const uint64_t *onv, int64_t n, int sorb, const double *jastrow, const double *prob, const double *eloc,
                                  const double *e_total, const double *pow, double *grad_jastrow, double *loss, void *workspace,
                                  void *stream) {
  pynqs::DeviceScope device_scope_(onv);
  if (n < 0 || n > 0x7fffffffll * kJGradWalkers || sorb < 1 || sorb > kMaxSorb) return set_error(PYNQS_EINVAL, "bad n/sorb");
  if (!jastrow || !grad_jastrow || (n > 0 && (!onv || !prob || !eloc || !e_total || !workspace))) return set_error(PYNQS_EINVAL, "null pointer");
  const int len = (sorb - 1) / 64 + 1;
  const int64_t groups = (n + kJGradWalkers - 1) / kJGradWalkers;
  hipStream_t st = (hipStream_t)stream;
  double *partial = (double *)workspace;
  if (groups > 0) {
    DISPATCH_LEN(len, {
      hipLaunchKernelGGL((jastrow_grad_partial_kernel<LEN>), dim3((uint32_t)groups), dim3(kBlock), 0, st, onv, n, sorb, jastrow, prob, eloc,
                         e_total, pow, partial);
    });
  }
  const uint32_t g2 = (uint32_t)((jastrow_pairs(sorb) + 1 + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(jastrow_grad_reduce_kernel, dim3(g2), dim3(kBlock), 0, st, partial, groups, sorb, grad_jastrow, loss);
  return check_launch("jastrow_grad");
}
