// kernels_rbm_sr.hip -- stochastic reconfiguration (the natural gradient of vmc/grad/sr.py) for the reference's RBM amplitudes
// (vmc/ansatz/rbm/rbm.py:186-211), matrix-free: the reference materialises O[n][P], forms S = <O* O> - <O*><O> as a dense P x P matrix
// and inverts it; here  (S + shift) d = F  is solved by conjugate gradients on the product
//     c_n = sum_k (O_nk - Obar_k) z_k = x_n . z_a + sum_h tanh(theta_nh) (z_b,h + sum_o z_W,ho x_no) - Obar . z,
//     y_k = sum_n p_n conj(O_nk) c_n,        (S v)_k = y_k  (real parameters)  or  (Re y_k, Im y_k)  ((re, im) pairs),
// with O = (x_o, tanh theta_h, tanh theta_h x_o) an outer product of two short vectors formed from the packed bits: nothing of size
// n x P or P x P exists.  The inner sum of c_n is theta with the parameters' places taken by z, so a product is the gradient kernel's two
// halves (kernels_rbm_grad.hip): the fma chain over the orbitals, then the [32 walkers] x [32 hidden units] x [sorb + 1] outer products.
//   prepare : once per solve.  Workgroup of 32 walkers as in the gradient kernel: theta, tanh (the overflow-free forms), tanh -> table
//             [H][n](x2) (walkers fastest: the reads of a wave are contiguous), and the workgroup's share of Obar = sum_n p_n O_n;
//             then the fixed-order sum over the workgroups.
//   matvec  : (1) Obar . z, one workgroup; (2) per 32 walkers: thread (walker w, group q of 8) forms its share of c_w over hidden units
//             4 q .. 4 q + 3 of every 32 with tanh from the table, LDS sum over q in a fixed order, g_w = p_w c_w, then the outer
//             products sum_w conj(tanh theta_wh) g_w (x_wo | 1) and sum_w g_w x_wo; (3) the fixed-order sum over the workgroups.
//   cg_step : the vector part of an iteration in ONE workgroup (P_real <= 2 x 29 160 at the largest size served), the scalars in device
//             memory, dot products in a fixed order; a `done` flag turns later steps into no-ops so that the host enqueues several
//             iterations between read-backs.
//   Jastrow-RBM (JAS; psi = exp(a.x + x^T M x) prod_h 2cosh theta_h, real parameters): O gains the block x_i x_j, P = H sorb + H + sorb +
//             sorb^2, and c_n the term x_n^T Z x_n with Z the jastrow block of z.  Only the symmetric part of Z reaches it:
//             x^T Z x = sum_i Z_ii + sum_{i<j} (Z_ij + Z_ji) x_i x_j.  The 8 threads of a walker share the rows (row i: thread i mod 8) and
//             add the entries S_ij = Z_ij + Z_ji with the sign of x_j, then the row with the sign of x_i: no multiply.  S is staged in LDS
//             when it leaves room for two workgroups per CU (sorb <= 128), else read from Z in the L2 (the addresses are the same for the
//             32 walkers of a half-wave).  The thread of a walker adds the eight shares AFTER the RBM sum, so Z = 0 leaves the RBM blocks'
//             bits.  The outputs sum_w g_w x_wi x_wj are formed for i <= j only, the sign from two bits, and kept behind the visible-bias
//             block in the paired-rows order of jas_pair_at; the reduce kernel writes (i, j) and (j, i) from the same sum: the Jastrow
//             block of y is bit-symmetric.
// Everything is float64 and bit-reproducible.
#include "detcore.h"
#include "launch.h"
#include "rbm_math.h"

namespace pynqs {

constexpr int kSrWalkers = 32;  // per workgroup
constexpr int kSrHidden = 32;   // per pass: 4 per thread, 8 threads per walker
constexpr int kSrCgBlock = 1024;

__host__ __device__ static inline int64_t sr_nout(int sorb, int H) { return (int64_t)H * (sorb + 1) + sorb; }  // per workgroup: (W[h][:], b[h]) rows, then a
static inline int64_t sr_table_doubles(int64_t n, int H, bool cplx) { return n * H * (cplx ? 2 : 1); }

// The upper triangle i <= j of an [sorb][sorb] matrix as ceil(sorb / 2) rows of sorb + 1: rows r and sorb - 1 - r of the triangle
// (sorb - r and r + 1 entries) share one.  Odd sorb: the middle row pairs with itself and its second half stays empty.
__host__ __device__ static inline int jas_pair_count(int sorb) { return ((sorb + 1) / 2) * (sorb + 1); }
__device__ __forceinline__ int jas_pair_at(int sorb, int i, int j) {  // i <= j
  return i < (sorb + 1) / 2 ? i * (sorb + 1) + (j - i) : (sorb - 1 - i) * (sorb + 1) + j + 1;
}
__device__ __forceinline__ bool jas_pair_decode(int sorb, int k, int &i, int &j) {
  const int r = k / (sorb + 1), c = k - r * (sorb + 1);
  if (c < sorb - r) { i = r; j = r + c; return true; }
  i = sorb - 1 - r; j = c - 1;
  return i != r;
}
constexpr int kSrJasLdsBytes = 66 * 1024;  // S in LDS up to here: sorb <= 128 (66 048 bytes beside 13 KiB of static LDS, two workgroups per CU)
static inline bool sr_jas_in_lds(int sorb) { return (int64_t)jas_pair_count(sorb) * 8 <= kSrJasLdsBytes; }

// PREP: A = weights, B = hidden bias; writes the table and the partial sums of Obar.  Otherwise: A, B, VA = z_W, z_b, z_a (the vector's
// blocks in the parameters' layout), dot = Obar . z; reads the table and writes the partial sums of y.
// JAS (0: none; 1: S from Z in global memory; 2: S staged in the dynamic LDS): Z = the jastrow block of z (unused by PREP).
template <int LEN, bool CPLX, bool PREP, int JAS = 0>
__global__ __launch_bounds__(kBlock) void rbm_sr_partial_kernel(const uint64_t *__restrict__ onv, int64_t n, int sorb, int H,
                                                                const double *__restrict__ A, const double *__restrict__ B,
                                                                const double *__restrict__ VA, const double *__restrict__ prob,
                                                                double *__restrict__ table, const double *__restrict__ dot,
                                                                double *__restrict__ partial, int64_t stride,
                                                                const double *__restrict__ Z = nullptr) {
  static_assert(!JAS || !CPLX, "the Jastrow-RBM has real parameters");
  constexpr int C = CPLX ? 2 : 1;
  constexpr int NQ = kBlock / kSrWalkers;  // threads per walker
  constexpr int HC = kSrHidden / NQ;
  __shared__ uint64_t xs[kSrWalkers][LEN];
  __shared__ double tc[kSrWalkers][kSrHidden + 1][C];  // PREP: tanh(theta_h) p_w; else conj(tanh(theta_h)) g_w; +1: bank spread
  __shared__ double cf[kSrWalkers][C];                 // PREP: p_w; else g_w = p_w c_w
  __shared__ double cq[NQ][kSrWalkers][C];             // the threads' shares of c_w
  __shared__ double cjq[JAS != 0 && !PREP ? NQ : 1][kSrWalkers];  // JAS: their shares of x_w^T Z x_w
  const int tid = threadIdx.x, w = tid % kSrWalkers, q = tid / kSrWalkers;
  const int64_t i = (int64_t)blockIdx.x * kSrWalkers + w;
  const bool valid = i < n;
  const int64_t row = valid ? i : n - 1;
  uint64_t ket[LEN];
#pragma unroll
  for (int k = 0; k < LEN; ++k) ket[k] = onv[row * LEN + k];
  const double pr = valid ? prob[i] : 0.0;
  if (q == 0) {
#pragma unroll
    for (int k = 0; k < LEN; ++k) xs[w][k] = ket[k];
  }
  double gr = pr, gi = 0.0;  // the walker's weight in the sums
  if constexpr (!PREP) {
    double cj = 0.0;  // this thread's rows of x^T Z x
    if constexpr (JAS != 0) {
      extern __shared__ __attribute__((aligned(16))) double ssym[];  // JAS 2: S (diagonal: Z_ii) in the order of jas_pair_at
      if constexpr (JAS == 2) {
        const int np2 = jas_pair_count(sorb);
        for (int k = tid; k < np2; k += kBlock) {
          int a, b;
          if (jas_pair_decode(sorb, k, a, b)) ssym[k] = a == b ? Z[(size_t)a * sorb + a] : Z[(size_t)a * sorb + b] + Z[(size_t)b * sorb + a];
        }
        __syncthreads();
      }
      for (int a = q; a < sorb; a += NQ) {
        const int at = jas_pair_at(sorb, a, a) - a;  // + b: (a, b)
        double r = 0.0;
#pragma unroll
        for (int wd = 0; wd < LEN; ++wd) {
          const int b0 = max(a + 1, 64 * wd), b1 = min(sorb, 64 * wd + 64);
          if (b0 >= b1) continue;
          uint64_t bits = ket[wd] >> (b0 & 63);
#pragma unroll 4
          for (int b = b0; b < b1; ++b) {
            const double sv = JAS == 2 ? ssym[at + b] : Z[(size_t)a * sorb + b] + Z[(size_t)b * sorb + a];
            r += (bits & 1ull) ? sv : -sv;
            bits >>= 1;
          }
        }
        cj += pm1_of<LEN>(ket, a) > 0.0 ? r : -r;
        cj += JAS == 2 ? ssym[at + a] : Z[(size_t)a * sorb + a];
      }
    }
    // ---- c_w: this thread's hidden units
    double cr = 0.0, ci = 0.0;
    for (int h0 = 0; h0 < H; h0 += kSrHidden) {
      double tr[HC], ti[HC];
#pragma unroll
      for (int j = 0; j < HC; ++j) {
        const int h = min(h0 + HC * q + j, H - 1);
        tr[j] = CPLX ? B[2 * h] : B[h];
        ti[j] = CPLX ? B[2 * h + 1] : 0.0;
      }
      for (int o = 0; o < sorb; ++o) {
        const double x = pm1_of<LEN>(ket, o);
#pragma unroll
        for (int j = 0; j < HC; ++j) {
          const int h = min(h0 + HC * q + j, H - 1);
          if constexpr (CPLX) {
            tr[j] = fma(x, A[((size_t)h * sorb + o) * 2], tr[j]);
            ti[j] = fma(x, A[((size_t)h * sorb + o) * 2 + 1], ti[j]);
          } else {
            tr[j] = fma(x, A[(size_t)h * sorb + o], tr[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < HC; ++j) {
        const int hl = h0 + HC * q + j, h = min(hl, H - 1);
        if (hl < H) {
          const double yr = table[((int64_t)h * n + row) * C];
          if constexpr (CPLX) {
            const double yi = table[((int64_t)h * n + row) * C + 1];
            cr += yr * tr[j] - yi * ti[j];
            ci += yr * ti[j] + yi * tr[j];
          } else {
            cr = fma(yr, tr[j], cr);
          }
        }
      }
    }
    cq[q][w][0] = cr;
    if constexpr (CPLX) cq[q][w][1] = ci;
    if constexpr (JAS != 0) cjq[q][w] = cj;
    __syncthreads();
    if (q == 0) {
      double ar = 0.0, ai = 0.0;  // x . z_a
      for (int o = 0; o < sorb; ++o) {
        const double x = pm1_of<LEN>(ket, o);
        ar = fma(x, CPLX ? VA[2 * o] : VA[o], ar);
        if constexpr (CPLX) ai = fma(x, VA[2 * o + 1], ai);
      }
#pragma unroll
      for (int k = 0; k < NQ; ++k) {
        ar += cq[k][w][0];
        if constexpr (CPLX) ai += cq[k][w][1];
      }
      if constexpr (JAS != 0) {  // after the RBM sum: Z = 0 leaves its bits
        double jr = 0.0;
#pragma unroll
        for (int k = 0; k < NQ; ++k) jr += cjq[k][w];
        ar += jr;
      }
      ar -= dot[0];
      if constexpr (CPLX) ai -= dot[1];
      cf[w][0] = pr * ar;
      if constexpr (CPLX) cf[w][1] = pr * ai;
    }
    __syncthreads();
    gr = cf[w][0];
    if constexpr (CPLX) gi = cf[w][1];
  } else {
    if (q == 0) {
      cf[w][0] = pr;
      if constexpr (CPLX) cf[w][1] = 0.0;
    }
  }
  double *__restrict__ out = partial + (int64_t)blockIdx.x * stride;
  const int SP = sorb + 1;  // outputs per hidden unit: W[h][0..sorb-1], b[h]
  for (int h0 = 0; h0 < H; h0 += kSrHidden) {
    double yr[HC], yi[HC];
    if constexpr (PREP) {
      // ---- theta, tanh for hidden units h0 + 4 q .. + 4 of walker w
      double tr[HC], ti[HC];
#pragma unroll
      for (int j = 0; j < HC; ++j) {
        const int h = min(h0 + HC * q + j, H - 1);
        tr[j] = CPLX ? B[2 * h] : B[h];
        ti[j] = CPLX ? B[2 * h + 1] : 0.0;
      }
      for (int o = 0; o < sorb; ++o) {
        const double x = pm1_of<LEN>(ket, o);
#pragma unroll
        for (int j = 0; j < HC; ++j) {
          const int h = min(h0 + HC * q + j, H - 1);
          if constexpr (CPLX) {
            tr[j] = fma(x, A[((size_t)h * sorb + o) * 2], tr[j]);
            ti[j] = fma(x, A[((size_t)h * sorb + o) * 2 + 1], ti[j]);
          } else {
            tr[j] = fma(x, A[(size_t)h * sorb + o], tr[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < HC; ++j) {
        // tanh(a + ib) = (s (1 - e^2) + 2 i e sin 2b) / (1 + e^2 + 2 e cos 2b),  e = exp(-2 |a|), s = sign(a)
        const double ax = fabs(tr[j]), e = exp(-2.0 * ax), s = tr[j] < 0.0 ? -1.0 : 1.0;
        if constexpr (CPLX) {
          double sn, cs;
          sincos_mod(2.0 * ti[j], sn, cs);
          const double den = fma(2.0 * e, cs, fma(e, e, 1.0));
          yr[j] = s * (1.0 - e * e) / den;
          yi[j] = 2.0 * e * sn / den;
        } else {
          yr[j] = s * (1.0 - e) / (1.0 + e);
          yi[j] = 0.0;
        }
        const int hl = h0 + HC * q + j;
        if (valid && hl < H) {
          table[((int64_t)hl * n + i) * C] = yr[j];
          if constexpr (CPLX) table[((int64_t)hl * n + i) * C + 1] = yi[j];
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < HC; ++j) {
        const int h = min(h0 + HC * q + j, H - 1);
        yr[j] = table[((int64_t)h * n + row) * C];
        yi[j] = CPLX ? -table[((int64_t)h * n + row) * C + 1] : 0.0;  // conj(tanh theta)
      }
    }
    if (h0) __syncthreads();  // the previous pass' sums have read tc
#pragma unroll
    for (int j = 0; j < HC; ++j) {
      const int hh = HC * q + j;
      const bool live = h0 + hh < H;
      if constexpr (CPLX) {
        tc[w][hh][0] = live ? yr[j] * gr - yi[j] * gi : 0.0;
        tc[w][hh][1] = live ? yr[j] * gi + yi[j] * gr : 0.0;
      } else {
        tc[w][hh][0] = live ? yr[j] * gr : 0.0;
      }
    }
    __syncthreads();
    // ---- this pass' outputs: (hh, o), o = sorb: the hidden bias
    const int nout = min(kSrHidden, H - h0) * SP;
    for (int k = tid; k < nout; k += kBlock) {
      const int hh = k / SP, o = k - hh * SP;
      double ar = 0.0, ai = 0.0;
      if (o < sorb) {
        const int word = o >> 6, bit = o & 63;
#pragma unroll 8
        for (int v = 0; v < kSrWalkers; ++v) {
          const bool up = (xs[v][word] >> bit) & 1ull;
          const double a = tc[v][hh][0];
          ar += up ? a : -a;
          if constexpr (CPLX) { const double b = tc[v][hh][1]; ai += up ? b : -b; }
        }
      } else {
#pragma unroll 8
        for (int v = 0; v < kSrWalkers; ++v) {
          ar += tc[v][hh][0];
          if constexpr (CPLX) ai += tc[v][hh][1];
        }
      }
      const int64_t at = (int64_t)(h0 + hh) * SP + o;
      out[C * at] = ar;
      if constexpr (CPLX) out[C * at + 1] = ai;
    }
  }
  // ---- visible bias: sum_w g_w x_wo
  const int64_t off_vb = (int64_t)H * SP;
  for (int o = tid; o < sorb; o += kBlock) {
    const int word = o >> 6, bit = o & 63;
    double ar = 0.0, ai = 0.0;
    for (int v = 0; v < kSrWalkers; ++v) {
      const bool up = (xs[v][word] >> bit) & 1ull;
      ar += up ? cf[v][0] : -cf[v][0];
      if constexpr (CPLX) ai += up ? cf[v][1] : -cf[v][1];
    }
    out[C * (off_vb + o)] = ar;
    if constexpr (CPLX) out[C * (off_vb + o) + 1] = ai;
  }
  if constexpr (JAS != 0) {
    // ---- jastrow, i <= j: sum_w g_w x_wi x_wj
    const int64_t off_j = off_vb + sorb;
    const int np2 = jas_pair_count(sorb);
    for (int k = tid; k < np2; k += kBlock) {
      int a, b;
      double ar = 0.0;
      if (jas_pair_decode(sorb, k, a, b)) {
        const int wa = a >> 6, ba = a & 63, wb = b >> 6, bb = b & 63;
#pragma unroll 8
        for (int v = 0; v < kSrWalkers; ++v) {
          const bool same = ((xs[v][wa] >> ba) & 1ull) == ((xs[v][wb] >> bb) & 1ull);
          const double g = cf[v][0];
          ar += same ? g : -g;
        }
      }
      out[off_j + k] = ar;
    }
  }
}

// out (flat, the parameters' layout: weights [H][sorb], hidden_bias [H], visible_bias [sorb], x2 for pairs) = the workgroups' partial
// sums in a fixed order
// JAS: the jastrow block [sorb][sorb] follows; its partial sums hold i <= j (jas_pair_at), written to (i, j) and (j, i)
template <bool CPLX, bool JAS = false>
__global__ __launch_bounds__(kBlock) void rbm_sr_reduce_kernel(const double *__restrict__ partial, int64_t stride, int ngroups, int sorb, int H,
                                                               double *__restrict__ flat) {
  static_assert(!JAS || !CPLX, "the Jastrow-RBM has real parameters");
  constexpr int C = CPLX ? 2 : 1;
  constexpr int NS = kBlock / 64;  // a block owns 64 outputs; its NS waves take contiguous slices of the workgroups' partial sums
  __shared__ double part[NS][64][2];
  const int SP = sorb + 1;
  const int64_t nrbm = sr_nout(sorb, H), nout = nrbm + (JAS ? jas_pair_count(sorb) : 0);
  const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int64_t k = (int64_t)blockIdx.x * 64 + lane;
  const int per = (ngroups + NS - 1) / NS, g_lo = min(slice * per, ngroups), g_hi = min(g_lo + per, ngroups);
  double re = 0.0, im = 0.0;
  if (k < nout) {
    constexpr int RU = 16;  // loads in flight (the additions keep their order)
    for (int g0 = g_lo; g0 < g_hi; g0 += RU) {
      double vr[RU], vi[RU];
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        const bool in = g0 + u < g_hi;
        vr[u] = in ? partial[(int64_t)(g0 + u) * stride + C * k] : 0.0;
        vi[u] = CPLX && in ? partial[(int64_t)(g0 + u) * stride + C * k + 1] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < RU; ++u) { re += vr[u]; im += vi[u]; }
    }
  }
  part[slice][lane][0] = re;
  part[slice][lane][1] = im;
  __syncthreads();
  if (slice != 0 || k >= nout) return;
  re = 0.0; im = 0.0;
#pragma unroll
  for (int sl = 0; sl < NS; ++sl) { re += part[sl][lane][0]; im += part[sl][lane][1]; }  // fixed order: reproducible
  if constexpr (JAS) {
    if (k >= nrbm) {
      int a, b;
      if (jas_pair_decode(sorb, (int)(k - nrbm), a, b)) {
        double *__restrict__ m = flat + (int64_t)H * sorb + H + sorb;
        m[(size_t)a * sorb + b] = re;
        m[(size_t)b * sorb + a] = re;
      }
      return;
    }
  }
  int64_t at;
  if (k < (int64_t)H * SP) {
    const int64_t h = k / SP;
    const int o = (int)(k - h * SP);
    at = o < sorb ? h * sorb + o : (int64_t)H * sorb + h;
  } else {
    at = (int64_t)H * sorb + H + (k - (int64_t)H * SP);
  }
  flat[C * at] = re;
  if constexpr (CPLX) flat[C * at + 1] = im;
}

// sum of one value per thread over the workgroup, the same bits in every thread: a tree over LDS in a fixed order
template <int BLOCK>
__device__ __forceinline__ double block_sum(double v, double *sh) {
  __syncthreads();  // (sh may still be read from the previous sum)
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int d = BLOCK / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
    __syncthreads();
  }
  return sh[0];
}

// dot[0..C-1] = Obar . z = sum_k Obar_k z_k (complex product for pairs, no conjugate), one workgroup, fixed order
template <bool CPLX>
__global__ __launch_bounds__(kBlock) void rbm_sr_dot_kernel(const double *__restrict__ obar, const double *__restrict__ z, int64_t np,
                                                            double *__restrict__ dot) {
  __shared__ double sh[kBlock];
  double re = 0.0, im = 0.0;
  for (int64_t k = threadIdx.x; k < np; k += kBlock) {
    if constexpr (CPLX) {
      const double a = obar[2 * k], b = obar[2 * k + 1], c = z[2 * k], d = z[2 * k + 1];
      re += a * c - b * d;
      im += a * d + b * c;
    } else {
      re = fma(obar[k], z[k], re);
    }
  }
  const double sr = block_sum<kBlock>(re, sh);
  double si = 0.0;
  if constexpr (CPLX) si = block_sum<kBlock>(im, sh);
  if (threadIdx.x == 0) {
    dot[0] = sr;
    if constexpr (CPLX) dot[1] = si;
  }
}

// The vector part of conjugate gradients on (S + shift) d = rhs.  sc (PYNQS_SR_* slots): rho = r.r, |rhs|^2, done, iterations, the last
// true |r|^2, the last p.Ap, converged, breakdown.
//   mode 0: d = 0, r = p = rhs, rho = |rhs|^2; done (and converged) at once when rhs = 0.
//   mode 1: (no-op when done)  Ap = y * inv_world + shift p;  alpha = rho / p.Ap;  d += alpha p;  r -= alpha Ap;  rho' = r.r;
//           p = r + (rho' / rho) p;  done when rho' <= tol^2 |rhs|^2  (or p.Ap <= 0: breakdown).  y is overwritten with Ap.
//   mode 2: y = S d from the product:  r = rhs - (y * inv_world + shift d), the TRUE residual;  converged and done when |r|^2 <= tol^2 |rhs|^2,
//           else p = r, rho = |r|^2 and done is cleared: CG goes on from d.
__global__ __launch_bounds__(kSrCgBlock) void rbm_sr_cg_kernel(int mode, int64_t np, double *__restrict__ y, const double *__restrict__ rhs,
                                                               double *__restrict__ d, double *__restrict__ r, double *__restrict__ p,
                                                               double *__restrict__ sc, double inv_world, double shift, double tol) {
  __shared__ double sh[kSrCgBlock];
  const int tid = threadIdx.x;
  if (mode == 0) {
    double acc = 0.0;
    for (int64_t k = tid; k < np; k += kSrCgBlock) {
      const double b = rhs[k];
      d[k] = 0.0; r[k] = b; p[k] = b;
      acc = fma(b, b, acc);
    }
    const double rho = block_sum<kSrCgBlock>(acc, sh);
    if (tid == 0) {
      const double stop = rho == 0.0 ? 1.0 : 0.0;
      sc[PYNQS_SR_RHO] = rho; sc[PYNQS_SR_RHS2] = rho; sc[PYNQS_SR_DONE] = stop; sc[PYNQS_SR_ITER] = 0.0;
      sc[PYNQS_SR_TRUE2] = rho; sc[PYNQS_SR_PAP] = 0.0; sc[PYNQS_SR_CONVERGED] = stop; sc[PYNQS_SR_BREAKDOWN] = 0.0;
    }
    return;
  }
  const double rho = sc[PYNQS_SR_RHO], rhs2 = sc[PYNQS_SR_RHS2], done = sc[PYNQS_SR_DONE];
  if (mode == 1) {
    if (done != 0.0) return;  // (the same value in every thread: written by an earlier launch)
    double acc = 0.0;
    for (int64_t k = tid; k < np; k += kSrCgBlock) {
      const double ap = fma(shift, p[k], y[k] * inv_world);
      y[k] = ap;
      acc = fma(p[k], ap, acc);
    }
    const double pap = block_sum<kSrCgBlock>(acc, sh);
    if (!(pap > 0.0)) {
      if (tid == 0) { sc[PYNQS_SR_PAP] = pap; sc[PYNQS_SR_DONE] = 1.0; sc[PYNQS_SR_BREAKDOWN] = 1.0; }
      return;
    }
    const double alpha = rho / pap;
    acc = 0.0;
    for (int64_t k = tid; k < np; k += kSrCgBlock) {
      d[k] = fma(alpha, p[k], d[k]);
      const double rk = fma(-alpha, y[k], r[k]);
      r[k] = rk;
      acc = fma(rk, rk, acc);
    }
    const double rho2 = block_sum<kSrCgBlock>(acc, sh);
    const double beta = rho2 / rho;
    for (int64_t k = tid; k < np; k += kSrCgBlock) p[k] = fma(beta, p[k], r[k]);
    if (tid == 0) {
      sc[PYNQS_SR_RHO] = rho2; sc[PYNQS_SR_PAP] = pap; sc[PYNQS_SR_ITER] += 1.0;
      if (rho2 <= tol * tol * rhs2) sc[PYNQS_SR_DONE] = 1.0;
    }
    return;
  }
  double acc = 0.0;
  for (int64_t k = tid; k < np; k += kSrCgBlock) {
    const double rk = rhs[k] - fma(shift, d[k], y[k] * inv_world);
    r[k] = rk;
    acc = fma(rk, rk, acc);
  }
  const double rr = block_sum<kSrCgBlock>(acc, sh);
  const bool ok = rr <= tol * tol * rhs2;
  if (!ok)
    for (int64_t k = tid; k < np; k += kSrCgBlock) p[k] = r[k];
  if (tid == 0) {
    sc[PYNQS_SR_TRUE2] = rr;
    sc[PYNQS_SR_CONVERGED] = ok ? 1.0 : 0.0;
    sc[PYNQS_SR_DONE] = ok ? 1.0 : 0.0;
    if (!ok) sc[PYNQS_SR_RHO] = rr;
  }
}

static inline bool sr_args_ok(int64_t n, int sorb, int H, int flavour) {
  return n >= 0 && n <= 0x7fffffffll * kSrWalkers && sorb >= 1 && sorb <= kMaxSorb && H >= 1 &&
         (flavour == PYNQS_RBM_REAL || flavour == PYNQS_RBM_COMPLEX);
}

}  // namespace pynqs

using namespace pynqs;

extern "C" int64_t pynqs_rbm_sr_workspace(int64_t n, int sorb, int nhidden, int flavour) {
  if (!sr_args_ok(n, sorb, nhidden, flavour)) return -1;
  const bool cplx = flavour == PYNQS_RBM_COMPLEX;
  const int64_t groups = (n + kSrWalkers - 1) / kSrWalkers;
  return (sr_table_doubles(n, nhidden, cplx) + groups * sr_nout(sorb, nhidden) * (cplx ? 2 : 1) + 2) * 8;
}

// JAS: the Jastrow-RBM (flavour real): VA + sorb = Z for the product, the jastrow block behind every vector
template <bool PREP, bool JAS = false>
static int sr_launch(const uint64_t *onv, int64_t n, int sorb, int H, int flavour, const double *A, const double *B, const double *VA,
                     const double *prob, void *workspace, const double *obar, double *flat, hipStream_t st, const char *what) {
  const bool cplx = flavour == PYNQS_RBM_COMPLEX;
  const int C = cplx ? 2 : 1;
  const int len = (sorb - 1) / 64 + 1;
  const int64_t nout = sr_nout(sorb, H) + (JAS ? jas_pair_count(sorb) : 0);
  const int64_t groups = (n + kSrWalkers - 1) / kSrWalkers, stride = nout * C;
  double *table = (double *)workspace;
  double *partial = table + sr_table_doubles(n, H, cplx);
  double *dot = partial + groups * stride;
  if (groups > 0) {
    if constexpr (!PREP) {
      const int64_t np = (int64_t)H * sorb + H + sorb + (JAS ? (int64_t)sorb * sorb : 0);
      if (cplx) hipLaunchKernelGGL((rbm_sr_dot_kernel<true>), dim3(1), dim3(kBlock), 0, st, obar, A, np, dot);  // (A = the whole flat z)
      else hipLaunchKernelGGL((rbm_sr_dot_kernel<false>), dim3(1), dim3(kBlock), 0, st, obar, A, np, dot);
    }
    if constexpr (JAS) {
      const double *Z = PREP ? nullptr : VA + sorb;
      const bool lds = !PREP && sr_jas_in_lds(sorb);
      const size_t dyn = lds ? (size_t)jas_pair_count(sorb) * 8 : 0;
#define PYNQS_SR(J)                                                                                                                       \
  do {                                                                                                                                    \
    auto kern = rbm_sr_partial_kernel<LEN, false, PREP, J>;                                                                               \
    /* above 64 KiB of LDS a kernel has to be told; the static arrays take 11 KiB of that */                                              \
    if (dyn > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) != hipSuccess) \
      return check_launch("hipFuncSetAttribute");                                                                                         \
    hipLaunchKernelGGL(kern, dim3((uint32_t)groups), dim3(kBlock), dyn, st, onv, n, sorb, H, A, B, VA, prob, table, dot, partial, stride, Z); \
  } while (0)
      DISPATCH_LEN(len, {
        if constexpr (PREP) PYNQS_SR(1);  // (no Z: only the jastrow block of Obar)
        else if (lds) PYNQS_SR(2);
        else PYNQS_SR(1);
      });
#undef PYNQS_SR
    } else {
#define PYNQS_SR(CP)                                                                                                                      \
  hipLaunchKernelGGL((rbm_sr_partial_kernel<LEN, CP, PREP>), dim3((uint32_t)groups), dim3(kBlock), 0, st, onv, n, sorb, H, A, B, VA, prob, table, \
                     dot, partial, stride, (const double *)nullptr)
      DISPATCH_LEN(len, {
        if (cplx) PYNQS_SR(true);
        else PYNQS_SR(false);
      });
#undef PYNQS_SR
    }
  }
  const uint32_t g2 = (uint32_t)((nout + 63) / 64);
  if constexpr (JAS) hipLaunchKernelGGL((rbm_sr_reduce_kernel<false, true>), dim3(g2), dim3(kBlock), 0, st, partial, stride, (int)groups, sorb, H, flat);
  else if (cplx) hipLaunchKernelGGL((rbm_sr_reduce_kernel<true>), dim3(g2), dim3(kBlock), 0, st, partial, stride, (int)groups, sorb, H, flat);
  else hipLaunchKernelGGL((rbm_sr_reduce_kernel<false>), dim3(g2), dim3(kBlock), 0, st, partial, stride, (int)groups, sorb, H, flat);
  return check_launch(what);
}

extern "C" int pynqs_rbm_sr_prepare(const uint64_t *onv, int64_t n, int sorb, const double *weights, const double *hidden_bias, int nhidden,
                                    int flavour, const double *prob, void *workspace, double *obar, void *stream) {
  pynqs::DeviceScope device_scope_(obar);
  if (!sr_args_ok(n, sorb, nhidden, flavour)) return set_error(PYNQS_EINVAL, "rbm_sr_prepare: bad n/sorb/nhidden/flavour");
  if (!weights || !hidden_bias || !obar || !workspace || (n > 0 && (!onv || !prob))) return set_error(PYNQS_EINVAL, "null pointer");
  return sr_launch<true>(onv, n, sorb, nhidden, flavour, weights, hidden_bias, nullptr, prob, workspace, nullptr, obar, (hipStream_t)stream,
                         "rbm_sr_prepare");
}

extern "C" int pynqs_rbm_sr_matvec(const uint64_t *onv, int64_t n, int sorb, int nhidden, int flavour, const double *prob, const void *workspace,
                                   const double *obar, const double *v, double *y, void *stream) {
  pynqs::DeviceScope device_scope_(y);
  if (!sr_args_ok(n, sorb, nhidden, flavour)) return set_error(PYNQS_EINVAL, "rbm_sr_matvec: bad n/sorb/nhidden/flavour");
  if (!obar || !v || !y || !workspace || (n > 0 && (!onv || !prob))) return set_error(PYNQS_EINVAL, "null pointer");
  const int64_t C = flavour == PYNQS_RBM_COMPLEX ? 2 : 1, nw = (int64_t)nhidden * sorb * C, nb = (int64_t)nhidden * C;
  return sr_launch<false>(onv, n, sorb, nhidden, flavour, v, v + nw, v + nw + nb, prob, (void *)workspace, obar, y, (hipStream_t)stream,
                          "rbm_sr_matvec");
}

extern "C" int pynqs_rbm_sr_cg_step(int mode, int64_t np, double *y, const double *rhs, double *d, double *r, double *p, double *scalars,
                                    double inv_world, double diag_shift, double tol, void *stream) {
  pynqs::DeviceScope device_scope_(scalars);
  if (mode < PYNQS_SR_CG_INIT || mode > PYNQS_SR_CG_RESIDUAL || np < 1) return set_error(PYNQS_EINVAL, "rbm_sr_cg_step: bad mode or length");
  if (!rhs || !d || !r || !p || !scalars || (mode != PYNQS_SR_CG_INIT && !y)) return set_error(PYNQS_EINVAL, "null pointer");
  hipLaunchKernelGGL(rbm_sr_cg_kernel, dim3(1), dim3(kSrCgBlock), 0, (hipStream_t)stream, mode, np, y, rhs, d, r, p, scalars, inv_world,
                     diag_shift, tol);
  return check_launch("rbm_sr_cg_step");
}

// ---- the Jastrow-RBM: the same kernels with JAS, the jastrow block [sorb][sorb] behind every vector
extern "C" int64_t pynqs_jrbm_sr_workspace(int64_t n, int sorb, int nhidden) {
  if (!sr_args_ok(n, sorb, nhidden, PYNQS_RBM_REAL)) return -1;
  const int64_t groups = (n + kSrWalkers - 1) / kSrWalkers;
  return (sr_table_doubles(n, nhidden, false) + groups * (sr_nout(sorb, nhidden) + jas_pair_count(sorb)) + 2) * 8;
}

extern "C" int pynqs_jrbm_sr_prepare(const uint64_t *onv, int64_t n, int sorb, const double *weights, const double *hidden_bias, int nhidden,
                                     const double *prob, void *workspace, double *obar, void *stream) {
  pynqs::DeviceScope device_scope_(obar);
  if (!sr_args_ok(n, sorb, nhidden, PYNQS_RBM_REAL)) return set_error(PYNQS_EINVAL, "jrbm_sr_prepare: bad n/sorb/nhidden");
  if (!weights || !hidden_bias || !obar || !workspace || (n > 0 && (!onv || !prob))) return set_error(PYNQS_EINVAL, "null pointer");
  return sr_launch<true, true>(onv, n, sorb, nhidden, PYNQS_RBM_REAL, weights, hidden_bias, nullptr, prob, workspace, nullptr, obar,
                               (hipStream_t)stream, "jrbm_sr_prepare");
}

extern "C" int pynqs_jrbm_sr_matvec(const uint64_t *onv, int64_t n, int sorb, int nhidden, const double *prob, const void *workspace,
                                    const double *obar, const double *v, double *y, void *stream) {
  pynqs::DeviceScope device_scope_(y);
  if (!sr_args_ok(n, sorb, nhidden, PYNQS_RBM_REAL)) return set_error(PYNQS_EINVAL, "jrbm_sr_matvec: bad n/sorb/nhidden");
  if (!obar || !v || !y || !workspace || (n > 0 && (!onv || !prob))) return set_error(PYNQS_EINVAL, "null pointer");
  const int64_t nw = (int64_t)nhidden * sorb, nb = nhidden;
  return sr_launch<false, true>(onv, n, sorb, nhidden, PYNQS_RBM_REAL, v, v + nw, v + nw + nb, prob, (void *)workspace, obar, y,
                                (hipStream_t)stream, "jrbm_sr_matvec");
}
