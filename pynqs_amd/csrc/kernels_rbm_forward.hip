// kernels_rbm_forward.hip -- psi(x) of the reference's RBM amplitudes (vmc/ansatz/rbm/rbm.py:186-211) on a LIST of determinants, straight
// from the packed bits: the amplitude forward of the REDUCE local energy (vmc/energy/eloc.py:299-303, flip.py:44-50: `Func` on the distinct
// x') when the ansatz is an RBM.
//
// The PyTorch module does theta = X W^T as a GEMM on the +-1 matrix X [n, sorb] and then ~15 element-wise kernels on [n, H] arrays: for the
// 1.5 M distinct x' of 8192 Fe2S2 walkers that is a 1 GB theta array read and written a dozen times (3.5 ms per step, 70 % of the REDUCE
// step).  Here one lane owns one determinant and never leaves registers: x_o = +-1, so theta_h = b_h + sum_o (+-W_ho) is sorb fused
// multiply-adds per hidden unit with W_ho wave-uniform (scalar loads, no LDS, no bank conflicts), eight hidden units at a time; then
// ln 2cosh(theta_h) is summed and psi = exp(a.x + sum) written: 8 or 16 bytes of output per determinant, 8 len bytes of input.
//   real parameters :  psi = exp(a.x) prod_h 2cosh(theta_h)         (flavour REAL)
//                      psi = tanh(a.x) prod_h 2cosh(theta_h)        (TANH)
//                      psi = exp(i (a.x + sum_h ln 2cosh(theta_h))) (PHASE, complex output)
//   complex parameters (re, im pairs):  psi = exp(a.x) prod_h 2cosh(theta_h), complex output (PYNQS_RBM_COMPLEX)
// The product prod_h 2cosh(theta_h) is formed as a product, not as exp(sum ln ...): 2cosh t = e^|t| (1 + e^{-2|t|}) keeps the large
// factor as an exponent that is summed, and the bounded factors (1 + e^{-2|t|}) in (1, 2] -- complex: (1 + rho cos phi) + i rho sin phi,
// modulus in [0, 2] -- are multiplied up and renormalised by a power of two every eight hidden units, so nothing overflows or
// underflows for any theta.  One exp (+ one sincos) per hidden unit instead of exp + log (+ sincos + atan2): 0.98 -> 0.5 ms per
// 1.6 M determinants with 40 complex hidden units.
#include "detcore.h"
#include "launch.h"
#include "rbm_math.h"

namespace pynqs {

constexpr int kHChunk = 8;

// running product of the bounded factors with its binary exponent split off (renormalised by the caller every few factors)
struct Prod {
  double re = 1.0, im = 0.0;  // mantissa
  double lin = 0.0, ang = 0.0;  // sum of the |Re theta| (natural-log scale of the modulus) and of the s * Im theta (phase)
  int e2 = 0;
  __device__ __forceinline__ void renorm() {
    int k;
    (void)frexp(fmax(fabs(re), fabs(im)), &k);
    re = ldexp(re, -k); im = ldexp(im, -k);
    e2 += k;
  }
  // false once a factor or the product left the range of a double (inf, or the nan of inf - inf / inf * 0): it stays that way
  __device__ __forceinline__ bool finite() const { return fabs(re) < __builtin_inf() && fabs(im) < __builtin_inf(); }
  // *= 2cosh(x + iy) = e^{s(x + iy)} (1 + e^{-2s(x + iy)}),  s = sign(x)
  template <bool CPLX>
  __device__ __forceinline__ void times_2cosh(double x, double y) {
    const double ax = fabs(x);
    const double rho = exp(-2.0 * ax);
    lin += ax;
    if constexpr (CPLX) {
      const double sy = x < 0.0 ? -y : y;
      double sn, cs;
      sincos_mod(-2.0 * sy, sn, cs);
      const double u = fma(rho, cs, 1.0), v = rho * sn;
      const double nr = re * u - im * v;
      im = fma(re, v, im * u);
      re = nr;
      ang += sy;
    } else {
      re *= 1.0 + rho;
    }
  }
};

// psi from the product of the hidden units' factors and a.x = axr + i axi.  Contraction is off in here and the two fused multiply-adds are
// written out: which product a compiler contracts with which sum depends on the code around the call (ln 2 e2 is one such product), and
// the kernels that share this function must share its bits
template <int FLAVOUR>
__device__ __forceinline__ void write_psi(double *__restrict__ psi, int64_t i, const Prod &P, double axr, double axi) {
#pragma clang fp contract(off)
  const double kLn2 = 0.693147180559945309417;
  if constexpr (FLAVOUR == PYNQS_RBM_REAL) {
    psi[i] = P.re * exp(axr + P.lin + kLn2 * (double)P.e2);
  } else if constexpr (FLAVOUR == PYNQS_RBM_TANH) {
    psi[i] = tanh(axr) * P.re * exp(P.lin + kLn2 * (double)P.e2);
  } else if constexpr (FLAVOUR == PYNQS_RBM_PHASE) {
    double sn, cs;
    sincos(axr + P.lin + log(P.re) + kLn2 * (double)P.e2, &sn, &cs);  // (the phase IS the logarithm of the real flavour's amplitude)
    psi[2 * i] = cs; psi[2 * i + 1] = sn;
  } else {
    const double m = exp(axr + P.lin + kLn2 * (double)P.e2);
    double sn, cs;
    sincos(axi + P.ang, &sn, &cs);
    psi[2 * i] = m * fma(P.re, cs, -(P.im * sn));
    psi[2 * i + 1] = m * fma(P.re, sn, P.im * cs);
  }
}

// psi of one determinant from scratch (every lane of the wave takes part: the parameter loads are wave-uniform scalar loads)
template <int LEN, int FLAVOUR>
__device__ __forceinline__ void rbm_forward_row(const uint64_t (&ket)[LEN], int sorb, int H, const double *__restrict__ W,
                                                const double *__restrict__ hb, const double *__restrict__ vb, Prod &P, double &axr, double &axi) {
  constexpr bool CPLX = FLAVOUR == PYNQS_RBM_COMPLEX;
  for (int h0 = 0; h0 < H; h0 += kHChunk) {
    double tr[kHChunk], ti[kHChunk];
#pragma unroll
    for (int j = 0; j < kHChunk; ++j) {
      const int h = min(h0 + j, H - 1);
      tr[j] = CPLX ? hb[2 * h] : hb[h];
      ti[j] = CPLX ? hb[2 * h + 1] : 0.0;
    }
    for (int o = 0; o < sorb; ++o) {
      const double x = pm1_of<LEN>(ket, o);
#pragma unroll
      for (int j = 0; j < kHChunk; ++j) {
        const int h = min(h0 + j, H - 1);  // (wave-uniform address: a scalar load)
        if constexpr (CPLX) {
          tr[j] = fma(x, W[((size_t)h * sorb + o) * 2], tr[j]);
          ti[j] = fma(x, W[((size_t)h * sorb + o) * 2 + 1], ti[j]);
        } else {
          tr[j] = fma(x, W[(size_t)h * sorb + o], tr[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kHChunk; ++j)
      if (h0 + j < H) P.template times_2cosh<CPLX>(tr[j], ti[j]);
    P.renorm();
  }
  axr = 0.0; axi = 0.0;
  if (vb) {
    for (int o = 0; o < sorb; ++o) {
      const double x = pm1_of<LEN>(ket, o);
      if constexpr (CPLX) { axr = fma(x, vb[2 * o], axr); axi = fma(x, vb[2 * o + 1], axi); }
      else axr = fma(x, vb[o], axr);
    }
  }
}

template <int LEN, int FLAVOUR>
__global__ __launch_bounds__(kBlock) void rbm_forward_kernel(const uint64_t *__restrict__ onv, int64_t n, int sorb, int H,
                                                             const double *__restrict__ W, const double *__restrict__ hb,
                                                             const double *__restrict__ vb, double *__restrict__ psi) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t row = i < n ? i : n - 1;  // (idle lanes repeat the last determinant: the parameter loads must stay wave-uniform)
  uint64_t ket[LEN];
#pragma unroll
  for (int w = 0; w < LEN; ++w) ket[w] = onv[row * LEN + w];
  Prod P;  // prod_h 2cosh(theta_h) = exp(P.lin + i P.ang) * (P.re + i P.im) * 2^P.e2
  double axr, axi;
  rbm_forward_row<LEN, FLAVOUR>(ket, sorb, H, W, hb, vb, P, axr, axi);
  if (i >= n) return;
  write_psi<FLAVOUR>(psi, i, P, axr, axi);
}

// The real flavour times the two-body Jastrow factor exp(x^T M x) (vmc/ansatz/rbm/rbm_other.py, class Jastrow; M [sorb][sorb], any real
// matrix), from scratch like the kernel above: x^T M x = sum_i x_i (sum_j M_ij x_j), the rows summed one by one (M_ij wave-uniform: scalar
// loads) -- sorb^2 fused multiply-adds per determinant next to the sorb x H of theta, at most 2 sorb - 2 of them rounding on sum |M_ij|.
template <int LEN>
__global__ __launch_bounds__(kBlock) void jrbm_forward_kernel(const uint64_t *__restrict__ onv, int64_t n, int sorb, int H,
                                                              const double *__restrict__ W, const double *__restrict__ hb,
                                                              const double *__restrict__ vb, const double *__restrict__ M,
                                                              double *__restrict__ psi) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t row = i < n ? i : n - 1;  // (idle lanes repeat the last determinant)
  uint64_t ket[LEN];
#pragma unroll
  for (int w = 0; w < LEN; ++w) ket[w] = onv[row * LEN + w];
  Prod P;
  double axr, axi;
  rbm_forward_row<LEN, PYNQS_RBM_REAL>(ket, sorb, H, W, hb, vb, P, axr, axi);
  double xmx = 0.0;
  for (int a = 0; a < sorb; ++a) {
    double r = 0.0;
    for (int b = 0; b < sorb; ++b) r = fma(pm1_of<LEN>(ket, b), M[(size_t)a * sorb + b], r);
    xmx = fma(pm1_of<LEN>(ket, a), r, xmx);
  }
  if (i >= n) return;
  write_psi<PYNQS_RBM_REAL>(psi, i, P, axr + xmx, axi);
}

// ---- psi on the distinct x' of a REDUCE front end, each from its parent walker -----------------------------------------------------
// x' = x with <= 4 orbitals flipped, and   prod_h 2cosh(theta_h) = exp(sum_h theta_h) prod_h (1 + q_h),   q_h = exp(-2 theta_h).
// Flipping orbital o to x'_o = +-1 changes theta_h by +-2 W_ho:  q_h *= exp(-+4 W_ho),  sum_h theta_h += +-2 sum_h W_ho,  a.x += +-2 a_o.
// So a child costs, per hidden unit, 4 (complex) multiplications by table entries and one by (1 + q): no exponential, no sine, no loop over
// the orbitals.  The table (caller-owned, pynqs_rbm_children_table_bytes) holds
//   parents [nwalkers][H + 2] : q_h(x) for h < H, then sum_h theta_h(x), then a.x
//   factors [2 sorb + 1][HP]  : row 2 o (x'_o = +1) / 2 o + 1 (x'_o = -1): exp(-+4 W_ho) for h < H, +-2 sum_h W_ho, +-2 a_o;
//                               the last row (1, ..., 1, 0, 0) stands for "no flip"; HP = H + 2 made odd (rows start in different banks)
//   flag    one double after the factors, raised if some parent has Re theta_h < -340, where q_h = exp(-2 theta_h) leaves the range of a
//           double: the children kernel then computes every row from scratch (rbm_forward_row, the plain kernel's body).  Raised means
//           non-zero for the two-launch prepare (which resets it), equal to the call's stamp for the one-launch prepare (which cannot)
// all entries real or (re, im) by the flavour.
// The factors 1 + q_h are NOT bounded for negative theta_h (the plain forward's are: it uses |theta_h|): q_h = e^100 for theta_h = -50, and
// eight such factors between two renorm() calls, or one q_h beyond e^709 after four flips, overflow although psi itself is an ordinary
// number.  An overflow cannot pass unseen -- inf and nan survive every later multiplication -- so both kernels look at the finished
// product once (Prod::finite) and compute a row whose product is not finite from scratch, as they do for strangers; the inner loops are
// as they were.  What could lose digits without overflowing is an UNDERFLOW on the way from q_h(parent) to q_h(child) followed by a large
// factor; with |4 W_ho| <= 80 (factors within e^+-80) every intermediate of a q_h(child) >= 1e-17 is a normal number, and an entry with
// |4 Re W_ho| > 80 is stored as nan: a child that flips such an orbital gets a nan product and goes the same way.
__host__ __device__ inline int children_hp(int H) { return (H + 2) | 1; }

// (re, im) = sum_k W_ko, k ascending: the factor table's entry H before its factor +-2, and what the sums blocks of the one-launch prepare
// kernel form again for themselves (the same loop: the same bits)
template <bool CPLX>
__device__ __forceinline__ void sum_w_column(const double *__restrict__ W, int sorb, int H, int o, double &re, double &im) {
  constexpr int C = CPLX ? 2 : 1;
  re = 0.0; im = 0.0;
#pragma unroll 16
  for (int k = 0; k < H; ++k) {  // (independent loads: 16 in flight)
    re += W[((size_t)k * sorb + o) * C];
    if constexpr (CPLX) im += W[((size_t)k * sorb + o) * C + 1];
  }
}

// entry idx of the factor table
template <bool CPLX>
__device__ __forceinline__ void children_factor_entry(int idx, int sorb, int H, const double *__restrict__ W, const double *__restrict__ vb,
                                                      double *__restrict__ factors) {
  constexpr int C = CPLX ? 2 : 1;
  const int HP = children_hp(H);
  if (idx >= (2 * sorb + 1) * HP) return;
  const int row = idx / HP, h = idx - row * HP, o = row >> 1;
  const double sign = (row & 1) ? -1.0 : 1.0;  // x'_o
  double re = 0.0, im = 0.0;
  if (row == 2 * sorb) {
    re = h < H ? 1.0 : 0.0;
  } else if (h < H) {
    const double wr = W[((size_t)h * sorb + o) * C], wi = CPLX ? W[((size_t)h * sorb + o) * C + 1] : 0.0;
    const double m = fabs(4.0 * wr) <= 80.0 ? exp(-4.0 * sign * wr) : __builtin_nan("");  // (nan: see above; also for a nan weight)
    if constexpr (CPLX) {
      double sn, cs;
      sincos(-4.0 * sign * wi, &sn, &cs);
      re = m * cs; im = m * sn;
    } else {
      re = m;
    }
  } else if (h == H) {
    sum_w_column<CPLX>(W, sorb, H, o, re, im);
    re *= 2.0 * sign; im *= 2.0 * sign;
  } else if (h == H + 1 && vb) {
    re = 2.0 * sign * vb[(size_t)o * C];
    if constexpr (CPLX) im = 2.0 * sign * vb[(size_t)o * C + 1];
  }
  factors[(size_t)idx * C] = re;
  if constexpr (CPLX) factors[(size_t)idx * C + 1] = im;
}

template <bool CPLX>
__global__ __launch_bounds__(kBlock) void rbm_children_factors_kernel(int sorb, int H, const double *__restrict__ W, const double *__restrict__ vb,
                                                                      double *__restrict__ factors) {
  constexpr int C = CPLX ? 2 : 1;
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx == 0) factors[(size_t)(2 * sorb + 1) * children_hp(H) * C] = 0.0;  // the flag (the parents kernel, launched next, may raise it)
  children_factor_entry<CPLX>(idx, sorb, H, W, vb, factors);
}

constexpr int kParentChunk = 4;

// q_h of walker `row` for the hidden units h0 .. h0 + kParentChunk - 1; a theta_h out of range stores `raised` in the flag word
template <int LEN, bool CPLX>
__device__ __forceinline__ void children_parent_chunk(const uint64_t (&ket)[LEN], bool live, int h0, int sorb, int H, const double *__restrict__ W,
                                                      const double *__restrict__ hb, double *__restrict__ flag, double raised,
                                                      double *__restrict__ out) {
  constexpr int C = CPLX ? 2 : 1;
  double tr[kParentChunk], ti[kParentChunk];
#pragma unroll
  for (int j = 0; j < kParentChunk; ++j) {
    const int h = min(h0 + j, H - 1);
    tr[j] = CPLX ? hb[2 * h] : hb[h];
    ti[j] = CPLX ? hb[2 * h + 1] : 0.0;
  }
  for (int o = 0; o < sorb; ++o) {
    const double x = pm1_of<LEN>(ket, o);
#pragma unroll
    for (int j = 0; j < kParentChunk; ++j) {
      const int h = min(h0 + j, H - 1);  // (wave-uniform address: a scalar load)
      tr[j] = fma(x, W[((size_t)h * sorb + o) * C], tr[j]);
      if constexpr (CPLX) ti[j] = fma(x, W[((size_t)h * sorb + o) * C + 1], ti[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < kParentChunk; ++j) {
    if (h0 + j < H && live) {
      if (!(tr[j] > -340.0)) *flag = raised;  // (also for nan)
      const double m = exp(-2.0 * tr[j]);
      if constexpr (CPLX) {
        double sn, cs;
        sincos_mod(-2.0 * ti[j], sn, cs);
        out[(size_t)(h0 + j) * 2] = m * cs;
        out[(size_t)(h0 + j) * 2 + 1] = m * sn;
      } else {
        out[h0 + j] = m;
      }
    }
  }
}

// sum_h theta_h = sum_h b_h + sum_o x_o sum_h W_ho and a.x of walker `row`: f + o fstride holds (2 sum_h W_ho, 2 a_o) as C doubles each
// (rows 2 o of the factor table from their entry H on, or a copy of just these)
template <int LEN, bool CPLX>
__device__ __forceinline__ void children_parent_sums(const uint64_t (&ket)[LEN], bool live, int sorb, int H, const double *__restrict__ hb,
                                                     const double *__restrict__ f, size_t fstride, double *__restrict__ out) {
  constexpr int C = CPLX ? 2 : 1;
  double sr = 0.0, si = 0.0, axr = 0.0, axi = 0.0;
  for (int h = 0; h < H; ++h) {
    sr += hb[(size_t)h * C];
    if constexpr (CPLX) si += hb[(size_t)h * C + 1];
  }
  for (int o = 0; o < sorb; ++o) {
    const double x = pm1_of<LEN>(ket, o);
    const double *__restrict__ fo = f + (size_t)o * fstride;  // (wave-uniform addresses)
    sr = fma(0.5 * x, fo[0], sr);
    axr = fma(0.5 * x, fo[C], axr);
    if constexpr (CPLX) { si = fma(0.5 * x, fo[1], si); axi = fma(0.5 * x, fo[C + 1], axi); }
  }
  if (!live) return;
  out[(size_t)H * C] = sr;
  out[(size_t)(H + 1) * C] = axr;
  if constexpr (CPLX) { out[(size_t)H * C + 1] = si; out[(size_t)(H + 1) * C + 1] = axi; }
}

// The two-launch form (pynqs_rbm_children_prepare): one lane per (walker, chunk of kParentChunk = 4 hidden units): blockIdx.y is the chunk, so
// that W_ho stays wave-uniform and 8192 walkers are 10 x 128 waves, not 128 (80 -> 28 us with chunks of 8 -> 17 us for Fe2S2).  Chunk 0 also
// leaves sum_h theta_h = sum_h b_h + sum_o x_o sum_h W_ho (from the factor table's sum_h W_ho, built by the launch before this one) and a.x.
template <int LEN, bool CPLX>
__global__ __launch_bounds__(kBlock) void rbm_children_parents_kernel(const uint64_t *__restrict__ onv, int64_t n, int sorb, int H,
                                                                      const double *__restrict__ W, const double *__restrict__ hb,
                                                                      const double *__restrict__ vb, const double *__restrict__ factors,
                                                                      double *__restrict__ table) {
  constexpr int C = CPLX ? 2 : 1;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t row = i < n ? i : n - 1;
  uint64_t ket[LEN];
#pragma unroll
  for (int w = 0; w < LEN; ++w) ket[w] = onv[row * LEN + w];
  double *__restrict__ out = table + (size_t)row * (size_t)(H + 2) * C;
  const int HP = children_hp(H);
  children_parent_chunk<LEN, CPLX>(ket, i < n, (int)blockIdx.y * kParentChunk, sorb, H, W, hb,
                                   const_cast<double *>(factors) + (size_t)(2 * sorb + 1) * HP * C, 1.0, out);
  if (blockIdx.y != 0) return;
  // rows 2 o of the factor table: entry H = +2 sum_h W_ho, entry H + 1 = +2 a_o
  children_parent_sums<LEN, CPLX>(ket, i < n, sorb, H, hb, factors + (size_t)H * C, (size_t)2 * HP * C, out);
}

// The one-launch form (pynqs_rbm_children_prepare_stamped): the same table, bit for bit, from one grid with three kinds of block --
//   blockIdx.y <  nchunks      parent chunks as above, without chunk 0's extra sums (they were the critical path of the launch)
//   blockIdx.y == nchunks      sums blocks: sum_h theta_h and a.x per walker; what they need of the factor table -- 2 sum_h W_ho, 2 a_o --
//                              they form in LDS themselves, in the factor kernel's order of additions (sorb x H loads from the L2 per block)
//   blockIdx.y == nchunks + 1  factor blocks: the parameters' factor table
// (blockIdx.x beyond a kind's count: nothing to do).  Nothing in the launch depends on anything else in it, so the flag cannot be "reset,
// then maybe raised": a parent out of range stores this call's STAMP instead, and the children kernel compares the word with its own.
template <int LEN, bool CPLX>
__global__ __launch_bounds__(kBlock) void rbm_children_prepare_kernel(const uint64_t *__restrict__ onv, int64_t n, int sorb, int H,
                                                                      const double *__restrict__ W, const double *__restrict__ hb,
                                                                      const double *__restrict__ vb, double *__restrict__ factors,
                                                                      double *__restrict__ table, int nchunks, double stamp) {
  constexpr int C = CPLX ? 2 : 1;
  __shared__ double fs[kMaxSorb][2][C];  // the sums blocks' (2 sum_h W_ho, 2 a_o)
  if ((int)blockIdx.y == nchunks + 1) {
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx < (int64_t)(2 * sorb + 1) * children_hp(H)) children_factor_entry<CPLX>((int)idx, sorb, H, W, vb, factors);
    return;
  }
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if ((int64_t)blockIdx.x * kBlock >= n) return;  // (the whole block)
  const int64_t row = i < n ? i : n - 1;
  uint64_t ket[LEN];
#pragma unroll
  for (int w = 0; w < LEN; ++w) ket[w] = onv[row * LEN + w];
  double *__restrict__ out = table + (size_t)row * (size_t)(H + 2) * C;
  if ((int)blockIdx.y < nchunks) {
    children_parent_chunk<LEN, CPLX>(ket, i < n, (int)blockIdx.y * kParentChunk, sorb, H, W, hb,
                                     factors + (size_t)(2 * sorb + 1) * children_hp(H) * C, stamp, out);
    return;
  }
  for (int o = threadIdx.x; o < sorb; o += kBlock) {
    double re, im;
    sum_w_column<CPLX>(W, sorb, H, o, re, im);
    fs[o][0][0] = re * 2.0;  // (the table's row 2 o: sign +1)
    fs[o][1][0] = vb ? 2.0 * vb[(size_t)o * C] : 0.0;
    if constexpr (CPLX) {
      fs[o][0][1] = im * 2.0;
      fs[o][1][1] = vb ? 2.0 * vb[(size_t)o * C + 1] : 0.0;
    }
  }
  __syncthreads();
  children_parent_sums<LEN, CPLX>(ket, i < n, sorb, H, hb, &fs[0][0][0], (size_t)2 * C, out);
}

// what the children kernels make of the flag word: a stamped call (stamp != 0) takes the word for raised only if it holds its own stamp --
// a stale stamp of an earlier call into the same buffer or the garbage of a fresh one is "not raised", and garbage that happens to equal
// the stamp sends the call down the from-scratch path, which is correct for every input; the unstamped pair resets the word to 0 itself
__device__ __forceinline__ bool children_flag_raised(double word, double stamp) { return stamp != 0.0 ? word == stamp : word != 0.0; }

#ifndef PYNQS_CHILD_BLOCK
#define PYNQS_CHILD_BLOCK 1024
#endif
constexpr int kChildBlock = PYNQS_CHILD_BLOCK;  // the factor table (up to 64 KB of LDS) is shared by the workgroup's waves: large workgroups, more waves per CU
constexpr int kChildWaveRows = 16;            // the wave form: consecutive rows a wave takes at a time
#ifndef PYNQS_CHILD_MAX_BLOCKS
#define PYNQS_CHILD_MAX_BLOCKS 256
#endif
// the LDS form's grid: a workgroup copies the factor table once and strides over the rows.  One workgroup per CU of an MI355X (its 16 waves are
// all the registers of the chunked schedule allow on a CU); measured at 256, 512 and 1024 (profiles/children_chunked_trace.txt)
constexpr int64_t kChildMaxBlocks = PYNQS_CHILD_MAX_BLOCKS;
constexpr int64_t kChildMaxWaveBlocks = 256 * 32;  // the wave form's grid

// The arithmetic of one hidden unit of a child, shared by the two schedules of the LDS kernel below.  Every fused multiply-add is an fma()
// and every product that is left (__dmul_rn: a plain product here) feeds an fma or another product, never a sum, so floating-point
// contraction finds nothing to fuse differently in one schedule than in the other: the sequence is the one the compiler chose for the
// per-unit loop before the schedules were two.
//   q *= f  (slots 0..2, and slot 3 with complex parameters)
template <bool CPLX>
__device__ __forceinline__ void children_times_factor(double &qr, double &qi, double fr, double fi) {
  if constexpr (CPLX) {
    const double t = __dmul_rn(qi, fi);
    const double nr = fma(qr, fr, -t);
    qi = fma(qr, fi, __dmul_rn(qi, fr));
    qr = nr;
  } else {
    qr = __dmul_rn(qr, fr);
  }
}
//   the last slot and P *= 1 + q  (real parameters: 1 + q f is ONE fma)
template <bool CPLX>
__device__ __forceinline__ void children_times_one_plus(Prod &P, double qr, double qi, double fr, double fi) {
  if constexpr (CPLX) {
    children_times_factor<true>(qr, qi, fr, fi);
    const double u = __dadd_rn(qr, 1.0);
    const double t = __dmul_rn(P.im, qi);
    const double nr = fma(P.re, u, -t);
    P.im = fma(P.re, qi, __dmul_rn(P.im, u));
    P.re = nr;
  } else {
    P.re = __dmul_rn(P.re, fma(qr, fr, 1.0));
  }
}

constexpr int kChildGroupCplx = 4;  // complex parameters: factors of a slot read at a time (8: the kernel spills; real parameters take all 8)
// q_h of the parent's row tp for the kHChunk hidden units from h0 on (all of them below H: the caller's business), kept as the table has
// them, re next to im: a 16-byte load lands where it is used
template <bool CPLX>
struct ChildQ {
  double v[kHChunk][CPLX ? 2 : 1];
};
template <bool CPLX>
__device__ __forceinline__ void children_load_q(const double *__restrict__ tp, int h0, ChildQ<CPLX> &q) {
  constexpr int C = CPLX ? 2 : 1;
#pragma unroll
  for (int j = 0; j < kHChunk; ++j)
#pragma unroll
    for (int c = 0; c < C; ++c) q.v[j][c] = tp[(size_t)(h0 + j) * C + c];
}

// one full chunk of the chunked schedule: the factors of a slot are read for all kHChunk units (consecutive LDS words per lane), the kHChunk
// chains advance side by side, and the last slot feeds P in ascending h; renorm() as after every chunk
template <bool CPLX>
__device__ __forceinline__ void children_chunk(Prod &P, ChildQ<CPLX> &q, const double *__restrict__ wl, const int (&at)[4], int h0) {
  constexpr int C = CPLX ? 2 : 1;
  constexpr int G = CPLX ? kChildGroupCplx : kHChunk;  // factors read at a time
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int g = 0; g < kHChunk; g += G) {
      double f[G][C];
#pragma unroll
      for (int j = 0; j < G; ++j)
#pragma unroll
        for (int c = 0; c < C; ++c) f[j][c] = wl[(size_t)(at[s] + h0 + g + j) * C + c];
#pragma unroll
      for (int j = 0; j < G; ++j) {
        double zero = 0.0;
        double &qi = CPLX ? q.v[g + j][C - 1] : zero;
        const double fi = CPLX ? f[j][C - 1] : 0.0;
        if (s < 3) children_times_factor<CPLX>(q.v[g + j][0], qi, f[j][0], fi);
        else children_times_one_plus<CPLX>(P, q.v[g + j][0], qi, f[j][0], fi);
      }
    }
  }
  P.renorm();
}

// the from-scratch evaluation of the LDS kernel's rare paths (the raised flag, a wave with a stranger)
template <int LEN, int FLAVOUR>
__device__ __forceinline__ void children_row_from_scratch(const uint64_t *__restrict__ onv, int64_t row, int sorb, int H,
                                                       const double *__restrict__ W, const double *__restrict__ hb,
                                                       const double *__restrict__ vb, Prod &P, double &axr, double &axi) {
  uint64_t ket[LEN];
#pragma unroll
  for (int w = 0; w < LEN; ++w) ket[w] = onv[row * LEN + w];
  P = Prod();
  rbm_forward_row<LEN, FLAVOUR>(ket, sorb, H, W, hb, vb, P, axr, axi);
}

// Row i of the LDS kernel from its parent's row of the table and the factor table wl in LDS: P and a.x, and whether the row has to be
// computed from scratch instead (a stranger, or a product that left the range of a double).
// FORM 0 (PYNQS_CHILDREN_CHUNKED): kHChunk hidden units at a time -- their q_h(parent) loaded together, the factors read a slot at a time
// for the chunk, eight q_h chains side by side, P *= 1 + q_h in ascending h; the H % kHChunk units left over one by one.  With REAL / TANH /
// PHASE parameters the next chunk's q_h are requested into a second buffer before this chunk's arithmetic.  With COMPLEX parameters they
// are NOT: two chunks of q_h (64 registers) next to the factors and the row's own state do not fit the 128 registers of a 1024-thread
// workgroup -- built that way the kernel spilled 32 of them and ran slower than form 1 (115 against 103 us on the flagship; 91 us as it is,
// at the same grid: DESIGN 8, "The children kernel") -- so a chunk's eight loads go out together and the CU's other waves cover their one
// round trip.  FORM 1 (PYNQS_CHILDREN_PER_UNIT): one hidden unit after the other, each waiting for its own loads (the schedule before there
// were two).  The same operations on the same operands in the same order: the same bits.
template <int LEN, bool CPLX, int FORM>
__device__ __forceinline__ bool children_row_from_table(const uint64_t *__restrict__ onv, int64_t i, const int32_t *__restrict__ parent,
                                                        const uint64_t *__restrict__ walkers, int64_t nwalkers,
                                                        const double *__restrict__ table, const double *__restrict__ wl, int sorb, int H,
                                                        Prod &P, double &axr, double &axi) {
  constexpr int C = CPLX ? 2 : 1;
  const int HP = children_hp(H);
  int64_t p = parent[i];
  // a row that is NOT its parent with at most four orbitals flipped (a parent index out of range, a row the caller put there itself) is
  // computed from scratch instead of being truncated to four flips silently
  bool stranger = p < 0 || p >= nwalkers;
  p = stranger ? 0 : p;
  const double *__restrict__ tp = table + (size_t)p * (size_t)(H + 2) * C;
  constexpr bool kChunked = FORM == PYNQS_CHILDREN_CHUNKED;
  const int hfull = kChunked ? H - H % kHChunk : 0;  // hidden units the chunked schedule takes
  // the first chunk is requested as soon as the parent is known, ahead of the comparison with the parent's determinant
  ChildQ<CPLX> qa;
  if (hfull > 0) children_load_q<CPLX>(tp, 0, qa);
  // the rows of the factor table for the flipped orbitals ("no flip" for the unused slots)
  int at[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) at[q] = 2 * sorb * HP;
  int k = 0, nflip = 0;
#pragma unroll
  for (int w = 0; w < LEN; ++w) {
    const uint64_t xc = onv[i * LEN + w];
    uint64_t d = xc ^ walkers[p * LEN + w];
    nflip += __popcll(d);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (d && k < 4) {
        const int b = __builtin_ctzll(d);
        d &= d - 1;
        const int r = (2 * (64 * w + b) + (((xc >> b) & 1ull) ? 0 : 1)) * HP;
        // (k is a small per-lane counter: the slots are selected, not indexed)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q == k) at[q] = r;
        ++k;
      }
    }
  }
  P = Prod();
  if constexpr (!CPLX) {
    // two buffers taking turns (no copy between them): while one chunk is worked on, the next one's q_h are on their way into the other
    ChildQ<CPLX> qb;
    for (int h0 = 0; h0 < hfull; h0 += 2 * kHChunk) {
      if (h0 + kHChunk < hfull) children_load_q<CPLX>(tp, h0 + kHChunk, qb);
      children_chunk<CPLX>(P, qa, wl, at, h0);
      if (h0 + kHChunk >= hfull) break;
      if (h0 + 2 * kHChunk < hfull) children_load_q<CPLX>(tp, h0 + 2 * kHChunk, qa);
      children_chunk<CPLX>(P, qb, wl, at, h0 + kHChunk);
    }
  } else {
    for (int h0 = 0; h0 < hfull; h0 += kHChunk) {
      if (h0 > 0) children_load_q<CPLX>(tp, h0, qa);
      children_chunk<CPLX>(P, qa, wl, at, h0);
    }
  }
  for (int h0 = hfull; h0 < H; h0 += kHChunk) {
#pragma unroll
    for (int j = 0; j < kHChunk; ++j) {
      const int h = h0 + j;
      if (h < H) {
        double qr = tp[(size_t)h * C], qi = CPLX ? tp[(size_t)h * C + 1] : 0.0;
#pragma unroll
        for (int q = 0; q < 3; ++q)
          children_times_factor<CPLX>(qr, qi, wl[(size_t)(at[q] + h) * C], CPLX ? wl[(size_t)(at[q] + h) * C + 1] : 0.0);
        children_times_one_plus<CPLX>(P, qr, qi, wl[(size_t)(at[3] + h) * C], CPLX ? wl[(size_t)(at[3] + h) * C + 1] : 0.0);
      }
    }
    P.renorm();
  }
  axr = tp[(size_t)(H + 1) * C];
  axi = CPLX ? tp[(size_t)(H + 1) * C + 1] : 0.0;
  P.lin = tp[(size_t)H * C];
  P.ang = CPLX ? tp[(size_t)H * C + 1] : 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    P.lin += wl[(size_t)(at[q] + H) * C];
    axr += wl[(size_t)(at[q] + H + 1) * C];
    if constexpr (CPLX) {
      P.ang += wl[(size_t)(at[q] + H) * C + 1];
      axi += wl[(size_t)(at[q] + H + 1) * C + 1];
    }
  }
  return stranger || nflip > 4 || !P.finite();  // (a product that overflowed: see the table's description)
}

constexpr int kChildStage = 4;  // 16-byte loads a thread has in flight while the factor table is copied into LDS (64 KB / 1024 threads)
// what a row that has to be computed from scratch holds between the two loops of the LDS kernel: a nan no arithmetic produces.  (Were
// an ordinary row ever to end on these bits it would be computed from scratch as well, which is right for every row.)
constexpr long long kChildAgainBits = 0x7ff8c41d5eedc41dll;

// A thread per row, in two loops.  The first takes every row from the tables and leaves a mark in psi where that will not do (strangers,
// overflowed products); the second, entered only by waves that left a mark -- or by all of them when the flag is raised: then there is no
// first loop -- computes the marked rows from scratch (the whole wave walks the parameters, the marked rows keep the result).  So the
// from-scratch code and its constants exist once and outside the hot loop.  The mark lives in the caller's psi between the two loops (a
// marked row costs one more store and load): the thread that wrote it reads it and only rows below the count are touched, but psi is
// scratch for the length of the launch and NOTHING MAY READ IT CONCURRENTLY.  Both forms share the staging, this tail and write_psi: form 1
// is the earlier kernel's schedule of the hidden units, not that kernel instruction for instruction.
template <int LEN, int FLAVOUR, int FORM>
__global__ __launch_bounds__(kChildBlock) void rbm_forward_children_kernel(const uint64_t *__restrict__ onv, int64_t n, const int32_t *__restrict__ count_dev,
                                                                      const int32_t *__restrict__ parent, const uint64_t *__restrict__ walkers,
                                                                      int64_t nwalkers, const double *__restrict__ table,
                                                                      const double *__restrict__ factors, int sorb, int H,
                                                                      const double *__restrict__ W, const double *__restrict__ hb,
                                                                      const double *__restrict__ vb, double *__restrict__ psi, double stamp) {
  constexpr bool CPLX = FLAVOUR == PYNQS_RBM_COMPLEX;
  constexpr int C = CPLX ? 2 : 1;
  constexpr int CO = (CPLX || FLAVOUR == PYNQS_RBM_PHASE) ? 2 : 1;  // doubles of psi per row
  extern __shared__ __attribute__((aligned(16))) double wl[];
  const int HP = children_hp(H);
  int64_t cnt = n;
  if (count_dev) cnt = min((int64_t)max(*count_dev, 0), n);
  const int64_t first = (int64_t)blockIdx.x * kChildBlock + threadIdx.x, stride = (int64_t)gridDim.x * kChildBlock;
  // (grid-uniform) parents out of range: every row from scratch
  const bool raised = children_flag_raised(factors[(size_t)(2 * sorb + 1) * HP * C], stamp);
  bool again = raised;  // some row of this thread is for the second loop
  if (!raised) {
    // the factor table into LDS, the same image either way: 16-byte loads from the first 16-byte boundary on, all of a thread's loads in
    // flight before its stores; the double before that boundary (a table that starts 8 bytes off) and the odd one at the end by themselves
    const int total = (2 * sorb + 1) * HP * C;
    const int head = (int)(((uintptr_t)factors >> 3) & 1);
    const int nvec = (total - head) >> 1;  // (total >= 9: never 0)
    const double2 *__restrict__ src = reinterpret_cast<const double2 *>(factors + head);
    for (int base = threadIdx.x; base < nvec; base += kChildBlock * kChildStage) {
      double2 v[kChildStage];
#pragma unroll
      for (int b = 0; b < kChildStage; ++b) v[b] = src[min(base + b * kChildBlock, nvec - 1)];
#pragma unroll
      for (int b = 0; b < kChildStage; ++b) {
        const int idx = base + b * kChildBlock;
        if (idx < nvec) { wl[head + 2 * idx] = v[b].x; wl[head + 2 * idx + 1] = v[b].y; }
      }
    }
    if (threadIdx.x == 0 && head) wl[0] = factors[0];
    if (threadIdx.x == 64 % kChildBlock && head + 2 * nvec < total) wl[total - 1] = factors[total - 1];
    __syncthreads();
    for (int64_t i = first; i < cnt; i += stride) {
      Prod P;
      double axr, axi;
      if (children_row_from_table<LEN, CPLX, FORM>(onv, i, parent, walkers, nwalkers, table, wl, sorb, H, P, axr, axi)) {
        again = true;
        psi[CO * i] = __longlong_as_double(kChildAgainBits);
      } else {
        write_psi<FLAVOUR>(psi, i, P, axr, axi);
      }
    }
  }
  if (!__ballot(again)) return;
  for (int64_t i = first; i < cnt; i += stride) {
    const bool mine = raised || (again && __double_as_longlong(psi[CO * i]) == kChildAgainBits);
    if (!__ballot(mine)) continue;
    Prod P;
    double axr, axi;
    children_row_from_scratch<LEN, FLAVOUR>(onv, i, sorb, H, W, hb, vb, P, axr, axi);
    if (mine) write_psi<FLAVOUR>(psi, i, P, axr, axi);
  }
}

// The same for factor tables beyond the LDS (sorb x num_hidden above ~64 x 64: 235 KB at 120 x 120): ONE WAVE PER ROW, the lanes over the
// hidden units.  Lane l forms q_h = q_h(parent) prod_{o in F} f_h(o) and its product of (1 + q_h) for h = l, l + 64, ...: the parent's row
// and the (at most four) factor rows are read as consecutive 8- / 16-byte words by consecutive lanes, from the L2 (the factor table is shared
// by every row, a parent's row by its few hundred children); the 64 partial products meet in a butterfly (mantissa and exponent kept apart:
// Prod).  4 row loads per hidden unit instead of sorb multiply-adds.  What is the same for all lanes of the row (the parent, the flipped
// orbitals, the table offsets) is computed on the scalar unit: the row number goes through readfirstlane, which tells the compiler so.
template <int LEN, int FLAVOUR>
__global__ __launch_bounds__(kBlock) void rbm_forward_children_wave_kernel(const uint64_t *__restrict__ onv, int64_t n, const int32_t *__restrict__ count_dev,
                                                                           const int32_t *__restrict__ parent, const uint64_t *__restrict__ walkers,
                                                                           int64_t nwalkers, const double *__restrict__ table,
                                                                           const double *__restrict__ factors, int sorb, int H,
                                                                           const double *__restrict__ W, const double *__restrict__ hb,
                                                                           const double *__restrict__ vb, double *__restrict__ psi, double stamp) {
  constexpr bool CPLX = FLAVOUR == PYNQS_RBM_COMPLEX;
  constexpr int C = CPLX ? 2 : 1;
  const int HP = children_hp(H);
  int64_t cnt = n;
  if (count_dev) cnt = min((int64_t)max(*count_dev, 0), n);
  if (children_flag_raised(factors[(size_t)(2 * sorb + 1) * HP * C], stamp)) {  // (grid-uniform) parents out of range: every row from scratch, a thread per row
    const int64_t rounds = (cnt + (int64_t)gridDim.x * kBlock - 1) / ((int64_t)gridDim.x * kBlock);
    for (int64_t r = 0; r < rounds; ++r) {
      const int64_t i = ((int64_t)r * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
      const int64_t row = i < cnt ? i : cnt - 1;
      uint64_t ket[LEN];
#pragma unroll
      for (int w = 0; w < LEN; ++w) ket[w] = onv[row * LEN + w];
      Prod P;
      double axr, axi;
      rbm_forward_row<LEN, FLAVOUR>(ket, sorb, H, W, hb, vb, P, axr, axi);
      if (i < cnt) write_psi<FLAVOUR>(psi, i, P, axr, axi);
    }
    return;
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t nwaves = (int64_t)gridDim.x * (kBlock / 64);
  // a wave takes kWaveRows consecutive rows at a time (the children of a walker follow each other in the distinct list: the parent's row and
  // the factor rows of its occupied orbitals stay in the CU's L1)
  constexpr int kWaveRows = kChildWaveRows;
  for (int64_t i0 = ((int64_t)blockIdx.x * (kBlock / 64) + wave) * kWaveRows; i0 < cnt; i0 += nwaves * kWaveRows)
  for (int64_t i = i0; i < min(i0 + kWaveRows, cnt); ++i) {  // (wave-uniform)
    int64_t p = parent[i];
    bool stranger = p < 0 || p >= nwalkers;  // (see the kernel above)
    p = stranger ? 0 : p;
    int at[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) at[q] = 2 * sorb * HP;
    int k = 0, nflip = 0;
#pragma unroll
    for (int w = 0; w < LEN; ++w) {
      const uint64_t xc = onv[i * LEN + w];
      uint64_t d = xc ^ walkers[p * LEN + w];
      nflip += __popcll(d);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (d && k < 4) {
          const int b = __builtin_ctzll(d);
          d &= d - 1;
          const int r = (2 * (64 * w + b) + (((xc >> b) & 1ull) ? 0 : 1)) * HP;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (q == k) at[q] = r;
          ++k;
        }
      }
    }
    const auto from_scratch = [&]() {  // (every lane the same row)
      uint64_t ket[LEN];
#pragma unroll
      for (int w = 0; w < LEN; ++w) ket[w] = onv[i * LEN + w];
      Prod P2;
      double a2r, a2i;
      rbm_forward_row<LEN, FLAVOUR>(ket, sorb, H, W, hb, vb, P2, a2r, a2i);
      if (lane == 0) write_psi<FLAVOUR>(psi, i, P2, a2r, a2i);
    };
    if (stranger || nflip > 4) {  // (wave-uniform, rare)
      from_scratch();
      continue;
    }
    const double *__restrict__ tp = table + (size_t)p * (size_t)(H + 2) * C;
    Prod P;
    for (int h = lane; h < H; h += 64) {
      double qr = tp[(size_t)h * C], qi = CPLX ? tp[(size_t)h * C + 1] : 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double fr = factors[(size_t)(at[q] + h) * C];
        if constexpr (CPLX) {
          const double fi = factors[(size_t)(at[q] + h) * C + 1];
          const double nr = qr * fr - qi * fi;
          qi = fma(qr, fi, qi * fr);
          qr = nr;
        } else {
          qr *= fr;
        }
      }
      if constexpr (CPLX) {  // P *= 1 + q
        const double u = 1.0 + qr;
        const double nr = P.re * u - P.im * qi;
        P.im = fma(P.re, qi, P.im * u);
        P.re = nr;
      } else {
        P.re *= 1.0 + qr;
      }
      P.renorm();
    }
    // the lanes' products: mantissas multiplied, exponents added, in a butterfly (every lane ends with the full product)
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const double orr = __shfl_xor(P.re, d), oi = CPLX ? __shfl_xor(P.im, d) : 0.0;
      const int oe = __shfl_xor(P.e2, d);
      if constexpr (CPLX) {
        const double nr = P.re * orr - P.im * oi;
        P.im = fma(P.re, oi, P.im * orr);
        P.re = nr;
      } else {
        P.re *= orr;
      }
      P.e2 += oe;   // (mantissas in [0.5, 1): 64 of them multiply to >= 2^-64, no renormalisation on the way)
    }
    P.renorm();
    if (__ballot(!P.finite())) {  // (a product that overflowed: see the table's description; the ballot keeps the branch wave-uniform)
      from_scratch();
      continue;
    }
    if (lane == 0) {
      double axr = tp[(size_t)(H + 1) * C], axi = CPLX ? tp[(size_t)(H + 1) * C + 1] : 0.0;
      P.lin = tp[(size_t)H * C];
      P.ang = CPLX ? tp[(size_t)H * C + 1] : 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        P.lin += factors[(size_t)(at[q] + H) * C];
        axr += factors[(size_t)(at[q] + H + 1) * C];
        if constexpr (CPLX) {
          P.ang += factors[(size_t)(at[q] + H) * C + 1];
          axi += factors[(size_t)(at[q] + H + 1) * C + 1];
        }
      }
      write_psi<FLAVOUR>(psi, i, P, axr, axi);
    }
  }
}

}  // namespace pynqs

using namespace pynqs;

extern "C" int pynqs_rbm_forward(const uint64_t *onv, int64_t n, int sorb, const double *weights, const double *hidden_bias,
                                 const double *visible_bias, int nhidden, int flavour, double *psi, void *stream) {
  pynqs::DeviceScope device_scope_(onv);
  if (n < 0 || n > 0x7fffffffll * kBlock || sorb < 1 || sorb > kMaxSorb || nhidden < 1) return set_error(PYNQS_EINVAL, "bad n/sorb/nhidden");
  if (flavour != PYNQS_RBM_REAL && flavour != PYNQS_RBM_TANH && flavour != PYNQS_RBM_PHASE && flavour != PYNQS_RBM_COMPLEX)
    return set_error(PYNQS_EINVAL, "bad flavour");
  if (n == 0) return PYNQS_OK;
  if (!onv || !weights || !hidden_bias || !psi) return set_error(PYNQS_EINVAL, "null pointer");
  const int len = (sorb - 1) / 64 + 1;
  const uint32_t grid = (uint32_t)((n + kBlock - 1) / kBlock);
  hipStream_t st = (hipStream_t)stream;
#define PYNQS_RF(F) hipLaunchKernelGGL((rbm_forward_kernel<LEN, F>), dim3(grid), dim3(kBlock), 0, st, onv, n, sorb, nhidden, weights, hidden_bias, visible_bias, psi)
  DISPATCH_LEN(len, {
    switch (flavour) {
      case PYNQS_RBM_REAL: PYNQS_RF(PYNQS_RBM_REAL); break;
      case PYNQS_RBM_TANH: PYNQS_RF(PYNQS_RBM_TANH); break;
      case PYNQS_RBM_PHASE: PYNQS_RF(PYNQS_RBM_PHASE); break;
      default: PYNQS_RF(PYNQS_RBM_COMPLEX); break;
    }
  });
#undef PYNQS_RF
  return check_launch("rbm_forward");
}

extern "C" int pynqs_jrbm_forward(const uint64_t *onv, int64_t n, int sorb, const double *weights, const double *hidden_bias,
                                  const double *visible_bias, const double *jastrow, int nhidden, double *psi, void *stream) {
  pynqs::DeviceScope device_scope_(onv);
  if (n < 0 || n > 0x7fffffffll * kBlock || sorb < 1 || sorb > kMaxSorb || nhidden < 1) return set_error(PYNQS_EINVAL, "bad n/sorb/nhidden");
  if (n == 0) return PYNQS_OK;
  if (!onv || !weights || !hidden_bias || !jastrow || !psi) return set_error(PYNQS_EINVAL, "null pointer");
  const int len = (sorb - 1) / 64 + 1;
  const uint32_t grid = (uint32_t)((n + kBlock - 1) / kBlock);
  DISPATCH_LEN(len, {
    hipLaunchKernelGGL((jrbm_forward_kernel<LEN>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, onv, n, sorb, nhidden, weights, hidden_bias,
                       visible_bias, jastrow, psi);
  });
  return check_launch("jrbm_forward");
}

static size_t children_lds_bytes(int sorb, int nhidden, int flavour) {
  return (size_t)(2 * sorb + 1) * (size_t)children_hp(nhidden) * (flavour == PYNQS_RBM_COMPLEX ? 16 : 8);
}

static bool children_flavour_ok(int flavour) {
  return flavour == PYNQS_RBM_REAL || flavour == PYNQS_RBM_TANH || flavour == PYNQS_RBM_PHASE || flavour == PYNQS_RBM_COMPLEX;
}

// (every shape: the factor table in LDS when it fits 64 KB, else a wave per row with the table read from the L2)
extern "C" int pynqs_rbm_forward_children_supported(int sorb, int nhidden, int flavour) {
  if (sorb < 1 || sorb > kMaxSorb || nhidden < 1 || !children_flavour_ok(flavour)) return 0;
  return 1;
}
static bool children_table_in_lds(int sorb, int nhidden, int flavour) {
  static const int force = getenv("PYNQS_RBM_CHILDREN_WAVE") ? atoi(getenv("PYNQS_RBM_CHILDREN_WAVE")) : -1;  // 1: the wave form everywhere
  return force != 1 && children_lds_bytes(sorb, nhidden, flavour) <= 64 * 1024;
}

extern "C" int64_t pynqs_rbm_children_table_bytes(int64_t nwalkers, int sorb, int nhidden, int flavour) {
  if (nwalkers < 0 || sorb < 1 || sorb > kMaxSorb || nhidden < 1 || !children_flavour_ok(flavour)) return -1;
  const int64_t c = flavour == PYNQS_RBM_COMPLEX ? 16 : 8;
  return nwalkers * (nhidden + 2) * c + (int64_t)children_lds_bytes(sorb, nhidden, flavour) + 8;
}

static int children_prepare_check(const uint64_t *walkers, int64_t nwalkers, int sorb, const double *weights, const double *hidden_bias,
                                  int nhidden, int flavour, void *table) {
  if (nwalkers < 0 || nwalkers > 0x7fffffffll * kBlock || sorb < 1 || sorb > kMaxSorb || nhidden < 1 || !children_flavour_ok(flavour))
    return set_error(PYNQS_EINVAL, "bad nwalkers/sorb/nhidden/flavour");
  if (!weights || !hidden_bias || !table || (nwalkers > 0 && !walkers)) return set_error(PYNQS_EINVAL, "null pointer");
  return PYNQS_OK;
}

extern "C" int pynqs_rbm_children_prepare(const uint64_t *walkers, int64_t nwalkers, int sorb, const double *weights, const double *hidden_bias,
                                          const double *visible_bias, int nhidden, int flavour, void *table, void *stream) {
  pynqs::DeviceScope device_scope_(table);
  if (const int rc = children_prepare_check(walkers, nwalkers, sorb, weights, hidden_bias, nhidden, flavour, table)) return rc;
  const bool cplx = flavour == PYNQS_RBM_COMPLEX;
  const int len = (sorb - 1) / 64 + 1;
  hipStream_t st = (hipStream_t)stream;
  double *parents = (double *)table;
  double *factors = parents + (size_t)nwalkers * (size_t)(nhidden + 2) * (cplx ? 2 : 1);
  const uint32_t gf = (uint32_t)(((2 * sorb + 1) * children_hp(nhidden) + kBlock - 1) / kBlock);
  if (cplx) hipLaunchKernelGGL((rbm_children_factors_kernel<true>), dim3(gf), dim3(kBlock), 0, st, sorb, nhidden, weights, visible_bias, factors);
  else hipLaunchKernelGGL((rbm_children_factors_kernel<false>), dim3(gf), dim3(kBlock), 0, st, sorb, nhidden, weights, visible_bias, factors);
  if (nwalkers > 0) {
    const dim3 grid((uint32_t)((nwalkers + kBlock - 1) / kBlock), (uint32_t)((nhidden + kParentChunk - 1) / kParentChunk));
    if (grid.y > 65535u) return set_error(PYNQS_EINVAL, "too many hidden units");
    DISPATCH_LEN(len, {
      if (cplx)
        hipLaunchKernelGGL((rbm_children_parents_kernel<LEN, true>), grid, dim3(kBlock), 0, st, walkers, nwalkers, sorb, nhidden, weights,
                           hidden_bias, visible_bias, factors, parents);
      else
        hipLaunchKernelGGL((rbm_children_parents_kernel<LEN, false>), grid, dim3(kBlock), 0, st, walkers, nwalkers, sorb, nhidden, weights,
                           hidden_bias, visible_bias, factors, parents);
    });
  }
  return check_launch("rbm_children_prepare");
}

// a stamp is a call number in [1, 2^53): it travels as a double, the type of the flag word
static bool children_stamp_ok(uint64_t stamp) { return stamp >= 1 && stamp < (1ull << 53); }

extern "C" int pynqs_rbm_children_prepare_stamped(const uint64_t *walkers, int64_t nwalkers, int sorb, const double *weights,
                                                  const double *hidden_bias, const double *visible_bias, int nhidden, int flavour,
                                                  uint64_t stamp, void *table, void *stream) {
  pynqs::DeviceScope device_scope_(table);
  if (const int rc = children_prepare_check(walkers, nwalkers, sorb, weights, hidden_bias, nhidden, flavour, table)) return rc;
  if (!children_stamp_ok(stamp)) return set_error(PYNQS_EINVAL, "rbm_children_prepare_stamped: stamp must be in [1, 2^53)");
  const bool cplx = flavour == PYNQS_RBM_COMPLEX;
  const int len = (sorb - 1) / 64 + 1;
  double *parents = (double *)table;
  double *factors = parents + (size_t)nwalkers * (size_t)(nhidden + 2) * (cplx ? 2 : 1);
  const uint32_t gf = (uint32_t)(((2 * sorb + 1) * children_hp(nhidden) + kBlock - 1) / kBlock);
  const uint32_t gw = (uint32_t)((nwalkers + kBlock - 1) / kBlock), nchunks = (uint32_t)((nhidden + kParentChunk - 1) / kParentChunk);
  const dim3 grid(gw > gf ? gw : gf, nchunks + 2);
  if (grid.y > 65535u) return set_error(PYNQS_EINVAL, "too many hidden units");
  DISPATCH_LEN(len, {
    if (cplx)
      hipLaunchKernelGGL((rbm_children_prepare_kernel<LEN, true>), grid, dim3(kBlock), 0, (hipStream_t)stream, walkers, nwalkers, sorb, nhidden,
                         weights, hidden_bias, visible_bias, factors, parents, (int)nchunks, (double)stamp);
    else
      hipLaunchKernelGGL((rbm_children_prepare_kernel<LEN, false>), grid, dim3(kBlock), 0, (hipStream_t)stream, walkers, nwalkers, sorb, nhidden,
                         weights, hidden_bias, visible_bias, factors, parents, (int)nchunks, (double)stamp);
  });
  return check_launch("rbm_children_prepare_stamped");
}

// The grid of pynqs_rbm_forward_children and the rows it covers before a workgroup strides on: the one source of the launch below and of
// pynqs_rbm_forward_children_geometry.  LDS form: a thread per row on both routes.  Wave form: a wave per kChildWaveRows consecutive rows
// on the table route, a thread per row on the from-scratch route (the flag raised).
struct ChildrenGeometry {
  bool in_lds;
  int64_t blocks, table_rows, scratch_rows;
};
static ChildrenGeometry children_geometry(int64_t n, int sorb, int nhidden, int flavour) {
  ChildrenGeometry g;
  g.in_lds = children_table_in_lds(sorb, nhidden, flavour);
  if (g.in_lds) {
    g.blocks = (n + kChildBlock - 1) / kChildBlock;
    if (g.blocks > kChildMaxBlocks) g.blocks = kChildMaxBlocks;
    g.table_rows = g.scratch_rows = g.blocks * kChildBlock;
  } else {
    constexpr int64_t rows = (kBlock / 64) * kChildWaveRows;  // per workgroup
    g.blocks = (n + rows - 1) / rows;
    if (g.blocks > kChildMaxWaveBlocks) g.blocks = kChildMaxWaveBlocks;
    g.table_rows = g.blocks * rows;
    g.scratch_rows = g.blocks * kBlock;
  }
  return g;
}

extern "C" int pynqs_rbm_forward_children_geometry(int64_t n, int sorb, int nhidden, int flavour, int64_t *out4) {
  if (!out4) return set_error(PYNQS_EINVAL, "null pointer");
  if (n < 0 || n > 0x7fffffffll * kBlock || !pynqs_rbm_forward_children_supported(sorb, nhidden, flavour))
    return set_error(PYNQS_EINVAL, "rbm_forward_children_geometry: bad n/sorb/nhidden/flavour");
  const ChildrenGeometry g = children_geometry(n, sorb, nhidden, flavour);
  out4[0] = g.in_lds ? 0 : 1;
  out4[1] = g.blocks;
  out4[2] = g.table_rows;
  out4[3] = g.scratch_rows;
  return PYNQS_OK;
}

static int forward_children_launch(const uint64_t *onv, int64_t n, const int32_t *count_dev, const int32_t *parent, const uint64_t *walkers,
                                   int64_t nwalkers, const void *table, int sorb, const double *weights, const double *hidden_bias,
                                   const double *visible_bias, int nhidden, int flavour, double stamp, int form, double *psi, void *stream) {
  pynqs::DeviceScope device_scope_(onv);
  if (form != PYNQS_CHILDREN_CHUNKED && form != PYNQS_CHILDREN_PER_UNIT) return set_error(PYNQS_EINVAL, "rbm_forward_children: bad form");
  if (n < 0 || n > 0x7fffffffll * kBlock || nwalkers < 0 || sorb < 1 || sorb > kMaxSorb || nhidden < 1) return set_error(PYNQS_EINVAL, "bad n/sorb/nhidden");
  if (!pynqs_rbm_forward_children_supported(sorb, nhidden, flavour))
    return set_error(PYNQS_EINVAL, "rbm_forward_children: bad flavour");
  if (n == 0) return PYNQS_OK;
  if (!onv || !parent || !walkers || !table || !psi || !weights || !hidden_bias || nwalkers == 0) return set_error(PYNQS_EINVAL, "null pointer");
  const int len = (sorb - 1) / 64 + 1;
  const ChildrenGeometry geo = children_geometry(n, sorb, nhidden, flavour);
  const uint32_t grid = (uint32_t)geo.blocks;
  const size_t lds = children_lds_bytes(sorb, nhidden, flavour);
  const double *parents = (const double *)table;
  const double *factors = parents + (size_t)nwalkers * (size_t)(nhidden + 2) * (flavour == PYNQS_RBM_COMPLEX ? 2 : 1);
  hipStream_t st = (hipStream_t)stream;
  const bool in_lds = geo.in_lds;
#define PYNQS_RC(F)                                                                                                                          \
  do {                                                                                                                                       \
    if (in_lds && form == PYNQS_CHILDREN_CHUNKED)                                                                                            \
      hipLaunchKernelGGL((rbm_forward_children_kernel<LEN, F, PYNQS_CHILDREN_CHUNKED>), dim3(grid), dim3(kChildBlock), lds, st, onv, n,      \
                         count_dev, parent, walkers, nwalkers, parents, factors, sorb, nhidden, weights, hidden_bias, visible_bias, psi,     \
                         stamp);                                                                                                             \
    else if (in_lds)                                                                                                                         \
      hipLaunchKernelGGL((rbm_forward_children_kernel<LEN, F, PYNQS_CHILDREN_PER_UNIT>), dim3(grid), dim3(kChildBlock), lds, st, onv, n,     \
                         count_dev, parent, walkers, nwalkers, parents, factors, sorb, nhidden, weights, hidden_bias, visible_bias, psi,     \
                         stamp);                                                                                                             \
    else                                                                                                                                     \
      hipLaunchKernelGGL((rbm_forward_children_wave_kernel<LEN, F>), dim3(grid), dim3(kBlock), 0, st, onv, n, count_dev,                     \
                         parent, walkers, nwalkers, parents, factors, sorb, nhidden, weights, hidden_bias, visible_bias, psi, stamp);        \
  } while (0)
  DISPATCH_LEN(len, {
    switch (flavour) {
      case PYNQS_RBM_REAL: PYNQS_RC(PYNQS_RBM_REAL); break;
      case PYNQS_RBM_TANH: PYNQS_RC(PYNQS_RBM_TANH); break;
      case PYNQS_RBM_PHASE: PYNQS_RC(PYNQS_RBM_PHASE); break;
      default: PYNQS_RC(PYNQS_RBM_COMPLEX); break;
    }
  });
#undef PYNQS_RC
  return check_launch("rbm_forward_children");
}

// form: the LDS kernel's schedule, PYNQS_CHILDREN_CHUNKED or PYNQS_CHILDREN_PER_UNIT (the same bits; the wave form has one schedule and
// ignores it).  Per call: one process can run both.
extern "C" int pynqs_rbm_forward_children_form(const uint64_t *onv, int64_t n, const int32_t *count_dev, const int32_t *parent,
                                               const uint64_t *walkers, int64_t nwalkers, const void *table, int sorb, const double *weights,
                                               const double *hidden_bias, const double *visible_bias, int nhidden, int flavour, int form,
                                               double *psi, void *stream) {
  return forward_children_launch(onv, n, count_dev, parent, walkers, nwalkers, table, sorb, weights, hidden_bias, visible_bias, nhidden, flavour,
                                 0.0, form, psi, stream);
}

extern "C" int pynqs_rbm_forward_children(const uint64_t *onv, int64_t n, const int32_t *count_dev, const int32_t *parent,
                                          const uint64_t *walkers, int64_t nwalkers, const void *table, int sorb, const double *weights,
                                          const double *hidden_bias, const double *visible_bias, int nhidden, int flavour, double *psi,
                                          void *stream) {
  return pynqs_rbm_forward_children_form(onv, n, count_dev, parent, walkers, nwalkers, table, sorb, weights, hidden_bias, visible_bias, nhidden,
                                         flavour, PYNQS_CHILDREN_CHUNKED, psi, stream);
}

extern "C" int pynqs_rbm_forward_children_stamped_form(const uint64_t *onv, int64_t n, const int32_t *count_dev, const int32_t *parent,
                                                       const uint64_t *walkers, int64_t nwalkers, const void *table, int sorb,
                                                       const double *weights, const double *hidden_bias, const double *visible_bias,
                                                       int nhidden, int flavour, uint64_t stamp, int form, double *psi, void *stream) {
  if (!children_stamp_ok(stamp)) return set_error(PYNQS_EINVAL, "rbm_forward_children_stamped: stamp must be in [1, 2^53)");
  return forward_children_launch(onv, n, count_dev, parent, walkers, nwalkers, table, sorb, weights, hidden_bias, visible_bias, nhidden, flavour,
                                 (double)stamp, form, psi, stream);
}

extern "C" int pynqs_rbm_forward_children_stamped(const uint64_t *onv, int64_t n, const int32_t *count_dev, const int32_t *parent,
                                                  const uint64_t *walkers, int64_t nwalkers, const void *table, int sorb, const double *weights,
                                                  const double *hidden_bias, const double *visible_bias, int nhidden, int flavour,
                                                  uint64_t stamp, double *psi, void *stream) {
  return pynqs_rbm_forward_children_stamped_form(onv, n, count_dev, parent, walkers, nwalkers, table, sorb, weights, hidden_bias, visible_bias,
                                                 nhidden, flavour, stamp, PYNQS_CHILDREN_CHUNKED, psi, stream);
}
