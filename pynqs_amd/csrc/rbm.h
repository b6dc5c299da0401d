// rbm.h -- device-memory layout of the "RBM table": the parameters of a real restricted-Boltzmann-machine
// amplitude (PyNQS vmc/ansatz/rbm/rbm.py:186-211, rbm_type "real")
//     psi(x) = exp(a.x) * prod_h 2 cosh(theta_h(x)),   theta_h = b_h + sum_o W[h][o] x_o,   x_o = +-1,
// re-laid out for the fused local-energy kernel (kernels_rbm.hip), in caller-owned memory like the integral plan.
// All tables are double, hidden index fastest (a wave reads a row of one orbital with consecutive lanes):
//   Wt  [sorb][Hq]   W transposed (padding 0)
//   E4p [sorb][Hq]   exp(+4 W[h][o])   (padding 1)
//   E4m [sorb][Hq]   exp(-4 W[h][o])   (padding 1)
//   hb  [Hq]         hidden bias b (padding 0)
//   vb  [sorb]       visible bias a (0 when the caller passes none)
// Hq = row stride = H rounded up to a multiple of 8, plus 1: odd, so that in LDS (read with ds_read_b64: banks
// = 8-byte pairs of a 256-byte row, conflicts among 32 lanes) 32 consecutive rows start in 32 different pairs.
#pragma once

#include <stdint.h>

namespace pynqs {

struct RbmLayout {
  int sorb, H, Hq, Hloop;  // Hloop = H rounded up to a multiple of 8 (what the hidden-unit loop runs over)
  int64_t offWt, offE4p, offE4m, offHb, offVb, total;  // in doubles
};

inline bool make_rbm_layout(int sorb, int H, RbmLayout *L) {
  if (sorb < 1 || sorb > 192 || H < 1 || H > 8192) return false;
  L->sorb = sorb; L->H = H;
  L->Hloop = (H + 7) & ~7;
  L->Hq = L->Hloop + 1;
  const int64_t row = (int64_t)sorb * L->Hq;
  L->offWt = 0; L->offE4p = row; L->offE4m = 2 * row; L->offHb = 3 * row;
  L->offVb = L->offHb + L->Hq;
  L->total = (L->offVb + sorb + 1) & ~(int64_t)1;
  return true;
}

// The "Jastrow table" (pynqs_jastrow_table_build) of the two-body factor exp(x^T M x) that multiplies a real RBM (vmc/ansatz/rbm/
// rbm_other.py, class Jastrow, prod_dim = 1; M [sorb][sorb] real, any matrix), in caller-owned memory, all double, row-major [sorb][sorb]:
//   S   = M + M^T with a zero diagonal:  x^T M x = tr M + sum_{i<j} S_ij x_i x_j   (bitwise symmetric: a + b = b + a)
//   E4p = exp(+4 S_ij), E4m = exp(-4 S_ij): the pair factor of two flipped orbitals i, j of a walker is E4p where x_i = x_j, else E4m
//   tr  = sum_i M_ii (one double; it scales psi(x) only)
struct JastrowLayout {
  int sorb;
  int64_t offS, offE4p, offE4m, offTr, total;  // in doubles
};

constexpr int64_t jastrow_pairs(int sorb) { return (int64_t)sorb * sorb; }  // doubles per matrix (the kernels form the offsets from it)

inline bool make_jastrow_layout(int sorb, JastrowLayout *L) {
  if (sorb < 1 || sorb > 192) return false;
  const int64_t n2 = jastrow_pairs(sorb);
  L->sorb = sorb;
  L->offS = 0; L->offE4p = n2; L->offE4m = 2 * n2; L->offTr = 3 * n2;
  L->total = (3 * n2 + 2) & ~(int64_t)1;
  return true;
}

// The table of an RBM with COMPLEX parameters (pynqs_crbm_table_build), in caller-owned memory, complex double = 2 doubles, hidden index fastest, row stride Hs (odd: consecutive rows start in
// different 16-byte bank groups):  Wt [sorb][Hs] | E4p = exp(+4W) [sorb][Hs] | E4m = exp(-4W) [sorb][Hs] | hb [Hs] | vb [sorb]
struct CrbmLayout {
  int sorb, H, Hloop, Hs;  // Hloop = H rounded up to 2 (the hidden-unit loop), Hs = Hloop + 1
  int64_t offWt, offE4p, offE4m, offHb, offVb, total;  // in complex elements
};

inline bool make_crbm_layout(int sorb, int H, CrbmLayout *L) {
  if (sorb < 1 || sorb > 192 || H < 1 || H > 4096) return false;
  L->sorb = sorb; L->H = H;
  L->Hloop = (H + 1) & ~1;
  L->Hs = L->Hloop + 1;
  const int64_t row = (int64_t)sorb * L->Hs;
  L->offWt = 0; L->offE4p = row; L->offE4m = 2 * row; L->offHb = 3 * row;
  L->offVb = L->offHb + L->Hs;
  L->total = L->offVb + sorb;
  return true;
}

}  // namespace pynqs
