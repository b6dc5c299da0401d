"""Host-side yardstick of the Jastrow-RBM kernels (pynqs_eloc_jrbm, pynqs_jrbm_forward, pynqs_jastrow_grad; include/pynqs_amd.h), in
numpy longdouble: psi(x) = exp(a.x + x^T M x) prod_h 2cosh(theta_h), a real RBM (rbm_type "real") times the two-body Jastrow factor of
vmc/ansatz/rbm/rbm_other.py (M [sorb, sorb], any real matrix).  It shares no code with the kernels or with oracle/: the excitations,
matrix elements and the RBM's own ratios come from eloc_exact.structure / eloc_exact.walker and rbm_exact, by import.

Exact quantities.  r_k = r_k^RBM exp(Delta_k) with Delta_k = x'^T M x' - x^T M x formed DIRECTLY from the two +-1 rows and M (the kernel
uses the flip formula below; it is checked against this, never used for it); E = h_0 + sum_k h_k r_k; ln psi = ln psi_RBM + x^T M x.

The flip formula (what the kernel evaluates; tests/test_jrbm_exact.py checks the algebra and every sign by class).  S = M + M^T with a
zero diagonal, x^T M x = tr M + sum_{i<j} S_ij x_i x_j, and for x' = x with the orbitals F flipped
    Delta = -2 sum_{i in F} x_i r_i + 4 sum_{i<j in F} S_ij x_i x_j,     r_i = sum_{j != i} S_ij x_j.

Bounds, a priori (u = 2^-53; operations counted in kernels_rbm.hip JASTROW, kernels_rbm_forward.hip, kernels_jastrow.hip).
E_loc: eloc_exact.Walker.bound with kappa_k (the relative error of the ratio) enlarged by
    kappa_J,k = 2 (sorb + 1) sum_{o in F_k} R_o + 24 sum_{i<j in F_k} |S_ij| + 16,      R_o = sum_j |S_oj|.
  First term: r_o joins the exponent of C(o) = exp(-2 x_o ((a_o + r_o) + sum_h s_h W_ho)).  S_oj = M_oj + M_jo is rounded once (u R_o); r_o is
  a chain of sorb additions of which the first (to 0) and the one of S_oo = 0 are exact: at most sorb - 2 roundings on partial sums <= R_o;
  a_o + r_o and the sum with sum_h s_h W_ho round once each on R_o: sorb + 1 in all, doubled by the factor 2 of the exponent.  (The same two
  additions act on |a_o| + sum_h |W_ho| once more than in the plain kernel: eloc_exact's D = ceil(H / 64) + 7 counts ceil(H / 64) + 6 there.)
  Second term: the six (one for a single) pair factors exp(+-4 S_ij): 4 S_ij is exact, S_ij carries u |S_ij| from its own rounding, so
  4 u |S_ij| per factor in the exponent -- 24 covers the six whether they are multiplied one by one, as here, or exponentiated from one sum.
  Constant: six exponentials and, per column, six products (two for the four crossed pairs of a fast entry with a slow orbital pair,
  one that joins them, one for the two inner pairs, one that joins the two, one onto the running product): 12 <= 16.
psi(x), from pynqs_eloc_jrbm and pynqs_jrbm_forward:  |psi / psi_exact - 1| <= u [(sorb + H + 16) cond(x) + (2 sorb + 4) sum_ij |M_ij|],  cond
  as in rbm_exact.  pynqs_jrbm_forward sums x^T M x row by row: sorb - 1 rounding fused multiply-adds per row on sum_j |M_ij|, sorb - 1 for
  the rows on sum_ij |M_ij|: 2 sorb - 2, then the addition to a.x, the exponent's own sum and the exponential: <= 2 sorb + 1.
  pynqs_eloc_jrbm: sum_{i<j} S_ij x_i x_j = sum_o x_o r_o / 2 with r_o as above ((sorb - 1) u R_o each with S's own rounding, halved, and
  sum_o R_o / 2 <= sum_{i != j} |M_ij|: sorb - 1), summed apart from the RBM's exponent over lanes and waves -- of sorb terms at most
  sorb - 1 additions round, whatever the tree (adding zero is exact) -- then tr M (sorb - 1 on sum_i |M_ii|), the two additions that join
  them to the exponent and the exponential: <= 2 sorb + 2.
grad_M, per entry:  |got - exact| <= u (n + 8) 2 sum_n |p_n| |E_n - <E> c_n|,  for any fixed order of the n terms: f_n = p_n (E_n - <E> c_n)
  takes a fused multiply-add (one rounding of the difference, relative to itself) and a product, the n terms +-f_n at most n - 1
  roundings on sum_n |f_n|; the factor 2 is exact.
The Jastrow part of the loss, 2 sum_n f_n x_n^T M x_n:  |got - exact| <= u (2 sorb + n + 8) 2 sum_n |f_n| sum_ij |M_ij|  (x^T M x as in
  pynqs_jrbm_forward: 2 sorb - 2; the product with f_n and its two roundings; 64 walkers of a workgroup in turn, then the workgroups: < n)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import eloc_exact as X
import rbm_exact as R

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53

J_REGIMES = {"j-small": 0.05, "j-asym": 0.3, "j-strong": 1.0}


def jastrow_params(regime: str, sorb: int, seed: int = 0) -> np.ndarray:
    """M float64 [sorb, sorb], entries uniform in +-w (w = 0.05 "j-small", 0.3 "j-asym", 1.0 "j-strong"): a full random matrix, so
    M != M^T and the diagonal is not zero in every regime; "j-asym" is the one the tests name for that."""
    w = J_REGIMES[regime]
    g = np.random.default_rng([seed, sorb, len(regime), int(1000 * w)])
    M = 2.0 * w * (g.random((sorb, sorb)) - 0.5)
    assert not np.array_equal(M, M.T) and bool(np.diag(M).all())
    return M


def xmx(M: np.ndarray, x: np.ndarray) -> np.ndarray:
    """x^T M x of the +-1 rows x [n, sorb], longdouble [n], directly from the rows and M"""
    xl = np.asarray(x).astype(LD)
    return ((xl @ np.asarray(M, dtype=np.float64).astype(LD)) * xl).sum(1)


def s_matrix(M: np.ndarray) -> np.ndarray:
    """S = M + M^T with a zero diagonal, longdouble (exact: the sum of two doubles fits 64 bits of mantissa unless their exponents differ by
    more than 11, and then to 2^-64)"""
    Ml = np.asarray(M, dtype=np.float64).astype(LD)
    S = Ml + Ml.T
    S[np.diag_indices_from(S)] = 0
    return S


def flip_delta(M: np.ndarray, x: np.ndarray, flips) -> np.ndarray:
    """The flip formula of the module docstring for one +-1 row x [sorb] and the flipped orbitals of every column (int [m, 4], padded with
    -1): longdouble [m].  What the kernel evaluates -- for the test of the algebra, not for the reference."""
    S = s_matrix(M)
    xl = np.asarray(x).astype(LD)
    r = S @ xl  # (S_ii = 0)
    out = np.zeros(len(flips), dtype=LD)
    for k, F in enumerate(flips):
        F = [int(o) for o in F if o >= 0]
        d = LD(0)
        for i in F:
            d -= 2 * xl[i] * r[i]
        for a in range(len(F)):
            for b in range(a + 1, len(F)):
                d += 4 * S[F[a], F[b]] * xl[F[a]] * xl[F[b]]
        out[k] = d
    return out


def kappa_jastrow(M: np.ndarray, flips: np.ndarray) -> np.ndarray:
    """kappa_J,k of the module docstring, float64 [m]"""
    S = np.abs(s_matrix(M)).astype(np.float64)
    sorb = S.shape[0]
    Ro = S.sum(1)
    on = flips >= 0
    F = np.where(on, flips, 0)
    first = np.where(on, Ro[F], 0.0).sum(1)
    second = np.zeros(flips.shape[0])
    for a in range(4):
        for b in range(a + 1, 4):
            second += np.where(on[:, a] & on[:, b], S[F[:, a], F[:, b]], 0.0)
    return 2.0 * (sorb + 1) * first + 24.0 * second + 16.0


def walker(rbm: R.Rbm, M: np.ndarray, st: X.Structure) -> X.Walker:
    """eloc_exact.Walker of the Jastrow-RBM: r, E, |r|, kappa (+ kappa_J), A, ln psi of x (Walker.psi, with x^T M x) and lnmax over x and
    every x'.  M = 0 returns eloc_exact.walker's E and r bit for bit (exp(0) = 1 and the products by 1 are exact)."""
    assert rbm.kind == "real"
    w0 = X.walker(rbm, st)
    x = st.occ.astype(np.float64) * 2 - 1
    q0 = xmx(M, x[None, :])[0]
    qk = xmx(M, st.bits.astype(np.float64) * 2 - 1) if st.bits.shape[0] else np.zeros(0, dtype=LD)
    r = (w0.r * np.exp(qk - q0).astype(CLD)).astype(CLD)
    rabs = np.abs(r).astype(np.float64)
    E = st.h0 + (st.h.astype(CLD) * r).sum()
    A = st.a0 + float((st.a * rabs).sum())
    kappa = w0.kappa + kappa_jastrow(M, st.flips)
    e0 = w0.psi
    psi = R.Exact(e0.kind, e0.re + q0, e0.im, e0.vis, e0.cond, e0.y, e0.sech2)
    with np.errstate(divide="ignore"):
        ln_children = e0.re[0] + np.log(np.abs(w0.r).astype(LD)) + qk
    lnmax = float(max(np.abs(ln_children).max() if r.size else 0.0, abs(psi.re[0])))
    return X.Walker(st, E, r, rabs, kappa, w0.ext, A, psi, lnmax, w0.vis0, w0.ncross, False)


def exact_ld(rbm: R.Rbm, M: np.ndarray, x: np.ndarray) -> R.Exact:
    """rbm_exact.exact_ld with x^T M x added to Re ln psi, for the +-1 rows x [n, sorb]"""
    e = R.exact_ld(rbm, x)
    return R.Exact(e.kind, e.re + xmx(M, x), e.im, e.vis, e.cond, e.y, e.sech2)


def amp_bound(rbm: R.Rbm, M: np.ndarray, cond: np.ndarray) -> np.ndarray:
    """u [(sorb + H + 16) cond(x) + (2 sorb + 4) sum_ij |M_ij|]: the bound on |psi / psi_exact - 1|"""
    sorb = rbm.W.shape[1]
    return U * ((sorb + rbm.H + 16) * np.asarray(cond, dtype=np.float64) + (2 * sorb + 4) * float(np.abs(M).sum()))


def amp_ratio(rbm: R.Rbm, M: np.ndarray, got: np.ndarray, ex: R.Exact) -> np.ndarray:
    """|psi / psi_exact - 1| over amp_bound per row; inf where the kernel's value is not finite"""
    g = np.asarray(got, dtype=np.float64)
    ok = np.isfinite(g)
    err = np.abs(np.where(ok, g, 0).astype(LD) / np.exp(ex.re) - 1).astype(np.float64)
    return np.where(ok, err / amp_bound(rbm, M, ex.cond), np.inf)


@dataclass
class JGrad:
    """The estimator for M in longdouble: G [sorb, sorb] = 2 sum_n f_n x_i x_j, its per-entry bound, the Jastrow part of the loss and
    its bound, f_n."""
    G: np.ndarray
    bound: float
    loss: float
    bloss: float
    f: np.ndarray


def grad_exact(M: np.ndarray, x: np.ndarray, prob: np.ndarray, eloc: np.ndarray, e_total: float, powc=None) -> JGrad:
    n, sorb = x.shape
    c = np.ones(n, dtype=LD) if powc is None else np.asarray(powc, dtype=np.float64).astype(LD)
    f = np.asarray(prob, dtype=np.float64).astype(LD) * (np.asarray(eloc, dtype=np.float64).astype(LD) - LD(float(e_total)) * c)
    xl = x.astype(LD)
    G = 2 * (xl * f[:, None]).T @ xl
    sf = float(np.abs(f).sum())
    loss = float(2 * (f * xmx(M, x)).sum())
    return JGrad(G, U * (n + 8) * 2 * sf, loss, U * (2 * sorb + n + 8) * 2 * sf * float(np.abs(M).sum()), f)
