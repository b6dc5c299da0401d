"""Host-side yardstick of the reduced density matrices of a Jastrow-RBM (pynqs_rdm_jrbm; include/pynqs_amd.h, "reduced density matrices"),
psi(x) = exp(a.x + x^T M x) prod_h 2cosh(theta_h), in numpy longdouble.  It shares no code with the kernels: the estimator is
rdm_exact.estimator (plain loops over the excitations, signs from applying the operators one by one) with the amplitude from
jrbm_exact.exact_ld (x^T M x formed directly from the +-1 rows and M, never from the flip formula).  psi is formed as exp(ln psi - ln psi
of the first row), in longdouble, so that only differences of ln psi are exponentiated: the ratios psi(x') / psi(x) are all the estimator
uses, and they stay finite where psi itself would not.

Bound per slot, a priori:  |got_t - exact_t| <= (m_t + 2 + kappa) u A_t  (rdm_exact: m_t contributions, A_t = sum |w r|), kappa by path:
  "ratio"  (pynqs_rdm_scatter fed with correctly rounded ratios of this yardstick): kappa = 2, as in rdm_exact.
  "fused"  (pynqs_rdm_jrbm): one constant per case,
               kappa = rdm_exact.kappa_fused(rbm, sorb) + kappa_J,
               kappa_J = 2 (sorb + 1) (sum of the four largest R_o) + 24 (sum of the six largest |S_ij|, i < j) + 16,   R_o = sum_j |S_oj|,
           jrbm_exact.kappa_jastrow's count maximised over all excitations (at most four flipped orbitals, at most six pairs among them).
           Counted in kernels_rdm.hip (JASTROW), for the flip formula
               Delta = -2 xo (r_o0 + r_o1) - 2 xl (r_l0 + r_l1) + 4 S_o0o1 + 4 S_l0l1 - 4 (S_o0l0 + S_o0l1 + S_o1l0 + S_o1l1):
           * r_o (rdm_r_kernel): S_oj = M_oj + M_jo rounded once (u R_o); a chain of sorb fused multiply-adds of which the first (onto 0)
             and the one of S_oo = 0 are exact: sorb - 2 roundings on partial sums <= R_o.  The owner's two join their exponent by two
             additions (r_o0 + r_o1, then onto ln(owner factor) + visible term; the product by -2 xo is exact): sorb + 1 roundings on R_o,
             doubled by the factor 2.  The lane side's go through e_o = exp(-2 xl r_o) with no addition at all: sorb - 1, within the same count.
           * the pair terms: 4 S is exact and S carries its own rounding (4 u |S_ij|); 4 S_o0o1 is added onto the owner's visible term and
             rides two more additions of that exponent (3 in all); the item's five are three additions of the crossed sum, the
             subtraction from 4 S_l0l1 and the addition onto the lane constant's exponent: at most five additions on at most
             4 sum |S_ij| of the pairs involved: (4 + 5 x 4) = 24 per unit of sum |S_ij|.
           * the constant: the two exponentials e_l0, e_l1 (2 u each at most), their product and the product onto v: 6 <= 16.  (The
             lane constant's and the owner factor's exponentials exist in pynqs_rdm_rbm and are in kappa_fused.)
           * the additions above also round the RBM's share of the two exponents once more each (twice for the owner's: 4 S_o0o1 onto
             the visible term, the r term onto the sum).  kappa_fused counts H + 4 roundings per exponent; pynqs_rdm_rbm has at most
             H + 2 in the lane constant (H - 1 in the column sum, three to combine) and H in the owner's (of H nonzero terms at most
             H - 1 additions round, whatever the tree, and the visible term): H + 3 and H + 2 now, still within that count.
  "module" (pynqs_amd.rdm's generic route: JastrowRBM.forward on x and x', a division): one constant per case,
               kappa_module = 2 max over the case's rows of jrbm_exact.amp_bound / u + 4
           (the two amplitudes' bounds |psi / psi_exact - 1|, the division and the products).
Slots with A_t = 0 receive no contribution and must be exactly zero."""
from __future__ import annotations

import functools

import numpy as np

import jrbm_exact as J
import rbm_exact as R
import rdm_exact as X
import test_gpu_rdm as T0

LD, CLD = np.longdouble, np.clongdouble
U = X.U


def kappa_jastrow(M: np.ndarray) -> float:
    """kappa_J of the module docstring"""
    S = np.abs(J.s_matrix(M)).astype(np.float64)
    sorb = S.shape[0]
    Ro = np.sort(S.sum(1))[::-1]
    pairs = np.sort(S[np.triu_indices(sorb, 1)])[::-1]
    return 2.0 * (sorb + 1) * float(Ro[:4].sum()) + 24.0 * float(pairs[:6].sum()) + 16.0


def amplitude(rbm: R.Rbm, M: np.ndarray, seen=None):
    """rows 0/1 [m, sorb] -> psi(row) / psi(row 0), complex longdouble [m]; seen (a list) collects jrbm_exact.amp_bound / u of the rows"""
    def amp(rows):
        e = J.exact_ld(rbm, M, np.asarray(rows).astype(np.float64) * 2 - 1)
        if seen is not None:
            seen.append(float((J.amp_bound(rbm, M, e.cond) / U).max()))
        return np.exp(e.re - e.re[0]).astype(CLD)
    return amp


def estimate(rbm: R.Rbm, M: np.ndarray, occ: np.ndarray, w: np.ndarray):
    """(rdm_exact.Estimate of the Jastrow-RBM with kappa_fused = kappa of the "fused" path, kappa_module of the case)"""
    sorb = occ.shape[1]
    seen = []
    est = X.estimator(occ.astype(np.int8), w, amplitude=amplitude(rbm, M, seen))
    est.kappa_fused = X.kappa_fused(rbm, sorb) + kappa_jastrow(M)
    return est, 2.0 * max(seen) + 4.0


def bound(est: X.Estimate, path: str, kappa_module: float = float("nan")) -> np.ndarray:
    """(m_t + 2 + kappa) u A_t per slot of (rdm1 | rdm2)"""
    if path in ("ratio", "fused"):
        return est.bound(path)
    assert path == "module", path
    A = np.concatenate([est.A1, est.A2])
    m = np.concatenate([est.m1, est.m2]).astype(np.float64)
    return (m + 2.0 + kappa_module) * U * A


def ratio_rows(comb_occ: np.ndarray, rbm: R.Rbm, M: np.ndarray) -> np.ndarray:
    """psi(x'_k) / psi(x) for the rows comb_occ [n, ncomb, sorb] (0/1; column 0 = x) as correctly rounded doubles [n, ncomb]"""
    n, nc, sorb = comb_occ.shape
    e = J.exact_ld(rbm, M, comb_occ.reshape(n * nc, sorb).astype(np.float64) * 2 - 1)
    re = e.re.reshape(n, nc)
    return np.exp(re - re[:, :1]).astype(np.float64)


# (sorb, noA, noB, walkers (0: all 36 of the golden file), H, RBM regime, Jastrow regime): the shapes of test_gpu_rdm.CASES
CASES = [
    (8, 2, 2, 0, 3, "small", "j-small"), (8, 2, 2, 0, 8, "chunk-50", "j-asym"), (8, 2, 2, 0, 17, "alt30", "j-strong"),
    (12, 3, 2, 24, 8, "fe2s2", "j-asym"), (12, 3, 2, 24, 17, "one-338-w", "j-strong"),  # noA != noB, the hole side owns
    (10, 4, 4, 20, 3, "small", "j-strong"), (10, 4, 4, 20, 17, "chunk-50", "j-small"),  # the particle side owns
    (10, 1, 1, 20, 8, "alt30", "j-asym"),                                               # no same-spin doubles, no same-spin spectators
    (66, 3, 3, 16, 17, "one-338-w", "j-small"), (66, 3, 3, 16, 3, "small", "j-asym"),   # two words; orbitals 63, 64, 65 forced
]
IDS = ["-".join(map(str, c)) for c in CASES]


@functools.lru_cache(maxsize=None)
def case(c):
    """(rbm, M, occ, words, w, Estimate, kappa_module): the yardstick, once per case; walkers and weights as test_gpu_rdm._case"""
    sorb, noA, noB, n, H, regime, jregime = c
    occ = T0._occ(sorb, noA, noB, n)
    rbm = R.regime_params(regime, "real", sorb, H, 7)
    M = J.jastrow_params(jregime, sorb, seed=H)
    g = np.random.default_rng([sorb, H, len(regime)])
    w = g.random(occ.shape[0]) + 0.1
    w = w / w.sum()
    est, kmod = estimate(rbm, M, occ, w)
    return rbm, M, occ, R.pack_bits(occ.astype(bool)), w, est, kmod
