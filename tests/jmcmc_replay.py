"""Host side of the Jastrow-RBM chain tests (pynqs_mcmc_jrbm): exact ln|psi| of psi(x) = exp(a.x + x^T M x) prod_h 2cosh(theta_h) for
mcmc_replay.replay, which is used as it is.  ln|psi| = ln|psi_RBM| + x^T M x straight from M (not from the kernel's S = M + M^T), in
numpy longdouble, or with mpmath where the set of states is small (mcmc_replay.MP_WORK, the rule of mcmc_replay.Rbm); the longdouble
values are spot-checked against mpmath as there.

The tie window stays tau = 1e-10 (scale(x) + scale(x')) with
    scale = scale_RBM + sum_{i<j} |M_ij + M_ji| + |tr M|,
a bound on |x^T M x| that no state exceeds.  It is a priori: the kernel's Jastrow difference is a sum of at most 4 sorb + 6 terms
bounded by the entries of S, so its rounding error is below (4 sorb + 8) 1.1e-16 sum|S| < 1e-13 scale at sorb 192, and ln|psi|
accumulates at most 4096 such updates in the longest launch tested: < 5e-13 scale."""
from __future__ import annotations

from dataclasses import dataclass

import mpmath
import numpy as np

import mcmc_replay as R


@dataclass
class JRbm:
    """W [H, sorb], hb [H], vb [sorb], M [sorb, sorb] float64 (any real matrix).  The interface of mcmc_replay.Rbm."""
    W: np.ndarray
    hb: np.ndarray
    vb: np.ndarray
    M: np.ndarray

    @property
    def H(self) -> int:
        return self.W.shape[0]

    @property
    def rbm(self) -> R.Rbm:
        return R.Rbm("real", self.W, self.hb, self.vb)

    @property
    def jastrow_scale(self) -> float:
        S = self.M + self.M.T
        return float(np.abs(np.triu(S, 1)).sum() + abs(np.trace(self.M)))

    def lnabs_ld(self, x: np.ndarray):
        ld, scale = self.rbm.lnabs_ld(x)
        xl = x.astype(np.longdouble)
        xmx = ((xl @ self.M.astype(np.longdouble)) * xl).sum(1)
        return ld + xmx, scale + self.jastrow_scale

    def lnabs_mp(self, row: np.ndarray) -> mpmath.mpf:
        mp = mpmath.mp
        r = self.rbm.lnabs_mp(row)
        with mpmath.workdps(R.MP_DPS):
            xs = [int(v) for v in row]
            terms = [mp.mpf(float(self.M[i, j])) if xs[i] * xs[j] > 0 else -mp.mpf(float(self.M[i, j]))
                     for i in range(len(xs)) for j in range(len(xs))]
            return mp.fsum([r] + terms)

    def lnabs(self, x: np.ndarray, rng: np.random.Generator, nspot: int = 8):
        """(ln|psi| longdouble [n], scale [n], source) of the +-1 rows x: mpmath for all rows when the work is small, else longdouble with
        `nspot` rows checked against mpmath (to 1e-4 tau)."""
        ld, scale = self.lnabs_ld(x)
        if x.shape[0] * self.H * x.shape[1] <= R.MP_WORK:
            idx, source = np.arange(x.shape[0]), "mpmath"
        else:
            idx, source = rng.choice(x.shape[0], size=min(nspot, x.shape[0]), replace=False), "longdouble"
        for k in idx:
            m = self.lnabs_mp(x[k])
            err = abs(float(m - mpmath.mpf(str(ld[k])))) if np.isfinite(ld[k]) else np.inf
            assert err <= 1e-4 * R.TAU * scale[k], (k, float(m), ld[k], err)
            if source == "mpmath":
                ld[k] = np.longdouble(mpmath.nstr(m, 30))
        return ld, scale, source
