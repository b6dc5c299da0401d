"""Host-side exact reference of stochastic reconfiguration for the Jastrow-RBM (pynqs_jrbm_sr_prepare / _matvec and
pynqs_amd.sr.FusedJastrowRbmSR; include/pynqs_amd.h), psi(x) = exp(a.x + x^T M x) prod_h 2cosh(theta_h): rbm_sr_exact.SrExact with O
extended by the columns x_i x_j.  All in numpy longdouble from the float64 parameters, the +-1 rows and the probabilities alone; nothing
depends on a kernel's output.  (No tests here.)

Layout.  k runs over weights [H][sorb], hidden_bias [H], visible_bias [sorb], jastrow [sorb][sorb]: P = H sorb + H + sorb + sorb^2.
    O_nk = (tanh theta_nh x_no, tanh theta_nh, x_no, x_ni x_nj),   Obar = sum_n p_n O_n,   c = (O - Obar) z,   S v = y = O^T diag(p) c.
S does not depend on M: M enters the module and the energy gradient only (energy_gradient: the RBM blocks from rbm_exact.grad_exact,
the jastrow block from jrbm_exact.grad_exact).  real_form, S_dense, solve and residual are SrExact's own, on the wider O; c and matvec
are restated with pairwise sums (P is up to eight times the RBM's, and solve()'s floor is cond(S + shift) times the residual's rounding).

A-priori bound on the product (written before any kernel output was looked at; u = 2^-53; notation and the RBM blocks as in
rbm_sr_exact's docstring, whose derivation this follows).  With Z the jastrow block of z the kernel forms
    c_n = x.z_a + sum_h t_nh u_nh + q_n - Obar.z,      q_n = x^T Z x = sum_i Z_ii + sum_{i<j} S_ij x_i x_j,   S_ij = Z_ij + Z_ji,
q_n in this form: S_ij is rounded once; thread i mod 8 of the walker adds the entries of row i with the sign of x_j (at most sorb - 1
additions on partial sums <= sum_{j>i} |S_ij|), then the row with the sign of x_i and Z_ii to its share (2 ceil(sorb / 8) additions on
partial sums <= A = sum_ij |Z_ij|); the eight shares are added in turn (8) and their sum joins the RBM sum (1):
    |q_n - q_exact| <= u (1 + (sorb - 1) + 2 ceil(sorb / 8) + 8) A <= u (sorb + 2 ceil(sorb / 8) + 8) A,
and the additions that join q_n, x.z_a, the hidden units' shares and Obar.z now act on partial sums bounded by M_n + A.  Obar.z runs over
the longer vector (P / 256 terms per thread with the new P) and carries Obar's error on the jastrow block too.  So
    ec_n = rbm_sr_exact's ec_n with  M_n -> M_n + A,  P -> H sorb + H + sorb + sorb^2,  sum_k over all four blocks,
           + u (sorb + 2 ceil(sorb / 8) + 8) A.
The jastrow entries of y are sums of +-g_n, g_n = p_n c_n, over the walkers -- no tanh --, which is the visible-bias form:
    |y_ij - exact| <= u (4 + adds) sum_n p_n |c_n| + sum_n p_n ec_n,     adds = 42 + n / 128 + world,
the same number for every (i, j) (the kernel forms i <= j and writes (j, i) from the same sum); Obar's jastrow entries likewise with
p_n for p_n |c_n| and no carried error:  bobar_ij = u (4 + adds) sum_n p_n.  The table's bound is rbm_sr_exact's (prepare forms tanh theta
as before).  Probes whose exact product vanishes (a unit vector on M's diagonal: O_ii = 1 = Obar_ii; an antisymmetric Z with zero RBM
blocks: S_ij = 0 exactly, so q_n = 0 and c_n = -Obar.z) leave y = (1 - sum_n p_n) Obar c-terms at rounding level: for those the bound
is checked as an absolute one, at most 1e-12 sum_k |v_k|, as for one walker.  On every other probe of every case the bound must stay
below 1e-9 max_k |y_k| (tests/test_jrbm_sr_exact.py)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import jrbm_exact as J
import rbm_exact as R
import rbm_sr_exact as SE

LD, U = R.LD, R.U
SOLVE_FLOOR = SE.SOLVE_FLOOR


@dataclass
class JSrExact(SE.SrExact):
    """SrExact on O = (RBM columns, x_i x_j); rbm is the real RBM of the module's weights and biases"""

    @property
    def sorb(self) -> int:
        return self.x.shape[1]

    @property
    def nrbm(self) -> int:
        return self.rbm.H * self.sorb + self.rbm.H + self.sorb

    def c(self, v) -> np.ndarray:
        """(O - Obar) z with pairwise sums over the P terms (numpy's sum along the contiguous axis): sorb^2 more columns than the RBM's,
        and the refined solve's floor is cond(S + shift) times the rounding of this residual"""
        z = self.to_z(v)
        return (self.O * z[None, :]).sum(1) - (self.Obar * z).sum()

    def matvec(self, v) -> np.ndarray:
        """S v, flat longdouble, pairwise sums over the walkers too"""
        if getattr(self, "_OT", None) is None:
            self._OT = np.ascontiguousarray(self.O.T)
        g = self.p * self.c(v)
        return (self._OT * g[None, :]).sum(1)

    def _assemble(self, wgt, extra, ay, tanh_term, sorb, adds):
        rbm_part = super()._assemble(wgt, extra, ay, tanh_term, sorb, adds)
        return np.concatenate([rbm_part, np.full(sorb * sorb, U * (4 + adds) * wgt.sum() + extra.sum())])

    def product_bound(self, v) -> np.ndarray:
        """flat [P]: the bound on |(S v)_k - (S v)_exact_k| of the module docstring"""
        n, sorb, H, ay, S, adds, tanh_term = self._pieces()
        p = self.p.astype(np.float64)
        az = np.abs(np.asarray(v, dtype=np.float64).reshape(-1))
        aW, ab = az[:H * sorb].reshape(H, sorb), az[H * sorb:H * sorb + H]
        aa, A = az[H * sorb + H:self.nrbm], float(az[self.nrbm:].sum())
        Zh = ab + aW.sum(1)
        dotabs = float((np.abs(self.Obar).astype(np.float64) * az).sum())
        M = ay @ Zh + aa.sum() + dotabs + A
        ec = U * ((ay * ((sorb + 1) * Zh)[None, :]).sum(1)
                  + ((8 * np.maximum(1.0, ay) + (sorb + 2) * S[None, :] * self.ex.sech2) * Zh[None, :]).sum(1)
                  + (H / 8 + 20) * M + (sorb + 1) * aa.sum() + (self.P / 256 + 12) * dotabs
                  + (sorb + 2 * ((sorb + 7) // 8) + 8) * A) + float((self.obar_bound() * az).sum())
        pc = p * np.abs(self.c(v)).astype(np.float64)
        return self._assemble(pc, p * ec, ay, tanh_term, sorb, adds)


def sr_exact(rbm, x: np.ndarray, prob: np.ndarray, world: int = 1) -> JSrExact:
    assert rbm.kind == "real"
    base = SE.sr_exact(rbm, x, prob, world)
    n, sorb = x.shape
    xl = x.astype(LD)
    O = np.concatenate([base.O, (xl[:, :, None] * xl[:, None, :]).reshape(n, sorb * sorb)], 1)
    return JSrExact(rbm, x, base.p, base.ex, O, base.p @ O, world)


def energy_gradient(se: JSrExact, M: np.ndarray, prob, eloc, e_total, powc=None) -> np.ndarray:
    """F, flat longdouble: what FusedJastrowRbmGrad returns (the RBM blocks 2 G from rbm_exact.grad_exact, the jastrow block from
    jrbm_exact.grad_exact, whose G carries the factor 2)"""
    ge = R.grad_exact(se.rbm, se.x, prob, eloc, e_total, powc)
    gj = J.grad_exact(M, se.x, prob, eloc, e_total, powc)
    return np.concatenate([2 * ge.GW.real.reshape(-1), 2 * ge.Ghb.real, 2 * ge.Gvb.real, gj.G.reshape(-1)]).astype(LD)


def gradient_bound(se: JSrExact, M: np.ndarray, prob, eloc, e_total) -> np.ndarray:
    """flat [P]: the bounds of rbm_exact.grad_exact (x2: F = 2 G) and jrbm_exact.grad_exact on the entries of F"""
    ge = R.grad_exact(se.rbm, se.x, prob, eloc, e_total)
    gj = J.grad_exact(M, se.x, prob, eloc, e_total)
    return np.concatenate([2 * ge.bW.reshape(-1), 2 * ge.bhb, 2 * ge.bvb, np.full(se.sorb ** 2, gj.bound)])


# ---- seeded inputs shared by tests/test_jrbm_sr_exact.py and tests/test_gpu_jrbm_sr.py -------------------------------------------------
# (sorb, electrons per spin, H, n): the smallest shapes that cross the word boundaries (64, 128), the 32-walker workgroup, the
# 32-hidden-unit pass and the LDS limit for Z (sorb 120 stages it, sorb 184 reads it from global memory)
CASES = [(12, 3, 5, 64), (40, 15, 80, 1000), (40, 15, 37, 31), (40, 15, 80, 1), (66, 10, 7, 33), (72, 6, 9, 65), (120, 30, 70, 300),
         (184, 46, 33, 130)]
# (sorb, electrons per spin, H, n) for the product tests alone: sorb 13, the row of the paired-rows triangle that pairs with itself (odd
# sorb); sorb 128, the largest Z staged in LDS (66 048 bytes); sorb 129, the first read from global memory, odd and three words; n = 2049,
# 65 workgroups: the reduce kernel's second trip with its (i, j) and (j, i) writes.  H = 33: one unit in a second pass.
PRODUCT_SHAPES = [(13, 3, 5, 64), (128, 30, 33, 64), (129, 30, 33, 65), (12, 3, 5, 2049)]
# the real saturated regimes of rbm_sr_exact.SATURATED: (sorb, H, n, regime)
SATURATED = [c[1:] for c in SE.SATURATED if c[0] == "real"]


def case_inputs(sorb: int, no: int, H: int, n: int):
    """(rbm, M, words, prob, eloc, e_total): rbm_sr_exact.case_inputs("real", ...) and M from jrbm_exact.jastrow_params("j-asym")"""
    rbm, words, prob, eloc, e_total = SE.case_inputs("real", sorb, no, H, n)
    if sorb % 2:  # bench.synth_walkers fills sorb // 2 orbitals per spin: the last orbital of an odd sorb would be empty in every walker
        words = R.rand_words(n, sorb, 17)
    return rbm, J.jastrow_params("j-asym", sorb), words, prob, eloc, e_total


def saturated_inputs(sorb: int, H: int, n: int, regime: str):
    rbm, words, prob, eloc, e_total = SE.saturated_inputs("real", sorb, H, n, regime)
    return rbm, J.jastrow_params("j-asym", sorb), words, prob, eloc, e_total


DEGENERATE = ("unit M diag", "antisymmetric Z")  # probes whose exact product vanishes up to 1 - sum p


def probe_vectors(se: JSrExact, seed: int = 9):
    """[(name, v flat float64)]: random; a unit vector in each of the four blocks (off-diagonal for M); zero; a unit vector on M's
    diagonal; a random antisymmetric Z with zero RBM blocks"""
    g = np.random.default_rng([seed, se.P])
    H, sorb, nr = se.rbm.H, se.sorb, se.nrbm
    out = [("random", g.standard_normal(se.P))]
    i, j = sorb // 3, (2 * sorb) // 3 + 1
    assert i != j and j < sorb
    for name, k in (("unit W", (H // 2) * sorb + sorb // 3), ("unit hb", H * sorb + H - 1), ("unit vb", H * sorb + H + sorb // 2),
                    ("unit M", nr + i * sorb + j)):
        v = np.zeros(se.P)
        v[k] = 1.0
        out.append((name, v))
    out.append(("zero", np.zeros(se.P)))
    v = np.zeros(se.P)
    v[nr + (sorb // 2) * (sorb + 1)] = 1.0
    out.append(("unit M diag", v))
    a = g.standard_normal((sorb, sorb))
    v = np.zeros(se.P)
    v[nr:] = (a - a.T).reshape(-1)
    out.append(("antisymmetric Z", v))
    return out
