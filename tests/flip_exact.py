"""Host-side yardstick of the fused spin-flip-projected local energy (pynqs_eloc_rbm_signed / _flip, pynqs_eloc_jrbm_flip;
include/pynqs_amd.h), in numpy longdouble:

    E_proj(x) = sum_k h_k [psi(x'_k) + eta eta_m(x'_k) psi(flip x'_k)] / psi(x) / extra_norm^2        (vmc/energy/flip.py, _simple_flip)

over x'_0 = x and the singles and doubles of x; flip exchanges the orbitals 2k <-> 2k+1, eta_m(y) = (-1)^(doubly occupied spatial orbitals).
The excitations and matrix elements come from eloc_exact.structure, psi(x'_k) / psi(x) from eloc_exact.walker (jrbm_exact.walker with a
Jastrow factor), and psi(flip x'_k) by REALLY flipping the bits of x'_k and evaluating the ORIGINAL parameters on those rows
(rbm_exact.exact_ld / jrbm_exact.exact_ld).  No mirrored parameter table enters a value here: the kernels' trick (a second table on the same
walkers, a sign per column) is what is being checked.  Next to E_proj the parts the kernels return on the way:
    E    = sum_k h_k psi(x'_k) / psi(x)                                    the plain pass
    R    = psi(flip x) / psi(x)
    Ebar = sum_k eta_m(x'_k) eta_m(x) h_k psi(flip x'_k) / psi(flip x)     the signed pass
so that E_proj = [E + eta eta_m(x) R Ebar] / extra_norm^2 (tests/test_flip_exact.py checks that the two ways agree).

The bound per walker, a priori (u = 2^-53).  The kernels run eloc_exact's loop twice -- on the table (W, a, b) and on the mirrored table
(W[h][o^1], a[o^1], b), whose excitation k has the ratio psi(flip x'_k) / psi(flip x); the sign sigma_k is exact -- and then combine:
    B_proj = [ B + |R| Bbar + |R| |Ebar| (rel + relbar + 2 CM u) + 2 CM u |R| |Ebar| ] / extra_norm^2 + 4 CM u |E_proj|.
  B, Bbar: eloc_exact.Walker.bound of each pass (Bbar from the operation counts of the pass on the mirrored parameters: the only use of the
    mirrored table in this module, for the BOUND of what the kernel does, never for a value).
  rel, relbar: the relative error of psi(x) and of the mirrored pass' psi as the kernels write them (rbm_exact.amp_bound; "tanh": plus the
    visible factor's absolute term over |tanh(a.x)|; "pRBM": the phase error, absolute, of a unit-modulus number; Jastrow: jrbm_exact.amp_bound);
    the quotient R adds one rounding (CM = 1; complex, "pRBM": CM = 3 per operation).
  The combine: the product R Ebar (CM u |R Ebar|), its sum with E (u |E + ..|), extra_norm^2 and the division (2 u): within
    2 CM u |R| |Ebar| / extra_norm^2 + 4 CM u |E_proj|.
Ebar alone (pynqs_eloc_rbm_signed on the mirrored table): Bbar; its psi: relbar.

Two WRONG variants, for the non-vacuity condition of tests/test_flip_exact.py:
    sigma = +1:      Ebar without the signs (eta_m(x'_k) replaced by eta_m(x))
    E(flip x):       Ebar replaced by the plain local energy of the flipped walker, which equals Ebar only for spin-symmetric integrals."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import eloc_exact as X
import jrbm_exact as J
import rbm_exact as R

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53


def flip_bits(bits: np.ndarray) -> np.ndarray:
    """0/1 [..., sorb] with the orbitals 2k and 2k+1 exchanged"""
    out = np.empty_like(bits)
    out[..., 0::2], out[..., 1::2] = bits[..., 1::2], bits[..., 0::2]
    return out


def eta_m(bits: np.ndarray) -> np.ndarray:
    """(-1)^(number of doubly occupied spatial orbitals), float64 [...]"""
    return 1.0 - 2.0 * ((bits[..., 0::2] & bits[..., 1::2]).sum(-1) & 1)


def sigma_rule(occ: np.ndarray, flips: np.ndarray) -> np.ndarray:
    """The kernel's sign rule, sigma_k = (-1)^pi_k with pi_k = XOR_{o in F} occ(o^1) XOR #(spatial orbitals with both spin orbitals in F):
    for the test of the rule against eta_m(x'_k) eta_m(x) -- never used for the reference."""
    out = np.zeros(flips.shape[0], dtype=np.int64)
    for k, F in enumerate(flips):
        F = [int(o) for o in F if o >= 0]
        out[k] = sum(int(occ[o ^ 1]) for o in F) + sum(1 for o in F if o % 2 == 0 and o + 1 in F)
    return 1.0 - 2.0 * (out & 1)


def mirror_params(rbm: R.Rbm, M=None):
    """(Wm, am, b) with Wm[h][o] = W[h][o^1], am[o] = a[o^1] (and Mm[i][j] = M[i^1][j^1]): the kernels' second table"""
    idx = np.arange(rbm.W.shape[1]) ^ 1
    m = R.Rbm(rbm.kind, np.ascontiguousarray(rbm.W[:, idx]), rbm.hb.copy(), np.ascontiguousarray(rbm.vb[idx]))
    return m, (None if M is None else np.ascontiguousarray(np.asarray(M)[idx][:, idx]))


def _ratios(kind: str, num: R.Exact, den: R.Exact) -> np.ndarray:
    """psi(rows of num) / psi(the one row of den), clongdouble [n]"""
    mod = np.exp(num.re - den.re[0])
    if kind == "tanh":
        return (mod * num.vis / den.vis[0]).astype(CLD)
    ph = num.im - den.im[0]
    if kind == "pRBM":
        return (np.cos(ph) + 1j * np.sin(ph)).astype(CLD)
    return (mod * (np.cos(ph) + 1j * np.sin(ph))).astype(CLD)


def _rel_psi(rbm: R.Rbm, M, e: R.Exact) -> float:
    """the relative error of psi(x) as the kernels write it (module docstring), for the one row of e"""
    sorb = rbm.W.shape[1]
    rel = float(J.amp_bound(rbm, M, e.cond)[0]) if M is not None else float(R.amp_bound(sorb, rbm.H, e.cond)[0])
    if rbm.kind == "tanh":
        vis = float(e.vis[0])
        rel += U * ((sorb + 1) * float(np.abs(rbm.vb).sum()) * (1 - vis * vis) + 1) / abs(vis)
    return rel


@dataclass
class FlipWalker:
    """One walker.  E_proj, E, Ebar, R: clongdouble; w, wbar: eloc_exact.Walker of the two passes (wbar: the mirrored parameters, for the
    bound); sigma float64 [m] = eta_m(x'_k) eta_m(x); open_shell: flip x != x; wrong_sigma, wrong_eflip: E_proj of the two wrong variants."""
    E_proj: complex
    E: complex
    Ebar: complex
    R: complex
    w: X.Walker
    wbar: X.Walker
    sigma: np.ndarray
    eta_m_x: float
    norm: float
    rel: float
    relbar: float
    open_shell: bool
    wrong_sigma: complex
    wrong_eflip: complex

    @property
    def CM(self) -> float:
        return 3.0 if self.w.psi.kind == "pRBM" else 1.0

    def bound_bar(self) -> float:
        return self.wbar.bound()

    def bound(self) -> float:
        cm, r, eb = self.CM, float(abs(self.R)), float(abs(self.Ebar))
        inner = self.w.bound() + r * self.wbar.bound() + r * eb * (self.rel + self.relbar + 2 * cm * U) + 2 * cm * U * r * eb
        return inner / self.norm ** 2 + 4 * cm * U * float(abs(self.E_proj))


def walker(rbm: R.Rbm, st: X.Structure, eta: float, norm: float, M=None, h1e=None, h2e=None) -> FlipWalker:
    """M: the Jastrow matrix or None.  h1e, h2e (packed): for the wrong variant E(flip x), which needs the structure of the flipped walker;
    None: that variant is not evaluated (nan)."""
    kind = rbm.kind
    w = J.walker(rbm, M, st) if M is not None else X.walker(rbm, st)
    ev = (lambda rows: J.exact_ld(rbm, M, rows)) if M is not None else (lambda rows: R.exact_ld(rbm, rows))
    pm = lambda b: b.astype(np.float64) * 2 - 1  # noqa: E731
    fx = ev(pm(flip_bits(st.occ))[None, :])
    m = st.bits.shape[0]
    em_x = float(eta_m(st.occ))
    Rq = _ratios(kind, fx, w.psi)[0]
    h = st.h.astype(CLD)
    if m:
        fk = ev(pm(flip_bits(st.bits)))
        t_over_x = _ratios(kind, fk, w.psi)     # psi(flip x'_k) / psi(x)
        t_over_fx = _ratios(kind, fk, fx)       # psi(flip x'_k) / psi(flip x)
        em_k = eta_m(st.bits)
    else:
        t_over_x = t_over_fx = np.zeros(0, dtype=CLD)
        em_k = np.zeros(0)
    second = st.h0 * em_x * Rq + (h * em_k * t_over_x).sum()          # sum_k h_k eta_m(x'_k) psi(flip x'_k) / psi(x), k = 0 included
    E_proj = (w.E + eta * second) / LD(norm) ** 2
    sigma = em_k * em_x
    Ebar = st.h0 + (h * sigma * t_over_fx).sum()
    wrong_sigma = (w.E + eta * em_x * Rq * (st.h0 + (h * t_over_fx).sum())) / LD(norm) ** 2
    wrong_eflip = complex("nan")
    if h1e is not None:
        stf = X.structure(flip_bits(st.occ), h1e, h2e)
        wf = J.walker(rbm, M, stf) if M is not None else X.walker(rbm, stf)
        wrong_eflip = (w.E + eta * em_x * Rq * wf.E) / LD(norm) ** 2
    rbar, Mbar = mirror_params(rbm, M)
    wbar = J.walker(rbar, Mbar, st) if M is not None else X.walker(rbar, st)
    return FlipWalker(E_proj, w.E, Ebar, Rq, w, wbar, sigma, em_x, float(norm), _rel_psi(rbm, M, w.psi), _rel_psi(rbar, Mbar, wbar.psi),
                      bool((flip_bits(st.occ) != st.occ).any()), wrong_sigma, wrong_eflip)


def dense_reference(rbm: R.Rbm, occ_all: np.ndarray, Hmat: np.ndarray, eta: float, norm: float, M=None) -> np.ndarray:
    """E_proj of every determinant of a COMPLETE space (occ_all 0/1 [D, sorb], Hmat [D, D] = <i|H|j> from the oracle), the reference
    formula evaluated densely: sum_j H_ij [psi(j) + eta eta_m(j) psi(flip j)] / psi(i) / norm^2 with psi from rbm_exact.exact_ld on every
    row and on every flipped row.  longdouble / clongdouble [D]."""
    ev = (lambda rows: J.exact_ld(rbm, M, rows)) if M is not None else (lambda rows: R.exact_ld(rbm, rows))
    p = ev(occ_all.astype(np.float64) * 2 - 1).psi()
    pf = ev(flip_bits(occ_all).astype(np.float64) * 2 - 1).psi()
    num = p + eta * eta_m(occ_all) * pf
    return (Hmat.astype(LD).astype(CLD) @ num) / p / LD(norm) ** 2
