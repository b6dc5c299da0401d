"""Host-side yardstick of the reduced density matrices (include/pynqs_amd.h, "reduced density matrices"; pynqs_amd/rdm.py), in numpy
longdouble and plain Python: it shares no code with the kernels.

(a) estimator(): from the definition.  For every walker x (weight w_x) the same-spin singles, same-spin doubles and alpha-beta doubles
are enumerated in plain loops; the sign of <x'| a+_q a_h |x> or <x'| a+_q0 a+_q1 a_h1 a_h0 |x> (h0 > h1, q0 > q1) comes from applying
the operators one by one to the occupation list and counting the occupied orbitals below each; the ratio psi(x') / psi(x) comes from
rbm_exact.exact_ld (or from amplitudes the caller supplies).  Contributions (module docstring of the header):
    x' = x : +w on rdm1[p,p] (p occupied), +w on rdm2[tri(pq,pq)] (p > q occupied);
    single : s w Re r on rdm1[q sorb + h]; s sigma w Re r on rdm2[tri(pair(h,k), pair(q,k))] for every occupied k != h,
             sigma = -1 iff (h > k) != (q > k);
    double : s w Re r on rdm2[tri(pair(h0,h1), pair(q0,q1))].
Next to each slot's value it accumulates A_t = sum |w r| (the modulus of r, also for complex amplitudes: a complex ratio's rounding
error is relative to |r|, not to Re r), the count m_t and kmax_t = the largest per-contribution constant kappa (below) in the slot.

(b) fock_rdm(): for sorb = 8 the Jordan-Wigner matrices of a_p on the 256-dimensional Fock space give g1[p,q] = <psi|a+_p a_q|psi> and
G[P,Q] = <psi|a+_i a+_j a_l a_k|psi>, P = (i > j), Q = (k > l), directly; packed: rdm1[q sorb + p] = g1[p,q] (real psi: symmetric),
rdm2[tri(P,Q)] = G[P,Q] + G[Q,P] for P != Q and G[P,P] on the diagonal -- H = sum_pq h_pq a+_p a_q + sum_{P,Q} <ij||kl> a+_i a+_j a_l a_k
stores <ij||kl> once per unordered {P, Q}.

Tolerance.  |got_t - exact_t| <= c_t u A_t, u = 2^-53, with c_t derived from the operation count, a priori:
  * additions: a slot is the sum of m_t contributions, in any order (atomics) or in walker order plus the two additions that combine
    the directed tables: at most (m_t + 2) u A_t.
  * the contribution itself, relative error kappa u, by path:
    - "ratio" (pynqs_rdm_scatter fed with ratios that are correctly rounded doubles, as the tests do from the longdouble reference):
      the rounding of r (1/2), the product w r (1/2), this reference's own error in units of u (< 1):  kappa = 2.
    - "fused" (pynqs_rdm_rbm): theta_h is a chain of sorb fused multiply-adds on terms of modulus <= S_h = |b_h| + sum_o |W_ho|
      (error (sorb + 1) u S_h), shifted by the owner's two weights (one more rounding of modulus <= S_h and the weights' own sum:
      together (sorb + 3) u S_h).  ln of the ratio depends on theta through tanh theta'' - tanh theta, of modulus <= 2, so theta
      contributes 2 (sorb + 3) sum_h S_h.  Per hidden unit then: the table entries exp(-+4W) (4W exact, exp to 1 ulp: 2 u each, two of
      them and their product: 5 u), a_h and b_h (exp, an addition, a division: 3 u each; every term of b + a g is positive, no
      cancellation), the fma and the running product (2 u), the owner's factor (an exponential, two log1p, two additions on terms that
      the shift bounds: 6 u, taken relative through exp): 12 + 5 + 2 = 19 per unit, rounded up to 20 H.  The two exponentials of the
      lane constant and of the owner's factor carry the absolute error of their arguments, sums of H + 4 terms bounded by
      sum_h |W_ho| and |a_o| over the four orbitals: 4 (H + 4) max_o (sum_h |W_ho| + |a_o|) ... written as 4 (H + 4) Wmax.  The final
      products (w, the two constants, the sign, this reference): 8.
          kappa_fused = 2 (sorb + 3) sum_h S_h + 20 H + 4 (H + 4) Wmax + 8      (one constant for all slots of a case)
    - "module" (pynqs_amd.rdm on its generic path: psi(x') and psi(x) from the module's own forward, then a division): each amplitude
      is exp of a sum of H logarithms of modulus <= |tanh theta_h| S_h + ln 2 plus a.x, i.e. of modulus <= cond(x) + H ln 2 with
      rbm_exact's cond(x); theta as above, the H additions and the functions add (sorb + H + 16) u relative to that sum:
          kappa_module = (sorb + H + 16) (cond(x) + cond(x') + 2 H ln 2) + 4.
  c_t = m_t + 2 + kappa.  Slots with A_t = 0 receive no contribution at all and must be exactly zero."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import rbm_exact as R

LD = np.longdouble
U = 2.0 ** -53


def pair_index(hi: int, lo: int) -> int:
    return hi * (hi - 1) // 2 + lo


def tri(ij: int, kl: int) -> int:
    P, Q = max(ij, kl), min(ij, kl)
    return P * (P + 1) // 2 + Q


def sizes(sorb: int):
    pair = sorb * (sorb - 1) // 2
    return sorb * sorb, pair * (pair + 1) // 2


def _apply(occ: list, ops) -> int:
    """apply (kind, orbital) operators left to right (the rightmost operator of the string first) to the occupation list in place;
    returns the sign, 0 if the string annihilates the state"""
    sign = 1
    for kind, o in ops:
        if occ[o] == (1 if kind == "c" else 0):
            return 0
        if sum(occ[:o]) & 1:
            sign = -sign
        occ[o] = 1 if kind == "c" else 0
    return sign


def excitations(occ: np.ndarray):
    """[(flipped orbitals, sign, targets)] of one determinant; targets = [(which, slot, factor)], which 1 / 2 = rdm1 / rdm2"""
    sorb = occ.size
    o = [int(v) for v in occ]
    occupied = [p for p in range(sorb) if o[p]]
    empty = [p for p in range(sorb) if not o[p]]
    out = []
    for h in occupied:
        for q in empty:
            if (h ^ q) & 1:
                continue
            s = _apply(list(o), [("a", h), ("c", q)])
            targets = [(1, q * sorb + h, 1.0)]
            for k in occupied:
                if k == h:
                    continue
                sigma = -1.0 if (h > k) != (q > k) else 1.0
                targets.append((2, tri(pair_index(max(h, k), min(h, k)), pair_index(max(q, k), min(q, k))), sigma))
            out.append(((h, q), s, targets))
    for a, h0 in enumerate(occupied):
        for h1 in occupied[:a]:
            for b, q0 in enumerate(empty):
                for q1 in empty[:b]:
                    # spin is conserved: the holes' spins are the particles' spins
                    if sorted((h0 & 1, h1 & 1)) != sorted((q0 & 1, q1 & 1)):
                        continue
                    s = _apply(list(o), [("a", h0), ("a", h1), ("c", q1), ("c", q0)])  # a+_q0 a+_q1 a_h1 a_h0 |x>
                    out.append(((h0, h1, q0, q1), s, [(2, tri(pair_index(h0, h1), pair_index(q0, q1)), 1.0)]))
    return out


@dataclass
class Estimate:
    sorb: int
    rdm1: np.ndarray  # longdouble
    rdm2: np.ndarray
    A1: np.ndarray    # float64: sum |contribution|
    A2: np.ndarray
    m1: np.ndarray    # int64: contributions per slot
    m2: np.ndarray
    k1: np.ndarray    # float64: largest kappa_module in the slot
    k2: np.ndarray
    sum_w: float
    kappa_fused: float

    def flat(self):
        return np.concatenate([self.rdm1, self.rdm2])

    def bound(self, path: str) -> np.ndarray:
        """c_t u A_t per slot of (rdm1 | rdm2), float64 (module docstring)"""
        A = np.concatenate([self.A1, self.A2])
        m = np.concatenate([self.m1, self.m2]).astype(np.float64)
        if path == "ratio":
            kappa = 2.0
        elif path == "fused":
            kappa = self.kappa_fused
        else:
            assert path == "module", path
            kappa = np.concatenate([self.k1, self.k2])
        return (m + 2.0 + kappa) * U * A


def kappa_fused(rbm, sorb: int) -> float:
    S = float(R.hidden_scale(rbm).sum())
    wmax = float((np.abs(rbm.W).sum(0) + np.abs(rbm.vb)).max())
    H = rbm.H
    return 2.0 * (sorb + 3) * S + 20.0 * H + 4.0 * (H + 4) * wmax + 8.0


def estimator(occ: np.ndarray, w: np.ndarray, rbm=None, amplitude=None) -> Estimate:
    """(a).  occ: 0/1 [n, sorb]; w [n]; the amplitudes from `rbm` (rbm_exact.Rbm, kind "real" or "complex") through exact_ld, or from
    amplitude(rows 0/1 [m, sorb]) -> complex longdouble [m]."""
    n, sorb = occ.shape
    n1, n2 = sizes(sorb)
    val = [np.zeros(n1, dtype=LD), np.zeros(n2, dtype=LD)]
    A = [np.zeros(n1), np.zeros(n2)]
    m = [np.zeros(n1, dtype=np.int64), np.zeros(n2, dtype=np.int64)]
    km = [np.zeros(n1), np.zeros(n2)]
    wl = np.asarray(w, dtype=np.float64).astype(LD)
    H = rbm.H if rbm is not None else 0
    for i in range(n):
        o = occ[i]
        occupied = [p for p in range(sorb) if o[p]]
        for p in occupied:
            val[0][p * sorb + p] += wl[i]; A[0][p * sorb + p] += abs(float(wl[i])); m[0][p * sorb + p] += 1
        for a, p in enumerate(occupied):
            for q in occupied[:a]:
                t = tri(pair_index(p, q), pair_index(p, q))
                val[1][t] += wl[i]; A[1][t] += abs(float(wl[i])); m[1][t] += 1
        ex = excitations(o)
        if not ex:
            continue
        rows = np.repeat(o[None, :].astype(np.int8), len(ex) + 1, 0)
        for k, (flip, _, _) in enumerate(ex):
            rows[k + 1, list(flip)] ^= 1
        if rbm is not None:
            e = R.exact_ld(rbm, rows.astype(np.float64) * 2 - 1)
            r = np.exp(e.re[1:] - e.re[0]) * (np.cos(e.im[1:] - e.im[0]) + 1j * np.sin(e.im[1:] - e.im[0]))
            kap = (sorb + H + 16) * (e.cond[1:] + e.cond[0] + 2 * H * np.log(2.0)) + 4
        else:
            psi = amplitude(rows)
            r = psi[1:] / psi[0]
            kap = np.full(len(ex), 2.0)
        for k, (_, s, targets) in enumerate(ex):
            c = wl[i] * r[k].real * s
            ca = abs(float(wl[i])) * float(abs(r[k]))
            for which, t, f in targets:
                val[which - 1][t] += c * f
                A[which - 1][t] += ca
                m[which - 1][t] += 1
                km[which - 1][t] = max(km[which - 1][t], float(kap[k]))
    return Estimate(sorb, val[0], val[1], A[0], A[1], m[0], m[1], km[0], km[1], float(wl.sum()),
                    kappa_fused(rbm, sorb) if rbm is not None and rbm.kind == "real" else float("nan"))


def ratio_rows(comb_occ: np.ndarray, rbm) -> np.ndarray:
    """psi(x'_k) / psi(x) for the rows comb_occ [n, ncomb, sorb] (0/1; column 0 = x) as correctly rounded doubles: float64 [n, ncomb]
    for a real RBM, (re, im) pairs [n, ncomb, 2] for complex parameters"""
    n, nc, sorb = comb_occ.shape
    e = R.exact_ld(rbm, comb_occ.reshape(n * nc, sorb).astype(np.float64) * 2 - 1)
    re, im = e.re.reshape(n, nc), e.im.reshape(n, nc)
    mag = np.exp(re - re[:, :1])
    if rbm.kind == "real":
        return mag.astype(np.float64)
    ph = im - im[:, :1]
    return np.ascontiguousarray(np.stack([(mag * np.cos(ph)).astype(np.float64), (mag * np.sin(ph)).astype(np.float64)], -1))


# ---- (b) Fock space ------------------------------------------------------------------------------------------------------------------
def _jw(sorb: int):
    """a_p as dense matrices on the 2^sorb Fock space; basis index = sum_o n_o 2^o; a_p |..n_p..> = (-1)^(sum_{o<p} n_o) n_p |..0..>"""
    dim = 1 << sorb
    idx = np.arange(dim)
    ops = []
    for p in range(sorb):
        a = np.zeros((dim, dim))
        has = (idx >> p) & 1 == 1
        below = np.array([bin(int(v) & ((1 << p) - 1)).count("1") for v in idx])
        src = idx[has]
        a[src ^ (1 << p), src] = np.where(below[has] & 1, -1.0, 1.0)
        ops.append(a)
    return ops


def fock_rdm(occ: np.ndarray, psi: np.ndarray):
    """(rdm1, rdm2) packed, longdouble, of the normalised state sum_x psi_x |x> (real psi) from the Jordan-Wigner matrices"""
    n, sorb = occ.shape
    assert sorb <= 10
    vec = np.zeros(1 << sorb, dtype=LD)
    for o, c in zip(occ, psi):
        vec[int(sum(int(b) << k for k, b in enumerate(o)))] = c
    vec = vec / np.sqrt((vec * vec).sum())
    a = [m.astype(LD) for m in _jw(sorb)]
    av = [m @ vec for m in a]                 # a_q |psi>
    n1, n2 = sizes(sorb)
    rdm1, rdm2 = np.zeros(n1, dtype=LD), np.zeros(n2, dtype=LD)
    for p in range(sorb):
        for q in range(sorb):
            rdm1[q * sorb + p] = av[p] @ av[q]  # <psi| a+_p a_q |psi>
    pairs = [(i, j) for i in range(sorb) for j in range(i)]
    pv = {(k, l): a[l] @ av[k] for k, l in pairs}  # a_l a_k |psi>
    for (i, j) in pairs:
        for (k, l) in pairs:
            P, Q = pair_index(i, j), pair_index(k, l)
            if Q > P:
                continue
            # <psi| a+_i a+_j a_l a_k |psi> = (a_j a_i psi) . (a_l a_k psi)
            g = (a[j] @ av[i]) @ pv[(k, l)]
            rdm2[tri(P, Q)] = g if P == Q else 2 * g  # real psi: G[P,Q] = G[Q,P]
    return rdm1, rdm2
