"""Host-side yardstick of the local-energy kernels that take their amplitudes from a table or a list: the SAMPLE_SPACE entries
(pynqs_eloc_sample_space, _hash, _flip, _hash_flip, _keys, _indexed; kernels_eloc.hip, kernels_eloc_keys.hip) and the contraction of the
REDUCE front end (pynqs_reduce_contract; kernels_reduce_onepass.hip), in numpy longdouble and plain Python.  It shares no code with the
kernels or with oracle/: the excitations, their signs and the matrix elements come from eloc_exact.structure (rdm_exact.excitations),
membership in the table is decided by comparing determinant bits on the host, and every quotient is formed in longdouble, whose
exponent range (to 1e4932) is immune to the amplitude scales 2^k the tests run: E_loc is homogeneous of degree 0 in psi.

Per walker x with columns k = 0 (x itself, h_0 = <x|H|x>) and k >= 1 (the singles and doubles x'_k, h_k = <x|H|x'_k>):
  * plain sum      E(x) = sum_{k: x'_k in S} h_k psi(x'_k) / psi(x),  psi(x) = the table's value of x (0 if x is not in S);
  * partner sum    sum_k h_k eta(x'_k) t(flip x'_k) / t(x): flip exchanges the occupations of the orbitals 2j and 2j + 1, eta =
                   (-1)^(doubly occupied spatial orbitals of x'), t(x) is given by the caller (the kernels' psi0 input);
  * REDUCE form    sum over the kept columns |h_k| >= eps of h_k A(x'_k), plus sum over the drawn columns of (c_k / N) sign(h_k) S A(x'_k),
                   S = sum_{|h_j| < eps} |h_j|, all over A(x).  Which columns were drawn and their integer hit counts c_k are discrete
                   selection data the caller reads from the front end's records; S, the weights, the sum and the quotient are formed here.

The bound, a priori (u = 2^-53; first order in u, as in eloc_exact.py; operations counted in the three .hip files):
    |E_got - E_exact| <= [ sum_k dw_k |A_k| + m u sum_k wabs_k |A_k| ] / |A(x)| + c_q u |E_exact|.
  dw_k, the error of the weight the kernel multiplies A_k with:
    - a matrix element is a sum of t_k stored numbers (diagonal: nele + nele (nele - 1) / 2; a single: nele; a double: one), in any order
      (fast_diag / fast_single / finish_double; the key-major kernel's diagonal() and its singles loop): at most t_k roundings on
      a_k = sum |stored terms|:  dw_k = t_k u_T a_k, u_T the unit of the integrals' type (the front end's records of float32 integrals
      are float32 sums: u_T = 2^-24; the SAMPLE_SPACE kernels are float64 only).  wabs_k = a_k >= |h_k|.
    - a drawn record's weight is c_k (S / N) (reduce_draw.h, reduce_list.h: `scale = Srow / nsample`, `scale * hits`, a cast to the
      records' type): S is a float64 sum of the m_s sub-eps |h_j| in any order, (m_s - 1) u S, of elements that carry t_j u_T a_j each;
      a division, a product (2 u) and the cast (u_T):  dw_k = (c_k / N) (sum_j t_j u_T a_j + (m_s + 1) u S) + u_T |w_k|.  wabs_k = |w_k|.
  m u sum wabs |A|: the product w_k A_k (LookupSink::accumulate, Candidates::add: `re += h * vr`; the key-major kernel and the
    contraction: fma / `ar += w * re`; one rounding at most, on real and imaginary part separately, so the modulus of the error is
    within u of the modulus of the term) and the additions.  m counts the non-zero terms; adding a zero is exact.  The tile scheduler
    gives a lane whatever tiles are free, the lanes meet in a butterfly, the waves in LDS, the chunks of a walker through float atomics
    on a zeroed word: the order is free.  In ANY order a term passes through at most m - 1 inexact additions (each one merges the group
    of terms it belongs to with another non-empty group), each within u of a partial sum of modulus <= sum wabs |A|: (m - 1) u, and
    1 u for the product.
  c_q, the quotient: 1 for real amplitudes (one division), 3 for complex ones.  (3 u is the figure of a complex quotient that is formed
    without intermediate cancellation; the textbook form (a conj b) / |b|^2 the kernels keep -- after rescaling numerator and divisor by
    one power of two, which is exact -- spends two roundings on each part of the numerator, two on |b|^2 and one on the division,
    (3 + 2 sqrt 2) u on the modulus in the worst case.  The tests hold the kernels to 3 u: the stricter figure.)
  psi(x) as returned by the kernels is a copy of the table's value: bit-exact.
Power-of-two scaling: with A -> 2^k A every product, sum and quotient above scales exactly unless something under- or overflows, so a
kernel that adds in a fixed order must return THE SAME BITS at every k; the yardstick's own E must not move by more than the roundings
of longdouble quotients of exactly scaled numbers (none: asserted to 4 ulps in tests/test_ss_exact.py).
The RBM end-to-end case (amplitudes from pynqs_rbm_forward[_children] or the module, then the contraction): each amplitude is within
rbm_exact.amp_bound(sorb, H, cond) of its exact value, relative; the bound above with dw_k += (amp_bound(x'_k) + amp_bound(x)) a_k and the
quotient's c_q u per term (the unfused path divides column by column)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

import eloc_exact as X

LD, CLD, U = X.LD, X.CLD, X.U
U32 = 2.0 ** -24


def scaled(values: np.ndarray, k: int) -> np.ndarray:
    """values 2^k in the values' own type (float64 / complex128: the kernels' input; longdouble: the yardstick's); exact unless it
    leaves the type's range"""
    v = np.asarray(values)
    if np.iscomplexobj(v):
        return np.ldexp(v.real, k) + 1j * np.ldexp(v.imag, k)
    return np.ldexp(v, k)


def as_ld(values: np.ndarray) -> np.ndarray:
    return np.asarray(values).astype(CLD if np.iscomplexobj(values) else LD)


def flip_bits(bits: np.ndarray) -> np.ndarray:
    """occupations of the orbitals 2j and 2j + 1 exchanged; bits uint8 [m, sorb], sorb even"""
    m, sorb = bits.shape
    return np.ascontiguousarray(bits.reshape(m, sorb // 2, 2)[:, :, ::-1].reshape(m, sorb))


def eta(bits: np.ndarray) -> np.ndarray:
    """(-1)^(doubly occupied spatial orbitals), float64 [m]"""
    return 1.0 - 2.0 * ((bits[:, 0::2] & bits[:, 1::2]).sum(1) & 1)


class Table:
    """the sample space: distinct determinants (uint8 0/1 [nk, sorb]); find() compares bits"""

    def __init__(self, key_bits: np.ndarray) -> None:
        self.bits = np.ascontiguousarray(key_bits, dtype=np.uint8)
        self.index = {row.tobytes(): i for i, row in enumerate(self.bits)}
        assert len(self.index) == self.bits.shape[0], "keys must be distinct"

    def find(self, bits: np.ndarray) -> np.ndarray:
        """position of every row of bits in the table, -1 if it is not there"""
        get = self.index.get
        return np.array([get(row.tobytes(), -1) for row in np.ascontiguousarray(bits, dtype=np.uint8)], dtype=np.int64)


@dataclass
class Columns:
    """A walker's columns against a table (what does not depend on the amplitudes): pos [m + 1] of x'_k (flip: of flip x'_k) in the
    table, -1 if absent; column 0 is x itself.  w longdouble: the weights h_k (flip: eta h_k); dw, wabs float64 (module docstring)."""
    st: X.Structure
    pos: np.ndarray
    w: np.ndarray
    dw: np.ndarray
    wabs: np.ndarray


def columns(st: X.Structure, table: Table, flip: bool = False) -> Columns:
    bits = np.concatenate([st.occ[None, :], st.bits])
    h = np.concatenate([[st.h0], st.h]).astype(LD)
    a = np.concatenate([[st.a0], st.a])
    t = np.concatenate([[st.t0], st.t]).astype(np.float64)
    if flip:
        h = h * eta(bits).astype(LD)
        bits = flip_bits(bits)
    return Columns(st, table.find(bits), h, U * t * a, a)


@dataclass
class Result:
    """E: complex longdouble (meaningless where zero is set); psi: the divisor; zero: the divisor is 0 (the kernels must return a
    non-finite value); A = sum wabs |A_k| / |A(x)|; m: non-zero terms; bound: on |E_got - E| (module docstring); top: the largest
    modulus of a term or of the sum (no sum may reach 2^1023), low: the smallest non-zero |w_k A_k| (none may be subnormal)."""
    E: complex
    psi: complex
    zero: bool
    A: float
    m: int
    bound: float
    top: float
    low: float


def contract(w: np.ndarray, dw: np.ndarray, wabs: np.ndarray, amp: np.ndarray, psi_x, cplx: bool, per_term_cq: bool = False) -> Result:
    """sum_k w_k amp_k / psi_x with its bound; w longdouble [m], dw, wabs float64 [m], amp (complex) longdouble [m]"""
    amp = amp.astype(CLD)
    aabs = np.abs(amp)
    terms = w.astype(CLD) * amp
    live = (wabs > 0) & (aabs > 0)
    m = int(live.sum())
    num = terms.sum()
    T = (wabs.astype(LD) * aabs).sum()
    top = float(np.log2(T)) if T > 0 else -np.inf
    tl = np.abs(terms[np.abs(terms) > 0])
    low = float(np.log2(tl.min())) if tl.size else np.inf
    psi_x = CLD(psi_x)
    if psi_x == 0:
        return Result(CLD(np.nan), psi_x, True, float("nan"), m, float("nan"), top, low)
    E = num / psi_x
    px = np.abs(psi_x)
    cq = 3.0 if cplx else 1.0
    err = ((dw.astype(LD) * aabs).sum() + (m + (cq if per_term_cq else 0.0)) * U * T) / px + cq * U * np.abs(E)
    return Result(E, psi_x, False, float(T / px), m, float(err), top, low)


def table_sum(c: Columns, values_ld: np.ndarray, psi_x=None) -> Result:
    """the plain sum (psi_x None: psi(x) is the table's value of column 0) or, for columns(..., flip=True), the partner sum over the
    caller's psi_x; values_ld: the table's amplitudes, (complex) longdouble [nk]"""
    cplx = np.iscomplexobj(values_ld)
    amp = np.where(c.pos >= 0, values_ld[np.maximum(c.pos, 0)], 0)
    return contract(c.w, c.dw, c.wabs, amp, amp[0] if psi_x is None else psi_x, cplx)


# ---- REDUCE -----------------------------------------------------------------------------------------------------------------------
def eps_in_largest_gap(structs, lo: float = 0.25, hi: float = 0.75):
    """(eps, half width): the middle of the largest gap between consecutive |h_k| of all the walkers' columns, among the gaps whose
    lower end lies between the quantiles lo and hi of the |h_k| that do not exceed the smallest |<x|H|x>| (some columns are kept, some are
    not, <x|H|x> of every walker is, and no |h_k| is within half the gap of eps)"""
    v = np.sort(np.concatenate([np.abs(np.concatenate([[s.h0], s.h])).astype(np.float64) for s in structs]))
    v = v[v <= min(abs(float(s.h0)) for s in structs)]  # (column 0 brings psi(x): it stays among the kept)
    assert v.size >= 8
    i0, i1 = int(lo * v.size), int(hi * v.size)
    i = i0 + int(np.argmax(np.diff(v[i0:i1 + 1])))
    return float((v[i] + v[i + 1]) / 2), float((v[i + 1] - v[i]) / 2)


def weight_margin(st: X.Structure, u_t: float) -> float:
    """the largest rounding error of a computed |h_k| of this walker: a column whose |h_k| is farther than this from eps is kept or
    dropped alike in float32, float64 and longdouble"""
    return float(u_t * max(st.t0 * st.a0, float((st.t * st.a).max()) if st.t.size else 0.0))


def reduce_columns(st: X.Structure, table: Table, eps: float, drawn: Optional[dict] = None, N: int = 0, u_t: float = U) -> Columns:
    """The REDUCE form's weights.  drawn: {column k (0 = x itself, k >= 1: excitation k - 1 of st): hits c_k} read from the records."""
    c = columns(st, table)
    h, a = c.w, c.wabs
    t = np.concatenate([[st.t0], st.t]).astype(np.float64)
    kept = np.abs(h) >= LD(eps)
    w = np.where(kept, h, LD(0))
    dw = np.where(kept, u_t * t * a, 0.0)
    wabs = np.where(kept, a, 0.0)
    if drawn:
        sub = ~kept
        S = np.abs(h[sub]).sum()
        dS = float((u_t * t[sub] * a[sub]).sum()) + (int(sub.sum()) + 1) * U * float(S)
        assert sum(drawn.values()) == N and N > 0
        for k, hits in drawn.items():
            assert sub[k] and hits >= 1, (k, hits)
            w[k] = LD(hits) / LD(N) * np.sign(h[k]) * S
            wabs[k] = float(abs(w[k])) * (1 + 2 * u_t)
            dw[k] = hits / N * dS + u_t * wabs[k]
    return Columns(st, c.pos, w, dw, wabs)


def row_sum(st: X.Structure, eps: float) -> np.longdouble:
    h = np.concatenate([[st.h0], st.h]).astype(LD)
    return np.abs(h[np.abs(h) < LD(eps)]).sum()


def rbm_reduce(w: X.Walker, cond_rows: np.ndarray, H: int) -> Result:
    """eps = 0 through an RBM: E and the ratios from eloc_exact.walker (log domain), the amplitudes' own errors from rbm_exact.amp_bound;
    cond_rows float64 [m + 1]: rbm_exact's cond of x and of every x'"""
    import rbm_exact as R

    st = w.st
    sorb = st.occ.size
    ab = R.amp_bound(sorb, H, cond_rows)
    a = np.concatenate([[st.a0], st.a])
    t = np.concatenate([[st.t0], st.t]).astype(np.float64)
    r = np.concatenate([[CLD(1)], w.r])
    res = contract(np.concatenate([[st.h0], st.h]).astype(LD), U * t * a + (ab + ab[0]) * a, a, r, CLD(1), True, per_term_cq=True)
    assert abs(complex(res.E - w.E)) <= 64 * R.U_LD * res.A
    return res
