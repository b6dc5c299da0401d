"""Host-side yardstick of the fused local-energy and Green's-row kernels (pynqs_eloc_rbm / _flavour, pynqs_eloc_crbm, pynqs_green_rbm;
include/pynqs_amd.h), in numpy longdouble and plain Python: it shares no code with the kernels or with oracle/.

E_loc(x) = h_0 + sum_k h_k r_k over the singles and doubles x'_k of x, r_k = psi(x'_k) / psi(x).
  * structure(): the excitations come from rdm_exact.excitations (plain loops; the sign from applying the operators one by one), the
    matrix elements h_k = s_k sum_t f_t h[slot_t] from the packed integrals in longdouble, the diagonal h_0 = sum_p h1e[pp] +
    sum_{p>q} h2e[tri(pq,pq)].  Next to h_k: a_k = sum_t |h[slot_t]| and t_k = the number of terms.
  * walker(): theta of x in longdouble; theta of x'_k = theta - 2 sum_{o in F_k} W_ho x_o (the 2 or 4 flipped orbitals; in longdouble
    this is the row's own theta to 4 more roundings at 2^-64), then rbm_exact.exact_from_theta -- the very function rbm_exact.exact_ld
    evaluates on a row (tests/test_eloc_exact.py checks the two against each other) -- gives ln psi and tanh theta of every x'.
    |r_k| = exp(Delta Re ln psi), arg r_k = Delta Im ln psi; "tanh": times tanh(a.x') / tanh(a.x); "pRBM": |r_k| = 1.
  * green(): the fixed-node row from the same h_k r_k: g_k = -h_k r_k where h_k r_k < 0, else 0 and h_k r_k goes to v_sf;
    g_0 = max(0, Lambda - h_0 - v_sf); the columns follow an order the caller gives as the bits of every x' (the tests take it from the
    oracle's comb) and are matched to the excitations by those bits -- never by a kernel's output.

The bound, a priori (u = 2^-53; operations counted in kernels_rbm.hip / kernels_rbm_complex.hip; CM = 1 for the real kernel, 3 for complex
arithmetic: a complex product, quotient or fused multiply-add is within 3 u of its modulus, cexp adds exp's and sincos' ulp and
u |Im z| of its argument):
    |E_got - E_exact| <= u [ (t_0 + c_add) a_0 + sum_k a_k ((t_k + kappa_k + c_add + 1) |r_k| + ext_k) ]              per walker,
    |g_k - g_k,exact| <= u a_k ((t_k + kappa_k + 2) |r_k| + ext_k)                                                     per row entry.
t_k: a matrix element is a sum of t_k stored numbers (diagonal: nele one-body and nele (nele - 1) / 2 two-body terms; a single: one
  one-body and nele - 1 two-body terms; a double: one stored number): at most t_k roundings on a_k, whatever the order.
c_add: the additions that collect a walker's columns.  A lane owns blocks of 4 x 4 (complex: 2 x 4) columns and adds them in turn; the
  tiles of 64 blocks go to whichever wave is free, so one lane may see every tile: cpb ntiles additions, cpb = 16 (8), ntiles =
  ceil(blocks / 64), blocks = sum over the four classes (singles; alpha-alpha, beta-beta: hole pairs x particle pairs; alpha-beta:
  alpha singles x beta singles) of ceil(fast / 4 (2)) ceil(slow / 4).  Then 6 steps of the wave butterfly, up to 16 waves, h_0, and on
  the chunked path the atomics of up to ntiles / 4 workgroups in any order:   c_add = cpb ntiles + ntiles + 24.   The "+ 1" is the product h_k r_k.
kappa_k, the relative error of the ratio (for the hidden units' product; absolute error of ln r_k), per hidden unit h:
  1. theta_h is a chain of sorb additions on terms of modulus <= S_h = |b_h| + sum_o |W_ho|: (sorb + 1) u S_h.  The kernel's ratio is an
     exact identity in the computed theta (cosh(theta - delta) / cosh(theta) = e^(-s delta) (m + m rho prod q) for either sign s), so the
     error enters ln r_k through d/dtheta [ln cosh(theta - delta) - ln cosh theta] = tanh theta' - tanh theta:
     (sorb + 1) S_h |tanh theta'_kh - tanh theta_h|, per column from Exact.y of the rows.
  2. the factor F = m + n^4 Q, Q = prod_{o in F} q(o).  m = 1 / (1 + exp(-2 |theta|)): an exponential, an addition, a division: 4 CM u.
     n = (m rho)^(1/4) = exp(-(|theta| + ln 2cosh theta) / 4): the sum of two numbers <= |theta| + 0.7 is rounded twice and goes through
     the exponential, (|theta| + 1.4) u relative, in every one of the four rows; a row is n exp(+-4 W) (4 W exact, an exponential, a
     product: 1.5 CM u); three products join the rows and the fma adds m: n^4 Q carries (4 |theta| + 13 CM) u <= (4 S_h + 13 CM) u.
     Relative to F these weigh |m / F| = |1 - w| and |n^4 Q / F| = |w|, w = (1 - s tanh theta') / 2 (real parameters: w in [0, 1]; complex
     ones: both can exceed 1 next to a zero of cosh theta').  The running product adds CM:
         4 CM |1 - w_kh| + (13 CM + 4 S_h) |w_kh| + CM.
  3. C(o) = exp(-2 x_o (a_o + sum_h s_h W_ho)) for the flipped orbitals: a lane adds its ceil(H / 64) terms s_h W_ho (the products are
     exact) in turn, the butterfly takes 6 steps, a_o joins: at most D = ceil(H / 64) + 7 roundings on sum_h |W_ho| + |a_o|, doubled by the
     factor 2, absolute in the exponent; the exponentials, the products C C and acc C C: 8 CM.
     kappa_k = sum_h [1. + 2.] + 2 D sum_{o in F_k} (sum_h |W_ho| + |a_o|) + 8 CM.
  Hidden units far from zero on the same side for x and x' have tanh theta' = tanh theta and w = 0 to e^(-2 |theta|): they cost 5 CM u, however
  large S_h is -- the coarse 2 (sorb + 3) sum_h S_h of rdm_exact.kappa_fused would be 1e5 u at eight units of -50.
"pRBM": the phase of r_k is ln t of the real flavour's ratio t, so kappa_k u is an ABSOLUTE error of the phase and |r_k| = 1; the logarithm
  adds u |ln t| = u |arg r_k|, sincos_moderate 3 u (two fused reductions by pi / 2 in two parts, exact to 1e-33 k; the polynomial < 1 ulp),
  the products h cos, h sin one more:   kappa_k += |Delta Im ln psi| + 5.
"tanh": r_k = t tanh(a.x') / tanh(a.x), and tanh(a.x') crosses zero, so its error is absolute: exp(2 a.x') = exp(2 a.x) prod exp(-4 x_o a_o)
  carries E u relative, E = 2 sorb sum_o |a_o| + 8 (a.x: sorb additions; five exponentials, four products); through
  tanh y = 1 - 2 / (e^(2y) + 1), d tanh / d ln z = sech^2 / 2, plus the division and the subtraction (2 u absolute):
      ext_k = |t_k| / |tanh(a.x)| (sech^2(a.x') E / 2 + 2),      |t_k| = exp(Delta Re ln psi),
  and 1 / tanh(a.x) carries sorb sum_o |a_o| sech^2(a.x) / |tanh(a.x)| + 2 relative, which joins kappa_k (as do two more products).
psi(x) written by the same kernels: rbm_exact.amp_ratio <= 1, as for pynqs_rbm_forward.
g_0 and E_loc of the Green's row: the walker bound plus 2 u (|Lambda| + A_x) for the two roundings of Lambda - (h_0 + v_sf)."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from math import comb as _binom

import numpy as np

import rbm_exact as R
import rdm_exact as D

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53
_CHUNK = 1024  # columns per call of exact_from_theta (memory: _CHUNK x H longdoubles a few times over)


@dataclass
class Structure:
    """What depends on the determinant and the integrals alone.  flips int [m, 4] (padded with -1); h longdouble [m]; a float64 [m];
    t int64 [m]; h0, a0, t0: the diagonal; bits uint8 [m, sorb]: x' of every column."""
    occ: np.ndarray
    flips: np.ndarray
    h: np.ndarray
    a: np.ndarray
    t: np.ndarray
    h0: np.longdouble
    a0: float
    t0: int
    bits: np.ndarray

    def blocks(self, fast: int) -> int:
        """blocks of fast x 4 columns, from the classes' sizes (module docstring, c_add)"""
        sorb = self.occ.size
        noA, noB = int(self.occ[0::2].sum()), int(self.occ[1::2].sum())
        nvA, nvB = (sorb + 1) // 2 - noA, sorb // 2 - noB
        up = lambda a, b: -(-a // b)  # noqa: E731
        classes = ((noA * nvA + noB * nvB, 1), (_binom(noA, 2), _binom(nvA, 2)), (_binom(noB, 2), _binom(nvB, 2)), (noA * nvA, noB * nvB))
        return sum(up(f, fast) * up(s, 4) for f, s in classes if f and s)

    def c_add(self, cplx: bool) -> float:
        ntiles = -(-self.blocks(2 if cplx else 4) // 64)
        return (8 if cplx else 16) * ntiles + ntiles + 24.0


def structure(occ: np.ndarray, h1e: np.ndarray, h2e: np.ndarray) -> Structure:
    occ = np.asarray(occ, dtype=np.uint8)
    sorb = occ.size
    occupied = [p for p in range(sorb) if occ[p]]
    d1 = [float(h1e[p * sorb + p]) for p in occupied]
    d2 = [float(h2e[D.tri(D.pair_index(p, q), D.pair_index(p, q))]) for a, p in enumerate(occupied) for q in occupied[:a]]
    diag = np.array(d1 + d2, dtype=np.float64)
    ex = D.excitations(occ)
    m = len(ex)
    flips = np.full((m, 4), -1, dtype=np.int64)
    sign = np.zeros(m, dtype=np.float64)
    seg, val = [], []
    for k, (flip, s, targets) in enumerate(ex):
        flips[k, :len(flip)] = flip
        sign[k] = s
        for which, slot, f in targets:
            seg.append(k)
            val.append(f * float((h1e if which == 1 else h2e)[slot]))
    seg, val = np.asarray(seg, dtype=np.int64), np.asarray(val, dtype=np.float64)
    h, a = np.zeros(m, dtype=LD), np.zeros(m, dtype=np.float64)
    np.add.at(h, seg, val.astype(LD))
    np.add.at(a, seg, np.abs(val))
    t = np.bincount(seg, minlength=m).astype(np.int64) if m else np.zeros(0, dtype=np.int64)
    bits = np.repeat(occ[None, :], m, 0)
    for j in range(4):
        rows = np.flatnonzero(flips[:, j] >= 0)
        bits[rows, flips[rows, j]] ^= 1
    return Structure(occ, flips, h * sign.astype(LD), a, t, diag.astype(LD).sum(), float(np.abs(diag).sum()), diag.size, bits)


@dataclass
class Walker:
    """The reference of one walker.  E: complex longdouble; r: complex longdouble [m]; rabs, kappa, ext: float64 [m] (module docstring);
    A = a_0 + sum a_k |r_k|; psi: rbm_exact.Exact of x itself (one row); cross: columns whose hidden units 1 / 2 change the side of zero
    with |theta|, |theta'| > 3 (the regime "cross")."""
    st: Structure
    E: complex
    r: np.ndarray
    rabs: np.ndarray
    kappa: np.ndarray
    ext: np.ndarray
    A: float
    psi: R.Exact
    lnmax: float       # max |Re ln psi| over x and every x'
    vis0: float        # tanh(a.x) ("tanh"), else 1
    ncross: int
    cplx: bool         # the complex kernel's counts

    @property
    def hr(self) -> np.ndarray:
        return self.st.h.astype(CLD) * self.r

    def col_bound(self) -> np.ndarray:
        """u a_k ((t_k + kappa_k + 2) |r_k| + ext_k): a row entry of the Green's kernel"""
        return U * self.st.a * ((self.st.t + self.kappa + 2.0) * self.rabs + self.ext)

    def bound(self) -> float:
        """the bound on |E_got - E_exact|"""
        c = self.st.c_add(self.cplx)
        return U * float((self.st.t0 + c) * self.st.a0 + (self.st.a * ((self.st.t + self.kappa + c + 1.0) * self.rabs + self.ext)).sum())


def _theta(rbm: R.Rbm, x: np.ndarray):
    """(a, b, axr, axi) of the +-1 rows x [n, sorb] in longdouble, as rbm_exact.exact_ld forms them"""
    xl = x.astype(LD)
    if rbm.kind == "complex":
        return (rbm.hb.real.astype(LD) + xl @ rbm.W.real.T.astype(LD), rbm.hb.imag.astype(LD) + xl @ rbm.W.imag.T.astype(LD),
                xl @ rbm.vb.real.astype(LD), xl @ rbm.vb.imag.astype(LD))
    return rbm.hb.astype(LD) + xl @ rbm.W.T.astype(LD), None, xl @ rbm.vb.astype(LD), None


def walker(rbm: R.Rbm, st: Structure, kernel_cplx: "bool | None" = None) -> Walker:
    """kernel_cplx: count the complex kernel's operations (default: for complex parameters; "cos" runs real-valued parameters (i W, i b)
    through it and arrives here as kind "complex")."""
    cplx = rbm.kind == "complex"
    kc = cplx if kernel_cplx is None else kernel_cplx
    CM = 3.0 if kc else 1.0
    sorb, H, m = st.occ.size, rbm.H, st.flips.shape[0]
    x = st.occ.astype(np.float64) * 2 - 1
    a0, b0, axr0, axi0 = _theta(rbm, x[None, :])
    e0 = R.exact_from_theta(rbm, a0, b0, axr0, axi0)
    S = R.hidden_scale(rbm).astype(np.float64)
    s0 = np.where(e0.y[0].real < 0, -1.0, 1.0)
    y0 = e0.y.astype(np.complex128 if cplx else np.float64)
    wsum = (np.abs(rbm.W).sum(0) + np.abs(rbm.vb)).astype(np.float64)
    sum_a = float(np.abs(rbm.vb).sum())
    parts = [rbm.W.real, rbm.W.imag, rbm.vb.real, rbm.vb.imag] if cplx else [rbm.W, None, rbm.vb, None]
    Wt = [None if p is None else np.ascontiguousarray(np.asarray(p).T).astype(LD) for p in parts]  # [sorb, H] x 2, [sorb] x 2
    re, im, vis = np.zeros(m, dtype=LD), np.zeros(m, dtype=LD), np.ones(m, dtype=LD)
    kappa = np.zeros(m)
    crossed = np.zeros(m, dtype=bool)

    def chunk(c0: int) -> None:
        F = st.flips[c0:c0 + _CHUNK]
        mc = F.shape[0]
        th = [None if w is None else np.repeat(base, mc, 0) for w, base in zip(Wt, (a0, b0, axr0, axi0))]
        for j in range(4):
            on = F[:, j] >= 0
            o = np.where(on, F[:, j], 0)
            xo = np.where(on, 2.0 * x[o], 0.0).astype(LD)  # theta' = theta - 2 W_ho x_o
            for i, w in enumerate(Wt):
                if w is not None:
                    th[i] = th[i] - (w[o] * (xo[:, None] if w.ndim == 2 else xo))
        e = R.exact_from_theta(rbm, *th)
        re[c0:c0 + mc], im[c0:c0 + mc], vis[c0:c0 + mc] = e.re, e.im, e.vis
        # (kappa is a bound: float64 serves.  A saturated unit's tanh rounds to +-1 there, and its w to 0 or 1: the truth to e^(-2 |theta|))
        yk = e.y.astype(np.complex128 if cplx else np.float64)
        dy = np.abs(yk - y0)
        w = (1 - s0[None, :] * yk) / 2
        kappa[c0:c0 + mc] = ((sorb + 1) * S[None, :] * dy + 4 * CM * np.abs(1 - w) + (13 * CM + 4 * S[None, :]) * np.abs(w) + CM).sum(1)
        if H >= 3:
            ty, t0y = yk[:, 1:3].real, y0[0, 1:3].real
            big = np.tanh(3.0)
            crossed[c0:c0 + mc] = ((np.sign(ty) != np.sign(t0y)[None, :]) & (np.abs(ty) > big) & (np.abs(t0y)[None, :] > big)).any(1)

    # the chunks are independent and numpy's loops release the interpreter lock: a few threads share them (the same numbers in any order)
    starts = list(range(0, m, _CHUNK))
    if len(starts) > 1:
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            list(pool.map(chunk, starts))
    else:
        for c0 in starts:
            chunk(c0)
    ncross = int(crossed.sum())
    on = st.flips >= 0
    kappa += 2.0 * (-(-H // 64) + 7) * np.where(on, wsum[np.where(on, st.flips, 0)], 0.0).sum(1) + 8 * CM
    ext = np.zeros(m)
    thid = np.exp(re - e0.re[0])
    vis0 = float(e0.vis[0])
    if rbm.kind == "tanh":
        r = (thid * vis / e0.vis[0]).astype(CLD)
        sech2 = (1 - vis * vis).astype(np.float64)
        ext = thid.astype(np.float64) / abs(vis0) * (sech2 * (2 * sorb * sum_a + 8) / 2 + 2)
        kappa += sorb * sum_a * (1 - vis0 * vis0) / abs(vis0) + 4
    elif rbm.kind == "pRBM":
        ph = im - e0.im[0]
        r = np.cos(ph) + 1j * np.sin(ph)
        kappa += np.abs(ph).astype(np.float64) + 5
    else:
        ph = im - e0.im[0]
        r = thid * (np.cos(ph) + 1j * np.sin(ph))
    r = r.astype(CLD)
    rabs = np.abs(r).astype(np.float64)
    E = st.h0 + (st.h.astype(CLD) * r).sum()
    A = st.a0 + float((st.a * rabs).sum())
    lnmax = float(max(np.abs(re).max() if m else 0.0, abs(e0.re[0])))
    return Walker(st, E, r, rabs, kappa, ext, A, e0, lnmax, vis0, ncross, kc)


@dataclass
class Green:
    """The fixed-node row of one walker in the caller's column order.  g [ncomb] (longdouble; g[0] the diagonal), keep [ncomb] bool
    (column 0 False), bound [ncomb] (float64; column 0: the walker bound with Lambda), sure [ncomb] bool: |h_k r_k| exceeds its bound, so
    that the sign decision is not a matter of rounding; v_sf, k0 = Lambda - h_0 - v_sf (unclamped), clamp."""
    g: np.ndarray
    keep: np.ndarray
    bound: np.ndarray
    sure: np.ndarray
    v_sf: np.longdouble
    k0: np.longdouble
    clamp: bool
    perm: np.ndarray  # excitation index of every column >= 1


def match_columns(w: Walker, comb_bits: np.ndarray) -> np.ndarray:
    """excitation index of every column of comb_bits [ncomb, sorb] (0/1; column 0 = x itself), by the bits of x' alone"""
    m = w.st.bits.shape[0]
    assert comb_bits.shape == (m + 1, w.st.occ.size) and bool((comb_bits[0] == w.st.occ).all())
    index = {row.tobytes(): k for k, row in enumerate(np.ascontiguousarray(w.st.bits))}
    assert len(index) == m  # the excitations are distinct determinants
    perm = np.array([index[row.tobytes()] for row in np.ascontiguousarray(comb_bits[1:].astype(np.uint8))], dtype=np.int64)
    assert np.array_equal(np.sort(perm), np.arange(m))
    return perm


def green(w: Walker, lam: float, perm: np.ndarray) -> Green:
    hr = w.hr.real
    keep = hr < 0
    v_sf = hr[~keep].sum()
    k0 = LD(lam) - w.st.h0 - v_sf
    m = hr.size
    g = np.zeros(m + 1, dtype=LD)
    g[1:] = np.where(keep, -hr, 0)[perm]
    g[0] = max(LD(0), k0)
    cb = w.col_bound()
    bound = np.concatenate([[w.bound() + 2 * U * (abs(lam) + w.A)], cb[perm]])
    sure = np.concatenate([[True], (np.abs(hr) > cb)[perm]])
    return Green(g, np.concatenate([[False], keep[perm]]), bound, sure, v_sf, k0, bool(k0 < 0), perm)


def lambda_in_largest_gap(walkers) -> float:
    """Lambda in the middle of the largest gap of the sorted h_0 + v_sf: some walkers clamp, some do not"""
    v = np.sort(np.array([float(w.st.h0 + w.hr.real[w.hr.real >= 0].sum()) for w in walkers]))
    assert v.size >= 2
    i = int(np.argmax(np.diff(v)))
    return float((v[i] + v[i + 1]) / 2)
