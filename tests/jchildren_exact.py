"""The cases and the a-priori bound of the Jastrow-RBM children amplitudes (pynqs_jastrow_children_prepare + pynqs_jastrow_children_apply
behind pynqs_rbm_forward_children; include/pynqs_amd.h), shared by tests/test_jchildren_cases.py (no GPU: a host mirror of the formula and
the mistakes that must not pass) and tests/test_gpu_jchildren.py.  Nothing here needs a GPU and nothing depends on a kernel's output.

Yardstick: jrbm_exact.exact_ld -- ln psi_RBM from rbm_exact in longdouble plus x'^T M x' formed DIRECTLY from the +-1 rows of x' and M in
longdouble (jrbm_exact.xmx).  It shares no code with the kernels and does not know about parents or flips.

What is evaluated (row r, parent p, x the PARENT's +-1 values, F the orbitals in which x'_r differs from x_p, |F| <= 4):
    S = M + M^T without its diagonal;  r_o = sum_j S_oj x_j;  q0[p] = tr M + 1/2 sum_o x_o r_o;
    psi[r] = psi_RBM(x'_r) exp(q0[p] + Delta_r),   Delta_r = -2 sum_{i in F} x_i r_i + 4 sum_{i<j in F} S_ij x_i x_j.
A stranger (parent out of range, or |F| > 4 against the named parent): exponent tr M + sum_{i<j} S_ij x'_i x'_j on its own bits.

Roundings, counted in pynqs_amd/csrc/kernels_jastrow_children.hip and kernels_jastrow.hip as written (u = 2^-53; an absolute error of the
exponent is a relative error of psi; R_o = sum_j |S_oj|, and sum_o R_o / 2 = sum_{i<j} |S_ij| <= sum_{i != j} |M_ij|):
  S_oj = M_oj + M_jo        one rounding, u |S_oj| (jastrow_table_kernel); the diagonal is an exact 0.
  r_o                       a chain of sorb fused multiply-adds from 0: the first (onto 0) and the one of S_oo = 0 are exact, so at most
                            sorb - 2 roundings on partial sums <= R_o; with S's own rounding (sorb - 1) u R_o.
  q0                        sum_o x_o r_o: a chain of sorb fused multiply-adds from 0, the first exact: sorb - 1 roundings on <= sum_o R_o,
                            and the r_o's own errors, (sorb - 1) u sum_o R_o: halved, (2 sorb - 2) u sum_{i != j} |M_ij|.  tr M: sorb - 1
                            roundings on sum_i |M_ii|.  fma(0.5, sum, tr M): one rounding on <= sum_ij |M_ij|.  In all at most
                            (2 sorb - 1) u sum_ij |M_ij|: inside the (2 sorb + 4) of jrbm_exact.amp_bound, which leaves 5 u sum_ij |M_ij|.
  lin = sum_{i in F} x_i r_i  a chain of four fused multiply-adds from 0 (empty slots add +-0): at most 3 roundings on <= sum_F R_i, plus
                            the r_i's own (sorb - 1): (sorb + 2) u sum_F R_i; in the exponent times 2 (exact): 2 (sorb + 2).
  pair = sum S_ij x_i x_j   x_i x_j = +-1 exact; a chain of six fused multiply-adds from 0: at most 5 roundings on <= sum |S_ij|, plus S's
                            own one: 6 u sum_{i<j in F} |S_ij|; times 4 (exact): 24.
  Delta = fma(-2, lin, 4 pair)  one rounding on |Delta| <= 2 sum_F R_i + 4 sum |S_ij|: + 2 and + 4.
  q0 + Delta                one rounding on |x'^T M x'| <= sum_ij |M_ij|: one of the 5 left above.
  exp, the product          exp is within one unit in the last place (2 u), the product u; the exponential turns the exponent's error
                            e into e (1 + e / 2 + ..), e < 1e-9 here: 3 u and second-order terms, inside the constant 16.
  Sum for a child:  amp_bound(rbm, M, cond) + u [2 (sorb + 3) sum_{o in F} R_o + 28 sum_{i<j in F} |S_ij| + 16].
  The issue proposed jrbm_exact.kappa_jastrow's constants, 2 (sorb + 1) and 24, counted for the local-energy kernel, where r_o joins an
  exponent directly and the pair factors are exponentials of single entries.  Here the four r_i are first SUMMED (3 roundings) and Delta is
  joined by one more fused multiply-add (1 rounding on both sums): 2 (sorb - 1 + 3) + 2 = 2 (sorb + 3) and 4 x 6 + 4 = 28.  The larger constants are used; neither was set from a measured error.
  A stranger:  sum_{i<j} S_ij x'_i x'_j as sum_i x'_i (sum_{j>i} S_ij x'_j): inner chains at most sorb - 2 roundings on sum_{j>i} |S_ij|, the
  outer chain sorb - 1 on sum_{i<j} |S_ij|, S's own one: at most 2 sorb u sum_{i<j} |S_ij| <= 2 sorb u sum_{i != j} |M_ij|; tr M as above; the
  sum with tr M one rounding: <= (2 sorb + 1) u sum_ij |M_ij|, inside amp_bound's (2 sorb + 4); exp and the product: + 16 u.

Conditions that keep a comparison from passing vacuously, asserted here on the reference alone: every row has |ln psi_RBM| <= R.LN_MAX
(rbm_exact.checked_case), every row has |ln psi_RBM + x'^T M x'| <= R.LN_MAX, every case has exactly its n rows, a non-stranger row differs
from its parent in at most four orbitals and a flip-stranger in more.

A case's rows are a seeded non-periodic GATHER from a pool of children made by rbm_exact.make_children (as tests/children_cases.py): a
wrapped row index cannot land on an equal row.  The reference is evaluated once per pool and gathered per case."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import children_cases as CC
import jrbm_exact as J
import rbm_exact as R

U = J.U
WORKGROUP = 256  # rows of a workgroup of the apply kernel (one thread per row, the grid is not capped: include/pynqs_amd.h)


@dataclass(frozen=True)
class Case:
    name: str
    sorb: int
    H: int
    regime: str       # rbm_exact.regime_params
    jregime: str      # jrbm_exact.J_REGIMES, or "zero" (M = 0) / "diag" (M diagonal)
    nw: int
    n: int
    order: str = "shuffled"
    strangers: bool = False
    seed: int = 0


# word counts and bit edges (make_children: no flip, 2 and 4 flips, the word edges, four flips in one word, flips over all words)
_WORDS = [
    Case("sorb2", 2, 3, "small", "j-asym", 257, 1025),
    Case("sorb12", 12, 3, "small", "j-asym", 257, 1025),
    Case("sorb64", 64, 5, "fe2s2", "j-strong", 257, 1025),
    Case("sorb66", 66, 8, "fe2s2", "j-asym", 257, 1025),
    Case("sorb130", 130, 9, "small", "j-strong", 257, 1025),  # |x^T M x| ~ 218, the RBM ("small") well inside the range
    Case("sorb192", 192, 4, "small", "j-strong", 257, 1025),  # ~ 302
    Case("sorb192-small", 192, 4, "fe2s2", "j-small", 257, 1025),
]
# row counts around the wave and the workgroup (n = 1025 is in every case above)
_ROWS = [Case(f"rows{n}", 12, 3, "small", "j-asym", 257, n) for n in (1, 63, 64, 65, WORKGROUP - 1, WORKGROUP, WORKGROUP + 1)]
_PARENTS = [Case(f"parents-{nw}-{o}", 66, 8, "fe2s2", "j-asym", nw, 2049, order=o) for nw in (1, 257, 5000) for o in CC.ORDERS]
_STRANGERS = [
    Case("strangers-one-word", 12, 9, "fe2s2", "j-asym", 1025, 2049, strangers=True),
    Case("strangers-three-words", 184, 9, "fe2s2", "j-asym", 257, 2049, strangers=True),
]
# theta ~ -50 on the first eight hidden units: rows the RBM kernel recomputes from scratch; the composition must hold on them too
_CHUNK = [Case("chunk-50", 40, 40, "chunk-50", "j-asym", 257, 3000)]
_IDENT = [Case("zero", 66, 8, "fe2s2", "zero", 257, 1025), Case("diag", 66, 8, "fe2s2", "diag", 257, 1025)]
_BY = {c.name: c for c in _WORDS + _ROWS + _PARENTS + _STRANGERS + _CHUNK + _IDENT}
WORD_CASES, ROW_CASES, PARENT_CASES = [c.name for c in _WORDS], [c.name for c in _ROWS], [c.name for c in _PARENTS]
STRANGER_CASES, CHUNK_CASES = [c.name for c in _STRANGERS], [c.name for c in _CHUNK]
COUNT_CASE = "sorb66"
ALL_CASES = list(_BY)
# the cases the mistakes are tried on ("j-asym" and "j-strong"; with "j-small" some mistakes are legitimately small, two orbitals have no
# six pairs to drop, and a case of a handful of rows need not hold a row of every kind)
MISTAKE_CASES = [c.name for c in _BY.values() if c.jregime in ("j-asym", "j-strong") and c.n >= 1025 and c.sorb >= 4]


def case(name: str) -> Case:
    return _BY[name]


def jastrow(c: Case) -> np.ndarray:
    if c.jregime == "zero":
        return np.zeros((c.sorb, c.sorb))
    if c.jregime == "diag":
        return np.diag(np.diag(J.jastrow_params("j-asym", c.sorb, c.seed)))
    return J.jastrow_params(c.jregime, c.sorb, c.seed)


def flips_of(rows: np.ndarray, parents: np.ndarray, sorb: int):
    """(flipped orbitals int [m, 4] padded with -1 -- the lowest four where more differ --, number of differing orbitals [m]) of rows
    against parents (uint64 [m, len] both)"""
    d = (R.pm1(rows, sorb) != R.pm1(parents, sorb))
    nf = d.sum(1)
    out = np.full((rows.shape[0], 4), -1, dtype=np.int64)
    for k, row in enumerate(d):
        o = np.flatnonzero(row)[:4]
        out[k, :o.size] = o
    return out, nf


def kappa_children(M: np.ndarray, flips: np.ndarray) -> np.ndarray:
    """2 (sorb + 3) sum_{o in F} R_o + 28 sum_{i<j in F} |S_ij| + 16 (module docstring), float64 [m]"""
    S = np.abs(J.s_matrix(M)).astype(np.float64)
    sorb = S.shape[0]
    Ro = S.sum(1)
    on = flips >= 0
    F = np.where(on, flips, 0)
    first = np.where(on, Ro[F], 0.0).sum(1)
    second = np.zeros(flips.shape[0])
    for a in range(4):
        for b in range(a + 1, 4):
            second += np.where(on[:, a] & on[:, b], S[F[:, a], F[:, b]], 0.0)
    return 2.0 * (sorb + 3) * first + 28.0 * second + 16.0


def bound(rbm, M: np.ndarray, cond: np.ndarray, flips: np.ndarray, stranger: np.ndarray) -> np.ndarray:
    """the per-row bound on |psi / psi_exact - 1|: a child of its named parent, or (stranger != 0) a row computed from scratch"""
    return J.amp_bound(rbm, M, cond) + U * np.where(stranger != 0, 16.0, kappa_children(M, flips))


@dataclass
class Built:
    case: Case
    n: int
    rbm: object
    M: np.ndarray
    parents: np.ndarray      # uint64 [nw, len]
    rows: np.ndarray         # uint64 [n, len]
    parent: np.ndarray       # int32 [n]: what the kernel is given (strangers: possibly out of range)
    true_parent: np.ndarray  # int32 [n]: the parent a row was made from
    stranger: np.ndarray     # int8 [n]: 0, or 1 + index into children_cases.STRANGER_KINDS
    flips: np.ndarray        # int64 [n, 4] against true_parent, padded with -1
    nflip: np.ndarray        # differing orbitals against true_parent
    ex: R.Exact              # the Jastrow-RBM's reference of the rows (re = ln psi_RBM + x'^T M x')
    ex_rbm: R.Exact          # the RBM's alone
    bound: np.ndarray        # float64 [n]

    def ratio(self, got: np.ndarray, sel=slice(None)) -> np.ndarray:
        """|psi / psi_exact - 1| over the bound per row; inf where the value is not finite"""
        g = np.asarray(got, dtype=np.float64)
        ok = np.isfinite(g)
        err = np.abs(np.where(ok, g, 0).astype(R.LD) / np.exp(self.ex.re[sel]) - 1).astype(np.float64)
        return np.where(ok, err / self.bound[sel], np.inf)


@functools.lru_cache(maxsize=None)
def _pool(sorb, H, regime, jregime, nw, strangers, seed):
    c = Case("", sorb, H, regime, jregime, nw, 0, strangers=strangers, seed=seed)
    g = np.random.default_rng([131, seed, sorb, H, nw])
    parents = R.rand_words(nw, sorb, 11 + seed)
    L = parents.shape[1]
    per = CC.POOL_MAX // CC.ROWS_PER_PARENT
    sub = np.arange(nw) if nw <= per else np.unique(np.concatenate([[0, nw - 1], g.choice(nw, per - 2, replace=False)]))
    pool, ppar, _ = R.make_children(parents[sub], sorb, 5 + seed)
    ppar = sub[ppar].astype(np.int32)
    nreg = pool.shape[0]
    skind = np.zeros(nreg, dtype=np.int8)
    if strangers:
        extra, epar, ekind = [], [], []
        named = np.unique(np.concatenate([[nw - 1], g.choice(nw, min(nw, 24), replace=False)]))
        for p in named:
            for kname in CC.STRANGER_KINDS[3:]:
                if kname == "fall":
                    fl = list(range(sorb))
                elif kname[0] == "f" or L == 1:
                    fl = list(g.choice(sorb, int(kname[1]), replace=False))
                else:
                    lo = 64 * (L - 1)
                    fl = list(g.choice(64, 4, replace=False)) + list(lo + g.choice(sorb - lo, int(kname[1]) - 4, replace=False))
                extra.append(R.flipped(parents[p], [int(o) for o in fl]))
                epar.append(p)
                ekind.append(1 + CC.STRANGER_KINDS.index(kname))
        pool = np.concatenate([pool, np.stack(extra)])
        ppar = np.concatenate([ppar, np.asarray(epar, dtype=np.int32)])
        skind = np.concatenate([skind, np.asarray(ekind, dtype=np.int8)])
    assert pool.shape[0] <= CC.POOL_MAX
    rbm, x, ex_rbm = R.checked_case("real", sorb, H, regime, pool, seed)
    M = jastrow(c)
    q = J.xmx(M, x)
    ex = R.Exact(ex_rbm.kind, ex_rbm.re + q, ex_rbm.im, ex_rbm.vis, ex_rbm.cond, np.zeros(0), np.zeros(0))
    assert float(np.abs(ex.re).max()) <= R.LN_MAX, (sorb, regime, jregime, float(np.abs(ex.re).max()))
    flips, nf = flips_of(pool, parents[ppar], sorb)
    assert int(nf[:nreg].max()) <= 4 and (not strangers or int(nf[nreg:].min()) >= 5)
    return rbm, M, parents, pool, ppar, skind, nreg, ex, CC.gather(ex_rbm, np.arange(pool.shape[0])), flips, nf


@functools.lru_cache(maxsize=None)
def build(name: str) -> Built:
    c = _BY[name]
    rbm, M, parents, pool, ppar, skind, nreg, ex, ex_rbm, flips, nf = _pool(c.sorb, c.H, c.regime, c.jregime, c.nw, c.strangers, c.seed)
    g = np.random.default_rng([137, c.seed, c.sorb, c.H, c.nw, c.n])
    n = c.n
    idx = g.integers(0, nreg, n)
    idx[n // 2] = int(np.flatnonzero(ppar[:nreg] == c.nw - 1)[0])  # the last parent is in use
    if n >= 8:
        idx[1] = int(np.flatnonzero(nf[:nreg] == 0)[0])  # a no-flip child, a two-flip and a four-flip one are in every case
        idx[2] = int(np.flatnonzero(nf[:nreg] == 2)[0])
        if c.sorb >= 4:
            idx[3] = int(np.flatnonzero(nf[:nreg] == 4)[0])
    if c.order == "runs":
        idx = idx[np.argsort(ppar[idx], kind="stable")]
    else:
        assert c.order == "shuffled"
    par = ppar[idx].copy()
    stranger = np.zeros(n, dtype=np.int8)
    if c.strangers:
        for j, i in enumerate(CC.stranger_positions(n)):
            k = j % len(CC.STRANGER_KINDS)
            stranger[i] = 1 + k
            if k < 3:
                par[i] = (-1, c.nw, c.nw + 5)[k]
            else:
                of_kind = np.flatnonzero(skind == 1 + k)
                idx[i] = of_kind[(j // len(CC.STRANGER_KINDS)) % of_kind.size]
                par[i] = ppar[idx[i]]
    rows = np.ascontiguousarray(pool[idx])
    assert rows.shape[0] == n and par.shape == (n,)
    e, er = CC.gather(ex, idx), CC.gather(ex_rbm, idx)
    b = bound(rbm, M, e.cond, flips[idx], stranger)
    out = Built(c, n, rbm, M, parents, rows, par.astype(np.int32), ppar[idx].astype(np.int32), stranger, flips[idx], nf[idx], e, er, b)
    assert bool(((out.nflip <= 4) | (out.stranger >= 4)).all()) and bool((out.nflip[out.stranger >= 4] >= 5).all())
    for a in (out.parents, out.rows, out.parent, out.true_parent, out.stranger, out.flips, out.nflip, out.bound, e.re, er.re):
        a.setflags(write=False)
    return out
