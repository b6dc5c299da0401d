"""The cases of tests/test_gpu_children_shapes.py (pynqs_rbm_forward_children where its control flow depends on the sizes: a second sweep of
the capped grid, the last workgroup / group of sixteen rows, the device count, many parents, strangers, the raised flag) and their exact
reference, shared with tests/test_children_cases.py, which checks on the CPU that every case is what its name says.  Nothing here needs a
GPU and nothing depends on a kernel's output.

A case's rows are a seeded random GATHER from a pool of at most POOL_MAX children, built with the recipe of rbm_exact.make_children (the
parent itself, flips at the word edges, four flips in one word, flips spread over all words): the pattern is not periodic, so a row index
that wrapped (i mod sweep, i - 1, ...) cannot land on an equal row by construction -- test_children_cases.py verifies it for every case.
The reference is evaluated ONCE on the pool (rbm_exact.checked_case: finiteness and conditioning asserted on the reference alone) and
gathered per row (gather).  The sweep sizes come from the library (pynqs_rbm_forward_children_geometry, a host entry), never from a
number written here: n = ("table", k) is k rows past one sweep of the table route, ("scratch", k) of the from-scratch route.

Seeds: every case uses seed 0; test_children_cases.py::test_mistakes_cannot_pass holds for all of them with it (no seed had to change)."""
from __future__ import annotations

import ctypes
import functools
from dataclasses import dataclass, replace

import numpy as np

import rbm_exact as R

POOL_MAX = 8192
ROWS_PER_PARENT = 12  # the most rows rbm_exact.make_children makes of one parent (three words, forced orbitals)
LDS_GROUP, WAVE_GROUP = 1024, 16  # rows of a workgroup of the LDS form / of a wave's group in the wave form (asserted against the query)
ORDERS = ("shuffled", "runs")
# strangers: a parent index out of range (the row itself is an ordinary one), and rows that differ from the NAMED parent in 5, 6 and sorb
# orbitals; "s5" / "s6": the first four flips in word 0 and the rest in the last word (one word: the same as f5 / f6)
STRANGER_KINDS = ("-1", "nw", "nw+5", "f5", "f6", "fall", "s5", "s6")


@dataclass(frozen=True)
class Case:
    name: str
    kind: str
    sorb: int
    H: int
    regime: str
    nw: int
    n: object            # int, or ("table" | "scratch", k): k rows past one sweep of that route
    form: str            # "lds" / "wave"
    order: str = "shuffled"
    raised: bool = False     # one parent, the last, with Re theta_0 < -340: every row from scratch
    strangers: bool = False
    seed: int = 0


_L = [
    Case("lds-second-sweep", "real", 12, 3, "small", 257, ("table", 1025), "lds"),
    Case("lds-three-workgroups", "complex", 12, 9, "fe2s2", 1025, 2049, "lds"),
    Case("lds-largest-real-table", "real", 64, 60, "fe2s2", 300, 4097, "lds"),
    Case("lds-complex-near-the-limit", "complex", 184, 9, "chunk-50", 257, 2049, "lds"),
    Case("lds-tanh", "tanh", 66, 8, "alt30", 300, 3000, "lds"),
    Case("lds-prbm", "pRBM", 130, 9, "small", 300, 3000, "lds"),
    Case("lds-overflow-one-338-w", "real", 40, 40, "one-338-w", 257, 3000, "lds"),
    Case("lds-overflow-chunk-50", "real", 40, 40, "chunk-50", 257, 3000, "lds"),
]
_W = [
    Case("wave-second-sweep", "real", 64, 62, "small", 300, ("table", 53), "wave"),
    Case("wave-complex", "complex", 32, 62, "fe2s2", 257, 135, "wave"),
    Case("wave-h129-one-parent", "real", 66, 129, "fe2s2", 1, 1000, "wave"),
    Case("wave-real-120x120", "real", 120, 120, "chunk-50", 257, 1000, "wave"),
    Case("wave-complex-136x150", "complex", 136, 150, "fe2s2", 257, 1000, "wave"),
    Case("wave-tanh", "tanh", 130, 64, "chunk-50", 257, 1000, "wave"),
    Case("wave-prbm", "pRBM", 184, 80, "alt30", 257, 1000, "wave"),
]
_BY = {c.name: c for c in _L + _W}
SHAPE_CASES = [c.name for c in _L + _W]

PARENT_CASES = []
for _base, _n in (("lds-three-workgroups", 2049), ("wave-second-sweep", 1000)):
    for _nw in (1, 257, 5000):
        for _order in ORDERS:
            _c = replace(_BY[_base], name=f"{_base.split('-')[0]}-parents-{_nw}-{_order}", nw=_nw, n=_n, order=_order)
            _BY[_c.name] = _c
            PARENT_CASES.append(_c.name)

_BY["lds-second-sweep-raised"] = replace(_BY["lds-second-sweep"], name="lds-second-sweep-raised", n=("scratch", 1025), raised=True)
_BY["wave-raised"] = replace(_BY["wave-second-sweep"], name="wave-raised", n=("scratch", 300), raised=True)
RAISED_CASES = ["lds-second-sweep-raised", "wave-raised"]
COUNT_CASES = ["lds-three-workgroups", "wave-second-sweep", "lds-second-sweep-raised"]

# (the last two: more than one word, so that "four flips in word 0, the rest in the last word" is what it says)
_BY["lds-strangers"] = replace(_BY["lds-three-workgroups"], name="lds-strangers", strangers=True)
_BY["wave-strangers"] = replace(_BY["wave-second-sweep"], name="wave-strangers", n=3000, strangers=True)
_BY["lds-strangers-three-words"] = replace(_BY["lds-complex-near-the-limit"], name="lds-strangers-three-words", strangers=True)
_BY["wave-strangers-two-words"] = replace(_BY["wave-real-120x120"], name="wave-strangers-two-words", n=1500, strangers=True)
STRANGER_CASES = ["lds-strangers", "wave-strangers", "lds-strangers-three-words", "wave-strangers-two-words"]

ALL_CASES = SHAPE_CASES + PARENT_CASES + RAISED_CASES + STRANGER_CASES


def case(name: str) -> Case:
    return _BY[name]


def flavour(kind: str) -> int:
    from pynqs_amd import _native as N

    return {"real": N.RBM_REAL, "tanh": N.RBM_TANH, "pRBM": N.RBM_PHASE, "complex": N.RBM_COMPLEX}[kind]


def geometry(kind: str, sorb: int, H: int, n: int):
    """(form, workgroups, rows per sweep of the table route, of the from-scratch route) of pynqs_rbm_forward_children on n rows: the
    library's own answer (a host entry: no GPU)"""
    from pynqs_amd import _native as N

    out = (ctypes.c_int64 * 4)()
    N.check(N.lib().pynqs_rbm_forward_children_geometry(int(n), sorb, H, flavour(kind), out), "pynqs_rbm_forward_children_geometry")
    return ("lds", "wave")[int(out[0])], int(out[1]), int(out[2]), int(out[3])


def full_sweeps(c: Case):
    """(rows per sweep of the table route, of the from-scratch route) once the grid has reached its cap"""
    _, _, table, scratch = geometry(c.kind, c.sorb, c.H, 1 << 30)
    return table, scratch


def rows_of(c: Case) -> int:
    if isinstance(c.n, int):
        return c.n
    route, k = c.n
    table, scratch = full_sweeps(c)
    return {"table": table, "scratch": scratch}[route] + k


def sweep_of(c: Case, n: int) -> int:
    """rows the launch for n rows covers per sweep on the route the case takes"""
    _, _, table, scratch = geometry(c.kind, c.sorb, c.H, n)
    return scratch if c.raised else table


def gather(ex: R.Exact, idx: np.ndarray) -> R.Exact:
    """the reference of the rows idx of an Exact: what rbm_exact.amp_ratio reads (ln psi, the visible factor, cond); tanh theta is left out"""
    none = np.zeros(0)
    return R.Exact(ex.kind, ex.re[idx], ex.im[idx], ex.vis[idx], ex.cond[idx], none, none)


def as_double(kind: str, psi: np.ndarray) -> np.ndarray:
    """exact psi (clongdouble) rounded to what a kernel returns: float64 ("real", "tanh") or complex128"""
    return psi.real.astype(np.float64) if kind in ("real", "tanh") else psi.astype(np.complex128)


def lowest_four(d: np.ndarray) -> np.ndarray:
    """the four lowest set bits of each row of uint64 [m, len] words (fewer where fewer are set): the flips a kernel that stopped at four
    would apply"""
    d = d.copy()
    out = np.zeros_like(d)
    for _ in range(4):
        free = np.ones(d.shape[0], dtype=bool)  # rows that have not given a bit in this round
        for w in range(d.shape[1]):
            low = d[:, w] & (~d[:, w] + np.uint64(1))
            low = np.where(free, low, np.uint64(0))
            out[:, w] |= low
            d[:, w] ^= low
            free &= low == 0
    return out


def raised_orbitals(sorb: int):
    return R.forced_orbitals(sorb)


def _parents(c: Case) -> np.ndarray:
    parents = R.rand_words(c.nw, c.sorb, 11 + c.seed)
    if c.regime == "one-338-w" or c.raised:
        f = R.forced_orbitals(c.sorb)
        bits = R.pm1(parents, c.sorb) > 0
        if c.regime == "one-338-w":  # every parent occupies the orbitals coupled to the saturated unit (theta = -330)
            bits[:, f] = True
        else:  # only the last parent occupies all four
            both = bits[:, f].all(1)
            bits[both, f[0]] = False
            bits[-1, f] = True
        parents = R.pack_bits(bits)
    return parents


def _params(c: Case):
    """None for the regime's own parameters; raised: hidden unit 0 with b = -300 and W = -11 on the four orbitals that only the last parent
    occupies together, 0 elsewhere: theta_0 = -344 for that parent, >= -322 for every other"""
    if not c.raised:
        return None
    rbm = R.regime_params(c.regime, c.kind, c.sorb, c.H, c.seed)
    W, hb = rbm.W.copy(), rbm.hb.copy()
    W[0, :] = 0.0
    W[0, raised_orbitals(c.sorb)] = -11.0
    hb[0] = -300.0
    return R.Rbm(rbm.kind, W, hb, rbm.vb)


def parent_theta(rbm, parents: np.ndarray, sorb: int) -> np.ndarray:
    """Re theta_h of the parents, longdouble [nw, H]"""
    x = R.pm1(parents, sorb).astype(R.LD)
    return rbm.hb.real.astype(R.LD) + x @ rbm.W.real.T.astype(R.LD)


def stranger_positions(n: int) -> np.ndarray:
    """Where the strangers sit, for both forms at once.  Waves of the LDS form are rows [64 w, 64 w + 64): wave 1 all strangers, wave 3 its
    first lane only, wave 5 its last lane only, waves 0, 2, 4 none.  Groups of the wave form are rows [16 g, 16 g + 16): group 40 has a
    stranger first, in the middle and last, group 44 is all strangers.  Then every 97th row from 1100 on (the later workgroups) and the
    last row."""
    assert n >= 1200
    pos = list(range(64, 128)) + [192, 383, 640, 647, 655] + list(range(704, 720)) + list(range(1100, n, 97)) + [n - 1]
    return np.unique(np.asarray(pos, dtype=np.int64))


@dataclass
class Built:
    case: Case
    n: int
    rbm: object
    parents: np.ndarray      # uint64 [nw, len]
    pool: np.ndarray         # uint64 [m, len]
    pool_parent: np.ndarray  # int32 [m]: the parent a pool row was made from
    pool_ex: R.Exact
    idx: np.ndarray          # int64 [n]: row i is pool[idx[i]]
    parent: np.ndarray       # int32 [n]: what the kernel is given (strangers: possibly out of range)
    stranger: np.ndarray     # int8 [n]: 0, or 1 + index into STRANGER_KINDS

    @property
    def rows(self) -> np.ndarray:
        return np.ascontiguousarray(self.pool[self.idx])

    def exact(self, sel=slice(None)) -> R.Exact:
        return gather(self.pool_ex, self.idx[sel])


@functools.lru_cache(maxsize=None)  # (a few MB per case: the reference of the pool without tanh theta, and the index arrays)
def build(name: str) -> Built:
    c = _BY[name]
    n = rows_of(c)
    g = np.random.default_rng([97, c.seed, c.sorb, c.H, c.nw])
    parents = _parents(c)
    L = parents.shape[1]
    per = POOL_MAX // ROWS_PER_PARENT
    if c.nw <= per:
        sub = np.arange(c.nw)
    else:  # a pool of at most POOL_MAX rows: children of a random subset of the parents, the first and the last among them
        sub = np.unique(np.concatenate([[0, c.nw - 1], g.choice(c.nw, per - 2, replace=False)]))
    force = R.forced_orbitals(c.sorb) if c.regime == "one-338-w" else None
    pool, ppar, _ = R.make_children(parents[sub], c.sorb, 5 + c.seed, force)
    ppar = sub[ppar].astype(np.int32)
    nreg = pool.shape[0]
    skind = np.zeros(nreg, dtype=np.int8)
    if c.strangers:
        extra, epar, ekind = [], [], []
        named = np.unique(np.concatenate([[c.nw - 1], g.choice(c.nw, min(c.nw, 24), replace=False)]))
        for p in named:
            for kname in STRANGER_KINDS[3:]:
                if kname == "fall":
                    flips = list(range(c.sorb))
                elif kname[0] == "f" or L == 1:
                    flips = list(g.choice(c.sorb, int(kname[1]), replace=False))
                else:
                    lo = 64 * (L - 1)
                    flips = list(g.choice(64, 4, replace=False)) + list(lo + g.choice(c.sorb - lo, int(kname[1]) - 4, replace=False))
                extra.append(R.flipped(parents[p], [int(o) for o in flips]))
                epar.append(p)
                ekind.append(1 + STRANGER_KINDS.index(kname))
        pool = np.concatenate([pool, np.stack(extra)])
        ppar = np.concatenate([ppar, np.asarray(epar, dtype=np.int32)])
        skind = np.concatenate([skind, np.asarray(ekind, dtype=np.int8)])
    assert pool.shape[0] <= POOL_MAX
    rbm, _, ex = R.checked_case(c.kind, c.sorb, c.H, c.regime, pool, c.seed, rbm=_params(c))
    idx = g.integers(0, nreg, n)
    idx[n // 2] = int(np.flatnonzero(ppar[:nreg] == c.nw - 1)[0])  # the last parent is in use
    if c.order == "runs":  # the children of a walker follow each other, as the front end emits them
        idx = idx[np.argsort(ppar[idx], kind="stable")]
    else:
        assert c.order == "shuffled"
    par = ppar[idx].copy()
    stranger = np.zeros(n, dtype=np.int8)
    if c.strangers:
        for j, i in enumerate(stranger_positions(n)):
            k = j % len(STRANGER_KINDS)
            stranger[i] = 1 + k
            if k < 3:
                par[i] = (-1, c.nw, c.nw + 5)[k]
            else:
                of_kind = np.flatnonzero(skind == 1 + k)
                idx[i] = of_kind[(j // len(STRANGER_KINDS)) % of_kind.size]
                par[i] = ppar[idx[i]]
    ex = gather(ex, np.arange(pool.shape[0]))
    for a in (parents, pool, ppar, idx, par, stranger, ex.re, ex.im, ex.vis, ex.cond):
        a.setflags(write=False)
    return Built(c, n, rbm, parents, pool, ppar, ex, idx, par, stranger)
