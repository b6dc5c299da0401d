"""Cases, inputs and yardstick for the hierarchical semi-stochastic REDUCE draws (tile first, then column inside the tile): the multi-pass
pynqs_reduce_count_sums / pynqs_reduce_sample behind energy.reduce_compact_sampled and the front end's flush_row32, flush, lookback,
list_cache and list_redraw forms, the last one also with its tile sums in global memory.  Their stream is not contractual, so nothing here
replays one: every assertion is about what a launch left behind, against the CPU oracle's rows (numpy, no GPU in this file).

    tests/test_reduce_hier_cases.py    the conditions the rows must meet, the case table against the host plan, the mutants
    tests/test_gpu_reduce_hier.py      every route on every family on the GPU

Families (sorb 24, 4 + 4 electrons, 1425 columns unless said otherwise; the sparse sets are synth_integrals(24, 1234 + s) with the
two-electron integrals kept with probability 0.01, then the one-electron ones with probability 0.15, masks from default_rng(100 + s);
1024 walkers rand_occ(1024, 24, 4, 4, seed=24)):
    A       sparse rows, eps 0.25, N 300, the sets A_SETS: over them every column is drawable for some walker and kept for some walker, so
            every tile edge of every form is the boundary of a draw, whatever the tile size; whole tiles are empty
    B       sets 0 and 1 with eps 1e3: nothing kept, the diagonal drawable
    C       eps between the two smallest distinct non-zero |H| of the batch: the walkers that hold the minimum have ONE drawable column, all
            others none.  The lone column is a double (sets 0, 1), the diagonal (2), a single (3), the row's last column (92)
    D1      N = 1 on four sets of A
    Dmax    the largest N at which the plan still names the form (N_MAX; 65535 for the multi-pass route and the look-back form), on eight
            walkers of set 92: six with a lone column (three times the row's last), two without width -- one count field holds all N
    Dpair   the same N on eight walkers of set 305 with eps between the second and third smallest |H|: walker 126's only drawable columns
            are the neighbours 124 and 125, the two halves of one word of packed 16-bit counts; and on eight walkers of set 0 under the
            same rule, four of them with two drawable columns a thousand columns apart: two tiles share the N draws, so that the second
            one's slot offset and its draw count are both large (the two 16-bit fields of a tile's packed word)
    E32     sets 0 and 1 with float32 integrals (|H| >= eps compared in float32)
    E2w/E3w the two- and three-word shapes of reduce_replay.CASES (sorb 66 with 3 + 1: 4308 columns, sorb 130 with 1 + 1: 4225), 64 walkers,
            N 3000 (the float32-row form ends near 3400 draws), twice: its dense integrals with eps 0.8, where every column is drawable and
            none reaches an expectation of 5 (all in the pooled cell: the records are held, the law is not), and the sparse set 0 of that
            sorb with eps 0.25, which gives the law its cells

check() holds one launch's records to (what refuses a wrong kernel is named in the assertion message):
    kept     the oracle's |H| >= eps set, values and kets, bit for bit
    drawn    distinct columns per walker, each with 0 < |H| < eps (never a kept column, an exact zero or padding), the oracle's ket, the sign
             of H; hits = rint(w N / (sign S)) with a fractional part inside the weight bound, at least 1, adding up to N per walker with
             width and absent for a walker without; S = the longdouble sum of the exact sub-eps |H|
    bounds   weight within (ncomb + 2) 2^-52 relative of (c / N) sign(H) S, row_sum within ncomb 2^-52 relative of S: the bounds of the
             short-row form's header.  They hold for every hierarchical form as they stand: each forms S by at most ncomb - 1 float64
             additions of non-negative terms (tile sums, then their sum; the multi-pass route adds the tile sums with torch.sum), every one
             within 2^-53 relative of a partial sum <= S, then scale = S / N and w = scale * c, one rounding each: (ncomb + 1) 2^-53 S in
             all, half the bound.  The float32-row form takes S from the same float64 sums, only the column inside a tile from the float32
             widths.  Float32 integrals: the stored weight is the float32 rounding of a number inside the bound.
    a lone column   all N hits on it, row_sum equal to its |H| bit for bit (a sum of one term)
    no width        row_sum == 0.0, no drawn record, every draw slot -1, the kept records as usual
The law: reduce_replay.chi_square (cells of expectation >= 5, one pooled cell per walker), pooled over the walkers and sets of a family,
threshold chi2.isf(1e-9, dof).  Families whose walkers have a single cell (C, Dmax, and D1 where N = 1 leaves only the pooled cell) have
dof 0: their law is the exact statement above, or none."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np

import reduce_replay as RR
from conftest import rand_occ, synth_integrals

LD = RR.LD
A_SETS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 21)   # 0 .. 11 leave 5 columns never drawable and 1 never kept; 12, 14 and 21 close that
C_SETS = (0, 1, 2, 3, 92)                                     # 92: found by a search over the integral seed for a lone LAST column
POOLED_CAP = 0.15
TILE = 256   # of the host samplers and mutants below; no assertion depends on a kernel's tile size


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Batch:
    """One set of rows.  integrals: ("sparse", s) or ("dense", seed).  eps: a number, "lone" (the midpoint of the two smallest distinct
    non-zero |H| of all `walkers` rows) or "pair" (of the second and third smallest).  pick: the walkers of the launch (None: all)."""
    name: str
    integrals: tuple
    eps: object
    sorb: int = 24
    noA: int = 4
    noB: int = 4
    walkers: int = 1024
    f32: bool = False
    pick: Optional[tuple] = None

    @property
    def n(self) -> int:
        return self.walkers if self.pick is None else len(self.pick)


@dataclass
class Rows:
    x: np.ndarray       # [n, 8 len] uint8
    h1: np.ndarray
    h2: np.ndarray
    eps: float
    hm: np.ndarray      # [n, ncomb], the integral dtype
    kets: np.ndarray    # [n, ncomb, 8 len]

    @functools.cached_property
    def keep(self):
        return RR.keep_mask(self.hm, self.eps)

    @functools.cached_property
    def sub(self):
        """the exact sub-eps |H| in longdouble, 0 on kept columns"""
        return np.where(self.keep, LD(0), np.abs(self.hm).astype(LD))

    @functools.cached_property
    def S(self):
        return self.sub.sum(1)

    @functools.cached_property
    def law(self):
        """|H| / S of the sub-eps columns (float64); all zero for a walker without width"""
        sub = self.sub
        s = sub.sum(1, keepdims=True)
        return (sub / np.where(s > 0, s, LD(1))).astype(np.float64)


def sparse_integrals(sorb: int, s: int):
    h1, h2 = synth_integrals(sorb, 1234 + s)
    g = np.random.default_rng(100 + s)
    h2 = h2 * (g.random(h2.shape) < 0.01)
    h1 = h1 * (g.random(h1.shape) < 0.15)
    return h1, h2


@functools.lru_cache(maxsize=None)
def _all_rows(integrals: tuple, sorb: int, noA: int, noB: int, walkers: int, f32: bool):
    from oracle import oracle as O

    kind, s = integrals
    h1, h2 = sparse_integrals(sorb, s) if kind == "sparse" else synth_integrals(sorb, s)
    if f32:
        h1, h2 = h1.astype(np.float32), h2.astype(np.float32)
    x = np.ascontiguousarray(O.pm01_to_onv(rand_occ(walkers, sorb, noA, noB, seed=sorb), sorb))
    h1, h2 = np.ascontiguousarray(h1), np.ascontiguousarray(h2)
    hm, kets = RR.oracle_rows(x, h1, h2, sorb, noA, noB)
    for a in (x, h1, h2, hm, kets):
        a.setflags(write=False)
    return x, h1, h2, hm, kets


def rows(b: Batch) -> Rows:
    """the oracle's rows of a batch: computed once per integral set, shared, read-only"""
    x, h1, h2, hm, kets = _all_rows(b.integrals, b.sorb, b.noA, b.noB, b.walkers, b.f32)
    eps = b.eps
    if isinstance(eps, str):
        a = np.abs(hm)
        u = np.unique(a[a > 0])
        k = {"lone": 0, "pair": 1}[eps]
        eps = float(0.5 * (u[k] + u[k + 1]))
    if b.pick is not None:
        i = np.array(b.pick)
        x, hm, kets = np.ascontiguousarray(x[i]), hm[i], kets[i]
    return Rows(x, h1, h2, float(eps), hm, kets)


# ---- routes and the case table ----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Route:
    """how a launch is brought to a form: cap_doubles / dedup of the ReduceFrontEnd under the module switches ROW_F32 / ROW_CACHE /
    TILE_SCRATCH_MIN_ROW of pynqs_amd.reduce_front (as reduce_replay.HIER does).  form / tile_sums_global: what the plan must name."""
    name: str
    form: str = ""
    tile_sums_global: bool = False
    cap_doubles: int = 0
    dedup: bool = True
    row_f32: bool = True
    row_cache: bool = True
    tile_min_row: int = 65536


ROUTES = [
    Route("multi"),
    Route("flush_row32", "flush_row32", False, 1100, dedup=False),
    Route("flush", "flush", False, 1100, dedup=False, row_f32=False),
    Route("lookback", "lookback", False, 1100),
    Route("list_cache", "list_cache", False, 600, row_f32=False),
    Route("list_redraw", "list_redraw", False, 600, row_f32=False, row_cache=False),
    Route("list_redraw_global", "list_redraw", True, 600, row_f32=False, row_cache=False, tile_min_row=64),
]
ROUTE_BY_NAME = {r.name: r for r in ROUTES}

# the largest N at which reduce_front.plan names the route's form for the Dmax / Dpair rows (float64, 1425 columns, 8 walkers), found by
# bisection over the plan; at N + 1 it names the look-back form (whose own end is the interface's 65535 draws: 65536 is refused)
N_MAX = {"multi": 65535, "flush_row32": 3456, "flush": 34148, "lookback": 65535, "list_cache": 37748, "list_redraw": 34148,
         "list_redraw_global": 17098}

_SPARSE = lambda s, **k: Batch(f"set{s}", ("sparse", s), **k)  # noqa: E731
DMAX_PICK = (12, 101, 115, 40, 48, 75, 0, 1)        # set 92: lone columns 1424, 1424, 1424, 1420, 1392, 1292; walkers 0 and 1 without width
DPAIR_PICK = (126, 45, 6, 9, 0, 1, 2, 3)            # set 305: columns {124, 125}, {122, 159}, {98}, {132}; four walkers without width
DFAR_PICK = (97, 641, 749, 798, 11, 17, 0, 1)       # set 0: columns {232, 1231}, {232, 1327}, {232, 1327}, {232, 1231}; two lone, two without width


@dataclass(frozen=True)
class Family:
    name: str
    batches: tuple
    N: int                  # 0: N_MAX of the route
    prime: bool = False     # front-end routes: a launch with eps 1e3 (every slot written) goes first, on the same buffers
    law: bool = True        # dof > 0 is required


FAMILIES = [
    Family("A", tuple(_SPARSE(s, eps=0.25) for s in A_SETS), 300),
    Family("B", tuple(_SPARSE(s, eps=1e3) for s in (0, 1)), 300),
    Family("C", tuple(_SPARSE(s, eps="lone") for s in C_SETS), 300, prime=True, law=False),
    Family("D1", tuple(_SPARSE(s, eps=0.25) for s in (0, 1, 2, 3)), 1, law=False),
    Family("Dmax", (_SPARSE(92, eps="lone", pick=DMAX_PICK),), 0, prime=True, law=False),
    Family("Dpair", (_SPARSE(305, eps="pair", pick=DPAIR_PICK), _SPARSE(0, eps="pair", pick=DFAR_PICK)), 0, prime=True),
    Family("E32", tuple(_SPARSE(s, eps=0.25, f32=True) for s in (0, 1)), 300),
    Family("E2w", (Batch("two_words", ("dense", 1234), 0.8, sorb=66, noA=3, noB=1, walkers=64),
                   Batch("two_words_sparse", ("sparse", 0), 0.25, sorb=66, noA=3, noB=1, walkers=64)), 3000),
    Family("E3w", (Batch("three_words", ("dense", 1234), 0.8, sorb=130, noA=1, noB=1, walkers=64),
                   Batch("three_words_sparse", ("sparse", 0), 0.25, sorb=130, noA=1, noB=1, walkers=64)), 3000),
]
FAMILY_BY_NAME = {f.name: f for f in FAMILIES}

# (row_f32_form, row cache present, tile scratch present) a front end of the route must answer.  The row cache is offered where the draws
# are dense in the row (64 N >= columns) and no float32 copy is: not at N = 1, where the cached LIST form cannot be reached at all.
_EXPECT = {"flush_row32": (2, False, False), "flush": (0, True, False), "lookback": (0, True, False), "list_cache": (0, True, False),
           "list_redraw": (0, False, False), "list_redraw_global": (0, False, True)}
_EXPECT_N1 = {**_EXPECT, "flush": (0, False, False), "lookback": (0, False, False), "list_cache": None}


def spec(family: str, route: str):
    """(N, expect) of a launch of the case table; None where the route cannot be brought to its form (list_cache at N = 1); expect is None
    for the multi-pass route"""
    f = FAMILY_BY_NAME[family]
    N = f.N or N_MAX[route]
    if route == "multi":
        return N, None
    e = (_EXPECT_N1 if N == 1 else _EXPECT)[route]
    return None if e is None else (N, e)


CASE_IDS = [(f.name, r.name) for f in FAMILIES for r in ROUTES if spec(f.name, r.name) is not None]


def kept_max(family: str) -> int:
    return max(int(rows(b).keep.sum(1).max()) for b in FAMILY_BY_NAME[family].batches)


# ---- what a launch left behind, and the yardstick -----------------------------------------------------------------------------------------------
@dataclass
class Records:
    """numpy copies of one launch: kept records (any order) and drawn records; row_sum / slots (srec_col as [n, N]) of a front end, None
    for the multi-pass route"""
    k_walker: np.ndarray
    k_col: np.ndarray
    k_w: np.ndarray
    k_onv: np.ndarray
    walker: np.ndarray
    col: np.ndarray
    w: np.ndarray
    onv: np.ndarray
    row_sum: Optional[np.ndarray] = None
    slots: Optional[np.ndarray] = None


@dataclass
class Figures:
    kept: int
    drawn: int
    lone: int
    no_width: int
    werr: float          # worst weight error / bound
    serr: float          # worst row_sum error / bound
    hits: np.ndarray     # [n, ncomb] int64


def check(r: Rows, rec: Records, N: int) -> Figures:
    hm, keep, sub, S = r.hm, r.keep, r.sub, r.S
    n, ncomb = hm.shape
    f32 = hm.dtype == np.float32
    assert rec.k_w.dtype == hm.dtype and rec.w.dtype == hm.dtype, "dtype of the weights"
    # kept records
    order = np.lexsort((rec.k_col, rec.k_walker))
    kw, kc = np.nonzero(keep)
    assert np.array_equal(rec.k_walker[order], kw) and np.array_equal(rec.k_col[order].astype(np.int64), kc), "kept set differs from the oracle's |H| >= eps"
    assert np.array_equal(rec.k_w[order], hm[kw, kc]), "kept values differ from the oracle's"
    assert np.array_equal(rec.k_onv[order], r.kets[kw, kc]), "kept kets differ from the oracle's"
    # drawn records
    w_, c_ = rec.walker.astype(np.int64), rec.col.astype(np.int64)
    assert bool(((c_ >= 0) & (c_ < ncomb)).all()) and bool(((w_ >= 0) & (w_ < n)).all()), "drawn column outside the row (padding)"
    flat = w_ * ncomb + c_
    assert np.unique(flat).size == flat.size, "a column is recorded twice for one walker"
    h = hm[w_, c_]
    assert not bool(keep[w_, c_].any()), "a kept column was drawn"
    assert bool((h != 0).all()), "a column of exactly zero width was drawn"
    assert np.array_equal(rec.onv, r.kets[w_, c_]), "a drawn record's ket is not the oracle's"
    assert bool((np.sign(rec.w) == np.sign(h)).all()), "a drawn record's weight has not the sign of H"
    sign = np.sign(h).astype(LD)
    bound_w = LD(ncomb + 2) * LD(2.0) ** -52
    creal = rec.w.astype(LD) * LD(N) / (sign * S[w_])
    c = np.rint(creal.astype(np.float64)).astype(np.int64)
    assert bool((c >= 1).all()), "a hit count below 1"
    frac_bound = c.astype(LD) * (bound_w + (LD(2.0) ** -24 if f32 else LD(0)))
    assert bool((np.abs(creal - c.astype(LD)) <= frac_bound).all()), "w N / (sign S) is no whole number within the weight bound"
    hits = np.zeros((n, ncomb), dtype=np.int64)
    hits[w_, c_] = c
    live = S > 0
    assert np.array_equal(hits.sum(1), np.where(live, N, 0)), "the hits of a walker do not add up to N (none for a walker without width)"
    want = c.astype(LD) / LD(N) * sign * S[w_]
    werr = 0.0
    if c.size:
        if not f32:
            rel = np.abs(rec.w.astype(LD) - want) / np.abs(want)
            werr = float((rel / bound_w).max())
            assert werr <= 1.0, f"weights: {werr} of the bound"
        else:   # the stored value is the float32 rounding of a number within the bound
            lo, hi = (want - bound_w * np.abs(want)).astype(np.float32), (want + bound_w * np.abs(want)).astype(np.float32)
            assert bool(((lo <= rec.w) & (rec.w <= hi)).all()), "weights (float32) outside the rounding of the bound"
            # (the figure: against the bound plus the float32 rounding of the store, 2^-24 (1 + bound) relative)
            werr = float((np.abs(rec.w.astype(LD) - want) / np.abs(want)).max() / (bound_w + LD(2.0) ** -24 * (1 + bound_w)))
    ndraw = (sub > 0).sum(1)
    lone = live & (ndraw == 1)
    assert bool(((hits.max(1) == N) & ((hits > 0).sum(1) == 1))[lone].all()), "a lone column does not hold all N hits"
    serr = 0.0
    if rec.row_sum is not None:
        rs = rec.row_sum.astype(LD)
        assert bool((rec.row_sum[~live] == 0.0).all()), "row_sum of a walker without width is not 0.0"
        lone_val = np.abs(hm).astype(np.float64).max(1, where=(sub > 0), initial=0.0)
        assert np.array_equal(rec.row_sum[lone], lone_val[lone]), "row_sum of a lone column is not its |H| bit for bit"
        if live.any():
            serr = float((np.abs(rs[live] - S[live]) / S[live]).max() / (LD(ncomb) * LD(2.0) ** -52))
        assert serr <= 1.0, f"row_sum: {serr} of the bound"
    if rec.slots is not None:
        used = rec.slots >= 0
        assert rec.slots.shape == (n, N) and bool((~used[~live]).all()), "a draw slot of a walker without width is not -1"
        assert np.array_equal(used.sum(1), (hits > 0).sum(1)), "draw slots in use differ from the distinct drawn columns"
    return Figures(int(kw.size), int(c.size), int(lone.sum()), int((~live).sum()), werr, serr, hits)


def pooled_chi_square(hits_list, law_list, N: int):
    """reduce_replay.chi_square pooled over the sets of a family: (statistic, dof, threshold chi2.isf(1e-9, dof))"""
    from scipy.stats import chi2

    stat, dof = 0.0, 0
    for hits, p in zip(hits_list, law_list):
        s, d, _ = RR.chi_square(hits, p, N)
        stat, dof = stat + s, dof + d
    return stat, dof, (float(chi2.isf(1e-9, dof)) if dof > 0 else 0.0)


def host_counts(r: Rows, N: int, rng) -> np.ndarray:
    """numpy's multinomial on the exact law, walker by walker: what the statistic makes of a correct sampler at the same shape"""
    p = r.law
    out = np.zeros(p.shape, dtype=np.int64)
    for i, q in enumerate(p):
        if q.sum() > 0:
            out[i] = rng.multinomial(N, q / q.sum())
    return out


# ---- a hierarchical sampler in numpy, and its mutants -----------------------------------------------------------------------------------------
MUTANTS = {
    # name: the assertion that refuses it
    "tile_by_columns": "chi-square",             # tile chosen in proportion to its number of drawable columns
    "kept_drawable": "a kept column was drawn",
    "empty_tile_dropped": "do not add up to N",  # tile sums floored at S / 64 (a guard against empty tiles), the draws that land in one dropped
    "power_1_2": "chi-square",                   # law proportional to |H|^1.2
    "f32_weights": "no whole number within the weight bound",   # weights rounded to float32 although the integrals are float64
    "sign_dropped": "has not the sign of H",
    "carry": "zero width was drawn|do not add up to N|does not hold all N",   # packed 16-bit counts added onto a word that was not cleared
}


def host_hier(r: Rows, N: int, rng, mutant: Optional[str] = None) -> Records:
    """Tile first (tiles of TILE columns, probability = tile sum / S), then the column inside the tile; kept records from the oracle.
    mutant: one of MUTANTS, each a single mistake."""
    assert mutant is None or mutant in MUTANTS
    hm, keep = r.hm, r.keep
    n, ncomb = hm.shape
    a = np.abs(hm).astype(np.float64)
    width = np.where(keep, 0.0, a)
    draw_w = a if mutant == "kept_drawable" else width ** 1.2 if mutant == "power_1_2" else width
    nt = (ncomb + TILE - 1) // TILE
    hits = np.zeros((n, ncomb), dtype=np.int64)
    for i in range(n):
        if not width[i].sum() > 0:
            continue
        wt = np.zeros(nt * TILE)
        wt[:ncomb] = draw_w[i]
        wt = wt.reshape(nt, TILE)
        ts = wt.sum(1)
        if mutant == "tile_by_columns":
            ts = (wt > 0).sum(1).astype(np.float64)
        if mutant == "empty_tile_dropped":
            ts = np.maximum(ts, ts.sum() / 64)
        per_tile = rng.multinomial(N, ts / ts.sum())
        for t in np.flatnonzero(per_tile):
            if not wt[t].sum() > 0:
                continue   # (only the mutant comes here)
            hits[i, t * TILE: (t + 1) * TILE][: ncomb - t * TILE] += rng.multinomial(per_tile[t], wt[t] / wt[t].sum())[: ncomb - t * TILE]
    if mutant == "carry":   # two 16-bit counts per word, added onto the words of an earlier launch of the same rows
        pad = np.zeros((n, ncomb + (ncomb & 1)), dtype=np.uint64)
        pad[:, :ncomb] = hits
        word = (2 * (pad[:, 0::2] + (pad[:, 1::2] << np.uint64(16)))) & np.uint64(0xFFFFFFFF)
        pad[:, 0::2], pad[:, 1::2] = word & np.uint64(0xFFFF), word >> np.uint64(16)
        hits = pad[:, :ncomb].astype(np.int64)
    S = r.S
    w_, c_ = np.nonzero(hits)
    w = (hits[w_, c_].astype(LD) / LD(N) * np.sign(hm[w_, c_]).astype(LD) * S[w_]).astype(np.float64)
    if mutant == "f32_weights":
        w = w.astype(np.float32).astype(np.float64)
    if mutant == "sign_dropped":
        w = np.abs(w)
    kw, kc = np.nonzero(keep)
    slots = np.full((n, N), -1, dtype=np.int32)
    for i in range(n):
        ci = c_[w_ == i]
        slots[i, : ci.size] = ci
    return Records(kw, kc.astype(np.int32), hm[kw, kc], r.kets[kw, kc], w_, c_.astype(np.int32), w.astype(hm.dtype), r.kets[w_, c_],
                   row_sum=S.astype(np.float64), slots=slots)
