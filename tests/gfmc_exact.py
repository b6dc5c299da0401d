"""The yardstick of the GFMC move (gfmc_sample_kernel behind pynqs_gfmc_sample and pynqs_gfmc_sample_rank; include/pynqs_amd.h) and the
cases of tests/test_gfmc_exact.py and tests/test_gpu_gfmc_exact.py.  Plain Python integers: it shares no code with the kernel or with
oracle/.

The law.  G >= 0 a row of m columns, S = sum G, C_k = G_0 + ... + G_k in exact arithmetic, C_{-1} = 0, tau = m 2^-52 S:
    index = k is acceptable  iff  C_{k-1} - tau < u S <= C_k + tau  and  (G_k > 0 or k = 0);       a row with S = 0 gives index 0;
    |beta - S| <= (m - 1) 2^-53 S.
tau: every running sum of the kernel is a float64 sum of at most m non-negative terms in some order, so it is within (m - 1) 2^-53 S of
its exact value; so is beta, and u * beta adds one rounding; two such quantities are compared.  The bracket alone does not keep a
zero-weight column out (C_{k-1} = C_k there): the positivity clause does.  A uniform farther than tau from every C_j leaves one column.

Exact arithmetic: a double is an integer times a power of two (frexp), so a row becomes integers on the scale of its smallest exponent
and the prefix sums are Python integers; a uniform is a / 2^b, and both sides of every comparison are multiplied out.  That is fast enough
for the rows of 300 001 columns too, so no row needs a longdouble sum with a slack of its own.

Cases: (family, m, u0).  A case has several seeded rows; every row carries its own uniforms (row_uniforms): the CDF boundaries
fl(C_j / S) with their neighbours at -1, +1, +2 ulp (boundary_uniforms), 1 - 2^-53, u = 0 where u0 says so, and random ones.  The
families with exact zeros next to positive columns at m >= 5 are the BOUNDARY cases: rows are added until at least NEAR_MIN uniforms lie
within 2^-52 S of some C_j and at least ZERO_MIN of them on a column that a zero-weight column follows."""
from __future__ import annotations

import bisect
import functools
import itertools
from collections import namedtuple
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
ONE_BELOW = 1.0 - U  # the largest uniform
NEAR_MIN, ZERO_MIN = 1000, 200
OFFSETS = (-1, 0, 1, 2)  # ulp neighbours of fl(C_j / S)
LONG = 16384  # rows beyond this get 8 uniforms (the GPU tests replicate them over 8 walkers)


class Row:
    """g float64 [m] >= 0; C: exact prefix sums as integers on the scale 2^e0; S = C[-1]"""

    def __init__(self, g) -> None:
        g = np.ascontiguousarray(g, dtype=np.float64)
        assert g.ndim == 1 and g.size >= 1 and bool(np.isfinite(g).all()) and bool((g >= 0).all())
        self.g, self.m = g, g.size
        mant, exp = np.frexp(g)
        mi = np.ldexp(mant, 53).astype(np.int64)  # exact: mant has 53 bits
        assert bool((np.ldexp(mi.astype(np.float64), exp - 53) == g).all())
        nz = g > 0
        self.e0 = int((exp[nz] - 53).min()) if nz.any() else 0
        shift = np.where(nz, exp - 53 - self.e0, 0)
        self.C = list(itertools.accumulate(int(a) << int(s) for a, s in zip(mi.tolist(), shift.tolist())))
        self.S = self.C[-1]

    def cum(self, k: int) -> int:
        return self.C[k] if k >= 0 else 0


def as_row(row) -> Row:
    return row if isinstance(row, Row) else Row(row)


def _ratio(u: float):
    u = float(u)
    assert 0.0 <= u < 1.0
    return u.as_integer_ratio()  # (a, q), q a power of two


def accepts(row, u: float, k: int) -> bool:
    """the law of the module docstring, in exact arithmetic"""
    r = as_row(row)
    k = int(k)
    if not 0 <= k < r.m:
        return False
    if r.S == 0:
        return k == 0
    if k and not r.g[k] > 0:
        return False
    a, q = _ratio(u)
    t = (a * r.S) << 52      # u S      } times 2^52 q
    tau = r.m * r.S * q      # tau      }
    return (r.cum(k - 1) << 52) * q - tau < t <= (r.C[k] << 52) * q + tau


def exact_index(row, u: float) -> int:
    """first k with C_k >= u S; 0 for a row of sum zero.  (For u > 0 that column has weight; u = 0 gives column 0 whatever its weight.)"""
    r = as_row(row)
    if r.S == 0:
        return 0
    a, q = _ratio(u)
    return bisect.bisect_left(r.C, -((-a * r.S) // q))


def nearest_boundary(row, u: float) -> int:
    """a column j with |u S - C_j| <= 2^-52 S (the last such column with weight, so that a zero-weight column may follow it), or -1"""
    r = as_row(row)
    if r.S == 0:
        return -1
    a, q = _ratio(u)
    t, eps = (a * r.S) << 52, r.S * q
    k = exact_index(r, u)
    for j in (k, k - 1):
        if 0 <= j < r.m and abs(t - (r.C[j] << 52) * q) <= eps:
            while j > 0 and not r.g[j] > 0:  # C_j = C_{j-1} across zeros: name the column that has the weight
                j -= 1
            return j
    return -1


def zero_follows(row, j: int) -> bool:
    r = as_row(row)
    return 0 <= j < r.m - 1 and r.g[j + 1] == 0


def beta_check(row, beta: float):
    """(|beta - S| <= (m - 1) 2^-53 S decided exactly, |beta - S| / bound as a float: 0 where beta is exact, inf where only the bound is 0)"""
    r = as_row(row)
    if not np.isfinite(beta):
        return False, float("inf")
    s = Fraction(r.S) * Fraction(2) ** r.e0
    err, bound = abs(Fraction(float(beta)) - s), (r.m - 1) * s / 2 ** 53
    return err <= bound, 0.0 if err == 0 else float(err / bound) if bound else float("inf")


def boundary_uniforms(row, per_column=OFFSETS, columns=None) -> np.ndarray:
    """for every column j with G_j > 0 (or those of `columns`): fl(C_j / S) and its neighbours at the ulp offsets of per_column, kept
    where 0 <= u < 1"""
    r = as_row(row)
    if r.S == 0:
        return np.zeros(0)
    cols = np.flatnonzero(r.g > 0) if columns is None else np.asarray(columns, dtype=np.int64)
    base = np.array([r.C[j] / r.S for j in cols.tolist()], dtype=np.float64)  # int / int: correctly rounded
    out = []
    for off in per_column:
        v = base.copy()
        for _ in range(abs(off)):
            v = np.nextafter(v, np.inf if off > 0 else -np.inf)
        out.append(v)
    u = np.stack(out, 1).reshape(-1) if out else np.zeros(0)
    return u[(u >= 0) & (u < 1)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases

Case = namedtuple("Case", "family m u0")
WIDTHS = (1, 2, 5, 63, 64, 65, 255, 256, 257, 513, 7877, 262_144, 262_145, 300_001)
LONG_WIDTHS = tuple(m for m in WIDTHS if m > LONG)
LADDER = (U, U, 1.0, 0.0)
LADDER_AT = (0, 1, 2, 3, 60, 61, 62, 63, 252, 253, 254, 255, 508, 509, 510, 511)  # lane offsets 0-3, 60-63, 252-255; across 64, 256 (and 512)
# The five-column counterexample: row, uniform, the sequential float64 answer, the answer in exact arithmetic.  In float64 the total
# rounds to 2 and the target to 1 + 2^-52, which the sequential running sum reaches at column 2; the Hillis-Steele scan is one ulp lower
# there and reaches it at the zero-weight column 3.  Exactly, S = 2 + 2^-52 and u S = 1 + 1.5 * 2^-52 + 2^-105 > C_2 = C_3 = 1 + 2^-52, so the
# first column that reaches it is 4: the law admits 2 and 4 (both within tau) and never 3.
COUNTEREXAMPLE = (np.array([U, U, 1.0, 0.0, 1.0]), 0.5 + U, 2, 4)
BOUNDARY_FAMILIES = ("zeros60", "tile-zeros", "chunk-end", "tile-end", "row-end", "ladder", "g0-zero")
FAMILIES = ("dense", "zeros60", "spike-first", "spike-mid", "spike-last", "tile-zeros", "chunk-end", "tile-end", "row-end", "ladder",
            "wide", "g0-zero", "all-zero")
LONG_FAMILIES = ("dense", "zeros60", "ladder", "tile-zeros", "all-zero")


def applies(family: str, m: int) -> bool:
    if m > LONG:
        return family in LONG_FAMILIES
    if family == "tile-zeros":
        return m > 256
    if family in ("chunk-end", "tile-end", "row-end", "g0-zero"):
        return m >= 2
    if family == "ladder":
        return m >= 5
    return True


def cases_of(m: int):
    out = [Case(f, m, True) for f in FAMILIES if applies(f, m)]
    if applies("g0-zero", m) and m <= LONG:
        out.append(Case("g0-zero", m, False))
    return out


CASES = [c for m in WIDTHS for c in cases_of(m)]


def case_id(c: Case) -> str:
    return f"{c.family}-m{c.m}" + ("" if c.u0 else "-no-u0")


def is_boundary(c: Case) -> bool:
    return c.family in BOUNDARY_FAMILIES and 5 <= c.m <= LONG


def _ordinary(rng, m: int, zeros: float) -> np.ndarray:
    g = rng.random(m) + 2.0 ** -20
    g[rng.random(m) < zeros] = 0.0
    return g


def make_row(family: str, m: int, rng) -> np.ndarray:
    if family == "dense":
        return _ordinary(rng, m, 0.0)
    if family in ("zeros60", "g0-zero"):
        g = _ordinary(rng, m, 0.6)
        if family == "g0-zero":
            g[0] = 0.0  # a clamped diagonal
            if not g.any():
                g[int(rng.integers(1, m))] = 1.0
        elif not g.any():
            g[int(rng.integers(0, m))] = 1.0
        return g
    if family.startswith("spike"):
        g = np.zeros(m)
        g[{"spike-first": 0, "spike-mid": m // 2, "spike-last": m - 1}[family]] = 3.0
        return g
    if family == "tile-zeros":  # whole tiles of 256 (of 512 too: pairs) are zero; the first column with weight lies in tile >= 1
        g = _ordinary(rng, m, 0.3)
        nt = -(-m // 256)
        dead = rng.random(nt) < 0.5
        dead[0] = True
        if nt > 4:
            dead[1] = True  # (at the doubled tile the first tile of 512 is empty as well)
        if dead.all():
            dead[-1] = False
        g[np.repeat(dead, 256)[:m]] = 0.0
        if not g.any():
            g[m - 1] = 1.0
        return g
    if family in ("chunk-end", "tile-end", "row-end"):  # zeros from a column with weight to the end of its chunk / tile / the row
        g = _ordinary(rng, m, 0.0)
        if family == "row-end":
            g[int(rng.integers(1, m)):] = 0.0
            return g
        span = 64 if family == "chunk-end" else 256
        for c0 in range(0, m, span):
            c1 = min(c0 + span, m)
            if c1 - c0 >= 2:
                g[int(rng.integers(c0 + 1, c1)):c1] = 0.0
        return g
    if family == "ladder":  # 2^-53, 2^-53, 1, 0 at the offsets of LADDER_AT (and of every further tile, shifted), ordinary columns between
        g = _ordinary(rng, m, 0.3)
        starts = [t + s for t in range(0, m, 1024) for s in LADDER_AT]
        rng.shuffle(starts)
        taken = np.zeros(m, dtype=bool)
        for s in starts:
            if s + 4 <= m and not taken[max(0, s - 1):s + 5].any():
                g[s:s + 4] = LADDER
                taken[s:s + 4] = True
        if m == 5:  # the counterexample's shape: the ladder, then one more column with weight
            g[:4] = LADDER
            g[4] = float(rng.choice([1.0, 0.5, 2.0, rng.random() + 0.5]))
        return g
    if family == "wide":
        g = 10.0 ** rng.uniform(-150.0, 150.0, m)
        g[rng.random(m) < 0.3] = 0.0
        if not g.any():
            g[0] = 1.0
        return g
    assert family == "all-zero", family
    return np.zeros(m)


def row_uniforms(row, rng, n: int, u0: bool) -> np.ndarray:
    """n uniforms for one row: u = 0 (where u0), 1 - 2^-53, the boundaries of columns that a zero-weight column follows, those of other
    columns, and random ones"""
    r = as_row(row)
    special = ([0.0] if u0 else []) + [ONE_BELOW]
    n_random = max(1, n // 8)
    room = max(0, n - len(special) - n_random)
    pos = np.flatnonzero(r.g > 0)
    zf = pos[[zero_follows(r, int(j)) for j in pos]] if pos.size else pos
    rest = np.setdiff1d(pos, zf)
    pick = lambda a, k: np.sort(rng.choice(a, size=min(k, a.size), replace=False)) if a.size and k > 0 else a[:0]  # noqa: E731
    k_z = min(zf.size, max(room // 4 - min(rest.size, room // 16), 0))
    cz = pick(zf, k_z)
    cr = pick(rest, room // 4 - cz.size)
    ub = boundary_uniforms(r, OFFSETS, np.concatenate([cz, cr]))[:room]
    fill = rng.random(n - len(special) - ub.size)
    u = np.concatenate([np.array(special), ub, fill])[:n]
    assert u.size == n and bool(((u >= 0) & (u < 1)).all())
    return u


Block = namedtuple("Block", "row u")  # one Row and the uniforms of the walkers it is replicated over


@functools.lru_cache(maxsize=None)
def blocks(c: Case):
    """the case's rows with their uniforms, seeded by the case alone.  Long rows: one row, 8 uniforms.  Boundary cases: rows of up to
    1024 uniforms until NEAR_MIN lie on a boundary and ZERO_MIN of those next to a zero-weight column.  Others: 4 rows."""
    seed = [FAMILIES.index(c.family), c.m, int(c.u0)]
    out = []
    if c.m > LONG:
        rng = np.random.default_rng(seed)
        r = Row(make_row(c.family, c.m, rng))
        return (Block(r, row_uniforms(r, rng, 8, c.u0)),)
    if not is_boundary(c):
        for i in range(4):
            rng = np.random.default_rng(seed + [i])
            r = Row(make_row(c.family, c.m, rng))
            out.append(Block(r, row_uniforms(r, rng, int(min(256, max(8, 5 * c.m))), c.u0)))
        return tuple(out)
    near = zero = 0
    for i in range(4000):
        rng = np.random.default_rng(seed + [i])
        r = Row(make_row(c.family, c.m, rng))
        # eight uniforms per column that a zero-weight column follows: its own four and those of one other column
        zf = int(((r.g[:-1] > 0) & (r.g[1:] == 0)).sum())
        u = row_uniforms(r, rng, min(256 if c.family == "ladder" else 1024, 8 * (zf + 1)), c.u0)
        out.append(Block(r, u))
        n_, z_ = count_boundary(r, u)
        near, zero = near + n_, zero + z_
        if near >= NEAR_MIN and zero >= ZERO_MIN and (c.family != "ladder" or i >= 7):  # (eight rows: the ladders' places are drawn per row)
            break
    return tuple(out)


def count_boundary(row, u) -> tuple:
    """(uniforms within 2^-52 S of some C_j, those of them whose column is followed by a zero-weight column)"""
    r = as_row(row)
    js = [nearest_boundary(r, x) for x in np.asarray(u).tolist()]
    return sum(j >= 0 for j in js), sum(j >= 0 and zero_follows(r, j) for j in js)


def check_moves(row, u, index) -> list:
    """the walkers whose index the law does not accept: [(walker, u, index, exact index, weight there)]"""
    r = as_row(row)
    bad = []
    for i, (x, k) in enumerate(zip(np.asarray(u).reshape(-1).tolist(), np.asarray(index).reshape(-1).tolist())):
        if not accepts(r, x, k):
            bad.append((i, x, int(k), exact_index(r, x), float(r.g[k]) if 0 <= k < r.m else None))
    return bad
