"""The shapes of tests/test_many_electron_cases.py (CPU) and tests/test_gpu_many_electron.py (GPU): the determinant kernels from 16 to 129
electrons, on one, two and three ONV words -- and, in plain Python, the arithmetic by which those kernels change their shape with the
electron count.  Formulas only: nothing here is imported from the library, so a changed constant there shows up as a regime that the
list no longer reaches (tests/test_many_electron_cases.py::test_the_list_reaches_every_regime), not as a silently moved test.

Where the formulas come from (nocc = the walker's electrons, nele = the count the caller passes; equal in every case here):
  * singles_tile (plan_dev.h): G lanes walk one single's row, G = 16, 32, 64 for nocc <= 16, <= 32, above; for nocc > 64 a second loop
    gathers the terms past lane 63.  A pass stages cap = max(1, min(16, QUARTER / (nocc | 1))) singles of a tile of up to 16; QUARTER is
    512 elements (kDiagTile / 4) except in the LIST forms of the one-launch REDUCE front end (reduce_list.h), which pass 256.
  * diag_wave (plan_dev.h): nele (nele + 1) / 2 terms in rounds of QUARTER; diag_by_wave (kernels_det.hip) in rounds of kHijDiagTile =
    512; diag_phase (detcore.h) in rounds of kDiagTile = 2048.
  * plan_chunks (launch.h): how a row of ncomb columns is cut into workgroups, defaults 4096 workgroups wanted, 2048 columns at least.
    The direct kernel gives chunk c the columns [c len, (c + 1) len); columns 1 .. d1 are the singles."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from conftest import rand_occ, synth_integrals

MAX_NELE = 120            # include/pynqs_amd.h: PYNQS_MAX_NELE
SINGLES_PER_TILE = 16     # plan_dev.h: kSinglesPerTile
QUARTER, QUARTER_LIST = 512, 256
HIJ_DIAG_TILE, DIAG_TILE = 512, 2048
WANT_WG, MIN_CHUNK = 4096, 2048

Case = namedtuple("Case", "sorb noA noB n")
# (sorb, noA, noB, walkers)
CASES = [Case(*c) for c in (
    # one word
    (40, 8, 8, 3), (40, 9, 8, 3), (40, 16, 16, 3), (40, 17, 16, 3), (40, 20, 18, 2),
    (40, 20, 20, 2),        # full shell: ncomb = 1
    (64, 31, 31, 3),        # no same-spin doubles
    (64, 32, 31, 2),        # no alpha singles: no opposite-spin doubles either
    (64, 32, 32, 2),        # ncomb = 1 with 5 rounds of the diagonal
    # two words
    (72, 8, 8, 2), (72, 9, 8, 2), (72, 32, 32, 2), (72, 33, 32, 2),
    (72, 35, 35, 2),        # 70 electrons, no same-spin doubles
    (72, 36, 35, 2),        # 71 electrons, beta singles only
    (128, 60, 60, 1), (128, 64, 64, 2),
    # three words
    (130, 3, 2, 2), (130, 9, 8, 2),
    (130, 60, 0, 1),        # 60 electrons of one spin
    (130, 65, 0, 2),        # 65 electrons and ncomb = 1
    (130, 61, 59, 1),       # the declared limit
    (136, 65, 64, 1),       # past it
    (192, 32, 0, 1))]       # d1 = 2048 = the chunk length: the only row that is cut inside its singles
GOLDEN = [c for c in CASES if c.sorb == 40 and 32 <= c.noA + c.noB <= 40]   # what the reference as shipped supports (40 electrons, one word)


def case_id(c: Case) -> str:
    return f"s{c.sorb}_a{c.noA}_b{c.noB}"


def words(c: Case) -> int:
    return (c.sorb - 1) // 64 + 1


def classes(c: Case):
    """(alpha singles, beta singles, alpha-alpha, beta-beta, alpha-beta doubles): excitation.cpp:20-42"""
    k = c.sorb // 2
    nvA, nvB = k - c.noA, k - c.noB
    pairs = lambda m: m * (m - 1) // 2  # noqa: E731
    sa, sb = c.noA * nvA, c.noB * nvB
    return sa, sb, pairs(c.noA) * pairs(nvA), pairs(c.noB) * pairs(nvB), sa * sb


def ncomb(c: Case) -> int:
    return sum(classes(c)) + 1


def boundaries(c: Case):
    """first column of every class and one past the last: [1, 1 + Sa, ..., ncomb]"""
    return [1 + int(v) for v in np.cumsum((0,) + classes(c))]


def group_width(nocc: int) -> int:
    return 16 if nocc <= 16 else (32 if nocc <= 32 else 64)


def cap(nocc: int, quarter: int = QUARTER) -> int:
    return max(1, min(SINGLES_PER_TILE, quarter // (nocc | 1)))


def passes(c: Case, quarter: int = QUARTER) -> int:
    """passes over the fullest singles tile of the row (0: the row has no singles)"""
    sa, sb = classes(c)[:2]
    fullest = min(SINGLES_PER_TILE, sa + sb)
    return -(-fullest // cap(c.noA + c.noB, quarter))


def rounds(nele: int, tile: int) -> int:
    return -(-(nele * (nele + 1) // 2) // tile)


def plan_chunks(nbatch: int, ncomb_: int):
    """(nchunks, chunk_len) of launch.h with its defaults"""
    c = 1 if nbatch >= WANT_WG else (WANT_WG + nbatch - 1) // nbatch
    c = max(1, min(c, (ncomb_ + MIN_CHUNK - 1) // MIN_CHUNK))
    length = ((ncomb_ + c - 1) // c + 255) & ~255
    return (ncomb_ + length - 1) // length, length


def cut_inside_singles(c: Case) -> bool:
    """some chunk of the direct kernel begins at a single that is not the first one"""
    nchunks, length = plan_chunks(c.n, ncomb(c))
    d1 = sum(classes(c)[:2])
    return nchunks > 1 and 1 < length <= d1


Regime = namedtuple("Regime", "words nele ncomb G gather cap512 cap256 passes512 passes256 wave hij phase nchunks chunk_len cut empty_same empty_opp")


def regime(c: Case) -> Regime:
    nele = c.noA + c.noB
    cl = classes(c)
    nchunks, length = plan_chunks(c.n, ncomb(c))
    return Regime(words(c), nele, ncomb(c), group_width(nele), nele > 64, cap(nele), cap(nele, QUARTER_LIST), passes(c), passes(c, QUARTER_LIST),
                  rounds(nele, QUARTER), rounds(nele, HIJ_DIAG_TILE), rounds(nele, DIAG_TILE), nchunks, length, cut_inside_singles(c),
                  ncomb(c) > 1 and (cl[2] == 0 or cl[3] == 0), ncomb(c) > 1 and cl[4] == 0)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def integrals(sorb: int):
    """the packed synthetic integrals of conftest.synth_integrals, float64 (168e6 numbers at sorb 192: two sizes are kept)"""
    return synth_integrals(sorb, seed=4321)


def occupations(c: Case) -> np.ndarray:
    """0/1 uint8 [n, sorb]"""
    occ = rand_occ(c.n, c.sorb, c.noA, c.noB, seed=7 * c.sorb + 3 * c.noA + c.noB)
    assert occ[:, 0::2].sum(1).tolist() == [c.noA] * c.n and occ[:, 1::2].sum(1).tolist() == [c.noB] * c.n
    return occ


def bits_of(onv: np.ndarray, sorb: int) -> np.ndarray:
    return np.ascontiguousarray(np.unpackbits(np.ascontiguousarray(onv), axis=-1, bitorder="little")[..., :sorb])


def column_sample(c: Case, width: int = 4096) -> np.ndarray:
    """`width` ascending columns of a long row: column 0, both neighbours of every class boundary, the last column, and runs of 64
    consecutive columns at seeded places (the generic pair kernel's singles are serial: a whole row of 1e6 columns is not for it)"""
    n = ncomb(c)
    assert n > width
    want = {0, n - 1} | {b + d for b in boundaries(c) for d in (-1, 0) if 0 <= b + d < n}
    g = np.random.default_rng(n)
    while len(want) < width:
        r0 = int(g.integers(0, n - 64))
        want |= set(range(r0, r0 + min(64, width - len(want))))
    cols = np.array(sorted(want), dtype=np.int64)
    assert cols.size == width
    return cols
