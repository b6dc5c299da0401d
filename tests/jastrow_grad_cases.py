"""The cases of tests/test_gpu_jastrow_grad.py (pynqs_jastrow_grad through the C ABI) and their inputs, as host arrays, seeded by the case;
a plain module without a GPU.  The yardstick and the a-priori bounds are jrbm_exact.grad_exact's,
    per entry   u (n + 8) 2 sum_n |f_n|,      loss   u (2 sorb + n + 8) 2 sum_n |f_n| sum_ij |M_ij|.
`transliteration` restates in float64 the order of additions that include/pynqs_amd.h documents for pynqs_jastrow_grad (the walkers in
groups of 64, each group in walker order; then the groups in their order; then the factor 2) and takes the mutants that
tests/test_jastrow_grad_cases.py holds against the bounds: what a kernel could get wrong at the shape of a case.  It shares no code
with the kernel and is used by the CPU test only."""
from __future__ import annotations

from collections import namedtuple
from fractions import Fraction

import numpy as np

import jrbm_exact as J
import rbm_exact as R

GROUP = 64  # walkers whose terms are added in turn before the groups are

# sorb, n, prob[::3] = 0 exactly, c_n = 0.5 + U(0, 1): the smallest shapes that reach each structure
Case = namedtuple("Case", "sorb n zeros pow")
CASES = [
    Case(2, 1, False, False),       # fewer outputs than threads; one walker; e_total offset from eloc[0] (else f = 0)
    Case(16, 65, False, False),     # sorb^2 = 256: the loss is the lone output of the second block of 256; a full group plus one walker
    Case(64, 63, False, False),     # bit 63 of word 0; one short group
    Case(66, 129, False, False),    # bits 64 and 65 in word 1; two full groups plus one walker
    Case(128, 128, False, False),   # bit 127; two full groups exactly
    Case(130, 513, False, False),   # bits 128 and 129 in word 2; 9 groups: a second round of eight groups, with a tail of one
    Case(192, 1025, False, False),  # the largest sorb; 17 groups: a third round
    Case(130, 513, True, True),     # exact zeros among the probabilities, with c_n
    Case(66, 129, True, False),     # exact zeros, without c_n
    Case(40, 512, False, False),    # 8 groups exactly: no tail
]

# seed of a case's inputs where seed 0 fails a share of tests/test_jastrow_grad_cases.py (chosen on the reference alone): case -> seed
CASE_SEED = {}

Inputs = namedtuple("Inputs", "words x prob eloc e_total pow M")


def case_id(c: Case) -> str:
    return f"s{c.sorb}-n{c.n}" + ("-zeros" if c.zeros else "") + ("-pow" if c.pow else "")


def groups(n: int) -> int:
    return (n + GROUP - 1) // GROUP


def has_tail(c: Case) -> bool:
    """the last group is short: walkers past the end stand in it with f = 0"""
    return c.n % GROUP != 0


def inputs(c: Case) -> Inputs:
    """words uint64 [n, len], x = +-1 float64 [n, sorb], prob (sum 1), eloc = -100 + N(0, 1), e_total (a float: the weighted mean; with one
    walker eloc[0] + 0.37, or f = 0 and the case tests nothing), pow (c_n or None), M ("j-asym": a full matrix with a diagonal)"""
    seed = CASE_SEED.get(c, 0)
    g = np.random.default_rng([seed, c.sorb, c.n, int(c.zeros), int(c.pow)])
    words = R.rand_words(c.n, c.sorb, seed=23 + seed)
    prob = g.random(c.n)
    if c.zeros:
        prob[::3] = 0.0
    prob /= prob.sum()
    eloc = -100.0 + g.standard_normal(c.n)
    e_total = float((prob * eloc).sum()) if c.n > 1 else float(eloc[0] + 0.37)
    powc = 0.5 + g.random(c.n) if c.pow else None
    return Inputs(words, R.pm1(words, c.sorb), prob, eloc, e_total, powc, J.jastrow_params("j-asym", c.sorb))


def _in_turn(terms: np.ndarray) -> np.ndarray:
    """the float64 sum over axis 0, one term after the other"""
    s = np.zeros(terms.shape[1:])
    for t in terms:
        s = s + t
    return s


MUTANTS = ("word0", "drop-last", "clamped-row", "no-factor-2", "no-pow", "no-trace")


def transliteration(inp: Inputs, mutant: "str | None" = None):
    """(grad float64 [sorb, sorb], loss float64) in the documented order of additions.  Mutants:
      word0        every orbital's bit read from word 0 (orbital o as o mod 64)
      drop-last    the last walker left out
      clamped-row  the walkers past the end of the last group counted as walker n - 1 with ITS f instead of 0
      no-factor-2  the gradient without its factor 2
      no-pow       c_n taken as 1
      no-trace     x^T M x as sum_{i<j} (M + M^T)_ij x_i x_j, without tr M"""
    assert mutant is None or mutant in MUTANTS
    x, M = inp.x, inp.M
    n, sorb = x.shape
    c = np.ones(n) if inp.pow is None or mutant == "no-pow" else inp.pow
    # f_n = p_n (E_n - <E> c_n): the difference rounded once, then the product
    d = np.array([float(Fraction(float(e)) - Fraction(inp.e_total) * Fraction(float(cn))) for e, cn in zip(inp.eloc, c)])
    f = inp.prob * d
    xg = x[:, np.arange(sorb) & 63] if mutant == "word0" else x
    pad = groups(n) * GROUP - n
    if mutant == "drop-last":
        f = f.copy()
        f[-1] = 0.0
    fpad = np.concatenate([f, np.full(pad, f[-1] if mutant == "clamped-row" else 0.0)])
    xpad = np.concatenate([xg, np.repeat(xg[-1:], pad, 0)])
    xm = np.concatenate([x, np.repeat(x[-1:], pad, 0)])
    # x^T M x: row by row, every row and the rows themselves one term after the other
    q = np.zeros(n + pad)
    for a in range(sorb):
        q = q + xm[:, a] * np.add.accumulate(xm * M[a][None, :], axis=1)[:, -1]
    if mutant == "no-trace":
        q = q - float(np.trace(M))
    share = 2.0 * (fpad * q)
    part_g, part_l = [], []
    for g0 in range(0, n + pad, GROUP):
        sl = slice(g0, g0 + GROUP)
        part_g.append(_in_turn(fpad[sl, None, None] * (xpad[sl, :, None] * xpad[sl, None, :])))
        part_l.append(_in_turn(share[sl]))
    grad = _in_turn(np.array(part_g))
    return (grad if mutant == "no-factor-2" else 2.0 * grad), float(_in_turn(np.array(part_l)))
