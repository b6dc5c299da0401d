"""The yardstick of the fixed-node Green's row with the Jastrow factor (pynqs_green_jrbm; include/pynqs_amd.h) and the cases of
tests/test_gpu_jgreen.py.  No new arithmetic: jrbm_exact.walker gives an eloc_exact.Walker whose ratios carry exp(Delta x^T M x) and whose
kappa carries kappa_J; eloc_exact.green turns it into the exact row with the per-entry bound u a_k ((t_k + kappa_k + 2) |r_k| + ext_k) and
the g_0 / E_loc bound Walker.bound + 2 u (|Lambda| + A).  The columns follow the oracle's comb, matched by the bits of x' alone
(eloc_exact.match_columns); Lambda lies in the largest gap of the walkers' h_0 + v_sf (eloc_exact.lambda_in_largest_gap), so that some
walkers clamp and some do not.  The walkers' references are those of tests/test_gpu_jrbm.py (one cache: a walker the two files share
is computed once)."""
from collections import namedtuple

import numpy as np

import eloc_exact as X
import jrbm_exact as J
import test_gpu_jrbm as TJ

Case, case_id = TJ.Case, TJ.case_id
R1 = TJ.R1  # the row's form is always "resident, one workgroup per walker"

CASES = (
    # one word, one tile; theta through zero ("cross"); saturated units ("chunk-50"); M != M^T with a diagonal
    [Case(12, 3, 3, 20, 4, reg, "j-asym", "syn", R1) for reg in ("small", "fe2s2", "cross", "chunk-50")] + [
        Case(12, 3, 3, 20, 4, "fe2s2", "j-strong", "syn", R1),
        Case(12, 3, 3, 20, 4, "cross", "j-small", "syn", R1),
        Case(12, 2, 4, 7, 4, "fe2s2", "j-asym", "syn", R1),        # unequal spins: the rotations of the two same-spin classes differ; H < 8
        Case(4, 1, 0, 6, 2, "small", "j-asym", "syn", R1),         # no doubles, one column
        Case(66, 3, 4, 40, 2, "cross", "j-asym", "syn", R1),       # two words, 14 387 columns, many tiles on one workgroup
        Case(130, 3, 2, 64, 2, "chunk-50", "j-small", "syn", R1),  # three words: the pair factors from the table in L2 only
        Case(40, 15, 15, 80, 2, "fe2s2", "j-asym", "fe2s2", R1)])  # the workload's own structure
L2_CASES = [CASES[1], CASES[-1]]    # run a second time with PYNQS_JRBM_PAIRS=l2; by default they read the triangle in LDS
ZERO_CASES = [CASES[2], CASES[8]]   # M = 0 gives pynqs_green_rbm's row: 12, 3 + 3 "cross" and 66, 3 + 4
STEP_CASE = Case(12, 3, 3, 20, 64, "small", "j-small", "syn", R1)  # green_kernel + sample_update against the generic route
STEP_SEED = 5                       # of rand_num; tests/test_jgreen_exact.py checks the margin to the edges of the cumulative rows
UNSUPPORTED = (40, 3, 2, 520)       # sorb, noA, noB, H with pynqs_eloc_jrbm_supported = 0 (sorb x H beyond the LDS: 41 x 521 doubles)

Rows = namedtuple("Rows", "ref lam rows")
_ROWS = {}


def columns(c: Case, occ: np.ndarray) -> np.ndarray:
    """bits [n, ncomb, sorb] of every column in the reference's order, from the oracle's comb"""
    from oracle import oracle

    comb, _ = oracle.comb(TJ._bra(occ), c.sorb, c.noA, c.noB)
    return np.unpackbits(comb, axis=-1, bitorder="little")[..., :c.sorb]


def zero_walker(c: Case, ref, w: X.Walker) -> X.Walker:
    """the same walker with M = 0 (the cache key of tests/test_jrbm_exact.py)"""
    key = ("zero", c.H, c.regime, c.ints, c.sorb, w.st.occ.tobytes())
    if key not in TJ._WALKER:
        TJ._WALKER[key] = J.walker(ref.rbm, np.zeros_like(ref.M), w.st)
    return TJ._WALKER[key]


def green_reference(c: Case) -> Rows:
    """(test_gpu_jrbm.Ref, Lambda, [eloc_exact.Green per walker]), computed once per case"""
    if c not in _ROWS:
        ref = TJ.reference(c)
        bits = columns(c, ref.occ)
        lam = X.lambda_in_largest_gap(ref.walkers)
        _ROWS[c] = Rows(ref, lam, [X.green(w, lam, X.match_columns(w, bits[i])) for i, w in enumerate(ref.walkers)])
    return _ROWS[c]


def zero_reference(c: Case) -> Rows:
    """the same for M = 0 at the Lambda of its own gap: what pynqs_green_jrbm and pynqs_green_rbm must both give"""
    key = ("zero", c)
    if key not in _ROWS:
        ref = TJ.reference(c)
        ws = [zero_walker(c, ref, w) for w in ref.walkers]
        bits = columns(c, ref.occ)
        lam = X.lambda_in_largest_gap(ws)
        _ROWS[key] = Rows(ref._replace(M=np.zeros_like(ref.M), walkers=ws), lam,
                          [X.green(w, lam, X.match_columns(w, bits[i])) for i, w in enumerate(ws)])
    return _ROWS[key]


def rbm_reference(c: Case):
    """test_gpu_eloc_exact.Ref of the plain RBM of the case (same parameters, same walkers; that file's cache)"""
    T = TJ.T
    return T.reference(T.Case("rbm", "real", c.sorb, c.noA, c.noB, c.H, c.n, c.regime, c.ints, c.form))


def step_rand(n: int) -> np.ndarray:
    """the uniforms of the step test, float64 [n, 1]"""
    return np.random.default_rng(STEP_SEED).random((n, 1))


def edge_margin(rows, rand: np.ndarray) -> float:
    """min over walkers and columns of |rand_i beta_i - (g_0 + ... + g_k)| / beta_i on the exact rows (the empty sum included)"""
    worst = np.inf
    for g, u in zip(rows, rand.reshape(-1)):
        cum = np.concatenate([[X.LD(0)], np.cumsum(g.g)])
        beta = cum[-1]
        worst = min(worst, float(np.abs(X.LD(float(u)) * beta - cum).min() / beta))
    return worst
