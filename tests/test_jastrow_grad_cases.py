"""Conditions on the reference alone for the cases of tests/test_gpu_jastrow_grad.py (tests/jastrow_grad_cases.py): no GPU.  For every
case the bounds of jrbm_exact.grad_exact are finite and positive, a float64 restatement of the documented order of additions stays
within one bound, and every way in which a kernel could go wrong at the shape of the case misses by more than ten bounds -- so a
comparison under the bounds cannot pass by being loose.  A case that does not meet a share gets another seed in
jastrow_grad_cases.CASE_SEED."""
import time

import numpy as np
import pytest

import jastrow_grad_cases as C
import jrbm_exact as J

MISS = 10.0  # bounds by which a mutant has to miss


@pytest.fixture(scope="module")
def refs():
    """inputs, yardstick and transliteration of every case, computed once"""
    out = {}
    for c in C.CASES:
        inp = C.inputs(c)
        out[c] = (inp, J.grad_exact(inp.M, inp.x, inp.prob, inp.eloc, inp.e_total, inp.pow), C.transliteration(inp))
    return out


def _ratios(ge: J.JGrad, grad: np.ndarray, loss: float):
    """(|grad - exact| / bound per entry, |loss - exact| / its bound)"""
    rg = np.abs(grad.astype(J.LD) - ge.G).astype(np.float64) / ge.bound
    return rg, abs(float(J.LD(loss) - J.LD(ge.loss))) / ge.bloss


def test_the_case_list_reaches_every_structure():
    cs = C.CASES
    assert len(set(cs)) == len(cs) == 10
    assert {(c.sorb - 1) // 64 + 1 for c in cs} == {1, 2, 3} and max(c.sorb for c in cs) == 192 and max(c.n for c in cs) == 1025
    assert any(c.sorb == 64 for c in cs) and any(c.sorb == 128 for c in cs)            # the last bit of a word
    assert any(c.sorb * c.sorb % 256 == 0 and c.sorb * c.sorb >= 256 for c in cs)      # the loss alone in a block of 256 outputs
    assert any(c.sorb * c.sorb < 256 for c in cs) and any(c.n == 1 for c in cs)
    ng = {C.groups(c.n) for c in cs}
    assert {1, 2, 3, 8, 9, 17} <= ng                                                   # one group; no tail at 8; a tail of one at 9 and 17
    assert any(C.has_tail(c) and c.n > C.GROUP for c in cs) and any(not C.has_tail(c) for c in cs)
    assert any(c.zeros and c.pow for c in cs) and any(c.zeros and not c.pow for c in cs)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_bounds_are_finite_and_the_documented_order_stays_within_them(case, refs):
    inp, ge, (grad, loss) = refs[case]
    sf = float(np.abs(ge.f).sum())
    assert sf > 0 and np.isfinite(ge.bound) and ge.bound > 0 and np.isfinite(ge.bloss) and ge.bloss > 0
    assert inp.words.shape == (case.n, (case.sorb - 1) // 64 + 1) and ge.G.shape == (case.sorb, case.sorb)
    assert not np.array_equal(inp.M, inp.M.T) and bool(np.diag(inp.M).all())
    if case.zeros:
        assert bool((inp.prob[::3] == 0).all()) and int((inp.prob == 0).sum()) == len(inp.prob[::3])
    assert abs(float(inp.prob.sum()) - 1) < 1e-12
    # every orbital is occupied by some walker and empty in another (but for one walker): no bit is the same throughout
    if case.n > 1:
        assert bool((np.abs(inp.x.sum(0)) < case.n).all())
    # the bound is a rounding bound, not a tolerance: far below the gradient
    assert float(np.abs(ge.G).max()) > 1e6 * ge.bound and abs(ge.loss) > 1e6 * ge.bloss
    rg, rl = _ratios(ge, grad, loss)
    print(f"{C.case_id(case)}: transliteration worst error / bound: gradient {rg.max():.3g}, loss {rl:.3g}")
    assert float(rg.max()) <= 1.0 and rl <= 1.0


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_every_mutant_of_the_documented_order_misses_by_ten_bounds(case, refs):
    inp, ge, _ = refs[case]
    sorb = case.sorb
    offdiag = ~np.eye(sorb, dtype=bool)

    def run(mutant):
        return _ratios(ge, *C.transliteration(inp, mutant))

    said = []
    if sorb > 64:  # word 0 read for every orbital: the entries with an orbital at or above 64 (a pair o, o + 64 k reads one bit twice)
        rg, _ = run("word0")
        high = np.add.outer(np.arange(sorb) >= 64, np.arange(sorb) >= 64) > 0
        share = float((rg[high] > MISS).mean())
        said.append(f"word0 {100 * share:.1f} % of {int(high.sum())}")
        assert share >= 0.90, (C.case_id(case), share)
        assert float(rg[~high].max()) <= 1.0
    rg, rl = run("drop-last")
    said.append(f"drop-last {100 * float((rg > MISS).mean()):.1f} % (min {rg.min():.3g})")
    assert bool((rg > MISS).all()), (C.case_id(case), float(rg.min()))
    if C.has_tail(case):
        rg, rl = run("clamped-row")
        said.append(f"clamped-row {100 * float((rg > MISS).mean()):.1f} % (min {rg.min():.3g}), loss {rl:.3g}")
        assert bool((rg > MISS).all()) and rl > MISS, (C.case_id(case), float(rg.min()), rl)
    # the factor 2: wherever the gradient is not zero by itself.  A diagonal entry is 2 sum_n f_n, which vanishes with <E> the weighted
    # mean and c = 1, so the share is asked of the other entries; the diagonal is seen where it is not zero
    rg, _ = run("no-factor-2")
    share = float((rg[offdiag] > MISS).mean())
    said.append(f"no-factor-2 {100 * share:.1f} % off the diagonal")
    assert share >= 0.90, (C.case_id(case), share)
    if case.n == 1 or case.pow:
        assert bool((rg > MISS).all())
    if case.pow:
        rg, rl = run("no-pow")
        said.append(f"no-pow {100 * float((rg > MISS).mean()):.1f} %, loss {rl:.3g}")
        assert float((rg > MISS).mean()) >= 0.90 and rl > MISS, (C.case_id(case), rl)
    # tr M enters the loss as 2 tr M sum_n f_n: visible where sum_n f_n is not zero by itself (one walker with the offset, or c_n);
    # elsewhere the figure is printed only -- no kernel could be told from its mutant there
    rg, rl = run("no-trace")
    said.append(f"no-trace loss {rl:.3g}")
    assert float(rg.max()) <= 1.0
    if case.n == 1 or case.pow:
        assert rl > MISS, (C.case_id(case), rl)
    print(f"{C.case_id(case)}: mutants missing by more than {MISS:g} bounds: " + "; ".join(said))


def test_the_references_are_quick():
    t0 = time.time()
    for c in C.CASES:
        inp = C.inputs(c)
        J.grad_exact(inp.M, inp.x, inp.prob, inp.eloc, inp.e_total, inp.pow)
    dt = time.time() - t0
    print(f"yardsticks of tests/test_gpu_jastrow_grad.py: {dt:.2f} s")
    assert dt < 30.0
