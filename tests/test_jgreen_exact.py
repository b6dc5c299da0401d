"""What tests/test_gpu_jgreen.py relies on, from the reference alone (no GPU): for every case listed in tests/jgreen_exact.py
  1. at the Lambda in the largest gap at least one walker clamps and at least one does not;
  2. no sign decision is a matter of rounding (eloc_exact.Green.sure everywhere), so the allowance for unsure entries hides nothing;
  3. the Jastrow factor, being positive, changes no sign decision: `keep` is the plain RBM's;
  4. a kernel that dropped the Jastrow factor cannot pass: for at least one walker the row differs from the row at M = 0 by more than
     10^6 of its own per-entry bounds;
and green() on a jrbm_exact.walker with M = 0 is green() on eloc_exact.walker bit for bit; the uniforms of the step test keep a relative
10^-6 away from every edge of the walkers' cumulative rows, so that the two routes must move every walker to the same x'."""
import time

import numpy as np
import pytest

import eloc_exact as X
import jgreen_exact as JG
import jrbm_exact as J
import rbm_exact as R
from conftest import rand_occ, synth_integrals


def test_gpu_cases_clamp_some_walkers_decide_every_sign_surely_and_cannot_pass_without_the_jastrow_factor():
    t0 = time.time()
    words = set()
    for c in JG.CASES:
        ref, lam, rows = JG.green_reference(c)
        assert len(rows) == c.n and np.isfinite(lam)
        clamps = [g.clamp for g in rows]
        assert any(clamps) and not all(clamps), (JG.case_id(c), clamps)
        far = 0.0
        for w, g in zip(ref.walkers, rows):
            assert bool(g.sure.all()), (JG.case_id(c), int((~g.sure).sum()))
            assert bool(np.isfinite(g.g.astype(np.float64)).all()) and bool((g.bound > 0).all()) and bool((g.g >= 0).all())
            w0 = JG.zero_walker(c, ref, w)
            g0 = X.green(w0, lam, g.perm)
            assert np.array_equal(g.keep, g0.keep), JG.case_id(c)
            if g.g.size > 1:
                far = max(far, float((np.abs(g.g[1:] - g0.g[1:]).astype(np.float64) / g.bound[1:]).max()))
        print(f"{JG.case_id(c)}: Lambda {lam:.6g}, clamped {sum(clamps)} of {c.n}, max |g_J - g_RBM| / bound {far:.3g}")
        assert far > 1e6, (JG.case_id(c), far)  # (every case has a single or a double)
        words.add((c.sorb - 1) // 64 + 1)
    assert words == {1, 2, 3}
    dt = time.time() - t0
    print(f"references of tests/test_gpu_jgreen.py: {dt:.1f} s")
    assert dt < 180.0


@pytest.mark.parametrize("sorb,noA,noB", [(12, 3, 3), (12, 2, 4), (4, 1, 0)])
def test_zero_jastrow_gives_the_rbm_row_bit_for_bit(sorb, noA, noB):
    h1, h2 = synth_integrals(sorb)
    rbm = R.regime_params("fe2s2", "real", sorb, 8, 0)
    occ = rand_occ(3, sorb, noA, noB, seed=3)
    sts = [X.structure(o, h1, h2) for o in occ]
    w0s, wjs = [X.walker(rbm, st) for st in sts], [J.walker(rbm, np.zeros((sorb, sorb)), st) for st in sts]
    lam = X.lambda_in_largest_gap(w0s)
    assert lam == X.lambda_in_largest_gap(wjs)
    for w0, wj in zip(w0s, wjs):
        perm = np.arange(w0.r.size)[::-1].copy()
        a, b = X.green(w0, lam, perm), X.green(wj, lam, perm)
        assert np.array_equal(a.g, b.g) and np.array_equal(a.keep, b.keep) and a.v_sf == b.v_sf and a.k0 == b.k0 and a.clamp == b.clamp
        assert bool((b.bound >= a.bound).all())  # (kappa_J's constant)


def test_step_uniforms_keep_away_from_the_edges_of_the_cumulative_rows():
    c = JG.STEP_CASE
    ref, lam, rows = JG.green_reference(c)
    assert len(rows) == c.n == 64
    margin = JG.edge_margin(rows, JG.step_rand(c.n))
    print(f"{JG.case_id(c)}: Lambda {lam:.6g}, clamped {sum(g.clamp for g in rows)} of {c.n}, min |u beta - edge| / beta {margin:.3g}")
    assert margin > 1e-6
    assert all(float(g.g.sum()) > 0 for g in rows)
