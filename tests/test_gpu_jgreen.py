"""pynqs_green_jrbm -- the fixed-node Green's row of a Jastrow-RBM trial function in one kernel -- through gfmc.green_kernel, against the
exact yardstick of tests/jgreen_exact.py (jrbm_exact.walker + eloc_exact.green, numpy longdouble; columns in the order of the oracle's
comb, matched by bits).  The only tolerances are the a-priori rounding bounds of those modules,
    |g_k - g_k,exact| <= u a_k ((t_k + kappa_k + kappa_J,k + 2) |r_k| + ext_k)                              per row entry,
    g_0, E_loc: eloc_exact.Walker.bound (+ 2 u (|Lambda| + A) for g_0)                                       per walker;
no walker and no column is left out.  tests/test_jgreen_exact.py checks on the CPU that in every case some walker clamps and some does
not, that no sign decision is a matter of rounding, and that the row at M = 0 is 10^6 bounds and more away.

Worst error / bound over all cases on an MI355X: row entries 0.071 (12, 3 + 3 cross x j-small), g_0 0.20 (fe2s2 x j-strong), E_loc 0.013
(4, 1 + 0); with the pair factors from L2: 0.030, 0.021, 0.0032.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import eloc_exact as X
import jgreen_exact as JG
import test_gpu_jrbm as TJ
from conftest import ROOT

pytestmark = pytest.mark.gpu

_dev, _bra, _report = TJ._dev, TJ._bra, TJ._report
T = TJ.T


def _module(ref):
    from pynqs_amd.rbm import JastrowRBM

    return JastrowRBM(_dev(ref.rbm.W), _dev(ref.rbm.hb), _dev(ref.rbm.vb), _dev(ref.M)).cuda()


def _green_kernel(c, ref, lam, module=None, **kw):
    """gfmc.green_kernel on the case's walkers with the JastrowRBM module (or `module`)"""
    from pynqs_amd import gfmc, public_function as pf

    h1, h2 = T.integrals(c.ints, c.sorb)
    x = _dev(_bra(ref.occ))
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        m = _module(ref) if module is None else module
        ab = lambda xx, func: pf.ansatz_batch(func, xx, 100000, c.sorb, x.device, torch.float64)  # noqa: E731
        return x, gfmc.green_kernel(x, lam, _dev(h1), _dev(h2), m, ab, c.sorb, c.noA + c.noB, c.noA, c.noB, **kw)
    finally:
        torch.set_default_dtype(old)


def _check_rows(c, what, ref, lam, rows, eloc, gk, neg):
    """every entry within its bound, every sure entry on the right side, clamp and g_0 = 0 as the yardstick's sign, E_loc within the
    walker bound"""
    gk, neg = gk.cpu().numpy(), neg.cpu().numpy()
    assert gk.shape == (c.n, rows[0].g.size) and neg.shape == (c.n,)
    worst, diag, zeros_wrong, unsure = [], [], 0, 0
    for i, (w, g) in enumerate(zip(ref.walkers, rows)):
        got = gk[i]
        err = np.where(np.isfinite(got), np.abs(got.astype(X.LD) - g.g).astype(np.float64), np.inf)
        # an entry whose |h_k r_k| lies below its own bound may fall on either side of the sign decision (none does in these cases:
        # tests/test_jgreen_exact.py)
        alt = np.where(g.sure, np.inf, np.abs(got.astype(X.LD) - np.where(g.keep, 0, -w.hr.real[np.concatenate([[0], g.perm])])).astype(np.float64))
        ratio = np.minimum(err, alt) / g.bound
        worst.append(ratio[1:])
        diag.append(ratio[0])
        kept, dropped = g.sure & g.keep, g.sure & ~g.keep
        kept[0] = dropped[0] = False
        zeros_wrong += int((got[kept] == 0).sum()) + int((got[dropped] != 0).sum())
        unsure += int((~g.sure).sum())
        assert bool(neg[i]) == g.clamp and (got[0] == 0) == g.clamp, (i, float(g.k0), float(got[0]))
    ratio, diag = np.concatenate(worst), np.array(diag)
    re_ = T.eloc_ratio(ref, eloc.cpu().numpy())
    msg = [_report(f"{what} {JG.case_id(c)} row entries (Lambda {lam:.6g}, clamped {int(neg.sum())} of {neg.size}, unsure signs {unsure})", ratio),
           _report(f"{what} {JG.case_id(c)} g_0", diag), _report(f"{what} {JG.case_id(c)} E_loc", re_)]
    assert unsure == 0
    assert zeros_wrong == 0, f"{zeros_wrong} entries on the wrong side of the sign decision"
    assert bool((ratio <= 1.0).all()) and bool((diag <= 1.0).all()) and bool((re_ <= 1.0).all()), msg


def _row_case(c, what):
    from pynqs_amd import _native as N, gfmc

    assert gfmc.FUSED_GREEN and N.lib().pynqs_eloc_jrbm_supported(c.sorb, c.noA + c.noB, c.noA, c.noB, c.H) == 1
    ref, lam, rows = JG.green_reference(c)
    _, (eloc, gk, comb, stop, neg) = _green_kernel(c, ref, lam)
    assert isinstance(comb, gfmc.CombRows), "the row did not come from pynqs_green_jrbm"
    assert stop is False and comb.shape == (c.n, rows[0].g.size, 8 * ((c.sorb - 1) // 64 + 1))
    _check_rows(c, what, ref, lam, rows, eloc, gk, neg)


@pytest.mark.parametrize("case", JG.CASES, ids=JG.case_id)
def test_greens_row_meets_the_rounding_bound_per_entry(case):
    if case in JG.L2_CASES:
        assert TJ.pairs_in_lds(case)  # (the default run of these two reads the walker's triangle in LDS)
    if case.sorb > 128:
        assert not TJ.pairs_in_lds(case)
    _row_case(case, "green_jrbm")


@pytest.mark.parametrize("case", JG.L2_CASES, ids=JG.case_id)
def test_pair_factors_read_from_the_table_meet_the_same_bounds(case, monkeypatch):
    assert TJ.pairs_in_lds(case)
    monkeypatch.setenv("PYNQS_JRBM_PAIRS", "l2")
    assert not TJ.pairs_in_lds(case)
    _row_case(case, "green_jrbm (pairs in L2)")


def _tables(ref):
    from pynqs_amd import C_extension as cx

    return cx.RBMTable(_dev(ref.rbm.W), _dev(ref.rbm.hb), _dev(ref.rbm.vb)), cx.JastrowTable(_dev(ref.M))


def _green_jrbm(c, ref, lam, tab, jtab):
    from pynqs_amd import C_extension as cx

    h1, h2 = T.integrals(c.ints, c.sorb)
    e, g, neg, _ = cx.green_jrbm(_dev(_bra(ref.occ)), _dev(h1), _dev(h2), tab, jtab, c.sorb, c.noA + c.noB, c.noA, c.noB, lam)
    return e.cpu().numpy(), g.cpu().numpy(), neg.cpu().numpy()


@pytest.mark.parametrize("case", JG.ZERO_CASES, ids=JG.case_id)
def test_zero_jastrow_gives_the_rbm_kernels_row_bit_for_bit(case):
    """M = 0: every pair factor is exp(0) = 1 and r_o = 0 exactly, so the entries k >= 1 are those of pynqs_green_rbm bit for bit; g_0 and
    E_loc have no fixed bits (the waves pull tiles from a counter): under the sum of the two calls' bounds.  Both rows also meet the
    yardstick's bounds at M = 0."""
    from pynqs_amd import C_extension as cx, _native as N

    c = case
    ref, lam, rows = JG.zero_reference(c)
    assert not ref.M.any()
    tab, jtab = _tables(ref)
    ej, gj, nj = _green_jrbm(c, ref, lam, tab, jtab)
    h1, h2 = T.integrals(c.ints, c.sorb)
    x = _dev(_bra(ref.occ))
    plan = cx.plan_for(_dev(h1), _dev(h2), c.sorb, x.device)
    er, gr, nr = torch.empty(c.n, dtype=torch.float64, device=x.device), torch.empty(gj.shape, dtype=torch.float64, device=x.device), \
        torch.empty(c.n, dtype=torch.uint8, device=x.device)
    N.check(N.lib().pynqs_green_rbm(x.data_ptr(), c.n, c.sorb, c.noA + c.noB, c.noA, c.noB, plan.data_ptr(), tab.data_ptr(), tab.nhidden, N.RBM_REAL,
                                    float(lam), er.data_ptr(), None, gr.data_ptr(), nr.data_ptr(), torch.cuda.current_stream().cuda_stream), "pynqs_green_rbm")
    er, gr, nr = er.cpu().numpy(), gr.cpu().numpy(), nr.cpu().numpy()
    differ = int((gj[:, 1:].view(np.uint64) != gr[:, 1:].view(np.uint64)).sum())
    print(f"M = 0 {JG.case_id(c)}: {differ} of {gj[:, 1:].size} entries k >= 1 differ in bits from pynqs_green_rbm's")
    assert differ == 0 and int((gj[:, 1:] != 0).sum()) > 0
    assert np.array_equal(nj, nr) and nj.tolist() == [int(g.clamp) for g in rows]
    rbm_walkers = JG.rbm_reference(c).walkers
    for i, (wj, wr, g) in enumerate(zip(ref.walkers, rbm_walkers, rows)):
        assert wj.E == wr.E  # (one exact row for both)
        be = wj.bound() + wr.bound()
        b0 = g.bound[0] + X.green(wr, lam, g.perm).bound[0]
        print(f"  walker {i}: |dE| / bound {abs(ej[i] - er[i]) / be:.3g}, |dg_0| / bound {abs(gj[i, 0] - gr[i, 0]) / b0:.3g}")
        assert abs(ej[i] - er[i]) <= be and abs(gj[i, 0] - gr[i, 0]) <= b0
    for what, (e, g, n) in (("green_jrbm at M = 0", (ej, gj, nj)), ("green_rbm", (er, gr, nr))):
        _check_rows(c, what, ref, lam, rows, torch.from_numpy(e), torch.from_numpy(g), torch.from_numpy(n))


@pytest.mark.parametrize("case", [JG.CASES[1], JG.CASES[-1]], ids=JG.case_id)
def test_two_calls_give_the_same_row(case):
    c = case
    ref, lam, _ = JG.green_reference(c)
    tab, jtab = _tables(ref)
    _, g1, n1 = _green_jrbm(c, ref, lam, tab, jtab)
    _, g2, n2 = _green_jrbm(c, ref, lam, tab, jtab)
    assert np.array_equal(g1[:, 1:].view(np.uint64), g2[:, 1:].view(np.uint64)) and np.array_equal(n1, n2)
    assert int((g1[:, 1:] != 0).sum()) > 0


def test_a_step_agrees_with_the_generic_route():
    """green_kernel + sample_update with one fixed rand_num, fused and through comb + module: E_loc and the row to the tolerances of
    tests/test_gpu_gfmc_golden.py, the clamp mask, x_new and the accepted count equal (the uniforms keep a relative 10^-6 away from every
    edge of the exact cumulative rows: tests/test_jgreen_exact.py)"""
    from pynqs_amd import gfmc

    c = JG.STEP_CASE
    ref, lam, _ = JG.green_reference(c)
    rnd = _dev(JG.step_rand(c.n))
    wgt = _dev(np.random.default_rng(1).random(c.n) + 0.5)
    out, old_g = {}, gfmc.FUSED_GREEN
    try:
        for fused in (True, False):
            gfmc.FUSED_GREEN = fused
            x, (eloc, gk, comb, _, neg) = _green_kernel(c, ref, lam)
            assert isinstance(comb, gfmc.CombRows) == fused
            x_new, w_new, beta, acc = gfmc.sample_update(x, wgt, comb, gk, rnd)
            out[fused] = [t.cpu().numpy() for t in (eloc, gk, neg, x_new, w_new, beta)] + [acc]
    finally:
        gfmc.FUSED_GREEN = old_g
    scale = max(1.0, float(np.abs(out[False][1]).sum(1).max()))
    np.testing.assert_allclose(out[True][0], out[False][0], rtol=0, atol=1e-8 * scale)
    np.testing.assert_allclose(out[True][1], out[False][1], rtol=1e-9, atol=1e-11 * scale)
    assert np.array_equal(out[True][2], out[False][2]) and 0 < int(out[True][2].sum()) < c.n
    assert np.array_equal(out[True][3], out[False][3])
    np.testing.assert_allclose(out[True][4], out[False][4], rtol=1e-10)
    assert out[True][6] == out[False][6] and 0 < out[True][6]


def test_rejections_and_the_generic_branch():
    """NULL jastrow_table / green / clamped and a shape pynqs_eloc_jrbm does not serve: PYNQS_EINVAL from the host-side checks (nothing is
    launched); green_kernel takes the generic branch for that shape and with a WF_LUT"""
    from pynqs_amd import C_extension as cx, _native as N, gfmc, public_function as pf
    from pynqs_amd.rbm import JastrowRBM

    c = JG.CASES[0]
    ref, lam, _ = JG.green_reference(c)
    tab, jtab = _tables(ref)
    h1, h2 = T.integrals(c.ints, c.sorb)
    x = _dev(_bra(ref.occ))
    plan = cx.plan_for(_dev(h1), _dev(h2), c.sorb, x.device)
    ncomb = cx.get_Num_SinglesDoubles(c.sorb, c.noA, c.noB) + 1
    e, g, neg = torch.zeros(c.n, dtype=torch.float64, device=x.device), torch.full((c.n, ncomb), -7.0, dtype=torch.float64, device=x.device), \
        torch.full((c.n,), 9, dtype=torch.uint8, device=x.device)
    st = torch.cuda.current_stream().cuda_stream

    def call(xx, n, sorb, noA, noB, pl, t, jt, H, gp, cp):
        return N.lib().pynqs_green_jrbm(xx.data_ptr(), n, sorb, noA + noB, noA, noB, pl.data_ptr(), t.data_ptr(), jt, H, float(lam), e.data_ptr(), None,
                                        gp, cp, st)

    for jt, gp, cp in ((None, g.data_ptr(), neg.data_ptr()), (jtab.data_ptr(), None, neg.data_ptr()), (jtab.data_ptr(), g.data_ptr(), None)):
        assert call(x, c.n, c.sorb, c.noA, c.noB, plan, tab, jt, c.H, gp, cp) == N.EINVAL
    sorb, noA, noB, H = JG.UNSUPPORTED
    assert N.lib().pynqs_eloc_jrbm_supported(sorb, noA + noB, noA, noB, H) == 0 and not cx.eloc_jrbm_supported(sorb, noA + noB, noA, noB, H)
    gen = np.random.default_rng(sorb)
    W, hb, vb, M = 0.02 * (gen.random((H, sorb)) - 0.5), 0.1 * (gen.random(H) - 0.5), 0.1 * (gen.random(sorb) - 0.5), 0.01 * (gen.random((sorb, sorb)) - 0.5)
    big, jbig = cx.RBMTable(_dev(W), _dev(hb), _dev(vb)), cx.JastrowTable(_dev(M))
    hb1, hb2 = T.integrals("syn", sorb)
    occ = T.walkers(sorb, noA, noB, 2, "small")
    xb = _dev(_bra(occ))
    plan_big = cx.plan_for(_dev(hb1), _dev(hb2), sorb, xb.device)
    assert call(xb, 2, sorb, noA, noB, plan_big, big, jbig.data_ptr(), H, g.data_ptr(), neg.data_ptr()) == N.EINVAL
    assert b"pynqs_eloc_jrbm_supported" in N.lib().pynqs_last_error()
    torch.cuda.synchronize()
    assert bool((g == -7.0).all()) and bool((neg == 9).all())  # nothing was launched
    # the generic branch: comb_x is the materialised tensor
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        m = JastrowRBM(_dev(W), _dev(hb), _dev(vb), _dev(M)).cuda()
        ab = lambda xx, func: pf.ansatz_batch(func, xx, 100000, sorb, xb.device, torch.float64)  # noqa: E731
        out = gfmc.green_kernel(xb, 0.0, _dev(hb1), _dev(hb2), m, ab, sorb, noA + noB, noA, noB)
        assert torch.is_tensor(out[2]) and out[2].shape[:2] == out[1].shape
        m = _module(ref)
        ab = lambda xx, func: pf.ansatz_batch(func, xx, 100000, c.sorb, x.device, torch.float64)  # noqa: E731
        with torch.no_grad():
            lut = pf.WavefunctionLUT(x[:2].contiguous(), m(_dev(ref.occ[:2].astype(np.float64) * 2 - 1)), c.sorb, device=x.device)
        out = gfmc.green_kernel(x, lam, _dev(h1), _dev(h2), m, ab, c.sorb, c.noA + c.noB, c.noA, c.noB, WF_LUT=lut)
        assert torch.is_tensor(out[2])
        fused = gfmc.green_kernel(x, lam, _dev(h1), _dev(h2), m, ab, c.sorb, c.noA + c.noB, c.noA, c.noB)
        assert isinstance(fused[2], gfmc.CombRows)
        np.testing.assert_allclose(out[1].cpu().numpy(), fused[1].cpu().numpy(), rtol=1e-9, atol=1e-11 * float(fused[1].abs().sum(1).max()))
    finally:
        torch.set_default_dtype(old)


def test_fixed_node_gfmc_with_a_jastrow_rbm_converges_to_the_fixed_node_energy():
    """examples/gfmc_jrbm_fixed_node.py: every row of the run comes from pynqs_green_jrbm (CombRows), no walker is clamped, and the mixed
    estimator lands on the lowest eigenvalue of the fixed-node Hamiltonian diagonalised in the full determinant space (statistical error
    about 0.015 with 8192 walkers; the margin of the RBM example's test on the same problem size and population), well below the trial
    function's variational energy"""
    from pynqs_amd import gfmc

    spec = importlib.util.spec_from_file_location("gfmc_jrbm_fixed_node", os.path.join(ROOT, "examples", "gfmc_jrbm_fixed_node.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = {"rows": 0, "fused": 0, "clamped": 0}
    orig = gfmc.green_kernel

    def counting(*a, **k):
        out = orig(*a, **k)
        seen["rows"] += 1
        seen["fused"] += int(isinstance(out[2], gfmc.CombRows))
        seen["clamped"] += int(out[4].sum())
        return out

    old = torch.get_default_dtype()
    try:
        gfmc.green_kernel = counting
        e_exact, e_fn, e_gfmc, e_vmc = mod.run(generations=100, walkers=8192, burn_in=30, log=lambda *a: None)
    finally:
        gfmc.green_kernel = orig
        torch.set_default_dtype(old)
    print(f"E_exact {e_exact:+.6f}  E_FN {e_fn:+.6f}  E_GFMC {e_gfmc:+.6f}  E_VMC {e_vmc:+.6f}")
    assert seen == {"rows": 100, "fused": 100, "clamped": 0}, seen
    assert e_exact <= e_fn + 1e-9 and e_fn <= e_vmc + 1e-9
    assert e_vmc - e_fn > 0.5
    assert abs(e_gfmc - e_fn) < 0.08, (e_gfmc, e_fn)
    assert e_gfmc < e_vmc - 0.25
