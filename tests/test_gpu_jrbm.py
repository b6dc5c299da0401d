"""The Jastrow-RBM kernels (pynqs_eloc_jrbm, pynqs_jrbm_forward, pynqs_jastrow_grad) and their Python layers against the exact yardstick of
tests/jrbm_exact.py (numpy longdouble; the ratio's Jastrow part formed directly from the two rows and M): every tolerance is an a-priori
rounding bound derived in that module's docstring,
    E_loc:   eloc_exact.Walker.bound with kappa_k + kappa_J,k                                            per walker,
    psi(x):  |psi / psi_exact - 1| <= u [(sorb + H + 16) cond(x) + (2 sorb + 4) sum_ij |M_ij|]           per walker, both kernels,
    grad_M:  |got - exact| <= u (n + 8) 2 sum_n |p_n| |E_n - <E> c_n|                                     per entry,
and rbm_exact's per-entry bound for the gradients of W, b, a.  No walker, column or gradient entry is left out.  The cases are the
smallest shapes at which each structure can go wrong; which form a case takes is asked of the library (pynqs_eloc_jrbm_form).
tests/test_jrbm_exact.py checks the yardstick itself on the CPU and that every case listed here is finite, well conditioned and such
that a kernel that dropped any part of the Jastrow factor could not pass."""
import functools
import importlib.util
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

import eloc_exact as X
import jrbm_exact as J
import rbm_exact as R
import test_gpu_eloc_exact as T
from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "sorb noA noB H n regime jreg ints form")
R1, RC = T.R1, T.RC

CASES = (
    # every combination of the RBM regimes with the Jastrow regimes: one word, one tile, one workgroup per walker
    [Case(12, 3, 3, 20, 4, reg, jreg, "syn", R1) for reg in ("small", "fe2s2", "cross", "chunk-50") for jreg in ("j-small", "j-asym", "j-strong")] + [
        Case(12, 3, 3, 20, 1025, "small", "j-asym", "syn", R1),   # many walkers, un-chunked
        Case(12, 2, 4, 7, 4, "fe2s2", "j-asym", "syn", R1),       # unequal spins, H below the chunk of eight
        Case(2, 1, 1, 3, 1, "small", "j-asym", "syn", R1),        # degenerate classes, no same-spin doubles (no excitation at all)
        Case(4, 1, 0, 6, 2, "small", "j-asym", "syn", R1),        # degenerate classes, no doubles
        Case(66, 3, 4, 40, 2, "cross", "j-asym", "syn", RC),      # two words, chunked
        Case(130, 3, 2, 64, 2, "chunk-50", "j-small", "syn", RC),  # three words, chunked
        Case(40, 15, 15, 80, 2, "fe2s2", "j-asym", "fe2s2", RC)])  # the workload's own structure, chunked

ROUTE_CASE = CASES[-1]          # through energy.local_energy, with <S-S+> (the shipped S-S+ integrals are Fe2S2's)
FALLBACK_CASE = CASES[4]        # 12, 3 + 3, fe2s2 x j-asym: the module route
FORWARD_RANDOM = (66, 40, 300, "fe2s2", "j-asym")  # sorb, H, determinants, regimes
FORWARD_SHAPES = [FORWARD_RANDOM[:3], (130, 9, 257), (192, 8, 65)]  # sorb, H, determinants: two words, three words, the largest sorb
GRAD_CASES = [(12, 20, 64, "fe2s2", "j-asym"), (40, 80, 32, "fe2s2", "j-asym")]  # sorb, H, n, regimes

# seeds of rbm_exact.regime_params / jrbm_exact.jastrow_params where seed 0 fails a condition of tests/test_jrbm_exact.py (on the reference
# alone): (sorb, H, regime, jreg) -> (RBM seed, Jastrow seed)
PARAM_SEED = {}


def case_id(c):
    return f"{c.sorb}.{c.noA}+{c.noB}-H{c.H}-n{c.n}-{c.regime}-{c.jreg}-{c.ints}"


@functools.lru_cache(maxsize=None)
def params(sorb: int, H: int, regime: str, jreg: str):
    s = PARAM_SEED.get((sorb, H, regime, jreg), (0, 0))
    return R.regime_params(regime, "real", sorb, H, s[0]), J.jastrow_params(jreg, sorb, s[1])


_WALKER = {}
Ref = namedtuple("Ref", "case rbm M occ walkers psi")


def reference(c: Case, ints=None, tag="E") -> Ref:
    """The yardstick of a case, computed once per (parameters, integrals, determinant) and shared by the tests; ints: other integrals
    than the case's own (the S-S+ integrals of the route test), with a tag of their own"""
    rbm, M = params(c.sorb, c.H, c.regime, c.jreg)
    occ = T.walkers(c.sorb, c.noA, c.noB, c.n, c.regime)
    h1, h2 = T.integrals(c.ints, c.sorb) if ints is None else ints
    ws = []
    for row in occ:
        ks = (tag, c.ints, c.sorb, row.tobytes())
        if ks not in T._STRUCT:
            T._STRUCT[ks] = X.structure(row, h1, h2)
        kw = ("jrbm", c.H, c.regime, c.jreg) + ks
        if kw not in _WALKER:
            _WALKER[kw] = J.walker(rbm, M, T._STRUCT[ks])
        ws.append(_WALKER[kw])
    cat = lambda f: np.concatenate([getattr(w.psi, f) for w in ws])  # noqa: E731
    return Ref(c, rbm, M, occ, ws, R.Exact(rbm.kind, cat("re"), cat("im"), cat("vis"), cat("cond"), cat("y"), cat("sech2")))


def form_of(c: Case) -> str:
    from pynqs_amd import _native as N

    assert N.lib().pynqs_eloc_jrbm_supported(c.sorb, c.noA + c.noB, c.noA, c.noB, c.H) == 1, case_id(c)
    f = N.lib().pynqs_eloc_jrbm_form(c.n, c.sorb, c.noA + c.noB, c.noA, c.noB, c.H)
    assert f >= 0 and not f & 1, (case_id(c), f)
    return "resident" + (" chunked" if f & 2 else " one")


def pairs_in_lds(c: Case) -> bool:
    """where the launch reads the pair factors: the walker's triangle in LDS (bit 2 of the form), else the table in L2"""
    from pynqs_amd import _native as N

    return bool(N.lib().pynqs_eloc_jrbm_form(c.n, c.sorb, c.noA + c.noB, c.noA, c.noB, c.H) & 4)


_dev, _bra, _report = T._dev, T._bra, T._report


def tables(ref: Ref):
    from pynqs_amd import C_extension as cx

    return cx.RBMTable(_dev(ref.rbm.W), _dev(ref.rbm.hb), _dev(ref.rbm.vb)), cx.JastrowTable(_dev(ref.M))


def run_kernel(c: Case, ref: Ref, ints=None, want_psi=True):
    from pynqs_amd import C_extension as cx

    h1, h2 = T.integrals(c.ints, c.sorb) if ints is None else ints
    tab, jtab = tables(ref)
    e, p = cx.eloc_jrbm(_dev(_bra(ref.occ)), _dev(h1), _dev(h2), tab, jtab, c.sorb, c.noA + c.noB, c.noA, c.noB, want_psi=want_psi)
    return e.cpu().numpy(), (p.cpu().numpy() if want_psi else None)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_local_energy_and_amplitudes_meet_the_rounding_bounds(case):
    """E_loc and psi(x) from cx.eloc_jrbm, psi(x) from cx.jrbm_forward on the same walkers"""
    from pynqs_amd import C_extension as cx

    c = case
    assert form_of(c) == c.form
    ref = reference(c)
    e, p = run_kernel(c, ref)
    pf_ = cx.jrbm_forward(_dev(_bra(ref.occ)), _dev(ref.rbm.W), _dev(ref.rbm.hb), _dev(ref.rbm.vb), _dev(ref.M), c.sorb).cpu().numpy()
    re_ = T.eloc_ratio(ref, e)
    rp, rf = J.amp_ratio(ref.rbm, ref.M, p, ref.psi), J.amp_ratio(ref.rbm, ref.M, pf_, ref.psi)
    msg = [_report(f"eloc_jrbm {case_id(c)} E_loc", re_), _report(f"eloc_jrbm {case_id(c)} psi(x)", rp),
           _report(f"jrbm_forward {case_id(c)} psi(x)", rf)]
    assert bool((re_ <= 1.0).all()) and bool((rp <= 1.0).all()) and bool((rf <= 1.0).all()), msg


@pytest.mark.parametrize("case", [CASES[4], CASES[-1]], ids=case_id)
def test_pair_factors_read_from_the_table_meet_the_same_bound(case, monkeypatch):
    """PYNQS_JRBM_PAIRS=l2: the pair factors from the table in L2, the form that sorb x H near the LDS limit and three-word determinants
    take by themselves, on shapes that keep the triangle in LDS by default"""
    c = case
    assert pairs_in_lds(c)
    monkeypatch.setenv("PYNQS_JRBM_PAIRS", "l2")
    assert not pairs_in_lds(c) and form_of(c) == c.form
    ref = reference(c)
    e, p = run_kernel(c, ref)
    re_, rp = T.eloc_ratio(ref, e), J.amp_ratio(ref.rbm, ref.M, p, ref.psi)
    msg = [_report(f"eloc_jrbm (pairs in L2) {case_id(c)} E_loc", re_), _report(f"eloc_jrbm (pairs in L2) {case_id(c)} psi(x)", rp)]
    assert bool((re_ <= 1.0).all()) and bool((rp <= 1.0).all()), msg


@pytest.mark.parametrize("sorb,H,n", FORWARD_SHAPES)
def test_forward_on_random_determinants_of_two_and_three_words(sorb, H, n):
    from pynqs_amd import C_extension as cx

    regime, jreg = FORWARD_RANDOM[3:]
    rbm, M = params(sorb, H, regime, jreg)
    words = R.rand_words(n, sorb, seed=5)
    ex = J.exact_ld(rbm, M, R.pm1(words, sorb))
    assert float(np.abs(ex.re).max()) <= R.LN_MAX
    onv = torch.from_numpy(words.view(np.uint8).reshape(n, -1)).cuda()
    got = cx.jrbm_forward(onv, _dev(rbm.W), _dev(rbm.hb), _dev(rbm.vb), _dev(M), sorb).cpu().numpy()
    ratio = J.amp_ratio(rbm, M, got, ex)
    msg = _report(f"jrbm_forward sorb {sorb} H {H} on {n} random determinants", ratio)
    assert bool((ratio <= 1.0).all()), msg


def _module(ref: Ref):
    from pynqs_amd.rbm import JastrowRBM

    return JastrowRBM(_dev(ref.rbm.W), _dev(ref.rbm.hb), _dev(ref.rbm.vb), _dev(ref.M)).cuda()


def _local_energy(c: Case, ref: Ref, calls, **kw):
    """energy.local_energy (SIMPLE) on the case's walkers with the JastrowRBM module; calls: the CX entries it used"""
    from pynqs_amd import energy, public_function as pf

    h1, h2 = T.integrals(c.ints, c.sorb)
    x = _dev(_bra(ref.occ))
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    names = ("eloc_rbm", "eloc_crbm", "eloc_jrbm")
    orig = {n: getattr(energy.CX, n) for n in names}
    try:
        for n, f in orig.items():
            setattr(energy.CX, n, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(f, n))
        assert energy.FUSED_RBM
        ab = lambda xx, func: pf.ansatz_batch(func, xx, 100000, c.sorb, x.device, torch.float64)  # noqa: E731
        return energy.local_energy(x, _dev(h1), _dev(h2), _module(ref), ab, c.sorb, c.noA + c.noB, c.noA, c.noB, **kw)
    finally:
        for n, f in orig.items():
            setattr(energy.CX, n, f)
        torch.set_default_dtype(old)


def test_energy_layer_takes_the_fused_branch_also_for_spin_raising():
    """energy.local_energy, SIMPLE, takes pynqs_eloc_jrbm: the call is seen at C_extension.eloc_jrbm, psi(x) has the bits cx.eloc_jrbm
    gives and E_loc is under its bound; <S-S+> comes from the same kernel with the S-S+ integrals, under the yardstick's bound for those
    integrals.  (E_loc itself has no fixed bits from launch to launch, here as in pynqs_eloc_rbm: the waves pull their tiles from a
    counter, so the order in which a walker's columns and <x|H|x> are added depends on which wave was free, and a chunked launch adds
    its parts with atomics.  psi(x) is summed in a fixed order.)"""
    c = FALLBACK_CASE
    ref, calls = reference(c), []
    el, _, ps, _ = _local_energy(c, ref, calls)
    e, p = run_kernel(c, ref)
    assert calls == ["eloc_jrbm"], calls
    r1 = T.eloc_ratio(ref, el.cpu().numpy())
    assert np.array_equal(ps.cpu().numpy(), p) and bool((r1 <= 1.0).all()), _report(f"local_energy {case_id(c)} E_loc", r1)
    c = ROUTE_CASE
    ref, calls = reference(c), []
    s = golden("eloc_spin_raising_fe2s2.npz")
    spin = (np.ascontiguousarray(s["h1e_spin"], dtype=np.float64), np.ascontiguousarray(s["h2e_spin"], dtype=np.float64))
    sref = reference(c, ints=spin, tag="S")
    el, sl, ps, _ = _local_energy(c, ref, calls, use_spin_raising=True, h1e_spin=_dev(spin[0]), h2e_spin=_dev(spin[1]))
    assert calls == ["eloc_jrbm", "eloc_jrbm"], calls
    e, p = run_kernel(c, ref)
    assert np.array_equal(ps.cpu().numpy(), p)
    re_, rs = T.eloc_ratio(ref, el.cpu().numpy()), T.eloc_ratio(sref, sl.cpu().numpy())
    msg = [_report(f"local_energy {case_id(c)} E_loc", re_), _report(f"local_energy {case_id(c)} <S-S+>", rs)]
    assert bool((re_ <= 1.0).all()) and bool((rs <= 1.0).all()), msg
    assert float(np.abs(sl.cpu().numpy()).max()) > 0


def test_module_route_agrees_with_the_yardstick():
    """energy.FUSED_RBM = False: get_comb_tensor plus the module's forward on every x', to the project's module-route tolerance"""
    from pynqs_amd import energy, public_function as pf

    c = FALLBACK_CASE
    ref = reference(c)
    h1, h2 = T.integrals(c.ints, c.sorb)
    x = _dev(_bra(ref.occ))
    old, old_flag = torch.get_default_dtype(), energy.FUSED_RBM
    torch.set_default_dtype(torch.float64)
    try:
        energy.FUSED_RBM = False
        ab = lambda xx, func: pf.ansatz_batch(func, xx, 100000, c.sorb, x.device, torch.float64)  # noqa: E731
        el, _, ps, _ = energy.local_energy(x, _dev(h1), _dev(h2), _module(ref), ab, c.sorb, c.noA + c.noB, c.noA, c.noB)
    finally:
        energy.FUSED_RBM = old_flag
        torch.set_default_dtype(old)
    want = np.array([float(w.E.real) for w in ref.walkers])
    d = np.abs(el.cpu().numpy() - want)
    print(f"module route {case_id(c)}: max |E - E_exact| {d.max():.3e} Ha")
    assert float(d.max()) <= 1e-8
    assert float(np.abs(ps.cpu().numpy() / np.exp(ref.psi.re).astype(np.float64) - 1).max()) <= 1e-10


@pytest.mark.parametrize("sorb,H,n,regime,jreg", GRAD_CASES, ids=lambda v: str(v))
def test_fused_gradient_meets_the_bounds_and_is_reproducible(sorb, H, n, regime, jreg):
    from pynqs_amd import grad as G
    from pynqs_amd.rbm import JastrowRBM

    rbm, M = params(sorb, H, regime, jreg)
    words = R.rand_words(n, sorb, seed=11)
    x = R.pm1(words, sorb)
    g = np.random.default_rng([sorb, n])
    prob = g.random(n)
    prob /= prob.sum()
    eloc = -100.0 + g.standard_normal(n)
    e_total = float((prob * eloc).sum())
    ge, gj = R.grad_exact(rbm, x, prob, eloc, e_total), J.grad_exact(M, x, prob, eloc, e_total)
    m = JastrowRBM(_dev(rbm.W), _dev(rbm.hb), _dev(rbm.vb), _dev(M)).cuda()
    onv = torch.from_numpy(words.view(np.uint8).reshape(n, -1)).cuda()
    fg = G.FusedJastrowRbmGrad(m, sorb)
    loss = fg(onv, _dev(prob), _dev(eloc), _dev(np.array(e_total)))
    got = {k: getattr(m, k).grad.detach().cpu().numpy().copy() for k in fg.names}
    loss1 = float(loss)
    # W, b, a: rbm_exact's per-entry bound; M: the bound of jrbm_exact, every entry
    errs = R.grad_errors(ge, got["weights"], got["hidden_bias"], got["visible_bias"], False)
    rm = np.where(np.isfinite(got["jastrow"]), np.abs(got["jastrow"].astype(J.LD) - gj.G).astype(np.float64), np.inf) / gj.bound
    msg = [_report(f"grad {k} sorb {sorb} n {n}", r.ravel()) for k, r in zip(("W", "b", "a"), errs)] + [_report(f"grad M sorb {sorb} n {n}", rm.ravel())]
    assert all(bool((r <= 1.0).all()) for r in errs) and bool((rm <= 1.0).all()), msg
    assert rm.shape == (sorb, sorb)
    # the loss: 2 sum f_n ln psi_n = the RBM's part + the Jastrow part, each under its bound
    want = ge.loss + gj.loss
    print(f"loss {loss1!r} exact {want!r} |diff| {abs(loss1 - want):.3e} bound {ge.bloss + gj.bloss:.3e}")
    assert abs(loss1 - want) <= ge.bloss + gj.bloss
    # two calls give the same bits
    loss2 = float(fg(onv, _dev(prob), _dev(eloc), _dev(np.array(e_total))))
    assert loss2 == loss1 and all(np.array_equal(getattr(m, k).grad.cpu().numpy(), got[k]) for k in fg.names)
    # grad() through the module
    m2 = JastrowRBM(_dev(rbm.W), _dev(rbm.hb), _dev(rbm.vb), _dev(M)).cuda()
    lm = G.grad(m2, _dev(x), _dev(prob), _dev(eloc), e_total, 1.0, torch.double)
    for k in fg.names:
        a, b = getattr(m2, k).grad.cpu().numpy(), got[k]
        rel = float(np.abs(a - b).max() / max(np.abs(a).max(), 1e-300))
        print(f"{k}: fused against grad() through the module, max |diff| / max |grad| {rel:.3e}")
        assert rel <= 1e-10, (k, rel)
    assert abs(float(lm) - loss1) <= 1e-10 * max(abs(loss1), 1.0)
    # extra_psi_pow: the same bound for M with c_n
    powc = 0.5 + g.random(n)
    gp = J.grad_exact(M, x, prob, eloc, e_total, powc)
    fg(onv, _dev(prob), _dev(eloc), _dev(np.array(e_total)), _dev(powc))
    rp = np.abs(m.jastrow.grad.cpu().numpy().astype(J.LD) - gp.G).astype(np.float64) / gp.bound
    assert bool((rp <= 1.0).all()), _report(f"grad M with extra_psi_pow sorb {sorb} n {n}", rp.ravel())


def test_example_optimises_both_ansaetze():
    spec = importlib.util.spec_from_file_location("vmc_rbm_jastrow", os.path.join(ROOT, "examples", "vmc_rbm_jastrow.py"))
    mod = importlib.util.module_from_spec(spec)
    old = torch.get_default_dtype()
    try:
        spec.loader.exec_module(mod)
        rbm, jrbm, e0 = mod.run(steps=30)
    finally:
        torch.set_default_dtype(old)
    assert len(rbm) == len(jrbm) == 30
    for name, h in (("RBM", rbm), ("Jastrow-RBM", jrbm)):
        assert h[-1] < h[0] and min(h) >= e0 - 1e-9, (name, h[0], h[-1], min(h), e0)
    assert abs(rbm[0] - jrbm[0]) <= 1e-12, (rbm[0], jrbm[0])  # M = 0 at step 0
    print(f"after 30 steps: RBM {rbm[-1]:+.8f}, Jastrow-RBM {jrbm[-1]:+.8f}, exact ground state {e0:+.8f}: "
          f"the {'Jastrow-RBM' if jrbm[-1] < rbm[-1] else 'RBM'} is lower")
