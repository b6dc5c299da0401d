"""The Jastrow-RBM yardstick of tests/jrbm_exact.py itself, and what does not need a GPU: with M = 0 it IS eloc_exact.walker; the flip
formula the kernel evaluates equals the direct difference of x^T M x for every excitation of every class; JastrowRBM.forward and its
autograd against the yardstick; the fused routes of the plain RBMs do not recognise the module (they would drop M); and, for every case
tests/test_gpu_jrbm.py lists, the conditions that keep a comparison from passing vacuously, from the reference alone."""
import time

import numpy as np
import pytest
import torch

import eloc_exact as X
import jrbm_exact as J
import rbm_exact as R
import test_gpu_jrbm as T
from conftest import rand_occ, synth_integrals

SHAPES = [(12, 3, 3), (12, 2, 4), (4, 1, 0), (2, 1, 1), (66, 3, 4)]


def _module(rbm, M):
    from pynqs_amd.rbm import JastrowRBM

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    return JastrowRBM(t(rbm.W), t(rbm.hb), t(rbm.vb), t(M))


@pytest.mark.parametrize("sorb,noA,noB", SHAPES)
def test_zero_jastrow_is_the_rbm_yardstick_bit_for_bit(sorb, noA, noB):
    h1, h2 = synth_integrals(sorb)
    rbm = R.regime_params("fe2s2", "real", sorb, 8, 0)
    for occ in rand_occ(2, sorb, noA, noB, seed=3):
        st = X.structure(occ, h1, h2)
        w0, w = X.walker(rbm, st), J.walker(rbm, np.zeros((sorb, sorb)), st)
        assert w.E == w0.E and np.array_equal(w.r, w0.r) and np.array_equal(w.rabs, w0.rabs)
        assert w.psi.re[0] == w0.psi.re[0] and w.lnmax == pytest.approx(w0.lnmax, rel=1e-15)
        assert bool((w.kappa == w0.kappa + 16.0).all())  # (no S: the constant of kappa_J alone)


@pytest.mark.parametrize("sorb,noA,noB", SHAPES)
def test_flip_formula_equals_the_direct_difference_in_every_class(sorb, noA, noB):
    """-2 sum_F x_i r_i + 4 sum_{i<j in F} S_ij x_i x_j = x'^T M x' - x^T M x, to 1e-17 of sum_ij |M_ij| (the scale of x^T M x; longdouble
    sums of sorb^2 terms), for random non-symmetric M with a diagonal and every single and double of a walker: hole-hole and
    particle-particle pairs enter with +, hole-particle pairs with -, through x_i x_j of the walker"""
    h1, h2 = synth_integrals(sorb)
    g = np.random.default_rng(sorb)
    M = 0.6 * (g.random((sorb, sorb)) - 0.5)
    assert not np.array_equal(M, M.T) and bool(np.diag(M).all())
    seen = set()
    for occ in rand_occ(3, sorb, noA, noB, seed=5):
        st = X.structure(occ, h1, h2)
        x = occ.astype(np.float64) * 2 - 1
        if not st.flips.shape[0]:
            continue
        direct = J.xmx(M, st.bits.astype(np.float64) * 2 - 1) - J.xmx(M, x[None, :])[0]
        flip = J.flip_delta(M, x, st.flips)
        assert float(np.abs(flip - direct).max()) <= 1e-17 * float(np.abs(M).sum()), float(np.abs(flip - direct).max())
        assert float(np.abs(direct).max()) > 1e-3
        for F in st.flips:
            F = [int(o) for o in F if o >= 0]
            seen.add((len(F), sum(o & 1 for o in F)))
        # tr M scales psi only: a diagonal changes no difference
        Md = M.copy()
        Md[np.diag_indices(sorb)] += 1.0
        assert float(np.abs(J.xmx(Md, st.bits.astype(np.float64) * 2 - 1) - J.xmx(Md, x[None, :])[0] - direct).max()) <= 1e-16 * sorb
    if (sorb, noA, noB) == (12, 3, 3):  # singles of either spin; alpha-alpha, alpha-beta, beta-beta doubles
        assert seen == {(2, 0), (2, 2), (4, 0), (4, 2), (4, 4)}, seen


@pytest.mark.parametrize("sorb,H,jreg", [(12, 20, "j-asym"), (12, 20, "j-strong"), (66, 40, "j-asym")])
def test_module_forward_meets_four_times_the_amplitude_bound(sorb, H, jreg):
    rbm, M = R.regime_params("fe2s2", "real", sorb, H, 0), J.jastrow_params(jreg, sorb)
    x = R.pm1(R.rand_words(50, sorb, seed=2), sorb)
    ex = J.exact_ld(rbm, M, x)
    assert float(np.abs(ex.re).max()) <= R.LN_MAX
    with torch.no_grad():
        got = _module(rbm, M)(torch.from_numpy(x)).numpy()
    ratio = J.amp_ratio(rbm, M, got, ex)
    print(f"JastrowRBM.forward sorb {sorb} {jreg}: worst error / bound {ratio.max():.3g}")
    assert bool((ratio <= 4.0).all())
    # and the factor is there: psi differs from the plain RBM's
    assert float(np.abs(ex.re - R.exact_ld(rbm, x).re).min()) > 1e-3


@pytest.mark.parametrize("sorb,H,n", [(12, 20, 64), (40, 80, 32)])
def test_autograd_of_the_module_gives_the_estimator_for_M(sorb, H, n):
    rbm, M = R.regime_params("fe2s2", "real", sorb, H, 0), J.jastrow_params("j-asym", sorb)
    x = R.pm1(R.rand_words(n, sorb, seed=11), sorb)
    g = np.random.default_rng([sorb, n])
    prob = g.random(n)
    prob /= prob.sum()
    eloc = -100.0 + g.standard_normal(n)
    e_total = float((prob * eloc).sum())
    gj = J.grad_exact(M, x, prob, eloc, e_total)
    m = _module(rbm, M)
    f = torch.from_numpy(gj.f.astype(np.float64))
    loss = 2 * (f * m(torch.from_numpy(x)).log()).sum()
    loss.backward()
    err = np.abs(m.jastrow.grad.numpy().astype(J.LD) - gj.G).astype(np.float64)
    print(f"autograd d/dM sorb {sorb} n {n}: worst error / bound {err.max() / gj.bound:.3g}")
    assert bool((err <= 4 * gj.bound).all())
    assert float(np.abs(gj.G).max()) > 1e3 * gj.bound


def test_fused_routes_of_the_plain_rbm_do_not_recognise_the_module():
    from pynqs_amd import C_extension as cx, energy, grad as G, rdm
    from pynqs_amd.rbm import JastrowRBM, RealRBM

    rbm, M = R.regime_params("fe2s2", "real", 12, 20, 0), J.jastrow_params("j-asym", 12)
    m = _module(rbm, M)
    assert isinstance(m, JastrowRBM) and not isinstance(m, RealRBM)
    assert getattr(m, "rbm_type", None) not in cx.RBM_FLAVOURS and getattr(m, "rbm_type", None) not in cx.RBM_TYPE_FLAVOUR
    assert [n for n, _ in m.named_parameters()] == ["weights", "hidden_bias", "visible_bias", "jastrow"]
    with pytest.raises(ValueError):
        G.FusedRbmGrad(m, 12)
    assert energy._real_rbm_params(m) is None and energy._complex_rbm_params(m) is None
    assert rdm._fused_params(m, 12, 6, 3, 3) is None
    wrapped = type("Wrapped", (), {"module": m})()  # (what DistributedDataParallel looks like to these functions)
    assert energy._real_rbm_params(wrapped) is None and rdm._fused_params(wrapped, 12, 6, 3, 3) is None
    assert energy._jastrow_rbm_params(m) is None  # (CPU parameters: the fused branch is for the GPU)


def test_gpu_cases_are_finite_well_conditioned_and_cannot_pass_without_the_jastrow_factor():
    t0 = time.time()
    jregs, words, forms = set(), set(), set()
    for c in T.CASES:
        ref = T.reference(c)
        assert len(ref.walkers) == c.n
        assert T.form_of(c) == c.form, (T.case_id(c), T.form_of(c))
        assert not (c.jreg == "j-strong" and c.sorb > 16)
        assert not np.array_equal(ref.M, ref.M.T) and bool(np.diag(ref.M).all())
        zero = np.zeros_like(ref.M)
        worst = np.inf
        for w in ref.walkers:
            b = w.bound()
            assert w.lnmax < 600.0, (T.case_id(c), w.lnmax)
            assert np.isfinite(complex(w.E).real) and np.isfinite(w.A) and np.isfinite(b) and b > 0
            assert b < 1e-9 * w.A, (T.case_id(c), b, w.A)
            key = ("zero", c.H, c.regime, c.ints, c.sorb, w.st.occ.tobytes())
            if key not in T._WALKER:
                T._WALKER[key] = J.walker(ref.rbm, zero, w.st)
            w0 = T._WALKER[key]
            if w.r.size:
                d = abs(complex(w.E - w0.E))
                assert d > 1e6 * b, (T.case_id(c), d, b)
                worst = min(worst, d / b)
            else:
                # a determinant without excitations (sorb 2, 1 + 1): E_loc = h_0 whatever M is; there the amplitude carries the factor
                assert w.E == w0.E
                dp = abs(float(np.expm1(w.psi.re[0] - w0.psi.re[0])))
                assert dp > 1e6 * float(J.amp_bound(ref.rbm, ref.M, w.psi.cond)[0]), (T.case_id(c), dp)
        print(f"{T.case_id(c)}: min |E(M) - E(0)| / bound {worst:.3g}, max bound / A {max(w.bound() / w.A for w in ref.walkers):.3g}, "
              f"max lnmax {max(w.lnmax for w in ref.walkers):.1f}")
        jregs.add(c.jreg)
        words.add((c.sorb - 1) // 64 + 1)
        forms.add(c.form)
    assert jregs == set(J.J_REGIMES) and words == {1, 2, 3} and forms == {T.R1, T.RC}
    # both homes of the pair factors are reached: the walker's triangle in LDS (one and two words, Fe2S2 among them) and the table in L2
    # (three words; tests/test_gpu_jrbm.py forces it for one word as well)
    homes = {(T.pairs_in_lds(c), c.sorb) for c in T.CASES}
    assert {(True, 12), (True, 40), (True, 66), (False, 130)} <= homes, homes
    # the other references of the GPU tests: finite amplitudes
    regime, jreg = T.FORWARD_RANDOM[3:]
    assert T.FORWARD_SHAPES[0] == T.FORWARD_RANDOM[:3] and {(s - 1) // 64 + 1 for s, _, _ in T.FORWARD_SHAPES} == {2, 3}
    for sorb, H, n in T.FORWARD_SHAPES:
        rbm, M = T.params(sorb, H, regime, jreg)
        assert float(np.abs(J.exact_ld(rbm, M, R.pm1(R.rand_words(n, sorb, seed=5), sorb)).re).max()) <= R.LN_MAX, (sorb, H, n)
    dt = time.time() - t0
    print(f"references of tests/test_gpu_jrbm.py: {dt:.1f} s")
    assert dt < 120.0
