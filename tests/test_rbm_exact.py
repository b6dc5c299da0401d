"""The exact RBM reference of tests/rbm_exact.py itself, on the CPU: longdouble against mpmath in every parameter regime of the GPU
tests, the evenness of psi in the hidden units, the reference against the vectors captured from the reference's own Python
(tests/golden: eloc_e2e_fe2s2, eloc_complex_module, eloc_rbm_flavours, grad_fe2s2), and the conditions that keep the GPU cases of
tests/test_gpu_rbm_exact.py from passing vacuously (finite normal psi in every row, bounded condition numbers, the form each
children shape takes).

Measured (x86-64 longdouble, 12 rows of 40 x 40 per regime and flavour): |ln psi_ld - ln psi_mpmath| / |ln psi| at most 1.7e-18 (the
regime with Im b = +-1000; elsewhere below 2e-19), i.e. under the 1e-17 asserted here and 3-4 orders below the float64 bounds it serves."""
import numpy as np
import pytest

import rbm_exact as R
import test_gpu_rbm_exact as T
from conftest import golden, pm1_from_onv

KINDS = ("real", "tanh", "pRBM", "complex")


def _regimes(kind):
    regs = [r for r in R.REGIMES_ANY + R.REGIMES_GRAD if not (kind == "tanh" and r == "novb")]  # (tanh(0) = 0: no amplitude at all)
    return regs + (list(R.REGIMES_COMPLEX) if kind == "complex" else [])


@pytest.mark.parametrize("kind", KINDS)
def test_longdouble_matches_mpmath_in_every_regime(kind):
    worst = 0.0
    for regime in _regimes(kind):
        words = R.rand_words(12, 40, 2)
        if regime == "one-338-w":
            bits = R.pm1(words, 40) > 0
            bits[:, R.forced_orbitals(40)] = True
            words = R.pack_bits(bits)
        rbm = R.regime_params(regime, kind, 40, 40, 0)
        x = R.pm1(words, 40)
        ex = R.exact_ld(rbm, x)
        w = R.check_against_mp(rbm, x, ex, np.arange(12))  # (asserts U_LD (sorb + H + 16) cond(x) per row)
        print(kind, regime, w)
        assert w["rel"] <= 1e-17, (regime, w)
        worst = max(worst, w["rel"])
    assert 0 < worst


@pytest.mark.parametrize("kind,sorb,H,regime", T.EVEN_CASES + [("complex", 40, 40, "imb1000"), ("real", 40, 40, "one-338")])
def test_reference_is_even_in_the_hidden_units(kind, sorb, H, regime):
    words = R.rand_words(40, sorb, 4)
    rbm, x, ex = R.checked_case(kind, sorb, H, regime, words)
    units = np.flatnonzero(np.random.default_rng(7).random(H) < 0.5)
    em = R.exact_ld(R.mirrored(rbm, units), x)
    tol = 2 * R.U_LD * (sorb + H + 16) * ex.cond
    d = np.abs(em.psi() / ex.psi() - 1).astype(np.float64)
    assert bool((d <= tol).all()), float((d / tol).max())
    assert np.allclose(em.cond, ex.cond, rtol=1e-14)
    # (and the mirror is not the identity: the phases of the hidden units change sign with them)
    assert not np.array_equal(R.mirrored(rbm, units).hb, rbm.hb)


def test_reference_reproduces_the_captured_python_amplitudes():
    """psi_simple of the reference's own runs (float64 PyTorch: its own rounding obeys the same bound, the operations are the same few)."""
    d0, dc, df = golden("eloc_e2e_fe2s2.npz"), golden("eloc_complex_module.npz"), golden("eloc_rbm_flavours.npz")
    for kind, rbm, onv, want in (("real", R.make("real", d0["W"], d0["hb"], d0["vb"]), d0["x"], d0["psi_simple"]),
                                 ("complex", R.make("complex", dc["Wc"], dc["hbc"], dc["vbc"]), dc["x"], dc["psi_simple"]),
                                 ("tanh", R.make("tanh", d0["W"], d0["hb"], d0["vb"]), df["x"], df["psi_simple_tanh"]),
                                 ("pRBM", R.make("pRBM", d0["W"], d0["hb"], d0["vb"]), df["x"], df["psi_simple_pRBM"])):
        x = pm1_from_onv(onv, 40)
        ex = R.exact(rbm, x, np.random.default_rng(0))
        ratio = R.amp_ratio(rbm, want, ex)
        print(kind, "captured psi: worst error / bound", float(ratio.max()), "bound", float(R.amp_bound(40, rbm.H, ex.cond).max()))
        assert want.shape == (32,) and bool((ratio <= 1.0).all()), (kind, float(ratio.max()))


@pytest.mark.parametrize("kind,amd,use_pow", [("real", -1, 0), ("real", 5, 1), ("complex", -1, 0), ("complex", 5, 1)])
def test_reference_reproduces_the_captured_python_gradients(kind, amd, use_pow):
    """grad_fe2s2.npz (vmc/grad/energy_grad.py through autograd in float64, one rank): every entry within the per-entry bound."""
    g, e0, d = golden("grad_fe2s2.npz"), golden("eloc_e2e_fe2s2.npz"), golden("eloc_flip_multipsi_fe2s2.npz")
    key = f"grad_{kind}_amd{amd}_pow{use_pow}"
    rbm = R.make("real", e0["W"], e0["hb"], e0["vb"]) if kind == "real" else R.make("complex", d["Wc"], d["hbc"], d["vbc"])
    x = pm1_from_onv(e0["x"], 40)
    ge = R.grad_exact(rbm, x, g[key + "_prob"], g[key + "_eloc"], g[key + "_e_total"].item(), g[key + "_pow"] if use_pow else None)
    errs = R.grad_errors(ge, g[f"{key}_ws1_params_weights"], g[f"{key}_ws1_params_hidden_bias"], g[f"{key}_ws1_params_visible_bias"],
                         kind == "complex")
    print(key, [float(e.max()) for e in errs], "bound / max|G|", float(ge.bW.max() / np.abs(ge.GW).max()))
    assert [e.size for e in errs] == [rbm.H * 40, rbm.H, 40] and all(bool((e <= 1.0).all()) for e in errs), [float(e.max()) for e in errs]


def test_gradient_reference_against_mpmath():
    """G_k of a small case summed with mpmath from mpmath's own tanh: the longdouble estimator agrees to 1e-17 of sum_n |f_n O_nk|."""
    import mpmath

    rbm, words, prob, eloc, e_total, pw = T.grad_inputs("complex", 12, 7, 31, "fe2s2", True, True, False)
    x = R.pm1(words, 12)
    ge = R.grad_exact(rbm, x, prob, eloc, e_total, pw)
    with mpmath.workdps(50):
        mp = mpmath.mp
        G = [[mp.mpc(0)] * 12 for _ in range(7)]
        A = [mp.mpf(0)] * 7
        for n in range(31):
            f = mp.mpf(float(prob[n])) * (mp.mpc(complex(eloc[n])) - mp.mpc(complex(e_total)) * mp.mpf(float(pw[n])))
            for h in range(7):
                th = mp.mpc(complex(rbm.hb[h])) + mp.fsum([mp.mpc(complex(rbm.W[h, o])) * int(x[n, o]) for o in range(12)])
                t = mp.conj(f) * mp.tanh(th)
                A[h] += abs(t)
                for o in range(12):
                    G[h][o] = G[h][o] + t * int(x[n, o])
        for h in range(7):
            for o in range(12):
                got = mp.mpc(R._mpf(ge.GW[h, o].real), R._mpf(ge.GW[h, o].imag))
                assert abs(got - G[h][o]) <= 1e-17 * A[h], (h, o)


def test_gpu_cases_are_finite_conditioned_and_take_the_form_they_name():
    """What the GPU tests assert on the reference before they touch the device, checked here for every listed case: |Re ln psi| <= 690
    in every row, cond(x) <= 1e4 for complex parameters, longdouble against mpmath on the spot-checked rows, the children's form."""
    for kind, sorb, H, n, regime in T.FORWARD_CASES:
        rbm, x, ex = R.checked_case(kind, sorb, H, regime, R.rand_words(n, sorb, 3))
        assert x.shape == (n, sorb)
    forms = set()
    for kind, sorb, H, regime, form in T.CHILD_CASES:
        assert R.children_form(sorb, H, kind) == form
        rbm, parents, rows, par, nflip, x, ex = T.children_case(kind, sorb, H, regime)
        assert set(nflip.tolist()) >= {0, 2, 4} and bool((np.diff(par) < 0).any())
        forms.add((form, kind == "complex", rows.shape[1]))
        if regime == "one-338-w":  # four flips take exp(-2 theta) of the saturated unit out of range, from parents well inside it
            h3 = 3 if H > 3 else 0
            th_p = (rbm.hb[h3] + R.pm1(parents, sorb) @ rbm.W[h3]).real
            th_c = (rbm.hb[h3] + x @ rbm.W[h3]).real
            assert float(th_p.min()) == -330.0 and float(th_c.min()) == -362.0
    assert forms >= {("lds", True, 1), ("lds", False, 1), ("lds", False, 2), ("lds", False, 3), ("lds", True, 3), ("wave", False, 2),
                     ("wave", True, 3), ("wave", False, 3), ("wave", True, 2)}
    for kind, sorb, H, regime in T.EVEN_CASES:
        T.children_case(kind, sorb, H, regime)
    for case in T.GRAD_CASES:
        kind, sorb, H, n = case[:4]
        rbm, words, prob, eloc, e_total, pw = T.grad_inputs(*case)
        ge = R.grad_exact(rbm, R.pm1(words, sorb), prob, eloc, e_total, pw)
        assert float(np.abs(ge.f).max()) > 0 and np.isfinite(ge.loss) and bool(np.isfinite(ge.bW).all() and (ge.bW > 0).all())
        if kind == "complex":
            assert float(R.exact_ld(rbm, R.pm1(words, sorb)).cond.max()) <= 1e4
        print(case, "bound / max|G|", float(ge.bW.max() / np.abs(ge.GW).max()))
