"""CPU side of stochastic reconfiguration: the exact host reference of tests/rbm_sr_exact.py against dense algebra, the conditions that
keep the GPU tests' a-priori bound from being vacuous (at most 1e-9 of max |S v| on every case; a float64 evaluation in another
summation order well inside it), the reference's own result (tests/golden/sr_fe2s2.npz, vmc/grad/sr.py:_calculate_sr) against the
exact solve, and the C ABI of the new entry points as far as it runs without a GPU."""
import numpy as np
import pytest

import rbm_exact as R
import rbm_sr_exact as SE
from conftest import golden


def _case(kind, sorb, no, H, n):
    rbm, words, prob, eloc, e_total = SE.case_inputs(kind, sorb, no, H, n)
    return SE.sr_exact(rbm, R.pm1(words, sorb), prob), prob, eloc, e_total


@pytest.mark.parametrize("kind,sorb,no,H,n", [("complex", 12, 3, 5, 64), ("real", 12, 3, 7, 40), ("real", 72, 6, 9, 65)])
def test_matrix_free_product_is_the_dense_matrix(kind, sorb, no, H, n):
    se, prob, eloc, e_total = _case(kind, sorb, no, H, n)
    S = se.S_dense()
    scale = float(np.abs(S).max())
    assert float(np.abs(S - S.T).max()) <= 1e-18 * scale
    c = se.c(np.random.default_rng(1).standard_normal(S.shape[0]))
    # sum_n p_n c_n = (1 - sum_n p_n) Obar.z, and the float64 probabilities add up to 1 within n u
    assert float(np.abs((se.p * c).sum())) <= 2 * n * R.U * float(np.abs(c).max())
    for name, v in SE.probe_vectors(se):
        y, want = se.matvec(v), S @ v.astype(R.LD)
        assert float(np.abs(y - want).max()) <= 1e-15 * float(np.abs(want).max()), name  # (longdouble: 2^-64 times the number of terms)
    # float64 eigenvalues: positive semi-definite up to rounding
    w = np.linalg.eigvalsh(S.astype(np.float64))
    assert w.min() >= -1e-14 * w.max()
    # the solve: the longdouble residual of d is at the level of longdouble rounding, for the reference's shift and a small one
    F = SE.energy_gradient(se, prob, eloc, e_total)
    for shift in (0.02, 1e-3):
        d, last = se.solve(F, shift)
        r = se.residual(F, d, shift)
        assert last <= SE.SOLVE_FLOOR and float(np.sqrt((r * r).sum())) <= 1e-15 * float(np.sqrt((F * F).sum())), (shift, last)
        dense = np.linalg.solve(S.astype(np.float64) + shift * np.eye(S.shape[0]), F.astype(np.float64))
        assert float(np.abs(dense - d).max()) <= 1e-9 * float(np.abs(d).max())


def _float64_product(se, v):
    """S v in float64, walkers in the opposite order and the centring applied to O first (another order of operations than the kernel's)"""
    O = se.O.astype(np.complex128 if se.cplx else np.float64)[::-1]
    p = se.p.astype(np.float64)[::-1]
    J = O - (p @ O)[None, :]
    z = se.to_z(v).astype(O.dtype)
    y = np.conj(J).T @ (p * (J @ z))
    return np.asarray(se.to_flat(y), dtype=np.float64)


@pytest.mark.parametrize("kind,sorb,no,H,n", SE.CASES + SE.PRODUCT_SHAPES)
def test_bound_is_tight_enough_to_mean_something(kind, sorb, no, H, n):
    se, *_ = _case(kind, sorb, no, H, n)
    _check_bound(se, f"{kind} {sorb}x{H} n {n}")


@pytest.mark.parametrize("kind,sorb,H,n,regime", SE.SATURATED)
def test_bound_on_saturated_hidden_units(kind, sorb, H, n, regime):
    rbm, words, prob, eloc, e_total = SE.saturated_inputs(kind, sorb, H, n, regime)
    se = SE.sr_exact(rbm, R.pm1(words, sorb), prob)
    assert float(np.abs(R.exact_ld(rbm, se.x).y).max()) > 1 - 1e-15  # a saturated unit is there
    _check_bound(se, f"{kind} {sorb}x{H} n {n} {regime}")


def _check_bound(se, what):
    for name, v in SE.probe_vectors(se):
        y = se.matvec(v)
        b = se.product_bound(v)
        ymax = float(np.abs(y).max())
        if name == "zero":
            assert ymax == 0.0 and float(b.max()) == 0.0
            continue
        if se.x.shape[0] == 1:  # one walker: O = Obar, S = 0; the bound is absolute then, on the scale sum_k |z_k| of the terms of c_n
            assert ymax <= 1e-18 and float(b.max()) <= 1e-12 * float(np.abs(v).sum()), (what, name, ymax, float(b.max()))
            continue
        err = np.abs(_float64_product(se, v).astype(R.LD) - y).astype(np.float64)
        print(f"{what} {name}: bound / max|y| {float(b.max()) / ymax:.3g}; float64 error / bound {float((err / b).max()):.3g}")
        assert float(b.max()) <= 1e-9 * ymax, (what, name, float(b.max()), ymax)
        assert bool((err <= b).all()), (what, name, float((err / b).max()))


def test_reference_fixture_is_the_exact_solve_within_its_recorded_distance():
    g, e0, f = golden("grad_fe2s2.npz"), golden("eloc_e2e_fe2s2.npz"), golden("sr_fe2s2.npz")
    rbm = R.make("real", e0["W"], e0["hb"], e0["vb"])
    words = np.ascontiguousarray(e0["x"]).view(np.uint64).reshape(32, -1)
    shift = float(f["diag_shift"])
    assert shift == 0.02
    for amd, pw in ((-1, 0), (5, 1)):
        key = f"grad_real_amd{amd}_pow{pw}"
        se = SE.sr_exact(rbm, R.pm1(words, 40), g[key + "_prob"])
        F = np.concatenate([g[f"{key}_ws1_params_{nm}"].reshape(-1) for nm in ("weights", "hidden_bias", "visible_bias")])
        d_ref = np.concatenate([f[f"sr_real_amd{amd}_pow{pw}_{nm}"].reshape(-1) for nm in ("weights", "hidden_bias", "visible_bias")])
        d, last = se.solve(F, shift)
        dist = float(np.sqrt(((d_ref - d) ** 2).sum()) / np.sqrt((d * d).sum()))
        stored = float(f[f"sr_real_amd{amd}_pow{pw}_dist"])
        print(f"{key}: reference to exact {dist:.3e} (stored {stored:.3e})")
        assert last <= SE.SOLVE_FLOOR and abs(dist - stored) <= 1e-3 * stored + 1e-16 and stored <= 1e-8


def test_c_abi_of_the_sr_entry_points():
    from pynqs_amd import _native as N

    lib = N.lib()
    groups = (1000 + 31) // 32
    assert lib.pynqs_rbm_sr_workspace(1000, 40, 80, N.RBM_REAL) == 8 * (1000 * 80 + groups * 3320 + 2)
    assert lib.pynqs_rbm_sr_workspace(1000, 40, 40, N.RBM_COMPLEX) == 8 * (2 * 1000 * 40 + groups * 2 * 1680 + 2)
    assert lib.pynqs_rbm_sr_workspace(0, 40, 40, N.RBM_COMPLEX) == 16
    for bad in ((-1, 40, 40, N.RBM_REAL), (10, 0, 40, N.RBM_REAL), (10, 193, 40, N.RBM_REAL), (10, 40, 0, N.RBM_REAL), (10, 40, 40, N.RBM_TANH)):
        assert lib.pynqs_rbm_sr_workspace(*bad) == -1
    assert lib.pynqs_rbm_sr_cg_step(7, 10, None, None, None, None, None, None, 1.0, 0.02, 1e-6, None) == N.EINVAL
    assert lib.pynqs_rbm_sr_matvec(None, 10, 40, 40, N.RBM_TANH, None, None, None, None, None, None) == N.EINVAL
    from pynqs_amd import sr  # noqa: F401  (importable without a GPU)
