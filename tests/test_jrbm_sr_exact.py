"""CPU side of stochastic reconfiguration for the Jastrow-RBM: the exact host reference of tests/jrbm_sr_exact.py against dense algebra
(S symmetric, positive semi-definite, zero on the rows of M's diagonal; the refined solve), the conditions that keep the GPU tests'
a-priori bound from being vacuous (at most 1e-9 of max |S v| on every case and every non-degenerate probe; a float64 evaluation in
another summation order inside it), and the C ABI of the new entry points as far as it runs without a GPU."""
import numpy as np
import pytest

import jrbm_sr_exact as JS
import rbm_exact as R
from conftest import golden


def _case(sorb, no, H, n):
    rbm, M, words, prob, eloc, e_total = JS.case_inputs(sorb, no, H, n)
    return JS.sr_exact(rbm, R.pm1(words, sorb), prob), M, prob, eloc, e_total


@pytest.mark.parametrize("sorb,no,H,n", [(12, 3, 5, 64), (12, 3, 7, 40), (20, 5, 6, 65)])
def test_matrix_free_product_is_the_dense_matrix(sorb, no, H, n):
    se, M, prob, eloc, e_total = _case(sorb, no, H, n)
    assert se.P == H * sorb + H + sorb + sorb * sorb
    S = se.S_dense()
    scale = float(np.abs(S).max())
    assert float(np.abs(S - S.T).max()) <= 1e-18 * scale
    off = 2 * abs(float(1 - se.p.sum()))  # y = O^T diag(p) c and S v = J^T diag(p) c differ by Obar sum_n p_n c_n, |c_n| <= 2 sum_k |v_k|
    for name, v in JS.probe_vectors(se):
        y, want = se.matvec(v), S @ v.astype(R.LD)
        assert float(np.abs(y - want).max()) <= 1e-15 * float(np.abs(want).max()) + off * float(np.abs(v).sum()), name
    w = np.linalg.eigvalsh(S.astype(np.float64))
    assert w.min() >= -1e-14 * w.max()
    # O_ii = 1 for every walker: the rows (and columns) of M's diagonal vanish, up to 1 - sum_n p_n
    diag = se.nrbm + np.arange(sorb) * (sorb + 1)
    assert float(np.abs(S[diag, :]).max()) <= 4 * n * R.U * scale
    # O_ij = O_ji: the rows of (i, j) and (j, i) are the same numbers
    Sm = S[se.nrbm:, :].reshape(sorb, sorb, -1)
    assert np.array_equal(Sm, Sm.transpose(1, 0, 2))
    # only the symmetric part of Z reaches c_n
    anti = dict(JS.probe_vectors(se))["antisymmetric Z"]
    assert float(np.abs(se.c(anti)).max()) <= 1e-17 * float(np.abs(anti).sum())
    F = JS.energy_gradient(se, M, prob, eloc, e_total)
    Fm = F[se.nrbm:].reshape(sorb, sorb)
    assert np.array_equal(Fm, Fm.T)
    for shift in (0.02, 1e-3):
        d, last = se.solve(F, shift)
        r = se.residual(F, d, shift)
        assert last <= JS.SOLVE_FLOOR and float(np.sqrt((r * r).sum())) <= 1e-15 * float(np.sqrt((F * F).sum())), (shift, last)
        dense = np.linalg.solve(S.astype(np.float64) + shift * np.eye(S.shape[0]), F.astype(np.float64))
        assert float(np.abs(dense - d).max()) <= 1e-9 * float(np.abs(d).max())
        # d_ii = F_ii / shift on M's diagonal
        assert float(np.abs(d[diag] - F[diag] / shift).max()) <= 1e-12 * float(np.abs(d).max())


@pytest.mark.parametrize("sorb,no,H,n", JS.CASES)
def test_refined_solve_meets_the_floor(sorb, no, H, n):
    se, M, prob, eloc, e_total = _case(sorb, no, H, n)
    F = JS.energy_gradient(se, M, prob, eloc, e_total)
    for shift in (0.02, 1e-3):
        d, last = se.solve(F, shift)
        print(f"{sorb}x{H} n {n} shift {shift}: last correction {last:.2e}")
        assert last <= JS.SOLVE_FLOOR, (shift, last)


def _float64_product(se, v):
    """S v in float64, walkers in the opposite order and the centring applied to O first (another order of operations than the kernel's)"""
    O = se.O.astype(np.float64)[::-1]
    p = se.p.astype(np.float64)[::-1]
    Jm = O - (p @ O)[None, :]
    return Jm.T @ (p * (Jm @ np.asarray(v, dtype=np.float64)))


def _check_bound(se, what):
    for name, v in JS.probe_vectors(se):
        y = se.matvec(v)
        b = se.product_bound(v)
        assert b.shape == y.shape
        ymax = float(np.abs(y).max())
        if name == "zero":
            assert ymax == 0.0 and float(b.max()) == 0.0
            continue
        if se.x.shape[0] == 1 or name in JS.DEGENERATE:
            # the exact product vanishes (one walker: O = Obar; M's diagonal: O_ii = Obar_ii = 1; antisymmetric Z: c_n = 0) up to
            # 1 - sum p: the bound is absolute then, on the scale sum_k |v_k| of the terms of c_n
            assert ymax <= 4 * se.x.shape[0] * R.U * float(np.abs(v).sum()) and float(b.max()) <= 1e-12 * float(np.abs(v).sum()), (what, name, ymax, float(b.max()))
            continue
        err = np.abs(_float64_product(se, v).astype(R.LD) - y).astype(np.float64)
        print(f"{what} {name}: bound / max|y| {float(b.max()) / ymax:.3g}; float64 error / bound {float((err / b).max()):.3g}")
        assert float(b.max()) <= 1e-9 * ymax, (what, name, float(b.max()), ymax)
        assert bool((err <= b).all()), (what, name, float((err / b).max()))


@pytest.mark.parametrize("sorb,no,H,n", JS.CASES + JS.PRODUCT_SHAPES)
def test_bound_is_tight_enough_to_mean_something(sorb, no, H, n):
    se, *_ = _case(sorb, no, H, n)
    _check_bound(se, f"{sorb}x{H} n {n}")


@pytest.mark.parametrize("sorb,H,n,regime", JS.SATURATED)
def test_bound_on_saturated_hidden_units(sorb, H, n, regime):
    rbm, M, words, prob, eloc, e_total = JS.saturated_inputs(sorb, H, n, regime)
    se = JS.sr_exact(rbm, R.pm1(words, sorb), prob)
    assert float(np.abs(se.ex.y).max()) > 1 - 1e-15  # a saturated unit is there
    _check_bound(se, f"{sorb}x{H} n {n} {regime}")


def test_reference_fixture_is_the_exact_solve_within_its_recorded_distance():
    """tests/golden/sr_jrbm_fe2s2.npz (make_golden_sr_jrbm.py): the reference's _calculate_sr with the x_i x_j columns, on the exact gradient"""
    g, e0, f = golden("grad_fe2s2.npz"), golden("eloc_e2e_fe2s2.npz"), golden("sr_jrbm_fe2s2.npz")
    rbm = R.make("real", e0["W"], e0["hb"], e0["vb"])
    words = np.ascontiguousarray(e0["x"]).view(np.uint64).reshape(32, -1)
    shift, key = float(f["diag_shift"]), "grad_real_amd-1_pow0"
    assert shift == 0.02
    se = JS.sr_exact(rbm, R.pm1(words, 40), g[key + "_prob"])
    F = JS.energy_gradient(se, np.zeros((40, 40)), g[key + "_prob"], np.asarray(g[key + "_eloc"]).real, float(np.asarray(g[key + "_e_total"]).real))
    assert np.array_equal(F.astype(np.float64), f["F"])  # the right-hand side the reference was given
    # its RBM blocks are the reference's own gradient (grad_fe2s2.npz) to that fixture's rounding
    Fr = np.concatenate([g[f"{key}_ws1_params_{nm}"].reshape(-1) for nm in ("weights", "hidden_bias", "visible_bias")])
    assert float(np.abs(Fr - f["F"][:se.nrbm]).max()) <= 1e-12 * float(np.abs(Fr).max())
    d_ref = np.concatenate([f[nm].reshape(-1) for nm in ("weights", "hidden_bias", "visible_bias", "jastrow")])
    d, last = se.solve(f["F"], shift)
    dist = float(np.sqrt(((d_ref - d) ** 2).sum()) / np.sqrt((d * d).sum()))
    stored = float(f["dist"])
    print(f"reference to exact {dist:.3e} (stored {stored:.3e})")
    assert last <= JS.SOLVE_FLOOR and abs(dist - stored) <= 1e-3 * stored + 1e-16 and stored <= 1e-8


def test_c_abi_of_the_jastrow_sr_entry_points():
    from pynqs_amd import _native as N

    lib = N.lib()
    groups = (1000 + 31) // 32
    assert lib.pynqs_jrbm_sr_workspace(1000, 40, 80) == 8 * (1000 * 80 + groups * (3320 + 20 * 41) + 2)
    assert lib.pynqs_jrbm_sr_workspace(33, 65, 7) == 8 * (33 * 7 + 2 * (7 * 66 + 65 + 33 * 66) + 2)  # odd sorb: ceil(65 / 2) rows of 66
    assert lib.pynqs_jrbm_sr_workspace(0, 40, 40) == 16
    for bad in ((-1, 40, 40), (10, 0, 40), (10, 193, 40), (10, 40, 0)):
        assert lib.pynqs_jrbm_sr_workspace(*bad) == -1
    assert lib.pynqs_jrbm_sr_prepare(None, 10, 40, None, None, 40, None, None, None, None) == N.EINVAL
    assert lib.pynqs_jrbm_sr_matvec(None, 10, 40, 40, None, None, None, None, None, None) == N.EINVAL
    assert lib.pynqs_jrbm_sr_matvec(None, 10, 193, 40, None, None, None, None, None, None) == N.EINVAL
    # the RBM entry keeps its formula
    assert lib.pynqs_rbm_sr_workspace(1000, 40, 80, N.RBM_REAL) == 8 * (1000 * 80 + groups * 3320 + 2)
    from pynqs_amd import sr

    assert issubclass(sr.FusedJastrowRbmSR, sr._FusedSR) and issubclass(sr.FusedRbmSR, sr._FusedSR)  # one CG driver, importable without a GPU
