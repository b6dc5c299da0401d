"""The Jastrow-RBM density-matrix yardstick of tests/jrdm_exact.py itself and what needs no GPU: the owner / item decomposition of the
flip formula that kernels_rdm.hip (JASTROW) evaluates equals x'^T M x' - x^T M x in every class of excitation and on both owner sides;
with M = 0 the yardstick is rdm_exact's own for the RBM; on the full sorb = 8 space it equals the Fock-space matrices of the
Jastrow-RBM state; and the host-only entries of the C ABI (pynqs_rdm_jrbm_supported, pynqs_rdm_jrbm_workspace)."""
import numpy as np
import pytest

import jrbm_exact as J
import jrdm_exact as JX
import rbm_exact as R
import rdm_exact as X
from conftest import golden, rand_occ

LD = np.longdouble


def _decomposed(S, x, owner, item):
    """Delta of the module docstring of jrdm_exact: owner orbitals all x = xo, item orbitals all x = -xo"""
    r = S @ x
    xo = x[owner[0]]
    xl = -xo
    assert all(x[o] == xo for o in owner) and all(x[o] == xl for o in item)
    d = -2 * xo * sum(r[o] for o in owner) - 2 * xl * sum(r[o] for o in item)
    if len(owner) == 2:
        d += 4 * S[owner[0], owner[1]] + 4 * S[item[0], item[1]]
    d -= 4 * sum(S[o, l] for o in owner for l in item)
    return d


def test_owner_item_decomposition_equals_the_direct_difference_in_every_class():
    sorb, noA, noB = 12, 3, 3
    M = J.jastrow_params("j-asym", sorb)
    S = J.s_matrix(M)
    scale = float(np.abs(M).sum())
    seen = set()
    for occ in rand_occ(3, sorb, noA, noB, seed=9):
        x = occ.astype(LD) * 2 - 1
        q0 = J.xmx(M, x[None, :])[0]
        occd, emp = [o for o in range(sorb) if occ[o]], [o for o in range(sorb) if not occ[o]]
        exc = [((h,), (q,), "single") for h in occd for q in emp if (h ^ q) & 1 == 0]
        for a, h0 in enumerate(occd):
            for h1 in occd[:a]:
                for b, p0 in enumerate(emp):
                    for p1 in emp[:b]:
                        if sorted((h0 & 1, h1 & 1)) == sorted((p0 & 1, p1 & 1)):
                            exc.append(((h0, h1), (p0, p1), "same-spin double" if (h0 ^ h1) & 1 == 0 else "alpha-beta double"))
        for holes, parts, cls in exc:
            xp = x.copy()
            xp[list(holes + parts)] *= -1
            direct = J.xmx(M, xp[None, :])[0] - q0
            for owner, item, side in ((holes, parts, "owner occupied"), (parts, holes, "owner empty")):
                d = _decomposed(S, x, owner, item)
                assert abs(float(d - direct)) <= 1e-17 * scale, (cls, side, holes, parts, float(d - direct))
                seen.add((cls, side))
            assert abs(float(direct)) > 0
    assert len(seen) == 6, seen


def _full_space(H, regime, jregime):
    occ = golden("c1_sorb8_all36.npz")["occ"].astype(np.int8)
    rbm = R.regime_params(regime, "real", 8, H, 7)
    M = J.jastrow_params(jregime, 8) if jregime else np.zeros((8, 8))
    return occ, rbm, M


def test_zero_jastrow_is_the_rbm_yardstick():
    occ, rbm, M = _full_space(3, "small", None)
    g = np.random.default_rng(5)
    w = g.random(occ.shape[0]) + 0.1
    w = w / w.sum()
    est, _ = JX.estimate(rbm, M, occ, w)
    ref = X.estimator(occ, w, rbm=rbm)
    for a, b in ((est.rdm1, ref.rdm1), (est.rdm2, ref.rdm2)):
        assert bool((np.abs(a - b) <= 2.0 ** -60 * np.abs(b)).all())
    assert np.array_equal(est.m1, ref.m1) and np.array_equal(est.m2, ref.m2)
    assert np.allclose(est.A1, ref.A1, rtol=1e-14, atol=0) and np.allclose(est.A2, ref.A2, rtol=1e-14, atol=0)
    assert est.kappa_fused == ref.kappa_fused + 16.0  # (no S: the constant of kappa_J alone)


@pytest.mark.parametrize("jregime", ["j-asym", "j-strong"])
def test_yardstick_equals_fock_space_of_the_jastrow_rbm_state(jregime):
    occ, rbm, M = _full_space(8, "fe2s2", jregime)
    e = J.exact_ld(rbm, M, occ.astype(np.float64) * 2 - 1)
    psi = np.exp(e.re - e.re.max())
    p = psi ** 2
    p = (p / p.sum()).astype(np.float64)
    est, _ = JX.estimate(rbm, M, occ, p)
    f1, f2 = X.fock_rdm(occ, psi)
    b = JX.bound(est, "ratio")
    b1, b2 = b[:f1.size] + 1e-18, b[f1.size:] + 1e-18
    assert bool((np.abs(est.rdm1 - f1).astype(np.float64) <= b1).all()), float(np.abs(est.rdm1 - f1).max())
    assert bool((np.abs(est.rdm2 - f2).astype(np.float64) <= b2).all()), float(np.abs(est.rdm2 - f2).max())
    # it cannot pass without the Jastrow factor: the RBM's own matrices differ by far more than the bound
    ref = X.estimator(occ, p, rbm=rbm)
    assert float(np.abs(ref.rdm2 - f2).max()) > 1e6 * float(b2.max())


def test_kappa_jastrow_dominates_every_excitation():
    """the case constant is jrbm_exact.kappa_jastrow's count maximised over the excitations"""
    sorb = 10
    M = J.jastrow_params("j-strong", sorb)
    g = np.random.default_rng(1)
    flips = np.stack([g.permutation(sorb)[:4] for _ in range(200)])
    flips[:50, 2:] = -1
    assert float(J.kappa_jastrow(M, flips).max()) <= JX.kappa_jastrow(M)
    assert JX.kappa_jastrow(np.zeros((4, 4))) == 16.0


def test_supported_and_workspace_of_the_jastrow_flavour():
    from pynqs_amd import _native as N

    lib = N.lib()
    assert lib.pynqs_rdm_jrbm_supported(8, 4, 2, 2, 17) == 1 and lib.pynqs_rdm_jrbm_supported(40, 30, 15, 15, 80) == 1
    assert lib.pynqs_rdm_jrbm_supported(8, 4, 2, 2, 600) == 0 and lib.pynqs_rdm_jrbm_supported(120, 60, 30, 30, 80) == 0
    assert lib.pynqs_rdm_jrbm_supported(8, 5, 2, 2, 8) == 0
    for n, sorb, H in ((0, 8, 3), (1, 8, 17), (8192, 40, 80), (300, 66, 17)):
        assert lib.pynqs_rdm_jrbm_workspace(n, sorb, H) == lib.pynqs_rdm_rbm_workspace(n, sorb, H) + 8 * n * sorb
    assert lib.pynqs_rdm_jrbm_workspace(-1, 8, 3) == -1 and lib.pynqs_rdm_jrbm_workspace(8, 7, 3) == -1
    # null pointers and sizes that are not served: PYNQS_EINVAL before anything touches a device
    assert lib.pynqs_rdm_jrbm(None, 0, 8, 4, 2, 2, None, None, None, 17, None, None, None, None) == N.EINVAL
    assert lib.pynqs_rdm_jrbm(None, 0, 8, 4, 2, 2, None, None, None, 600, None, None, None, None) == N.EINVAL
