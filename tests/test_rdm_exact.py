"""The yardstick of the reduced density matrices (tests/rdm_exact.py) checked against itself on the CPU: the estimator from the
definition (a) against the Jordan-Wigner matrices on the Fock space (b), identity E against the oracle's Hamiltonian matrix, and the
trace identities, on all 36 determinants of sorb 8 (2 alpha, 2 beta)."""
import numpy as np
import pytest

import rbm_exact as R
import rdm_exact as X
from conftest import golden, synth_integrals
from oracle import oracle as O

LD = np.longdouble


@pytest.fixture(scope="module")
def full_space():
    d = golden("c1_sorb8_all36.npz")
    occ = d["occ"].astype(np.int8)
    g = np.random.default_rng(11)
    psi = g.standard_normal(occ.shape[0])
    key = {tuple(int(b) for b in o): c for o, c in zip(occ, psi)}
    amp = lambda rows: np.array([key[tuple(int(b) for b in r)] for r in rows], dtype=LD).astype(np.clongdouble)  # noqa: E731
    p = psi.astype(LD) ** 2
    p = (p / p.sum()).astype(np.float64)
    est = X.estimator(occ, p, amplitude=amp)
    return d, occ, psi, p, est


def test_estimator_equals_fock_space(full_space):
    d, occ, psi, p, est = full_space
    f1, f2 = X.fock_rdm(occ, psi)
    # both sides are longdouble sums of at most a few hundred terms of modulus <= A_t; p itself is a rounded double (u relative)
    tol1, tol2 = 4 * X.U * est.A1 + 1e-18, 4 * X.U * est.A2 + 1e-18
    assert bool((np.abs(est.rdm1 - f1).astype(np.float64) <= tol1).all()), float(np.abs(est.rdm1 - f1).max())
    assert bool((np.abs(est.rdm2 - f2).astype(np.float64) <= tol2).all()), float(np.abs(est.rdm2 - f2).max())
    # slots nothing contributes to are zero on both sides, and there are slots of every kind that are not
    assert bool((f1[est.A1 == 0] == 0).all()) and bool((np.abs(f2[est.A2 == 0]) <= 1e-18).all())
    assert int((est.m1 > 0).sum()) == 8 + 2 * 4 * 3 and int((est.m2 > 0).sum()) > 100


@pytest.mark.parametrize("which", ["golden", "synthetic"])
def test_identity_E_against_the_hamiltonian_matrix(full_space, which):
    d, occ, psi, p, est = full_space
    sorb, nele = 8, 4
    h1, h2 = (d["h1e"], d["h2e"]) if which == "golden" else synth_integrals(sorb, seed=77)
    onv = O.pm01_to_onv(d["occ"], sorb)
    Hm = O.hij(onv, onv, h1, h2, sorb, nele).astype(LD)
    v = psi.astype(LD)
    want = (v @ (Hm @ v)) / (v @ v)
    got = (h1.astype(LD) * est.rdm1).sum() + (h2.astype(LD) * est.rdm2).sum()
    scale = float((np.abs(h1) * est.A1).sum() + (np.abs(h2) * est.A2).sum())
    assert abs(float(got - want)) <= 8 * X.U * scale, (float(got), float(want))
    assert abs(float(want)) > 1e-3


def test_traces(full_space):
    d, occ, psi, p, est = full_space
    sorb, nele = 8, 4
    diag1 = est.rdm1[[q * sorb + q for q in range(sorb)]].sum()
    pair = sorb * (sorb - 1) // 2
    diag2 = est.rdm2[[X.tri(t, t) for t in range(pair)]].sum()
    assert abs(float(diag1 - nele * LD(est.sum_w))) <= 64 * X.U
    assert abs(float(diag2 - nele * (nele - 1) // 2 * LD(est.sum_w))) <= 64 * X.U


def test_rbm_amplitudes_and_the_callback_agree():
    """the two ways estimator() takes its amplitudes give the same numbers, and ratio_rows is what it uses"""
    d = golden("c1_sorb8_all36.npz")
    occ = d["occ"].astype(np.int8)[:5]
    rbm = R.regime_params("small", "real", 8, 3, 5)
    w = np.full(5, 0.2)
    a = X.estimator(occ, w, rbm=rbm)
    amp = lambda rows: R.exact_ld(rbm, rows.astype(np.float64) * 2 - 1).psi()  # noqa: E731
    b = X.estimator(occ, w, amplitude=amp)
    assert float(np.abs(a.flat() - b.flat()).max()) <= 1e-17
    assert np.array_equal(a.m2, b.m2) and float(np.abs(a.A2 - b.A2).max()) <= 1e-15
    assert a.kappa_fused > 0 and bool((a.bound("fused") >= a.bound("ratio")).all())
