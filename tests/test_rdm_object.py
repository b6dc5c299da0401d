"""pynqs_amd.rdm.RDM on the CPU: energy(), dense(), spin_free(), natural_occupations() and spin_density() on the exact matrices of a
random state over all 36 determinants of sorb 8 (tests/rdm_exact.py), with spin-orbital integrals built from random spatial ones."""
import numpy as np
import pytest
import torch

import rdm_exact as X
from conftest import golden
from pynqs_amd import C_extension as cx
from pynqs_amd.rdm import RDM


@pytest.fixture(scope="module")
def state():
    d = golden("c1_sorb8_all36.npz")
    occ = d["occ"].astype(np.int8)
    psi = np.random.default_rng(3).standard_normal(36)
    key = {tuple(int(b) for b in o): c for o, c in zip(occ, psi)}
    amp = lambda rows: np.array([key[tuple(int(b) for b in r)] for r in rows], dtype=np.clongdouble)  # noqa: E731
    est = X.estimator(occ, psi ** 2 / (psi ** 2).sum(), amplitude=amp)
    return RDM(torch.from_numpy(est.rdm1.astype(np.float64)), torch.from_numpy(est.rdm2.astype(np.float64)), 8, 4, 2, 2)


def _spatial_integrals(K, seed):
    g = np.random.default_rng(seed)
    h = g.standard_normal((K, K)); h = h + h.T
    e = g.standard_normal((K,) * 4)
    e = e + e.transpose(1, 0, 2, 3); e = e + e.transpose(0, 1, 3, 2); e = e + e.transpose(2, 3, 0, 1)  # (pq|rs), 8-fold
    return h, e


def test_spin_free_energy_equals_the_packed_energy(state):
    K, s = 4, 8
    h, e = _spatial_integrals(K, 9)
    hso = np.zeros((s, s)); V = np.zeros((s,) * 4)
    for a in (0, 1):
        hso[a::2, a::2] = h
        for b in (0, 1):
            V[a::2, b::2, a::2, b::2] = e.transpose(0, 2, 1, 3)  # <ij|kl> = (ik|jl), spins of i, k and of j, l equal
    V = V - V.transpose(0, 1, 3, 2)
    h1, h2 = cx.compress_h1e_h2e(hso, V, s)
    want = float(state.energy(torch.from_numpy(h1), torch.from_numpy(h2)))
    g1, g2 = state.dense()
    assert abs((hso * g1).sum() + 0.25 * (V * g2).sum() - want) <= 1e-11 * (1 + abs(want))
    assert float(np.abs(g2 + g2.transpose(1, 0, 2, 3)).max()) <= 1e-15 and float(np.abs(g2 - g2.transpose(2, 3, 0, 1)).max()) <= 1e-15
    D, d = state.spin_free()
    assert abs((h * D).sum() + 0.5 * (e * d).sum() - want) <= 1e-11 * (1 + abs(want))
    assert abs(np.einsum("ppqq", d) - 4 * 3) <= 1e-12  # N (N - 1)


def test_occupations_and_spin_density(state):
    occ = state.natural_occupations()
    assert occ.shape == (4,) and bool((np.diff(occ) <= 0).all()) and bool((occ >= -1e-12).all()) and bool((occ <= 2 + 1e-12).all())
    assert abs(occ.sum() - 4) <= 1e-12
    assert abs(state.spin_density().sum()) <= 1e-12  # 2 alpha, 2 beta


def test_refusals():
    z = torch.zeros
    with pytest.raises(ValueError):
        RDM(z(63, dtype=torch.float64), z(406, dtype=torch.float64), 8, 4, 2, 2)
    with pytest.raises(ValueError):
        RDM(z(64, dtype=torch.float32), z(406, dtype=torch.float64), 8, 4, 2, 2)
    r = RDM(z(64, dtype=torch.float64), z(406, dtype=torch.float64), 8, 4, 2, 2)
    with pytest.raises(ValueError):
        r.energy(z(64, dtype=torch.float64), z(405, dtype=torch.float64))
