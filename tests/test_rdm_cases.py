"""tests/rdm_cases.py checked on the CPU: the grouped yardstick against rdm_exact.estimator on the same walkers, and the Python mirror of
the fused kernel's layout against the library's host-only entry points (workspace sizes, `_supported` on both sides of every edge)."""
import numpy as np
import pytest

import jrbm_exact as J
import jrdm_exact as JX
import rbm_exact as R
import rdm_cases as C
import rdm_exact as X
from conftest import golden, rand_occ

U_LD = R.U_LD


def _pool(sorb, noA, noB):
    if sorb == 8:
        return golden("c1_sorb8_all36.npz")["occ"].astype(np.int8)[:10]
    return rand_occ(10, sorb, noA, noB, seed=5).astype(np.int8)


def _same(a: X.Estimate, b: X.Estimate, n: int):
    A = np.concatenate([a.A1, a.A2])
    # both are longdouble sums of the same products in another order: n walkers, a few ulps of longdouble each
    assert bool((np.abs(a.flat() - b.flat()).astype(np.float64) <= 4 * n * U_LD * A).all()), float(np.abs(a.flat() - b.flat()).max())
    Ab = np.concatenate([b.A1, b.A2])
    assert bool((np.abs(A - Ab) <= 4 * n * X.U * A).all())
    assert bool(((A == 0) == (Ab == 0)).all())
    assert np.array_equal(a.m1, b.m1) and np.array_equal(a.m2, b.m2)
    assert np.array_equal(a.k1, b.k1) and np.array_equal(a.k2, b.k2)
    assert abs(a.sum_w - b.sum_w) <= 4 * n * X.U and (a.kappa_fused == b.kappa_fused or (np.isnan(a.kappa_fused) and np.isnan(b.kappa_fused)))


@pytest.mark.parametrize("shape", [(8, 2, 2), (12, 3, 2)], ids=["8-2-2", "12-3-2"])
def test_grouped_estimator_equals_the_plain_one(shape):
    sorb, noA, noB = shape
    pool = _pool(*shape)
    pick, w = C.draw(60, 10, seed=[sorb, 60])
    assert np.array_equal(np.unique(pick), np.arange(10)) and int(np.bincount(pick).max()) > 1
    w[::7] *= -1.0  # A_t sums |w|, the value w
    rbm = R.regime_params("alt30", "real", sorb, 8, 7)
    plain = X.estimator(pool[pick], w, rbm=rbm)
    group = C.grouped(pool, pick, w, rbm=rbm)
    _same(group, plain, 60)
    assert int(plain.m2.max()) > 10 and int(group.m2.max()) == int(plain.m2.max())  # m_t counts walkers, not pool entries
    # the Jastrow variant, through amplitude=, as jrdm_exact.estimate does
    M = J.jastrow_params("j-asym", sorb, seed=3)
    pj, kj = JX.estimate(rbm, M, pool[pick], w)
    gj, kg = C.grouped_jastrow(rbm, M, pool, pick, w)
    _same(gj, pj, 60)
    assert kj == kg and gj.kappa_fused == pj.kappa_fused > plain.kappa_fused
    assert float(np.abs(gj.flat() - group.flat()).max()) > 1e-6  # and it is another state


def test_grouped_estimator_ignores_pool_entries_nobody_picked():
    pool = _pool(8, 2, 2)
    pick = np.array([0, 3, 3, 0, 3])
    w = np.array([0.1, 0.2, 0.3, 0.25, 0.15])
    rbm = R.regime_params("small", "real", 8, 3, 7)
    _same(C.grouped(pool, pick, w, rbm=rbm), X.estimator(pool[pick], w, rbm=rbm), 5)


# ---- the layout mirror ----------------------------------------------------------------------------------------------------------------
NS = (0, 1, 255, 256, 257, 300, 1029, 1800, 5700, 8453, 70000)


def _lib():
    from pynqs_amd import _native as N

    return N.lib()


@pytest.mark.parametrize("sorb", [2, 4, 8, 12, 40, 64, 66, 80, 90, 92, 130, 192])
def test_workspace_sizes_equal_the_mirror(sorb):
    lib = _lib()
    for n in NS:
        for H in (1, 8, 17, 80, 512):
            assert lib.pynqs_rdm_rbm_workspace(n, sorb, H) == C.workspace_bytes(n, sorb, H), (n, sorb, H)
            assert lib.pynqs_rdm_jrbm_workspace(n, sorb, H) == C.workspace_bytes(n, sorb, H, jastrow=True), (n, sorb, H)


def test_workspace_refusals_equal_the_mirror():
    lib = _lib()
    for n, sorb, H in [(-1, 8, 8), (10, 7, 8), (10, 0, 8), (10, 194, 8), (10, 8, 0), (10, 8, 8193), (10, 8, 8192)]:
        assert lib.pynqs_rdm_rbm_workspace(n, sorb, H) == C.workspace_bytes(n, sorb, H), (n, sorb, H)
        assert lib.pynqs_rdm_jrbm_workspace(n, sorb, H) == C.workspace_bytes(n, sorb, H, jastrow=True), (n, sorb, H)
    assert C.workspace_bytes(10, 7, 8) == -1 and C.workspace_bytes(10, 8, 8192) > 0


def test_supported_equals_the_mirror_on_both_sides_of_every_edge():
    lib = _lib()

    def both(sorb, nele, noA, noB, H):
        r, j = lib.pynqs_rdm_rbm_supported(sorb, nele, noA, noB, H), lib.pynqs_rdm_jrbm_supported(sorb, nele, noA, noB, H)
        assert r == int(C.supported(sorb, nele, noA, noB, H)), ("rbm", sorb, nele, noA, noB, H)
        assert j == int(C.supported(sorb, nele, noA, noB, H, jastrow=True)), ("jrbm", sorb, nele, noA, noB, H)
        return r, j

    # K K <= 2048: sorb 90 is served, sorb 92 is not
    assert both(90, 4, 2, 2, 8) == (1, 1) and both(92, 4, 2, 2, 8) == (0, 0)
    assert both(88, 4, 2, 2, 8) == (1, 1) and both(192, 4, 2, 2, 8) == (0, 0) and both(194, 4, 2, 2, 8) == (0, 0)
    # odd sorb, sorb below 2
    assert both(9, 4, 2, 2, 8) == (0, 0) and both(65, 4, 2, 2, 8) == (0, 0) and both(0, 0, 0, 0, 8) == (0, 0) and both(2, 2, 1, 1, 8) == (1, 1)
    # H 512 against 513, H 0
    assert both(8, 4, 2, 2, 512) == (1, 1) and both(8, 4, 2, 2, 513) == (0, 0) and both(8, 4, 2, 2, 0) == (0, 0) and both(8, 4, 2, 2, 1) == (1, 1)
    # the 64 KiB of LDS: the largest H of either flavour and the next one
    for sorb in (40, 66, 80, 90):
        for jas in (False, True):
            Hm = C.max_hidden(sorb, jas)
            assert 0 < Hm
            r, j = both(sorb, 4, 2, 2, Hm)
            assert (j if jas else r) == 1
            if Hm < C.MAX_HIDDEN:
                r, j = both(sorb, 4, 2, 2, Hm + 1)
                assert (j if jas else r) == 0
                assert C.lds_bytes(sorb, Hm, True, jas) <= C.MAX_LDS < C.lds_bytes(sorb, Hm + 1, True, jas)
        # every H between the two flavours' limits: the real flavour alone
        for H in range(C.max_hidden(sorb, True) + 1, C.max_hidden(sorb, False) + 1):
            assert both(sorb, 4, 2, 2, H) == (1, 0)
    assert C.max_hidden(90) == 40 and C.lds_bytes(90, 40, True) == 65024 and C.max_hidden(90, True) < 40
    # electron counts
    assert both(8, 5, 2, 2, 8) == (0, 0) and both(8, 3, 2, 2, 8) == (0, 0) and both(8, 4, 2, 2, 8) == (1, 1)
    assert both(8, 5, 5, 0, 8) == (0, 0) and both(8, 4, 4, 0, 8) == (1, 1) and both(8, 5, 0, 5, 8) == (0, 0) and both(8, 8, 4, 4, 8) == (1, 1)
    assert both(8, 1, -1, 2, 8) == (0, 0) and both(8, 0, 0, 0, 8) == (1, 1)
    assert both(40, 30, 15, 15, 80) == (1, 1)
    # and a grid
    for sorb in (8, 40, 66, 90):
        for H in (1, 7, 8, 9, 16, 17, 40, 41, 48, 49, 80, 256, 257, 512):
            both(sorb, 4, 2, 2, H)


def test_the_regimes_of_the_gpu_cases():
    """(slices, chunks per slice) of the pair kernel and of the singles and diagonal kernels"""
    assert C.layout(300, 8, 8).regime() == ((2, 1), (2, 1))
    assert C.layout(1029, 12, 17).regime() == ((5, 1), (5, 1))
    assert C.layout(1800, 40, 17).regime() == ((4, 2), (8, 1))
    assert C.layout(8453, 66, 8).regime() == ((2, 17), (17, 2))
    assert C.layout(5700, 90, 8).regime() == ((2, 12), (12, 2))  # the 16 M doubles of a slice's tables bind
    L = C.layout(300, 8, 8)
    assert L.last_slice(False) == 44 and L.last_slice(True) == 44
    assert C.layout(1029, 12, 17).last_slice(True) == 5 and C.layout(8453, 66, 8).last_chunk() == 5
    # the regime does not depend on H, and few walkers are one slice of one chunk
    assert C.layout(1800, 40, 80).regime() == C.layout(1800, 40, 17).regime() and C.layout(36, 8, 512).regime() == ((1, 1), (1, 1))


def test_wave_counts_and_ballot_regimes():
    q = np.zeros(600, dtype=bool)
    q[[0, 70, 130, 200, 255, 256 + 64, 599]] = True
    c = C.wave_counts(q)
    assert c.tolist() == [[1, 1, 1, 2], [0, 1, 0, 0], [0, 1, 0, 0]]
    occ = np.zeros((300, 4), dtype=np.int8)
    occ[:, 0] = 1
    occ[100:, 1] = 1
    r = C.ballot_regimes(occ, 4, 1, 1)
    assert r == {"all_waves": True, "gap_then_hit": True, "empty_chunk": False}
    assert C.owner_qualifies(occ, (0, 1), False).sum() == 200 and C.owner_qualifies(occ, (2,), True).all()
    assert C.owner_empty(8, 3, 2) and not C.owner_empty(8, 2, 2) and len(C.pair_owners(8)) == 28
