"""pynqs_rdm_rbm, pynqs_rdm_jrbm and pynqs_rdm_scatter at the sizes their control flow depends on, against the longdouble yardsticks
tests/rdm_exact.py / tests/jrdm_exact.py with their a-priori slot bounds, unchanged: (m_t + 2 + kappa) u A_t, slots without any
contribution exactly zero.

Many walkers (M1 .. M4; the grouped yardstick of tests/rdm_cases.py: walkers drawn from a small pool): walkers in all four waves of a
chunk, several chunks per slice, several slices, short last slices and chunks, two words.  Every case asserts through the layout
mirror of tests/rdm_cases.py that it has the regime it is named for.  The walkers are the first n rows of a buffer that goes on for 256
valid determinants with weights of 1.0: a read past n stays inside the allocation and moves the result far beyond any bound.
New sizes, few walkers (W1 .. W5; the plain estimator): two hidden units per thread (H > 256), threads that stage a hidden unit and an
e_o (Jastrow, H + sorb > 256), the flagship shape (40, 15, 15) at H = 80, sorb 90 (lane items 5 to 7, the partly filled last item
row, the largest H within 64 KiB of LDS), electron counts at the edges.
Skipped walkers: rows with other electron counts or bits at and above sorb, through the C ABI (the Python wrapper refuses them).

The yardstick of a case is computed once and shared by the tests of that case.  Measured worst error / bound per case:
profiles/rdm_shapes.txt."""
import functools

import numpy as np
import pytest
import torch

import jrbm_exact as J
import jrdm_exact as JX
import rbm_exact as R
import rdm_cases as C
import rdm_exact as X
from conftest import golden, rand_occ, synth_integrals

pytestmark = pytest.mark.gpu

GUARD = 256  # rows behind the walkers: valid determinants, weight 1.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _onv(words):
    return _dev(words.view(np.uint8).reshape(words.shape[0], -1))


def _module(rbm, M=None):
    from pynqs_amd.rbm import JastrowRBM, RealRBM

    if M is None:
        return RealRBM(_dev(rbm.W), _dev(rbm.hb), _dev(rbm.vb)).cuda()
    return JastrowRBM(_dev(rbm.W), _dev(rbm.hb), _dev(rbm.vb), _dev(M)).cuda()


def _flat(rdm):
    return np.concatenate([rdm.rdm1.cpu().numpy(), rdm.rdm2.cpu().numpy()])


def _within(what, got, est, bound):
    want = est.flat()
    A = np.concatenate([est.A1, est.A2])
    assert got.shape == want.shape and bool(np.isfinite(got).all()), what
    err = np.abs(got.astype(R.LD) - want).astype(np.float64)
    live = A > 0
    assert bool((got[~live] == 0).all()), f"{what}: a slot without contributions is not exactly zero"
    ratio = err[live] / bound[live]
    k = int(np.argmax(ratio))
    print(f"{what}: worst error / bound {ratio[k]:.3g} over {int(live.sum())} live slots of {live.size}; max c_t {float((bound[live] / (X.U * A[live])).max()):.4g}; "
          f"max A_t {float(A.max()):.3g}")
    assert bool((err[live] <= bound[live]).all()), f"{what}: error / bound {ratio[k]:.3g} at live slot {k}"


def _native(flavour, onv, n, shape, wd, rbm, M=None):
    """pynqs_rdm_rbm / pynqs_rdm_jrbm ("real" / "jastrow") through the C ABI on the first n rows of onv and wd, workspace and results
    pre-filled with NaN: (rdm1 | rdm2) flat"""
    from pynqs_amd import C_extension as cx
    from pynqs_amd import _native as N

    sorb, noA, noB = shape
    H = rbm.H
    table = cx.RBMTable(_dev(rbm.W), _dev(rbm.hb), _dev(rbm.vb))
    n1, n2 = X.sizes(sorb)
    st = torch.cuda.current_stream().cuda_stream
    jas = flavour == "jastrow"
    size = (N.lib().pynqs_rdm_jrbm_workspace if jas else N.lib().pynqs_rdm_rbm_workspace)(n, sorb, H)
    assert size == C.workspace_bytes(n, sorb, H, jas)
    work = torch.full((max(size // 8, 1),), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((n1 + n2,), float("nan"), dtype=torch.float64, device="cuda")
    tail = (H, work.data_ptr(), out.data_ptr(), out[n1:].data_ptr(), st)
    if jas:
        jtable = cx.JastrowTable(_dev(M))
        N.check(N.lib().pynqs_rdm_jrbm(onv.data_ptr(), n, sorb, noA + noB, noA, noB, wd.data_ptr(), table.data_ptr(), jtable.data_ptr(), *tail), "jrbm")
    else:
        N.check(N.lib().pynqs_rdm_rbm(onv.data_ptr(), n, sorb, noA + noB, noA, noB, wd.data_ptr(), table.data_ptr(), *tail), "rbm")
    return out.cpu().numpy()


def _ratio_rows(words, shape, rbm):
    """correctly rounded psi(x'_k) / psi(x) of the real RBM for the rows `words`, in the package's own column order: float64 [rows, ncomb]"""
    from pynqs_amd import C_extension as cx

    sorb, noA, noB = shape
    comb, _ = cx.get_comb_tensor(_onv(words), sorb, noA + noB, noA, noB)
    bits = np.unpackbits(comb.cpu().numpy(), axis=2, bitorder="little")[:, :, :sorb]
    return X.ratio_rows(bits, rbm)


def _scatter(onv, wd, ratio, shape, size):
    from pynqs_amd import rdm as M_

    sorb, noA, noB = shape
    out = torch.zeros(size, dtype=torch.float64, device="cuda")
    M_.scatter(onv, wd, ratio, sorb, noA + noB, noA, noB, out)
    return out.cpu().numpy()


def _bound(est, flavour, path):
    return JX.bound(est, path) if flavour == "jastrow" else est.bound(path)


def _forced(occ, orbitals, settings):
    """walker i gets settings[i % len(settings)] (occupied / empty) on the given orbitals; the electrons come from and go to orbitals
    of the same spin outside them, so that the electron counts stay"""
    sorb = occ.shape[1]
    for i in range(occ.shape[0]):
        others = lambda o, v: [p for p in range(o & 1, sorb, 2) if p not in orbitals and occ[i, p] == v]  # noqa: E731
        for o in orbitals:
            if occ[i, o]:
                free = others(o, 0)
                occ[i, free[i % len(free)]], occ[i, o] = 1, 0
        for o, v in zip(orbitals, settings[i % len(settings)]):
            if v:
                full = others(o, 1)
                occ[i, full[i % len(full)]], occ[i, o] = 0, 1
    return occ


# ---- many walkers ---------------------------------------------------------------------------------------------------------------------
# shape, walkers, H, RBM regime, Jastrow regime, pool (0: all 36 determinants of the golden file), (slices, chunks per slice) of the pair
# kernel and of the singles and diagonal kernels
MANY = {
    "M1": ((8, 2, 2), 300, 8, "small", "j-asym", 0, ((2, 1), (2, 1))),
    "M2": ((12, 3, 2), 1029, 17, "alt30", "j-strong", 40, ((5, 1), (5, 1))),
    "M3": ((40, 15, 15), 1800, 17, "fe2s2", "j-small", 6, ((4, 2), (8, 1))),
    "M4": ((66, 2, 1), 8453, 8, "small", "j-asym", 48, ((2, 17), (17, 2))),
}


def _pool(name):
    shape, n, H, regime, jregime, npool, _ = MANY[name]
    sorb, noA, noB = shape
    if npool == 0:
        return golden("c1_sorb8_all36.npz")["occ"].astype(np.uint8)
    pool = rand_occ(npool, sorb, noA, noB, seed=sorb + npool)
    if name == "M4":
        # every setting of orbitals 63 (beta), 64 (alpha), 65 (beta) that one beta electron allows: six of them, eight entries each
        allowed = [(b63, a64, b65) for b63 in (0, 1) for a64 in (0, 1) for b65 in (0, 1) if b63 + b65 <= 1]
        pool = _forced(pool, (63, 64, 65), allowed)
        assert {tuple(r) for r in pool[:, 63:66]} == set(allowed)
    assert (pool[:, 0::2].sum(1) == noA).all() and (pool[:, 1::2].sum(1) == noB).all()
    return pool


@functools.lru_cache(maxsize=None)
def _many(name):
    """(pool, pick, w, rbm, M, walker words with the guard rows behind them, weights with the guard weights behind them)"""
    shape, n, H, regime, jregime, npool, _ = MANY[name]
    sorb = shape[0]
    pool = _pool(name)
    pick, w = C.draw(n, pool.shape[0], seed=[sorb, n])
    rbm = R.regime_params(regime, "real", sorb, H, 7)
    M = J.jastrow_params(jregime, sorb, seed=H)
    pw = R.pack_bits(pool.astype(bool))
    words = np.concatenate([pw[pick], pw[np.arange(GUARD) % pool.shape[0]]])
    return pool, pick, w, rbm, M, words, np.concatenate([w, np.ones(GUARD)])


@functools.lru_cache(maxsize=None)
def _many_est(name, flavour):
    pool, pick, w, rbm, M, _, _ = _many(name)
    if flavour == "jastrow":
        return C.grouped_jastrow(rbm, M, pool.astype(np.int8), pick, w)
    return C.grouped(pool.astype(np.int8), pick, w, rbm=rbm), float("nan")


@pytest.mark.parametrize("name", list(MANY))
def test_many_walker_cases_have_the_regime_they_are_named_for(name):
    from pynqs_amd import _native as N

    shape, n, H, _, _, _, regime = MANY[name]
    sorb, noA, noB = shape
    pool, pick, w, rbm, M, words, wbuf = _many(name)
    L = C.layout(n, sorb, H)
    assert L.regime() == regime, L.regime()
    assert N.lib().pynqs_rdm_rbm_workspace(n, sorb, H) == C.workspace_bytes(n, sorb, H)
    assert N.lib().pynqs_rdm_jrbm_workspace(n, sorb, H) == C.workspace_bytes(n, sorb, H, jastrow=True)
    assert N.lib().pynqs_rdm_rbm_supported(sorb, noA + noB, noA, noB, H) == 1 == N.lib().pynqs_rdm_jrbm_supported(sorb, noA + noB, noA, noB, H)
    assert words.shape[0] == n + GUARD and wbuf.shape[0] == n + GUARD and np.array_equal(np.unique(pick), np.arange(pool.shape[0]))
    seen = C.ballot_regimes(pool[pick], sorb, noA, noB)
    if name == "M1":
        assert seen["all_waves"] and L.last_slice(False) == 44 and L.last_slice(True) == 44 and not C.owner_empty(sorb, noA, noB)
    elif name == "M2":
        assert seen["all_waves"] and seen["gap_then_hit"] and L.last_slice(False) == 5 and L.last_slice(True) == 5
    elif name == "M3":
        assert C.owner_empty(sorb, noA, noB) and seen["all_waves"] and L.last_chunk() == 8  # (the slices are whole: 1800 = 7 x 256 + 8)
    else:
        assert seen["all_waves"] and seen["gap_then_hit"] and seen["empty_chunk"] and L.last_chunk() == 5 and words.shape[1] == 2
    # every chunk mixes pool entries
    chunks = [pick[b:b + C.KBLOCK] for b in range(0, n, C.KBLOCK)]
    assert all(np.unique(c).size > 1 for c in chunks[:-1])


@pytest.mark.parametrize("flavour", ["real", "jastrow"])
@pytest.mark.parametrize("name", list(MANY))
def test_many_walkers_fused(name, flavour):
    """the fused route through the module, and again through the C ABI on a workspace full of NaN: the same bits"""
    from pynqs_amd.rdm import reduced_density_matrices

    shape, n = MANY[name][:2]
    sorb, noA, noB = shape
    pool, pick, w, rbm, M, words, wbuf = _many(name)
    est, _ = _many_est(name, flavour)
    onv, wd = _onv(words), _dev(wbuf)
    m = _module(rbm, M if flavour == "jastrow" else None)
    a = reduced_density_matrices(onv[:n], wd[:n], m, sorb, noA + noB, noA, noB, fused=True)
    assert a.fused
    got = _flat(a)
    _within(f"{name} fused {flavour} {shape} n = {n}", got, est, _bound(est, flavour, "fused"))
    again = _native(flavour, onv, n, shape, wd, rbm, M)
    assert np.array_equal(got, again), "two fused calls differ in their bits"


@pytest.mark.parametrize("name", ["M1", "M2"])
def test_many_walkers_scatter_on_exact_ratios(name):
    shape, n = MANY[name][:2]
    pool, pick, w, rbm, M, words, wbuf = _many(name)
    est, _ = _many_est(name, "real")
    pw = R.pack_bits(pool.astype(bool))
    rows = _ratio_rows(pw, shape, rbm)
    ratio = np.concatenate([rows[pick], np.ones((GUARD, rows.shape[1]))])
    got = _scatter(_onv(words)[:n], _dev(wbuf)[:n], _dev(ratio)[:n], shape, est.flat().size)
    _within(f"{name} scatter {shape} n = {n}", got, est, est.bound("ratio"))


def test_many_walkers_generic_route():
    """fused=False: get_comb_tensor, the module's forward, psi(x') / psi(x), the scatter kernel, in chunks of 97 walkers (the last of 9)"""
    from pynqs_amd.rdm import reduced_density_matrices

    shape, n = MANY["M1"][:2]
    sorb, noA, noB = shape
    pool, pick, w, rbm, M, words, wbuf = _many("M1")
    est, _ = _many_est("M1", "real")
    a = reduced_density_matrices(_onv(words)[:n], _dev(wbuf)[:n], _module(rbm), sorb, noA + noB, noA, noB, fused=False, nbatch=97)
    assert not a.fused
    _within(f"M1 module {shape} n = {n}", _flat(a), est, est.bound("module"))


# ---- new sizes, few walkers -----------------------------------------------------------------------------------------------------------
def _few_inputs(case):
    """(rbm, M, occ, words, w) of (sorb, noA, noB, walkers (0: all 36 of the golden file), H, RBM regime, Jastrow regime, forced orbitals)"""
    sorb, noA, noB, n, H, regime, jregime, forced = case
    occ = golden("c1_sorb8_all36.npz")["occ"].astype(np.uint8) if n == 0 else rand_occ(n, sorb, noA, noB, seed=sorb + n)
    if forced:
        occ = _forced(occ, forced, [tuple((i >> k) & 1 for k in range(len(forced))) for i in range(1 << len(forced))])
    assert (occ[:, 0::2].sum(1) == noA).all() and (occ[:, 1::2].sum(1) == noB).all()
    rbm = R.regime_params(regime, "real", sorb, H, 7)
    M = J.jastrow_params(jregime, sorb, seed=H)
    g = np.random.default_rng([sorb, H, len(regime)])
    w = g.random(occ.shape[0]) + 0.1
    return rbm, M, occ, R.pack_bits(occ.astype(bool)), w / w.sum()


def _few_est(case, flavour):
    rbm, M, occ, words, w = _few_inputs(case)
    if flavour == "jastrow":
        # jrdm_exact.estimate, also for walkers without any excitation
        est = X.estimator(occ.astype(np.int8), w, amplitude=JX.amplitude(rbm, M))
        est.kappa_fused = X.kappa_fused(rbm, case[0]) + JX.kappa_jastrow(M)
        return est
    return X.estimator(occ.astype(np.int8), w, rbm=rbm)


_few_est_shared = functools.lru_cache(maxsize=None)(_few_est)


def _fused_few(case, flavour, est, traces=True):
    """the fused route through the module within the bound, the same bits through the C ABI, the traces"""
    from pynqs_amd.rdm import reduced_density_matrices

    sorb, noA, noB = case[:3]
    rbm, M, occ, words, w = _few_inputs(case)
    assert rbm.H == case[4]
    onv, wd = _onv(words), _dev(w)
    a = reduced_density_matrices(onv, wd, _module(rbm, M if flavour == "jastrow" else None), sorb, noA + noB, noA, noB, fused=True)
    assert a.fused
    got = _flat(a)
    _within(f"fused {flavour} {case}", got, est, _bound(est, flavour, "fused"))
    assert np.array_equal(got, _native(flavour, onv, onv.size(0), case[:3], wd, rbm, M)), "two fused calls differ in their bits"
    if traces:
        nele = noA + noB
        pair = sorb * (sorb - 1) // 2
        d2 = got[sorb * sorb:][[X.tri(t, t) for t in range(pair)]]
        assert abs(got[:sorb * sorb].reshape(sorb, sorb).trace() - nele * est.sum_w) <= 64 * max(nele, 1) * X.U
        assert abs(d2.sum() - nele * (nele - 1) / 2 * est.sum_w) <= 64 * max(nele * nele, 1) * X.U
    return got


def _scatter_few(case, est):
    rbm, M, occ, words, w = _few_inputs(case)
    got = _scatter(_onv(words), _dev(w), _dev(_ratio_rows(words, case[:3], rbm)), case[:3], est.flat().size)
    _within(f"scatter {case}", got, est, est.bound("ratio"))
    return got


# W1: two hidden units per thread
W1 = [(8, 2, 2, 0, H, regime, "j-asym", ()) for H in (257, 300, 512) for regime in ("small", "alt30")]


@pytest.mark.parametrize("case", W1, ids=[f"{c[4]}-{c[5]}" for c in W1])
def test_w1_more_than_256_hidden_units(case):
    assert case[4] > C.KBLOCK and C.supported(8, 4, 2, 2, case[4])
    _fused_few(case, "real", _few_est_shared(case, "real"))
    if case[4] == 300:
        _fused_few(case, "jastrow", _few_est_shared(case, "jastrow"))


# W2: H + sorb > 256, threads that stage a hidden unit and an e_o
W2 = [((12, 3, 2, 24, 250, "small", "j-strong", ()), "jastrow"), ((12, 3, 2, 24, 256, "alt30", "j-asym", ()), "jastrow"),
      ((12, 3, 2, 24, 256, "alt30", "j-asym", ()), "real")]


@pytest.mark.parametrize("case,flavour", W2, ids=[f"{c[4]}-{f}" for c, f in W2])
def test_w2_hidden_units_and_orbitals_staged_by_the_same_threads(case, flavour):
    assert case[4] + case[0] > C.KBLOCK >= case[4]
    _fused_few(case, flavour, _few_est_shared(case, flavour))


# W3: the flagship shape
W3 = (40, 15, 15, 6, 80, "fe2s2", "j-small", ())


@pytest.mark.parametrize("flavour", ["real", "jastrow"])
def test_w3_flagship_shape_fused(flavour):
    assert C.owner_empty(40, 15, 15)
    _fused_few(W3, flavour, _few_est_shared(W3, flavour))


def test_w3_flagship_shape_scatter():
    _scatter_few(W3, _few_est_shared(W3, "real"))


@pytest.mark.parametrize("flavour", ["real", "jastrow"])
def test_w3_identity_E_against_total_energy(flavour):
    """dot(h1e, rdm1) + dot(h2e, rdm2) = sum_x w_x E_loc(x) within the slot bounds weighted by the integrals' moduli"""
    from pynqs_amd import energy
    from pynqs_amd.rdm import reduced_density_matrices

    sorb, noA, noB = W3[:3]
    rbm, M, occ, words, w = _few_inputs(W3)
    est = _few_est_shared(W3, flavour)
    m, onv, wd = _module(rbm, M if flavour == "jastrow" else None), _onv(words), _dev(w)
    rdm = reduced_density_matrices(onv, wd, m, sorb, noA + noB, noA, noB)
    assert rdm.fused
    bound = _bound(est, flavour, "fused")
    for seed in (1234, 5):
        h1, h2 = synth_integrals(sorb, seed)
        eloc, _, _ = energy.total_energy(onv, -1, -1, _dev(h1), _dev(h2), m, sorb, noA + noB, noA, noB)
        want = float((wd * eloc.real).sum())
        got = float(rdm.energy(_dev(h1), _dev(h2)))
        allowed = float((np.abs(np.concatenate([h1, h2])) * bound).sum())
        print(f"W3 identity E {flavour}, integrals {seed}: {got:+.12f} against {want:+.12f}, |difference| / allowed {abs(got - want) / allowed:.3g}")
        assert abs(want) > 1e-3 and abs(got - want) <= allowed, (seed, got, want, allowed)


# W4: sorb 90, the last size the fused kernel serves; orbitals 63, 64 and 89 occupied / empty in every combination
W4 = [("real", 8, "small"), ("real", C.max_hidden(90), "fe2s2"), ("jastrow", C.max_hidden(90, True), "fe2s2")]


@pytest.mark.parametrize("flavour,H,regime", W4, ids=[f"{f}-{H}" for f, H, _ in W4])
def test_w4_sorb_90(flavour, H, regime):
    """items 5 to 7 (2025 of 2048 item slots exist) at H = 8; the largest H of either flavour launches with (nearly) all 64 KiB of LDS.
    The dense yardstick of 8 M slots takes about 0.5 GB: one per parameter set, not kept."""
    case = (90, 2, 2, 8, H, regime, "j-small", (63, 64, 89))
    assert 45 * 45 > 7 * C.KBLOCK and C.supported(90, 4, 2, 2, H, flavour == "jastrow") and not C.supported(90, 4, 2, 2, max(H, 40) + 1, flavour == "jastrow")
    if H > 8:
        assert not C.supported(90, 4, 2, 2, H + 1, flavour == "jastrow") and C.lds_bytes(90, H, True, flavour == "jastrow") > 56 * 1024
    occ = _few_inputs(case)[2]
    assert {tuple(r) for r in occ[:, [63, 64, 89]]} == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    _fused_few(case, flavour, _few_est(case, flavour))


def test_w4_sorb_92_is_refused():
    from pynqs_amd.rbm import RealRBM
    from pynqs_amd.rdm import reduced_density_matrices

    occ = rand_occ(8, 92, 2, 2, seed=92)
    onv, wd = _onv(R.pack_bits(occ.astype(bool))), _dev(np.full(8, 0.125))
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    m = RealRBM(z(8, 92), z(8), z(92)).cuda()
    assert not C.supported(92, 4, 2, 2, 8)
    with pytest.raises(ValueError):
        reduced_density_matrices(onv, wd, m, 92, 4, 2, 2, fused=True)
    assert not reduced_density_matrices(onv, wd, m, 92, 4, 2, 2).fused


# W5: electron counts at the edges
W5 = [(8, 3, 2, 20, 8, "small", "j-asym", ()),    # the first count past half filling: the particle side owns
      (10, 5, 2, 20, 8, "alt30", "j-asym", ()),   # a full alpha shell: alpha owners never qualify
      (8, 0, 2, 20, 8, "small", "j-strong", ()),  # no alpha electrons
      (8, 4, 4, 3, 8, "small", "j-asym", ())]     # nothing but the diagonal


@pytest.mark.parametrize("case", W5, ids=["-".join(map(str, c[:3])) for c in W5])
def test_w5_electron_count_edges(case):
    sorb, noA, noB = case[:3]
    est = _few_est_shared(case, "real")
    got = _fused_few(case, "real", est)
    _fused_few(case, "jastrow", _few_est_shared(case, "jastrow"))
    sc = _scatter_few(case, est)
    if (noA, noB) == (4, 4):
        diag = np.zeros(got.size, dtype=bool)
        diag[[p * sorb + p for p in range(sorb)]] = True
        diag[sorb * sorb + np.array([X.tri(t, t) for t in range(sorb * (sorb - 1) // 2)])] = True
        assert bool((got[~diag] == 0).all()) and bool((sc[~diag] == 0).all())
    else:
        assert C.owner_empty(sorb, noA, noB) == (case[:3] != (8, 0, 2)) and int((est.m1 > 0).sum()) > sorb


# ---- skipped walkers ------------------------------------------------------------------------------------------------------------------
SKIP_SHAPE, SKIP_N, SKIP_H = (12, 3, 2), 300, 8


@functools.lru_cache(maxsize=None)
def _skipped():
    """300 rows, every seventh not a walker of (12, 3, 2): one alpha electron too many, an alpha electron moved to beta, a valid
    determinant with a stray bit at orbital 12 or 63.  The valid walkers leave the last spatial orbital (10, 11) empty and every bad row
    occupies it, so that the slots of an electron in 10 or 11 are live through bad rows alone."""
    sorb, noA, noB = SKIP_SHAPE
    pool = np.zeros((30, sorb), dtype=np.uint8)
    pool[:, :10] = rand_occ(30, 10, noA, noB, seed=17)
    pick_all, w = C.draw(SKIP_N, 30, seed=[sorb, SKIP_N, 7])
    bad = np.arange(SKIP_N) % 7 == 3
    occ = pool[pick_all].copy()
    stray = np.zeros(SKIP_N, dtype=np.uint64)
    for k, i in enumerate(np.flatnonzero(bad)):
        a = int(np.flatnonzero(occ[i, 0:10:2])[k % noA]) * 2  # one of the row's alpha electrons
        if k % 4 == 0:
            occ[i, 10] = 1                 # (4, 2)
        elif k % 4 == 1:
            occ[i, a], occ[i, 11] = 0, 1   # (2, 3)
        else:
            occ[i, a], occ[i, 10] = 0, 1   # (3, 2), and a bit that is no orbital
            stray[i] = np.uint64(1) << np.uint64(12 if k % 4 == 2 else 63)
    words = R.pack_bits(occ.astype(bool))
    words[:, 0] |= stray
    assert int(bad.sum()) == 43 and bool((w[bad] > 0).all()) and not pool[:, 10:].any() and bool(occ[bad][:, 10:].any(1).all())
    rbm = R.regime_params("fe2s2", "real", sorb, SKIP_H, 7)
    M = J.jastrow_params("j-asym", sorb, seed=SKIP_H)
    return pool, pick_all, w, bad, words, rbm, M


@functools.lru_cache(maxsize=None)
def _skipped_est(flavour):
    pool, pick, w, bad, words, rbm, M = _skipped()
    if flavour == "jastrow":
        return C.grouped_jastrow(rbm, M, pool.astype(np.int8), pick[~bad], w[~bad])[0]
    return C.grouped(pool.astype(np.int8), pick[~bad], w[~bad], rbm=rbm)


def _dead_through_bad_rows(est):
    """slots that a bad row would feed and no valid walker does: an electron in orbital 10 or 11"""
    sorb = SKIP_SHAPE[0]
    dead = [est.A1[10 * sorb + 10], est.A1[11 * sorb + 11], est.A1[0 * sorb + 10]] + \
           [est.A2[X.tri(X.pair_index(10, q), X.pair_index(10, q))] for q in range(10)]
    assert all(a == 0 for a in dead) and est.A1[10 * sorb + 0] > 0  # (an excitation INTO orbital 10 is live)


@pytest.mark.parametrize("flavour", ["real", "jastrow"])
def test_walkers_of_other_electron_counts_are_skipped_by_the_fused_kernel(flavour):
    pool, pick, w, bad, words, rbm, M = _skipped()
    est = _skipped_est(flavour)
    _dead_through_bad_rows(est)
    assert C.layout(SKIP_N, 12, SKIP_H).regime() == ((2, 1), (2, 1))
    buf = np.concatenate([words, R.pack_bits(pool.astype(bool))[np.arange(GUARD) % 30]])
    got = _native(flavour, _onv(buf), SKIP_N, SKIP_SHAPE, _dev(np.concatenate([w, np.ones(GUARD)])), rbm, M)
    _within(f"skipped walkers, fused {flavour}", got, est, _bound(est, flavour, "fused"))


def test_walkers_of_other_electron_counts_are_skipped_by_the_scatter_kernel():
    pool, pick, w, bad, words, rbm, M = _skipped()
    est = _skipped_est("real")
    _dead_through_bad_rows(est)
    rows = _ratio_rows(R.pack_bits(pool.astype(bool)), SKIP_SHAPE, rbm)
    ratio = rows[pick].copy()
    ratio[bad] = 1.0
    got = _scatter(_onv(words), _dev(w), _dev(ratio), SKIP_SHAPE, est.flat().size)
    _within("skipped walkers, scatter", got, est, est.bound("ratio"))
