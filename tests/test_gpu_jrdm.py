"""pynqs_rdm_jrbm (the fused reduced-density-matrix kernel in its Jastrow flavour) and pynqs_amd.rdm for a JastrowRBM against the host
yardstick tests/jrdm_exact.py: every slot of rdm1 and rdm2 within that module's a-priori bound (its docstring derives the constants per
path), slots without any contribution exactly zero, the same bits on every call, the bits of pynqs_rdm_rbm at M = 0.  The yardstick of
a case is computed once (jrdm_exact.case) and shared by the tests of that case.

Measured worst error / bound per case of the fused route: see the README's test row."""
import os
import sys

import numpy as np
import pytest
import torch

import jrdm_exact as JX
import rbm_exact as R
import rdm_exact as X
from conftest import ROOT, synth_integrals

pytestmark = pytest.mark.gpu

CASES, IDS = JX.CASES, JX.IDS
SMALL = [c for c in CASES if c[0] in (8, 12)]  # the (8,2,2) and (12,3,2) cases


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _onv(words):
    return _dev(words.view(np.uint8).reshape(words.shape[0], -1))


def _module(rbm, M):
    from pynqs_amd.rbm import JastrowRBM

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


def _fused(case, M=None):
    from pynqs_amd.rdm import reduced_density_matrices

    sorb, noA, noB = case[:3]
    rbm, M0, occ, words, w, est, _ = JX.case(case)
    return reduced_density_matrices(_onv(words), _dev(w), _module(rbm, M0 if M is None else M), sorb, noA + noB, noA, noB, fused=True)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_route_meets_the_slot_bounds_and_is_reproducible(case):
    from pynqs_amd.rdm import reduced_density_matrices

    sorb, noA, noB = case[:3]
    rbm, M, occ, words, w, est, _ = JX.case(case)
    m = _module(rbm, M)
    a = reduced_density_matrices(_onv(words), _dev(w), m, sorb, noA + noB, noA, noB, fused=True)
    assert a.fused
    got = _flat(a)
    _within(f"fused {case}", got, est, JX.bound(est, "fused"))
    b = reduced_density_matrices(_onv(words), _dev(w), m, sorb, noA + noB, noA, noB)  # fused=None takes the same route
    assert b.fused and torch.equal(a.rdm1, b.rdm1) and torch.equal(a.rdm2, b.rdm2), "two fused calls differ in their bits"
    # traces
    nele = noA + noB
    pair = sorb * (sorb - 1) // 2
    d2 = got[sorb * sorb:][[X.tri(t, t) for t in range(pair)]]
    assert abs(got[:sorb * sorb].reshape(sorb, sorb).trace() - nele * est.sum_w) <= 64 * nele * X.U
    assert abs(d2.sum() - nele * (nele - 1) / 2 * est.sum_w) <= 64 * nele * nele * X.U


def _native_pair(case, M):
    """(pynqs_rdm_jrbm with the Jastrow matrix M, pynqs_rdm_rbm) on the case's walkers, through the C ABI"""
    from pynqs_amd import C_extension as cx
    from pynqs_amd import _native as N

    sorb, noA, noB, _, H = case[:5]
    rbm, _, occ, words, w, est, _ = JX.case(case)
    onv, wd = _onv(words), _dev(w)
    n = onv.size(0)
    table, jtable = cx.RBMTable(_dev(rbm.W), _dev(rbm.hb), _dev(rbm.vb)), cx.JastrowTable(_dev(M))
    n1 = sorb * sorb
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for jas in (True, False):
        size = (N.lib().pynqs_rdm_jrbm_workspace if jas else N.lib().pynqs_rdm_rbm_workspace)(n, sorb, H)
        work = torch.full((size // 8,), float("nan"), dtype=torch.float64, device="cuda")
        out = torch.full((est.flat().size,), float("nan"), dtype=torch.float64, device="cuda")
        tail = (H, work.data_ptr(), out.data_ptr(), out[n1:].data_ptr(), st)
        if jas:
            N.check(N.lib().pynqs_rdm_jrbm(onv.data_ptr(), n, sorb, noA + noB, noA, noB, wd.data_ptr(), table.data_ptr(), jtable.data_ptr(), *tail), "jrbm")
        else:
            N.check(N.lib().pynqs_rdm_rbm(onv.data_ptr(), n, sorb, noA + noB, noA, noB, wd.data_ptr(), table.data_ptr(), *tail), "rbm")
        outs.append(out.cpu().numpy())
    return outs


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[6], CASES[7], CASES[8]], ids=[IDS[1], IDS[3], IDS[6], IDS[7], IDS[8]])
def test_zero_jastrow_gives_the_bits_of_the_rbm_kernel(case):
    """(12,3,2) and (66,3,3): the hole side owns; (10,4,4): the particle side; every added term is +-0, every added factor 1"""
    sorb = case[0]
    j, r = _native_pair(case, np.zeros((sorb, sorb)))
    assert bool(np.isfinite(r).all()) and float(np.abs(r).max()) > 0
    assert np.array_equal(j, r), float(np.abs(j - r).max())
    # and it is the Jastrow matrix that moves the case's result: with M the two differ
    j2, _ = _native_pair(case, JX.case(case)[1])
    assert not np.array_equal(j2, r)


@pytest.mark.parametrize("case", [CASES[3], CASES[5]], ids=[IDS[3], IDS[5]])
def test_diagonal_of_the_jastrow_matrix_does_not_enter(case):
    M = JX.case(case)[1]
    d = np.random.default_rng(3).standard_normal(case[0])
    a, b = _fused(case), _fused(case, M + np.diag(d))
    assert torch.equal(a.rdm1, b.rdm1) and torch.equal(a.rdm2, b.rdm2)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_route_agrees_with_the_scatter_kernel_on_exact_ratios(case):
    """pynqs_rdm_scatter fed with correctly rounded ratios of the yardstick, in the package's own column order: within the "ratio"
    bound; the fused result differs from it by at most the sum of the two bounds"""
    from pynqs_amd import C_extension as cx
    from pynqs_amd import rdm as M_

    sorb, noA, noB = case[:3]
    rbm, M, occ, words, w, est, _ = JX.case(case)
    onv = _onv(words)
    comb, _ = cx.get_comb_tensor(onv, sorb, noA + noB, noA, noB)
    bits = np.unpackbits(comb.cpu().numpy(), axis=2, bitorder="little")[:, :, :sorb]
    out = torch.zeros(est.flat().size, dtype=torch.float64, device="cuda")
    M_.scatter(onv, _dev(w), _dev(JX.ratio_rows(bits, rbm, M)), sorb, noA + noB, noA, noB, out)
    got = out.cpu().numpy()
    _within(f"scatter {case}", got, est, JX.bound(est, "ratio"))
    f = _flat(_fused(case))
    diff, allowed = np.abs(f - got), JX.bound(est, "fused") + JX.bound(est, "ratio")
    assert bool((diff <= allowed).all()), float((diff / np.where(allowed > 0, allowed, 1)).max())


@pytest.mark.parametrize("case", SMALL, ids=["-".join(map(str, c)) for c in SMALL])
def test_generic_route_through_the_module(case):
    """fused=False: get_comb_tensor, JastrowRBM.forward on every x', psi(x') / psi(x), the scatter kernel, in chunks of 7 walkers"""
    from pynqs_amd.rdm import reduced_density_matrices

    sorb, noA, noB = case[:3]
    rbm, M, occ, words, w, est, kmod = JX.case(case)
    a = reduced_density_matrices(_onv(words), _dev(w), _module(rbm, M), sorb, noA + noB, noA, noB, fused=False, nbatch=7)
    assert not a.fused
    _within(f"module {case} (kappa_module {kmod:.4g})", _flat(a), est, JX.bound(est, "module", kmod))


def test_identity_E_against_total_energy():
    """one fused RDM, three integral sets: dot(h1e, rdm1) + dot(h2e, rdm2) = sum_x w_x E_loc(x) (pynqs_eloc_jrbm) within the slot bounds
    weighted by the integrals' moduli"""
    from pynqs_amd import energy
    from pynqs_amd.rdm import reduced_density_matrices

    case = CASES[3]
    sorb, noA, noB = case[:3]
    rbm, M, occ, words, w, est, _ = JX.case(case)
    m, onv, wd = _module(rbm, M), _onv(words), _dev(w)
    rdm = reduced_density_matrices(onv, wd, m, sorb, noA + noB, noA, noB)
    assert rdm.fused
    bound = JX.bound(est, "fused")
    for seed in (1234, 5, 99):
        h1, h2 = synth_integrals(sorb, seed)
        eloc, _, _ = energy.total_energy(onv, -1, -1, _dev(h1), _dev(h2), m, sorb, noA + noB, noA, noB)
        want = float((wd * eloc.real).sum())
        got = float(rdm.energy(_dev(h1), _dev(h2)))
        allowed = float((np.abs(np.concatenate([h1, h2])) * bound).sum())
        print(f"identity E, integrals {seed}: {got:+.12f} against {want:+.12f}, |difference| / allowed {abs(got - want) / allowed:.3g}")
        assert abs(want) > 1e-3 and abs(got - want) <= allowed, (seed, got, want, allowed)


def test_routing_and_refusals(monkeypatch):
    from pynqs_amd import _native as N
    from pynqs_amd import rdm as M_
    from pynqs_amd.rbm import JastrowRBM

    case = CASES[0]
    sorb, noA, noB = case[:3]
    rbm, M, occ, words, w, est, kmod = JX.case(case)
    m, onv, wd = _module(rbm, M), _onv(words), _dev(w)
    args = (sorb, noA + noB, noA, noB)
    assert M_.reduced_density_matrices(onv, wd, m, *args).fused
    assert M_.reduced_density_matrices(onv, wd, type("Wrapped", (), {"module": m})(), *args).fused  # (what DistributedDataParallel looks like)
    # the module flag
    monkeypatch.setattr(M_, "FUSED_RBM", False)
    r = M_.reduced_density_matrices(onv, wd, m, *args)
    assert not r.fused and M_.reduced_density_matrices(onv, wd, m, *args, fused=True).fused
    _within("FUSED_RBM = False", _flat(r), est, JX.bound(est, "module", kmod))
    monkeypatch.setattr(M_, "FUSED_RBM", True)
    # float32 parameters: generic
    assert not M_.reduced_density_matrices(onv, wd, _module(rbm, M).float(), *args).fused
    # 600 hidden units: not served, the generic route; fused=True refuses
    assert N.lib().pynqs_rdm_jrbm_supported(8, 4, 2, 2, 600) == 0
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    big = JastrowRBM(z(600, 8), z(600), z(8), z(8, 8)).cuda()
    r = M_.reduced_density_matrices(onv, wd, big, *args)
    assert not r.fused and abs(float(r.rdm1.view(8, 8).trace()) - 4 * est.sum_w) < 1e-12
    with pytest.raises(ValueError):
        M_.reduced_density_matrices(onv, wd, big, *args, fused=True)
    # `supported` answering 0 routes a served Jastrow-RBM to the scatter kernel too
    real = N.lib().pynqs_rdm_jrbm_supported
    monkeypatch.setattr(N.lib(), "pynqs_rdm_jrbm_supported", lambda *a: 0)
    r = M_.reduced_density_matrices(onv, wd, m, *args)
    monkeypatch.setattr(N.lib(), "pynqs_rdm_jrbm_supported", real)
    assert not r.fused
    # parameters on another device than the walkers
    cpu = JastrowRBM(*(torch.from_numpy(np.ascontiguousarray(a)) for a in (rbm.W, rbm.hb, rbm.vb, M)))
    with pytest.raises(ValueError):
        M_.reduced_density_matrices(onv, wd, cpu, *args, fused=True)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            M_.reduced_density_matrices(onv, wd, _module(rbm, M).to("cuda:1"), *args)
    # no walkers: zeros
    r = M_.reduced_density_matrices(onv[:0], wd[:0], m, *args)
    assert r.fused and float(r.rdm1.abs().max()) == 0.0 and float(r.rdm2.abs().max()) == 0.0
    # the C ABI refuses null pointers
    assert N.lib().pynqs_rdm_jrbm(onv.data_ptr(), 36, *args, wd.data_ptr(), None, None, 3, None, None, None, None) == N.EINVAL


def test_jrdm_example_runs():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import vmc_jrbm_rdm

    lines = []
    e_rdm, e_mean, occ, spin, e0 = vmc_jrbm_rdm.run(log=lines.append)
    print("\n".join(lines))
    assert any("fused route" in s for s in lines)
    assert abs(e_rdm - e_mean) <= 1e-10 * (1 + abs(e_mean)), (e_rdm, e_mean)
    assert e_mean > e0 - 1e-9
    assert occ.shape == (6,) and abs(occ.sum() - 6) <= 1e-10 and bool((occ >= 0).all()) and bool((occ <= 2).all())
    assert spin.shape == (6,) and abs(spin.sum()) <= 1e-10  # 3 alpha + 3 beta electrons
