"""pynqs_rdm_rbm (fused, real RBM) and pynqs_rdm_scatter (any ansatz) and pynqs_amd.rdm against the host yardstick tests/rdm_exact.py:
every slot of rdm1 and rdm2 within that module's a-priori bound c_t u A_t (its docstring derives c_t per path), slots without any
contribution exactly zero.  The yardstick of a case is computed once and shared by the tests of that case."""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import rbm_exact as R
import rdm_exact as X
from conftest import ROOT, golden, rand_occ, synth_integrals

pytestmark = pytest.mark.gpu

# (sorb, noA, noB, walkers (0: all 36 of the golden file), H, regime)
CASES = [
    (8, 2, 2, 0, 3, "small"), (8, 2, 2, 0, 8, "chunk-50"), (8, 2, 2, 0, 17, "alt30"), (8, 2, 2, 0, 8, "one-338-w"), (8, 2, 2, 0, 17, "tiny"),
    (12, 3, 2, 24, 8, "fe2s2"), (12, 3, 2, 24, 17, "one-338-w"),     # noA != noB, the hole side owns (5 of 12)
    (10, 4, 4, 20, 3, "small"), (10, 4, 4, 20, 17, "chunk-50"),      # the particle side owns (8 of 10); no same-spin doubles
    (10, 1, 1, 20, 8, "alt30"),                                      # no same-spin doubles, no same-spin spectators
    (66, 3, 3, 16, 17, "one-338-w"), (66, 3, 3, 16, 3, "small"),     # two words; orbitals 63, 64, 65 forced
]
IDS = ["-".join(map(str, c)) for c in CASES]


def _occ(sorb, noA, noB, n):
    if n == 0:
        return golden("c1_sorb8_all36.npz")["occ"].astype(np.uint8)
    occ = rand_occ(n, sorb, noA, noB, seed=sorb + n)
    if sorb == 66:
        # orbitals 63 (beta), 64 (alpha), 65 (beta) of the two-word determinants: occupied / empty in turn, electron counts kept
        for i in range(n):
            for o, want in zip(R.forced_orbitals(66)[1:], ((i >> 0) & 1, (i >> 1) & 1, (i >> 2) & 1)):
                if occ[i, o] != want:
                    same = [p for p in range(o & 1, 62, 2) if occ[i, p] == want]
                    occ[i, same[i % len(same)]], occ[i, o] = occ[i, o], want
        assert (occ[:, 0::2].sum(1) == noA).all() and (occ[:, 1::2].sum(1) == noB).all()
    return occ


@functools.lru_cache(maxsize=None)
def _case(case, kind="real"):
    """(rbm, occ, words, w, Estimate): the yardstick, once per case"""
    sorb, noA, noB, n, H, regime = case
    occ = _occ(sorb, noA, noB, n)
    rbm = R.regime_params(regime, kind, sorb, H, 7)
    g = np.random.default_rng([sorb, H, len(regime)])
    w = g.random(occ.shape[0]) + 0.1
    w = w / w.sum()
    est = X.estimator(occ.astype(np.int8), w, rbm=rbm)
    return rbm, occ, R.pack_bits(occ.astype(bool)), w, est


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _onv(words):
    return _dev(words.view(np.uint8).reshape(words.shape[0], -1))


def _module(rbm):
    from pynqs_amd.rbm import ComplexRBM, RealRBM

    if rbm.kind == "complex":
        return ComplexRBM(_dev(R.pairs(rbm.W)), _dev(R.pairs(rbm.hb)), _dev(R.pairs(rbm.vb))).cuda()
    return RealRBM(_dev(rbm.W), _dev(rbm.hb), _dev(rbm.vb)).cuda()


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
    print(f"{what}: worst error / bound {ratio[k]:.3g} over {int(live.sum())} live slots of {live.size}; max c_t {float((bound[live] / (X.U * A[live])).max()):.4g}")
    assert bool((err[live] <= bound[live]).all()), f"{what}: error / bound {ratio[k]:.3g} at live slot {k}"


def _scatter_exact(case, kind):
    """pynqs_rdm_scatter fed with correctly rounded ratios of the longdouble reference, in the package's own column order"""
    from pynqs_amd import C_extension as cx
    from pynqs_amd import rdm as M

    sorb, noA, noB = case[:3]
    rbm, occ, words, w, est = _case(case, kind)
    onv = _onv(words)
    comb, _ = cx.get_comb_tensor(onv, sorb, noA + noB, noA, noB)
    bits = np.unpackbits(comb.cpu().numpy(), axis=2, bitorder="little")[:, :, :sorb]
    r = X.ratio_rows(bits, rbm)
    ratio = torch.view_as_complex(_dev(r)) if kind == "complex" else _dev(r)
    out = torch.zeros(est.flat().size, dtype=torch.float64, device="cuda")
    M.scatter(onv, _dev(w), ratio, sorb, noA + noB, noA, noB, out)
    return out.cpu().numpy(), est


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_path_meets_the_slot_bounds_and_is_reproducible(case):
    from pynqs_amd.rdm import reduced_density_matrices

    sorb, noA, noB = case[:3]
    rbm, occ, words, w, est = _case(case)
    m = _module(rbm)
    a = reduced_density_matrices(_onv(words), _dev(w), m, sorb, noA + noB, noA, noB, fused=True)
    assert a.fused
    got = _flat(a)
    _within(f"fused {case}", got, est, est.bound("fused"))
    b = reduced_density_matrices(_onv(words), _dev(w), m, sorb, noA + noB, noA, noB)  # fused=None takes the same route
    assert b.fused and torch.equal(a.rdm1, b.rdm1) and torch.equal(a.rdm2, b.rdm2), "two fused calls differ in their bits"
    # traces
    nele = noA + noB
    pair = sorb * (sorb - 1) // 2
    d2 = got[sorb * sorb:][[X.tri(t, t) for t in range(pair)]]
    assert abs(got[:sorb * sorb].reshape(sorb, sorb).trace() - nele * est.sum_w) <= 64 * nele * X.U
    assert abs(d2.sum() - nele * (nele - 1) / 2 * est.sum_w) <= 64 * nele * nele * X.U


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_scatter_path_meets_the_slot_bounds_and_agrees_with_the_fused_path(case):
    from pynqs_amd.rdm import reduced_density_matrices

    sorb, noA, noB = case[:3]
    got, est = _scatter_exact(case, "real")
    _within(f"scatter {case}", got, est, est.bound("ratio"))
    rbm, occ, words, w, _ = _case(case)
    f = _flat(reduced_density_matrices(_onv(words), _dev(w), _module(rbm), sorb, noA + noB, noA, noB, fused=True))
    diff, allowed = np.abs(f - got), est.bound("fused") + est.bound("ratio")
    assert bool((diff <= allowed).all()), float((diff / np.where(allowed > 0, allowed, 1)).max())


COMPLEX_CASES = [CASES[0], CASES[5], CASES[8], (66, 3, 3, 8, 17, "small")]  # (8 two-word walkers: every setting of orbitals 63, 64, 65)


@pytest.mark.parametrize("case", COMPLEX_CASES, ids=["-".join(map(str, c)) for c in COMPLEX_CASES])
def test_scatter_path_with_complex_ratios(case):
    got, est = _scatter_exact(case[:5] + ("small" if case[5] == "one-338-w" else case[5],), "complex")
    _within(f"scatter complex {case}", got, est, est.bound("ratio"))


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[5], CASES[8]], ids=[IDS[0], IDS[3], IDS[5], IDS[8]])
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_generic_route_through_the_module(case, kind):
    """fused=False: get_comb_tensor, the module's forward, psi(x') / psi(x), the scatter kernel, in chunks of 7 walkers"""
    from pynqs_amd.rdm import reduced_density_matrices

    if kind == "complex":
        case = case[:5] + ("small" if case[5] == "one-338-w" else case[5],)
    sorb, noA, noB = case[:3]
    rbm, occ, words, w, est = _case(case, kind)
    a = reduced_density_matrices(_onv(words), _dev(w), _module(rbm), sorb, noA + noB, noA, noB, fused=False, nbatch=7)
    assert not a.fused
    _within(f"module {kind} {case}", _flat(a), est, est.bound("module"))


def test_identity_E_against_total_energy():
    """one RDM, three integral sets: dot(h1e, rdm1) + dot(h2e, rdm2) = sum_x w_x E_loc(x) (SIMPLE) within the slot bounds weighted by
    the integrals' moduli"""
    from pynqs_amd import energy
    from pynqs_amd.rdm import reduced_density_matrices

    case = CASES[5]
    sorb, noA, noB = case[:3]
    rbm, occ, words, w, est = _case(case)
    m, onv, wd = _module(rbm), _onv(words), _dev(w)
    rdm = reduced_density_matrices(onv, wd, m, sorb, noA + noB, noA, noB)
    bound = est.bound("fused")
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
    from pynqs_amd import rdm as M
    from pynqs_amd.rbm import RealRBM

    case = CASES[0]
    sorb, noA, noB = case[:3]
    rbm, occ, words, w, est = _case(case)
    m, onv, wd = _module(rbm), _onv(words), _dev(w)
    args = (sorb, noA + noB, noA, noB)
    assert N.lib().pynqs_rdm_rbm_supported(8, 4, 2, 2, 17) == 1 and N.lib().pynqs_rdm_rbm_supported(40, 30, 15, 15, 80) == 1
    assert N.lib().pynqs_rdm_rbm_supported(8, 4, 2, 2, 600) == 0 and N.lib().pynqs_rdm_rbm_supported(120, 60, 30, 30, 80) == 0
    assert N.lib().pynqs_rdm_rbm_supported(8, 5, 2, 2, 8) == 0
    # an RBM the fused kernel does not serve (600 hidden units) takes the generic route, and fused=True refuses it
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    big = RealRBM(z(600, 8), z(600), z(8)).cuda()
    r = M.reduced_density_matrices(onv, wd, big, *args)
    assert not r.fused and abs(float(r.rdm1.view(8, 8).trace()) - 4 * est.sum_w) < 1e-12
    with pytest.raises(ValueError):
        M.reduced_density_matrices(onv, wd, big, *args, fused=True)
    # `supported` answering 0 routes a served RBM to the scatter kernel too
    real = N.lib().pynqs_rdm_rbm_supported
    monkeypatch.setattr(N.lib(), "pynqs_rdm_rbm_supported", lambda *a: 0)
    r = M.reduced_density_matrices(onv, wd, m, *args)
    monkeypatch.setattr(N.lib(), "pynqs_rdm_rbm_supported", real)
    assert not r.fused
    _within("routed to scatter", _flat(r), est, est.bound("module"))
    # the module flag, other flavours and float32 parameters: generic
    monkeypatch.setattr(M, "FUSED_RBM", False)
    assert not M.reduced_density_matrices(onv, wd, m, *args).fused and M.reduced_density_matrices(onv, wd, m, *args, fused=True).fused
    monkeypatch.setattr(M, "FUSED_RBM", True)
    assert not M.reduced_density_matrices(onv, wd, RealRBM(_dev(rbm.W), _dev(rbm.hb), _dev(rbm.vb), rbm_type="tanh").cuda(), *args).fused
    assert not M.reduced_density_matrices(onv, wd, _module(rbm).float(), *args).fused
    # bad inputs
    for bad in (lambda: M.reduced_density_matrices(onv.to(torch.int8), wd, m, *args),
                lambda: M.reduced_density_matrices(onv.cpu(), wd, m, *args),
                lambda: M.reduced_density_matrices(onv[:, :4], wd, m, *args),
                lambda: M.reduced_density_matrices(onv, wd[:5], m, *args),
                lambda: M.reduced_density_matrices(onv, wd, m, 8, 5, 2, 2),
                lambda: M.reduced_density_matrices(onv, wd, m, 7, 4, 2, 2),
                lambda: M.reduced_density_matrices(onv, wd, m, 8, 4, 3, 1),  # the walkers have 2 + 2 electrons
                lambda: M.scatter(onv, wd, torch.zeros((36, 5), dtype=torch.float64, device="cuda"), *args, torch.zeros(64 + 406, dtype=torch.float64, device="cuda"))):
        with pytest.raises(ValueError):
            bad()
    # no walkers: zeros
    r = M.reduced_density_matrices(onv[:0], wd[:0], m, *args)
    assert float(r.rdm1.abs().max()) == 0.0 and float(r.rdm2.abs().max()) == 0.0


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs 2 GPUs")
def test_two_ranks_agree_with_one_rank(tmp_path):
    """two ranks on a split of the walkers (probabilities pre-scaled by 2) give the one-rank matrices within the bound, the same bits on
    both ranks"""
    import rdm_ranks_worker as Wk

    out = str(tmp_path / "rdm")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "rdm_ranks_worker.py"), out]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    ranks = [np.load(f"{out}_rank{k}.npz") for k in range(2)]
    assert np.array_equal(ranks[0]["flat"], ranks[1]["flat"]) and int(ranks[0]["n"]) + int(ranks[1]["n"]) == Wk.N
    rbm, occ, words, w = Wk.inputs()
    est = X.estimator(occ.astype(np.int8), w, rbm=rbm)
    # each rank's partial sums meet the bound of its own walkers, which the whole set's bound dominates; one more addition and the
    # division by the world size (exact) are inside the bound's "+ 2"
    _within("two ranks", ranks[0]["flat"], est, est.bound("fused"))


def test_rdm_example_runs():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import vmc_rbm_rdm

    lines = []
    e_rdm, e_mean, occ, e0 = vmc_rbm_rdm.run(log=lines.append)
    print("\n".join(lines))
    assert abs(e_rdm - e_mean) <= 1e-10 * (1 + abs(e_mean)), (e_rdm, e_mean)
    assert e_mean < -6.5 and e_mean > e0 - 1e-9  # (the SR example reaches -6.6 after 30 of these steps)
    assert occ.shape == (6,) and abs(occ.sum() - 6) <= 1e-10 and bool((occ >= -1e-10).all()) and bool((occ <= 2 + 1e-10).all())
