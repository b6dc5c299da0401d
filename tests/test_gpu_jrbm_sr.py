"""pynqs_jrbm_sr_prepare / _matvec and pynqs_amd.sr.FusedJastrowRbmSR (stochastic reconfiguration for the Jastrow-RBM, matrix-free)
against the exact host reference of tests/jrbm_sr_exact.py (numpy longdouble from the parameters, the bits and the probabilities alone).
Every tolerance is that module's a-priori rounding bound of the product, per entry, or follows from it as in tests/test_gpu_rbm_sr.py:
    |F - (S + shift) d|_2 <= tol |F|_2 + |bound(d)|_2,        |d - d_exact|_2 <= that / shift + the refined solve's floor.
tests/test_jrbm_sr_exact.py checks on the CPU that the bound stays below 1e-9 of max |S v| on every case listed here."""
import functools
import os
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import jrbm_sr_exact as JS
import rbm_exact as R
from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

U = R.U
ALL_CASES = [("case",) + c for c in JS.CASES] + [("saturated",) + c for c in JS.SATURATED]
PRODUCT_CASES = ALL_CASES + [("case",) + c for c in JS.PRODUCT_SHAPES]  # (the size branches of the kernels: the product tests alone)
_ids = lambda c: "-".join(map(str, c[1:]))  # noqa: E731


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _onv(words):
    return _dev(words.view(np.uint8).reshape(words.shape[0], -1))


def _module(rbm, M):
    from pynqs_amd.rbm import JastrowRBM

    return JastrowRBM(_dev(rbm.W), _dev(rbm.hb), _dev(rbm.vb), _dev(M)).cuda()


@functools.lru_cache(maxsize=2)
def _inputs(case):
    """(rbm, M, words, prob, eloc, e_total, sorb, the exact reference) of an entry of ALL_CASES, shared by the tests of a case"""
    if case[0] == "case":
        _, sorb, no, H, n = case
        inp = JS.case_inputs(sorb, no, H, n)
    else:
        _, sorb, H, n, regime = case
        inp = JS.saturated_inputs(sorb, H, n, regime)
    return inp + (sorb, JS.sr_exact(inp[0], R.pm1(inp[2], sorb), inp[3]))


def _norm(a):
    a = np.asarray(a).astype(R.LD)
    return float(np.sqrt((a * a).sum()))


def _worst(what, err, bound):
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    k = int(np.argmax(ratio))
    msg = f"{what}: worst error / bound {ratio.flat[k]:.3g} at {k} of {ratio.size}"
    print(msg)
    return bool((err <= bound).all()), msg


def _flat(tensors):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in tensors])


@pytest.mark.parametrize("case", PRODUCT_CASES, ids=_ids)
def test_prepare_and_product_meet_the_rounding_bound(case):
    from pynqs_amd.rbm import RealRBM
    from pynqs_amd.sr import FusedJastrowRbmSR, FusedRbmSR

    rbm, M, words, prob, eloc, e_total, sorb, se = _inputs(case)
    n, H, nr = words.shape[0], rbm.H, se.nrbm
    sr = FusedJastrowRbmSR(_module(rbm, M), sorb)
    assert sr.np == se.P
    onv, pd = _onv(words), _dev(prob)
    sr.prepare(onv, pd)
    # 1. the table of tanh theta and Obar
    table = sr.tanh_table().cpu().numpy()
    assert table.shape == (n, H)
    ok, msg = _worst("tanh table", np.abs(table.astype(R.LD) - se.ex.y).astype(np.float64), se.table_bound())
    assert ok, msg
    obar = sr.obar.cpu().numpy()
    ok, msg = _worst("Obar", np.abs(obar.astype(R.LD) - se.Obar).astype(np.float64), se.obar_bound())
    assert ok, msg
    om = obar[nr:].reshape(sorb, sorb)
    assert np.array_equal(om, om.T)
    # 2. the product on every probe
    outs = {}
    for name, v in JS.probe_vectors(se):
        y = sr.matvec(_dev(v))
        again = sr.matvec(_dev(v))
        assert torch.equal(y, again), name  # fixed order of additions
        y = y.cpu().numpy()
        want, b = se.matvec(v), se.product_bound(v)
        assert y.shape == want.shape and bool(np.isfinite(y).all())
        if name != "zero":
            if n > 1 and name not in JS.DEGENERATE:
                assert float(b.max()) <= 1e-9 * float(np.abs(want).max()), (name, float(b.max()), float(np.abs(want).max()))
            else:  # the exact product vanishes: the bound is an absolute one
                assert float(b.max()) <= 1e-12 * float(np.abs(v).sum()), (name, float(b.max()))
        ok, msg = _worst(f"product {name}", np.abs(y.astype(R.LD) - want).astype(np.float64), b)
        assert ok, msg
        ym = y[nr:].reshape(sorb, sorb)
        assert np.array_equal(ym, ym.T), f"{name}: the jastrow block of the product is not bit-symmetric"
        outs[name] = (v, y, b)
    # symmetry: u . S v = v . S u within sum_k (|u_k| bound_k(v) + |v_k| bound_k(u))
    g = np.random.default_rng(4)
    u = g.standard_normal(se.P)
    v, Sv, bv = outs["random"]
    Su = sr.matvec(_dev(u)).cpu().numpy()
    bu = se.product_bound(u)
    lhs, rhs = (u.astype(R.LD) * Sv).sum(), (v.astype(R.LD) * Su).sum()
    allowed = float((np.abs(u) * bv + np.abs(v) * bu).sum())
    print(f"symmetry: |u.Sv - v.Su| / allowed {abs(float(lhs - rhs)) / allowed:.3g}")
    assert abs(float(lhs - rhs)) <= allowed
    # Z = 0: the kernel adds the Jastrow term after the RBM sum, so the three RBM blocks are FusedRbmSR's bits on the same weights
    plain = FusedRbmSR(RealRBM(_dev(rbm.W), _dev(rbm.hb), _dev(rbm.vb)).cuda(), sorb)
    plain.prepare(onv, pd)
    assert torch.equal(plain.obar, sr.obar[:nr])
    v0 = v.copy()
    v0[nr:] = 0.0
    assert torch.equal(sr.matvec(_dev(v0))[:nr], plain.matvec(_dev(v0[:nr])))


def _solve_checks(se, sr, F, d, shift, tol, what):
    """the derived checks on a solution d of (S + shift) d = F; returns (|r|, allowed |r|, d_exact)"""
    bd = _norm(se.product_bound(d))
    r = se.residual(F, d, shift)
    nF = _norm(F)
    allowed = tol * nF + bd
    print(f"{what}: |r| / |F| {_norm(r) / nF:.3e} (tol {tol:.0e}), |bound(d)| / |F| {bd / nF:.3e}, {sr.iterations} iterations")
    assert _norm(r) <= allowed, (what, _norm(r), allowed)
    dx, last = se.solve(F, shift)
    assert last <= JS.SOLVE_FLOOR
    dist, dallowed = _norm(d.astype(R.LD) - dx), allowed / shift + last * _norm(dx)
    print(f"{what}: |d - d_exact| / |d| {dist / _norm(dx):.3e}, allowed {dallowed / _norm(dx):.3e}")
    assert dist <= dallowed, (what, dist, dallowed)
    return _norm(r), allowed, dx


@pytest.mark.parametrize("shift", [0.02, 1e-3])
@pytest.mark.parametrize("case", ALL_CASES, ids=_ids)
def test_solution_meets_the_derived_bounds(case, shift):
    from pynqs_amd.grad import FusedJastrowRbmGrad
    from pynqs_amd.sr import FusedJastrowRbmSR

    rbm, M, words, prob, eloc, e_total, sorb, se = _inputs(case)
    m = _module(rbm, M)
    tol = 1e-10
    sr = FusedJastrowRbmSR(m, sorb, diag_shift=shift, tol=tol, max_iter=4000)
    onv, pd, ed = _onv(words), _dev(prob), _dev(eloc)
    et = torch.as_tensor(e_total, device="cuda")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loss = sr(onv, pd, ed, et)
    assert sr.converged and 0 < sr.iterations <= 4000 and sr.residual <= tol * (1 + 1e-12)
    d = _flat([p.grad for p in m.parameters()])
    F = _flat(sr.energy_grad)
    assert all(p.grad.shape == p.shape for p in m.parameters()) and bool(np.isfinite(d).all())
    nr, allowed, dx = _solve_checks(se, sr, F, d, shift, tol, f"{case[1:]} shift {shift}")
    # the reported residual is the TRUE one (see tests/test_gpu_rbm_sr.py)
    nF = _norm(F)
    slack = _norm(se.product_bound(d)) + 8 * U * (nF + _norm(se.matvec(d)) + shift * _norm(d))
    assert abs(sr.residual * nF - nr) <= slack, (sr.residual * nF, nr, slack)
    # the jastrow block of the direction is bit-symmetric
    assert torch.equal(m.jastrow.grad, m.jastrow.grad.t())
    # energy_grad is what FusedJastrowRbmGrad installs for the same inputs, bit for bit; the loss too
    m2 = _module(rbm, M)
    loss2 = FusedJastrowRbmGrad(m2, sorb)(onv, pd, ed, et)
    assert all(torch.equal(a, p.grad) for a, p in zip(sr.energy_grad, m2.parameters())) and torch.equal(loss, loss2)
    # a second call: the same bits
    its = sr.iterations
    sr(onv, pd, ed, et)
    assert sr.iterations == its and np.array_equal(_flat([p.grad for p in m.parameters()]), d)
    # the public solve() with the caller's own right-hand side
    d2 = sr.solve(_dev(F)).cpu().numpy()
    assert np.array_equal(d2, d)


def _dense_direction(m, onv, sorb, prob, F, shift):
    """(S + shift)^-1 F with torch on the device: O with the x_i x_j columns from the module's own theta, dense S, torch.linalg.solve"""
    from pynqs_amd import C_extension as cx

    x = cx.onv_to_tensor(onv, sorb).to(torch.float64)
    t = torch.tanh(x @ m.weights.detach().t() + m.hidden_bias.detach())
    O = torch.cat([(t[:, :, None] * x[:, None, :]).reshape(x.size(0), -1), t, x, (x[:, :, None] * x[:, None, :]).reshape(x.size(0), -1)], 1)
    J = O - (prob @ O)[None, :]
    S = J.t() @ (prob[:, None] * J)
    S.diagonal().add_(shift)
    return torch.linalg.solve(S, F)


def test_dense_torch_solve_agrees_at_4096_walkers():
    """Fe2S2 shape, H 40 (P = 3 280), 4096 walkers = 128 workgroups: the dense formulation on the device gives the same direction within
    the derived bound plus the dense solve's own distance from the exact solution, measured here on the CPU at 1000 walkers (float64
    dense build and LAPACK solve against the refined solve) and required at or below 1e-9."""
    from pynqs_amd.sr import FusedJastrowRbmSR

    sorb, no, H, shift, tol = 40, 15, 40, 0.02, 1e-10
    rbm, M, words, prob, eloc, e_total = JS.case_inputs(sorb, no, H, 1000)
    se = JS.sr_exact(rbm, R.pm1(words, sorb), prob)
    assert se.P == 3280
    F = JS.energy_gradient(se, M, prob, eloc, e_total)
    Rm = se.real_form()
    dense = np.linalg.solve(Rm.T @ Rm + shift * np.eye(Rm.shape[1]), F.astype(np.float64))
    dx, last = se.solve(F, shift)
    dense_dist = _norm(dense - dx) / _norm(dx)
    print(f"dense float64 solve, 1000 walkers: {dense_dist:.3e} from the exact solution")
    assert last <= JS.SOLVE_FLOOR and dense_dist <= 1e-9
    rbm, M, words, prob, eloc, e_total = JS.case_inputs(sorb, no, H, 4096)
    se = JS.sr_exact(rbm, R.pm1(words, sorb), prob)
    m = _module(rbm, M)
    sr = FusedJastrowRbmSR(m, sorb, diag_shift=shift, tol=tol, max_iter=4000)
    onv, pd = _onv(words), _dev(prob)
    sr(onv, pd, _dev(eloc), torch.as_tensor(e_total, device="cuda"))
    assert sr.converged
    d = _flat([p.grad for p in m.parameters()])
    Fk = torch.cat([g.reshape(-1) for g in sr.energy_grad])
    want = _dense_direction(m, onv, sorb, pd, Fk, shift).cpu().numpy()
    allowed = (tol * _norm(Fk.cpu().numpy()) + _norm(se.product_bound(d))) / shift + dense_dist * _norm(d)
    dist = _norm(d - want)
    print(f"4096 walkers: {sr.iterations} iterations, |d - d_dense| / |d| {dist / _norm(d):.3e}, allowed {allowed / _norm(d):.3e}")
    assert dist <= allowed, (dist, allowed)


def test_iteration_limit_zero_gradient_refusals_and_no_walkers():
    from pynqs_amd.rbm import ComplexRBM, JastrowRBM, RealRBM
    from pynqs_amd.sr import FusedJastrowRbmSR, FusedRbmSR

    rbm, M, words, prob, eloc, e_total = JS.case_inputs(40, 15, 80, 1000)
    m = _module(rbm, M)
    onv, pd, ed, et = _onv(words), _dev(prob), _dev(eloc), torch.as_tensor(e_total, device="cuda")
    sr = FusedJastrowRbmSR(m, 40, max_iter=3)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        sr(onv, pd, ed, et)
    assert len(w) == 1 and issubclass(w[0].category, RuntimeWarning) and "3 iterations" in str(w[0].message)
    assert "FusedJastrowRbmSR" in str(w[0].message)
    assert not sr.converged and sr.iterations == 3 and sr.residual > sr.tol
    assert all(bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in m.parameters())
    # F = 0 (all local energies equal): d = 0 with no iteration
    sr = FusedJastrowRbmSR(m, 40)
    flat = torch.full_like(ed, -100.0)
    sr(onv, pd, flat, torch.as_tensor(-100.0, device="cuda"))
    assert sr.converged and sr.iterations == 0 and sr.residual == 0.0 and all(float(p.grad.abs().max()) == 0.0 for p in m.parameters())
    # refusals
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    with pytest.raises(ValueError):
        FusedJastrowRbmSR(RealRBM(z(4, 8), z(4), z(8)).cuda(), 8)
    with pytest.raises(ValueError):
        FusedJastrowRbmSR(ComplexRBM(z(4, 8, 2), z(4, 2), z(8, 2)).cuda(), 8)
    with pytest.raises(ValueError):
        FusedJastrowRbmSR(torch.nn.Linear(8, 1).double().cuda(), 8)
    with pytest.raises(ValueError):
        FusedJastrowRbmSR(JastrowRBM(z(4, 8), z(4), z(8), z(8, 8)).cuda().float(), 8)
    with pytest.raises(ValueError):
        FusedJastrowRbmSR(m, 40, tol=0.0)
    with pytest.raises(ValueError):
        FusedJastrowRbmSR(m, 40, diag_shift=-1e-3)
    with pytest.raises(ValueError):
        sr(onv, pd, ed.to(torch.complex128), et)
    with pytest.raises(ValueError):
        sr(torch.zeros((4, 16), dtype=torch.uint8, device="cuda"), pd[:4], ed[:4], et)
    with pytest.raises(ValueError):
        FusedRbmSR(m, 40)  # the plain RBMs' class would drop M
    # a replaced parameter is seen
    sr = FusedJastrowRbmSR(m, 40, tol=1e-8)
    sr(onv, pd, ed, et)
    first = _flat([p.grad for p in m.parameters()])
    m.weights = torch.nn.Parameter(m.weights.detach() * 0.5)
    sr(onv, pd, ed, et)
    assert m.weights.grad is not None and not np.array_equal(_flat([p.grad for p in m.parameters()]), first)
    # no walkers: d = 0
    rbm8 = R.make("real", *JS.SE.module_params("real", 8, 4, 1))
    m8 = _module(rbm8, JS.J.jastrow_params("j-asym", 8))
    sr8 = FusedJastrowRbmSR(m8, 8)
    loss = sr8(torch.zeros((0, 8), dtype=torch.uint8, device="cuda"), torch.zeros(0, dtype=torch.float64, device="cuda"),
               torch.zeros(0, dtype=torch.float64, device="cuda"), torch.zeros((), dtype=torch.float64, device="cuda"))
    assert float(loss) == 0.0 and sr8.iterations == 0 and all(float(p.grad.abs().max()) == 0.0 for p in m8.parameters())
    assert float(sr8.obar.abs().max()) == 0.0
    assert float(sr8.matvec(torch.ones(sr8.np, dtype=torch.float64, device="cuda")).abs().max()) == 0.0


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _two_ranks(split, out):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "jsr_ranks_worker.py"), split, out]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return [np.load(f"{out}_rank{k}.npz") for k in range(2)]


@pytest.mark.parametrize("split", ["even", "empty"])
def test_two_ranks_agree_with_one_rank(split, tmp_path):
    """Two ranks (fresh child processes, gloo, both on device 0) on uneven shards of 1027 walkers (514 + 513; "empty": 1027 + 0) with the
    probabilities pre-scaled by 2: the same iteration count and the same bits of d on both ranks, and the one-rank direction on all 1027
    walkers within the derived bound (each side is within (tol |F| + |bound(d)|) / shift of the exact solution of its own right-hand
    side; the two right-hand sides differ by the gradient kernels' rounding)."""
    import jsr_ranks_worker as Wk
    from pynqs_amd.sr import FusedJastrowRbmSR

    ranks = _two_ranks(split, str(tmp_path / split))
    assert int(ranks[0]["iterations"]) == int(ranks[1]["iterations"]) > 0 and bool(ranks[0]["converged"]) and bool(ranks[1]["converged"])
    assert np.array_equal(ranks[0]["d"], ranks[1]["d"]), "the ranks' directions differ in their bits"
    assert [int(r["n"]) for r in ranks] == ([514, 513] if split == "even" else [1027, 0])
    rbm, M, words, prob, eloc, e_total = Wk.inputs()
    se = JS.sr_exact(rbm, R.pm1(words, Wk.SORB), prob, world=2)
    m = _module(rbm, M)
    sr = FusedJastrowRbmSR(m, Wk.SORB, diag_shift=Wk.SHIFT, tol=Wk.TOL, max_iter=4000)
    sr(_onv(words), _dev(prob), _dev(eloc), torch.as_tensor(e_total, device="cuda"))
    d1, d2 = _flat([p.grad for p in m.parameters()]), ranks[0]["d"]
    F = _flat(sr.energy_grad)
    bF = _norm(JS.gradient_bound(se, M, prob, eloc, e_total))
    allowed = (2 * (Wk.TOL * _norm(F) + _norm(se.product_bound(d1))) + 2 * bF) / Wk.SHIFT
    dist = _norm(d1 - d2)
    print(f"{split}: {int(ranks[0]['iterations'])} iterations on two ranks, {sr.iterations} on one; |d2 - d1| / |d| {dist / _norm(d1):.3e}, "
          f"allowed {allowed / _norm(d1):.3e}")
    assert sr.converged and dist <= allowed, (dist, allowed)
    dm = ranks[0]["d"][se.nrbm:].reshape(Wk.SORB, Wk.SORB)
    assert np.array_equal(dm, dm.T)
    # each rank's direction also meets the bounds against the exact reference for the right-hand side the ranks agreed on
    _solve_checks(se, sr, ranks[0]["F"], d2, Wk.SHIFT, Wk.TOL, f"two ranks ({split})")


def test_direction_of_the_reference():
    """tests/golden/sr_jrbm_fe2s2.npz: the reference's own _calculate_sr (dense S, torch.linalg.inv) on 32 Fe2S2 walkers with
    per_sample = [the RBM's analytic_derivate, x_i x_j] and the exact gradient as right-hand side.  Tolerance: the derived bound of the
    solve plus twice the reference's recorded distance from the exact solution."""
    from pynqs_amd.sr import FusedJastrowRbmSR

    g, e0, f = golden("grad_fe2s2.npz"), golden("eloc_e2e_fe2s2.npz"), golden("sr_jrbm_fe2s2.npz")
    rbm = R.make("real", e0["W"], e0["hb"], e0["vb"])
    words = np.ascontiguousarray(e0["x"]).view(np.uint64).reshape(32, -1)
    shift, tol = float(f["diag_shift"]), 1e-11
    prob = g["grad_real_amd-1_pow0_prob"]
    se = JS.sr_exact(rbm, R.pm1(words, 40), prob)
    F = f["F"]
    want = np.concatenate([f[nm].reshape(-1) for nm in ("weights", "hidden_bias", "visible_bias", "jastrow")])
    m = _module(rbm, JS.J.jastrow_params("j-asym", 40))  # (S does not depend on M)
    sr = FusedJastrowRbmSR(m, 40, diag_shift=shift, tol=tol, max_iter=4000)
    sr.prepare(_onv(words), _dev(prob))
    d = sr.solve(_dev(F)).cpu().numpy()
    assert sr.converged
    allowed = (tol * _norm(F) + _norm(se.product_bound(d))) / shift + 2 * float(f["dist"]) * _norm(want)
    dist = _norm(d - want)
    print(f"{sr.iterations} iterations, |d - d_reference| / |d| {dist / _norm(want):.3e}, allowed {allowed / _norm(want):.3e}")
    assert dist <= allowed, (dist, allowed)
    _solve_checks(se, sr, F, d, shift, tol, "reference fixture")


def test_jastrow_sr_example_converges():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import vmc_jrbm_sr

    lines = []
    hist, e0 = vmc_jrbm_sr.run(log=lines.append)
    print("\n".join(lines))
    rises = np.diff(hist)
    # host replay with dense algebra: -5.556 524 after 10 steps, -6.391 214 after 30; the energy never rises
    assert len(hist) == 40 and float(rises.max()) <= 1e-9, (float(rises.max()), hist)
    assert hist[10] < -5.3 and hist[30] < -6.25 and hist[-1] > e0, (hist[10], hist[30], hist[-1], e0)


def test_jastrow_sr_example_with_mcmc_walkers():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import vmc_jrbm_sr

    lines = []
    hist, e0 = vmc_jrbm_sr.run(sampling="mcmc", nchains=8192, log=lines.append)
    print("\n".join(lines))
    assert hist[-1] < hist[0] - 3.0 and hist[-1] > e0 - 0.05, (hist[0], hist[-1], e0)
