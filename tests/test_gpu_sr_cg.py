"""pynqs_rbm_sr_cg_step (rbm_sr_cg_kernel) on its own, through the C ABI, and the loop of pynqs_amd.sr._FusedSR.solve on operators the test
supplies, against the host replay of tests/cg_exact.py.  Every comparison is bit equality (the vectors, the flags, the counter, the
guard words) or that module's a-priori bound gamma_m sum |terms|, m = ceil(np / 1024) + 10, on the kernel's sums; the driver tests add
the rounding of their own matrix-vector product, P 2^-52 | |A| |d| |.  tests/test_cg_exact.py proves on the CPU that the replay
refuses each of eleven mistakes at these sizes and that the driver's operators stagnate, converge and break down as claimed here."""
import math
import types
import warnings

import numpy as np
import pytest
import torch

import cg_exact as C
from cg_exact import BREAKDOWN, CONVERGED, DONE, INIT, ITER, PAP, RESIDUAL, RHO, RHS2, STEP, TRUE2

pytestmark = pytest.mark.gpu

LD = np.longdouble
GUARD = 3  # NaN words before, between and behind the six buffers


class Arena:
    """y, rhs, d, r, p and the scalars in ONE allocation, NaN guard words around each"""

    def __init__(self, n: int):
        self.n, self.off, o = n, {}, GUARD
        for k in C.VECTORS + ("sc",):
            self.off[k] = o
            o += (C.NSC if k == "sc" else n) + GUARD
        self.buf = torch.full((o,), math.nan, dtype=torch.float64, device="cuda")
        live = np.zeros(o, dtype=bool)
        for k, at in self.off.items():
            live[at:at + self.size(k)] = True
        self.guard = ~live
        assert int(self.guard.sum()) == 7 * GUARD
        g = np.random.default_rng([5, n])
        for k in C.VECTORS:  # finite junk: a call shows what it wrote
            self.put(k, g.standard_normal(n) + 3.0)
        self.put("sc", np.arange(C.NSC) + 0.5)

    def size(self, k):
        return C.NSC if k == "sc" else self.n

    def put(self, k, host):
        self.buf[self.off[k]:self.off[k] + self.size(k)].copy_(torch.from_numpy(np.ascontiguousarray(host, dtype=np.float64)))

    def ptr(self, k):
        return self.buf.data_ptr() + 8 * self.off[k]

    def read(self):
        """(State, the whole allocation) on the host; every guard word checked"""
        raw = self.buf.cpu().numpy()
        assert bool(np.isnan(raw[self.guard]).all()), f"guard words overwritten at {np.flatnonzero(self.guard & ~np.isnan(raw)).tolist()[:8]}"
        return C.State(*(raw[self.off[k]:self.off[k] + self.size(k)].copy() for k in C.VECTORS + ("sc",))), raw

    def call(self, mode, inv_world, shift, tol):
        from pynqs_amd import _native as N

        rc = N.lib().pynqs_rbm_sr_cg_step(mode, self.n, *(self.ptr(k) for k in C.VECTORS + ("sc",)), inv_world, shift, tol,
                                          torch.cuda.current_stream().cuda_stream)
        N.check(rc, "pynqs_rbm_sr_cg_step")


def _checked(arena, mode, inv_world, shift, tol, y=None):
    """one call with y uploaded first: (before, after, verdict, the allocation after); every derived property asserted"""
    if y is not None:
        arena.put("y", y)
    before, _ = arena.read()
    arena.call(mode, inv_world, shift, tol)
    after, raw = arena.read()
    v = C.verify_call(mode, before, after, inv_world, shift, tol)
    assert v.problems == [], (("INIT", "STEP", "RESIDUAL")[mode], v.problems)
    return before, after, v, raw


def _same_allocation(a, b):
    return C.same_bits(a, b)


@pytest.mark.parametrize("inv_world,shift", C.PARAMS, ids=lambda v: f"{v:.3g}")
@pytest.mark.parametrize("n", C.SIZES)
def test_step_kernel_is_the_replay_call_by_call(n, inv_world, shift):
    tol = C.SEQ_TOL
    pb = C.step_problem(n)
    order = [INIT] + [STEP] * 8 + [RESIDUAL] + [STEP] * 8

    def sequence(check):
        arena = Arena(n)
        arena.put("rhs", pb.rhs)
        st, raw = arena.read()
        raws, worst = [], {}
        for mode in order:
            y = None if mode == INIT else pb.product(st.p if mode == STEP else st.d, inv_world)
            if check:
                _, st, v, raw = _checked(arena, mode, inv_world, shift, tol, y)
                for k, q in v.ratios.items():
                    worst[k] = max(worst.get(k, 0.0), q)
            else:
                if y is not None:
                    arena.put("y", y)
                arena.call(mode, inv_world, shift, tol)
                st, raw = arena.read()
            raws.append(raw)
        return st, raws, worst

    st, raws, worst = sequence(True)
    print(f"sr_cg_exact: step np {n} inv_world {inv_world:.3g} shift {shift}: {int(st.sc[ITER])} iterations; worst scalar error / bound "
          + ", ".join(f"{k} {q:.3g}" for k, q in sorted(worst.items())))
    assert max(worst.values()) <= 1.0
    if n >= 1023:  # all sixteen steps were live and the RESIDUAL restarted: no call of the sequence was a no-op
        assert st.sc[ITER] == 16.0 and st.sc[DONE] == 0.0 and st.sc[CONVERGED] == 0.0 and st.sc[BREAKDOWN] == 0.0
    # a second run of the same sequence: the same bits after every call
    _, again, _ = sequence(False)
    assert all(_same_allocation(a, b) for a, b in zip(raws, again))


# ---- every branch once, at np = 1025 (one entry in the second stride) ------------------------------------------------------------------------
N1, IW, SHIFT = 1025, 0.5, 2.0 ** -10  # (powers of two: y = -(shift / inv_world) p gives Ap = 0 exactly)


def _started(steps, tol=C.SEQ_TOL, rhs=None):
    """an arena after INIT and `steps` STEPs of the step problem"""
    pb = C.step_problem(N1)
    arena = Arena(N1)
    arena.put("rhs", pb.rhs if rhs is None else rhs)
    _, st, _, _ = _checked(arena, INIT, IW, SHIFT, tol)
    for _ in range(steps):
        _, st, _, _ = _checked(arena, STEP, IW, SHIFT, tol, pb.product(st.p, IW))
    return pb, arena, st


def test_zero_right_hand_side_is_done_at_once():
    pb, arena, st = _started(0, rhs=np.zeros(N1))
    assert st.sc[DONE] == 1.0 and st.sc[CONVERGED] == 1.0 and st.sc[RHO] == 0.0 and st.sc[ITER] == 0.0 and not st.d.any()
    arena.put("y", pb.product(pb.rhs, IW))
    _, raw = arena.read()
    _checked(arena, STEP, IW, SHIFT, C.SEQ_TOL)
    assert _same_allocation(arena.read()[1], raw)  # a following STEP changes nothing, y included


def test_step_is_a_no_op_once_done_is_set():
    pb, arena, st = _started(2)
    assert st.sc[DONE] == 0.0 and st.sc[ITER] == 2.0
    sc = st.sc.copy()
    sc[DONE] = 1.0
    arena.put("sc", sc)
    arena.put("y", pb.product(st.p, IW))
    _, raw = arena.read()
    for _ in range(3):
        _checked(arena, STEP, IW, SHIFT, C.SEQ_TOL)
        assert _same_allocation(arena.read()[1], raw)  # all six buffers, y and the eight scalars included


@pytest.mark.parametrize("kind", ["negative", "zero", "nan"])
def test_breakdown(kind):
    pb, arena, st = _started(2)
    y = {"negative": -st.p, "zero": -(SHIFT / IW) * st.p, "nan": pb.product(st.p, IW)}[kind]
    if kind == "nan":
        y[700] = math.nan
    before, after, v, _ = _checked(arena, STEP, IW, SHIFT, C.SEQ_TOL, y)
    print(f"sr_cg_exact: breakdown {kind}: PAP {after.sc[PAP]!r}, error / bound {v.ratios['PAP']:.3g}")
    assert after.sc[BREAKDOWN] == 1.0 and after.sc[DONE] == 1.0 and after.sc[CONVERGED] == 0.0
    assert after.sc[ITER] == 2.0 and C.same_bits(after.sc[[RHO, RHS2, TRUE2]], before.sc[[RHO, RHS2, TRUE2]])
    assert all(C.same_bits(getattr(after, k), getattr(before, k)) for k in ("d", "r", "p", "rhs"))
    assert C.same_bits(after.y, C.fma_exact(SHIFT, before.p, y * IW))  # y holds Ap
    if kind == "negative":
        assert after.sc[PAP] < 0.0
    elif kind == "zero":
        assert after.sc[PAP] == 0.0 and not after.y.any()
    else:
        assert math.isnan(after.sc[PAP]) and int(np.isnan(after.y).sum()) == 1
    # a further STEP is a no-op
    _, raw = arena.read()
    _checked(arena, STEP, IW, SHIFT, C.SEQ_TOL)
    assert _same_allocation(arena.read()[1], raw)
    # the driver's next call: the true residual; it leaves BREAKDOWN and ITER alone and restarts (or reports NaN)
    _, res, _, _ = _checked(arena, RESIDUAL, IW, SHIFT, C.SEQ_TOL, pb.product(after.d, IW))
    assert res.sc[BREAKDOWN] == 1.0 and res.sc[ITER] == 2.0 and res.sc[CONVERGED] == 0.0 and res.sc[DONE] == 0.0


def test_residual_outside_the_tolerance_restarts():
    pb, arena, st = _started(2)
    sc = st.sc.copy()
    sc[RHO] *= 2.0  # stale on purpose (after two well-conditioned steps the true |r|^2 can be the recurrence's to the last bit)
    arena.put("sc", sc)
    before, after, v, _ = _checked(arena, RESIDUAL, IW, SHIFT, C.SEQ_TOL, pb.product(st.d, IW))
    assert C.same_bits(after.p, after.r) and not C.same_bits(after.p, before.p)
    assert C.same_bits(after.sc[[RHO]], after.sc[[TRUE2]]) and after.sc[RHO] != before.sc[RHO]
    assert after.sc[DONE] == 0.0 and after.sc[CONVERGED] == 0.0 and after.sc[ITER] == 2.0 and after.sc[BREAKDOWN] == 0.0
    assert after.sc[PAP] == before.sc[PAP] and C.same_bits(after.d, before.d)


def test_residual_inside_the_tolerance_converges_and_keeps_p_and_rho():
    pb, arena, st = _started(2)
    before, after, v, _ = _checked(arena, RESIDUAL, IW, SHIFT, 10.0, pb.product(st.d, IW))  # (tol 10: any residual meets it)
    assert C.same_bits(after.p, before.p) and not C.same_bits(after.p, after.r)
    assert after.sc[RHO] == before.sc[RHO] and after.sc[TRUE2] != before.sc[TRUE2]
    assert after.sc[DONE] == 1.0 and after.sc[CONVERGED] == 1.0 and after.sc[ITER] == 2.0 and after.sc[BREAKDOWN] == 0.0


def test_iteration_goes_on_from_the_iterate_after_a_residual():
    tol = 1e-8
    pb, arena, st = _started(3, tol)
    _, st, _, _ = _checked(arena, RESIDUAL, IW, SHIFT, tol, pb.product(st.d, IW))
    assert st.sc[DONE] == 0.0 and st.sc[ITER] == 3.0
    residuals = 1
    while st.sc[CONVERGED] == 0.0:
        assert st.sc[ITER] < 400 and residuals < 5 and st.sc[BREAKDOWN] == 0.0
        if st.sc[DONE] != 0.0:
            _, st, _, _ = _checked(arena, RESIDUAL, IW, SHIFT, tol, pb.product(st.d, IW))
            residuals += 1
        else:
            _, st, _, _ = _checked(arena, STEP, IW, SHIFT, tol, pb.product(st.p, IW))
    # the test's own residual of d in longdouble; its allowance: tol |rhs|, the rounding of the float64 product the kernel was handed
    # (n + 4 operations per entry on |dg d| + |u| sum |u d|) and the four roundings of r = rhs - (y inv_world + shift d)
    d, u, dg = st.d.astype(LD), pb.u.astype(LD), pb.dg.astype(LD)
    Ad = dg * d + u * (u * d).sum()
    r = pb.rhs.astype(LD) - (Ad + LD(SHIFT) * d)
    norm = lambda a: float(np.sqrt((a * a).sum()))  # noqa: E731
    e_op = C.gamma(N1 + 4) * (np.abs(dg * d) + np.abs(u) * np.abs(u * d).sum())
    allowed = tol * norm(pb.rhs) + norm(e_op) + 4 * C.U * (norm(pb.rhs) + norm(Ad) + SHIFT * norm(d))
    print(f"sr_cg_exact: continue after RESIDUAL: {int(st.sc[ITER])} iterations, {residuals} RESIDUAL calls, |r| / |rhs| {norm(r) / norm(pb.rhs):.3e} "
          f"(tol {tol:.0e}), allowed {allowed / norm(pb.rhs):.3e}")
    assert st.sc[ITER] > 3.0 and norm(r) <= allowed


# ---- the driver on operators the test supplies ---------------------------------------------------------------------------------------------
def _stub(case):
    from pynqs_amd import _native as N
    from pynqs_amd.sr import _FusedSR

    class StubSR(_FusedSR):
        _who = "StubSR"

        def __init__(self, A, shift, tol, max_iter, check_every):
            n = A.shape[0]
            grad = types.SimpleNamespace(N=N, module=None, H=1, flat=torch.zeros(n + 1, dtype=torch.float64, device="cuda"), shapes=[(n,)],
                                         params=[])
            self._setup(grad, n, shift, tol, max_iter, check_every)
            self.A = torch.from_numpy(A).cuda()
            self._onv = object()
            self.calls = []

        def _native_matvec(self, v, y):
            self.calls.append("d" if v is self.d else "p")
            y.copy_(self.A @ v)

    return StubSR(case.A, case.shift, case.tol, case.max_iter, case.check_every)


def _solve(sr, rhs):
    """(d on the host, warnings, products with p, products with d) of one solve"""
    sr.calls = []
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        d = sr.solve(torch.from_numpy(rhs).cuda()).cpu().numpy().copy()
    return d, [x for x in w if issubclass(x.category, RuntimeWarning)], sr.calls.count("p"), sr.calls.count("d")


def _true_residual(case, d):
    """(|rhs - (A + shift) d| / |rhs| in longdouble, the rounding of a float64 product A d on that scale: P 2^-52 | |A| |d| | / |rhs|)"""
    A, dl, rhs = case.A.astype(LD), d.astype(LD), case.rhs.astype(LD)
    r = rhs - (A @ dl + LD(case.shift) * dl)
    nr = float(np.sqrt((rhs * rhs).sum()))
    e = np.abs(A) @ np.abs(dl)
    return float(np.sqrt((r * r).sum())) / nr, A.shape[0] * 2.0 ** -52 * float(np.sqrt((e * e).sum())) / nr


def test_driver_converges_and_reports_the_true_residual():
    case = C.driver_case("convergent")
    sr = _stub(case)
    d, warned, steps, residuals = _solve(sr, case.rhs)
    true, slack = _true_residual(case, d)
    its = int(sr._sc[ITER].item())
    print(f"sr_cg_exact: driver convergent: {sr.iterations} iterations, {residuals - 1} restarts, {steps + residuals} products; residual "
          f"{sr.residual:.3e} reported, {true:.3e} in longdouble (tol {case.tol:.0e}, product rounding {slack:.1e})")
    assert sr.converged and not warned and sr.iterations == its and 0 < its <= case.max_iter - 20
    assert true <= case.tol + slack and abs(sr.residual - true) <= slack and sr.residual <= case.tol * (1 + 8 * C.U)
    assert residuals >= 1 and its <= steps < its + case.check_every


def test_driver_on_a_stagnating_solve_restarts_and_stops_at_max_iter():
    case = C.driver_case("stagnating")
    sr = _stub(case)
    d, warned, steps, residuals = _solve(sr, case.rhs)
    true, slack = _true_residual(case, d)
    restarts = residuals
    print(f"sr_cg_exact: driver stagnating: {sr.iterations} iterations, {residuals} products with d ({residuals - 1} restarts), {steps + residuals} products; "
          f"residual {sr.residual:.3e} reported, {true:.3e} in longdouble (tol {case.tol:.0e}, product rounding {slack:.1e})")
    assert len(warned) == 1 and "37 iterations" in str(warned[0].message)
    assert not sr.converged and sr.iterations == 37 == int(sr._sc[ITER].item())
    assert abs(sr.residual - true) <= slack and sr.residual > case.tol and true > case.tol
    assert residuals - 1 >= 2 and steps + residuals <= case.max_iter + restarts + 2
    # a second solve: the same bits and counts
    d2, warned2, steps2, residuals2 = _solve(sr, case.rhs)
    assert np.array_equal(d2, d) and (steps2, residuals2, len(warned2), sr.iterations) == (steps, residuals, 1, 37)


@pytest.mark.parametrize("name", ["indefinite", "nan"])
def test_driver_stops_on_a_breakdown_and_recovers(name):
    case, good = C.driver_case(name), C.driver_case("convergent")
    sr = _stub(case)
    d, warned, steps, residuals = _solve(sr, case.rhs)
    print(f"sr_cg_exact: driver {name}: {sr.iterations} iterations, {steps + residuals} products, BREAKDOWN {sr._sc[BREAKDOWN].item()}")
    assert sr._sc[BREAKDOWN].item() == 1.0  # the flag, not only its consequences
    assert not sr.converged and len(warned) == 1 and sr.iterations == 0
    assert steps <= case.check_every and residuals == 1
    if name == "indefinite":
        assert not d.any() and sr.residual == 1.0
    else:
        assert math.isnan(sr.residual)  # (not the 0 of a vanishing right-hand side)
    # the same object solves the convergent system afterwards: INIT clears BREAKDOWN
    sr.A, sr.diag_shift = torch.from_numpy(good.A).cuda(), good.shift
    d, warned, steps, residuals = _solve(sr, good.rhs)
    true, slack = _true_residual(good, d)
    assert sr.converged and not warned and sr._sc[BREAKDOWN].item() == 0.0 and true <= good.tol + slack


def test_driver_spends_exactly_max_iter_inside_a_batch():
    case = C.driver_case("short")
    sr = _stub(case)
    d, warned, steps, residuals = _solve(sr, case.rhs)
    true, slack = _true_residual(case, d)
    print(f"sr_cg_exact: driver short: {sr.iterations} iterations, {steps + residuals} products, residual {sr.residual:.3e}")
    assert (case.max_iter, case.check_every) == (11, 8)
    assert sr.iterations == 11 == int(sr._sc[ITER].item()) and steps == 11 and residuals == 1
    assert not sr.converged and len(warned) == 1 and abs(sr.residual - true) <= slack and sr.residual > case.tol
