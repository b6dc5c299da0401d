"""CPU side of the conjugate-gradient step and driver tests (tests/test_gpu_sr_cg.py): tests/cg_exact.py's fma_exact against
fractions.Fraction; its replay chained into a solver that reaches numpy's solution; a model of the step kernel (the kernel's order of
additions, written here from the header's description) that the replay accepts as it stands and refuses under each of eleven
mistakes, at the sizes and parameters of the GPU test; and the conditions the GPU driver tests rely on, proved on cg_replay."""
import math
from fractions import Fraction

import numpy as np
import pytest

import cg_exact as C
from cg_exact import BREAKDOWN, CONVERGED, DONE, INIT, ITER, PAP, RESIDUAL, RHO, RHS2, STEP, TRUE2


def _frac(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_fma_exact_is_the_fraction_form():
    g = np.random.default_rng(1)
    n = 4000
    a, b = g.standard_normal(n), g.standard_normal(n)
    M = g.integers(2 ** 52, 2 ** 53, n).astype(np.float64)  # whole numbers with 53 bits: one unit in the last place each
    cases = {
        "random": (a, b, g.standard_normal(n)),
        "scales": (a * 10.0 ** g.uniform(-30, 30, n), b * 10.0 ** g.uniform(-30, 30, n), g.standard_normal(n) * 10.0 ** g.uniform(-60, 60, n)),
        # c = -(a b) rounded, give or take a few units in the last place: the result is the low half of the product
        "cancellation": (a, b, -(a * b) * (1.0 + g.integers(-3, 4, n) * 2.0 ** -52)),
        # a b = +-1/2 exactly on a whole number: a tie, to the even neighbour; and a b = +-(1/2 - 2^-61), which rounds to 1/2 on its own:
        # the sum is 2^-61 below and above a tie, and an evaluation that rounds twice sends it to the even neighbour all the same
        "ties": (np.full(n, 0.5), np.ones(n), M),
        "negative ties": (np.full(n, -0.5), np.ones(n), M),
        "below ties": (np.full(n, 1.0 + 2.0 ** -30), np.full(n, 0.5 * (1.0 - 2.0 ** -30)), M),
        "above ties": (np.full(n, -(1.0 + 2.0 ** -30)), np.full(n, 0.5 * (1.0 - 2.0 ** -30)), M),
        # the product far below the last place of c, on either side: the rounding to odd must keep its sign
        "dust": (a * 2.0 ** -200, b, np.where(g.random(n) < 0.5, 1.0, 2.0 ** 52) * np.sign(g.standard_normal(n))),
        # results in the subnormal range and at its edge (the entry-by-entry path)
        "subnormal": (a[:400] * 2.0 ** -600, b[:400] * 2.0 ** -460, g.standard_normal(400) * 2.0 ** -1065),
        "subnormal cancel": (a[:400] * 2.0 ** -500, b[:400] * 2.0 ** -500, -(a[:400] * 2.0 ** -500) * (b[:400] * 2.0 ** -500)),
        "zeros": (np.array([0.0, -0.0, 0.0, -0.0, 3.0, 0.0, -0.0, 1.5, -1.5]), np.array([2.0, 2.0, -2.0, -2.0, 0.0, 0.0, 0.0, 2.0, 2.0]),
                  np.array([0.0, 0.0, -0.0, -0.0, 7.0, -5.0, 1.0, -3.0, 3.0])),
    }
    for name, (x, y, z) in cases.items():
        got = C.fma_exact(x, y, z)
        want = np.array([_frac(p, q, s) for p, q, s in zip(x, y, z)])
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        plain = x * y + z
        print(f"{name}: {int((plain != want).sum())} of {want.size} entries differ from the twice-rounded a*b + c")
    # most of these cases would catch a twice-rounded evaluation
    assert all(bool((cases[k][0] * cases[k][1] + cases[k][2] != C.fma_exact(*cases[k])).any()) for k in ("random", "cancellation", "above ties", "below ties"))
    # the IEEE sign of an exact zero: -0 only from (-0) + (-0); a cancellation gives +0
    x, y, z = cases["zeros"]
    res = C.fma_exact(x, y, z)
    assert res.tolist() == [0.0, 0.0, 0.0, 0.0, 7.0, -5.0, 1.0, 0.0, 0.0]
    assert np.signbit(res[res == 0.0]).tolist() == [False, False, True, False, False, False]  # only (0 x -2) + (-0)
    # scalars broadcast, NaN goes through
    assert C.fma_exact(2.0, np.array([1.0, math.nan]), 1.0).tolist()[0] == 3.0 and math.isnan(C.fma_exact(2.0, np.array([1.0, math.nan]), 1.0)[1])


def test_sum_bound_brackets_sums_in_any_order():
    g = np.random.default_rng(2)
    for n in (1, 5, 1025, 20000):
        a, b = g.standard_normal(n), g.standard_normal(n) * 10.0 ** g.uniform(-3, 3, n)
        hi, lo, bound = C.sum_bound(a, b)
        ex = sum(Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, b))
        assert hi == float(ex) and abs(float(ex - Fraction(hi)) - lo) <= 2.0 ** -100 * abs(hi)
        m = (n + 1023) // 1024 + 10
        assert bound >= C.gamma(m) * float(sum(abs(Fraction(float(x)) * Fraction(float(y))) for x, y in zip(a, b)))
        assert bound <= 1.0001 * C.gamma(m) * float(np.abs(a * b).sum())
        assert C.scalar_ratio(_kernel_sum(a, b), a, b) <= 1.0 and C.scalar_ratio(float(a[::-1] @ b[::-1]), a, b) <= 1.0
        assert C.scalar_ratio(hi * (1 + 40 * C.gamma(m)) + 1e-300, np.abs(a), np.abs(b)) > 1.0  # (all terms of one sign: the bound is relative)
    assert math.isnan(C.sum_bound(np.array([1.0, math.nan]), np.ones(2))[0])
    assert C.scalar_ratio(math.nan, np.array([1.0, math.nan]), np.ones(2)) == 0.0 and C.scalar_ratio(1.0, np.array([1.0, math.nan]), np.ones(2)) == math.inf
    assert C.scalar_ratio(math.nan, np.ones(2), np.ones(2)) == math.inf


# ---- a solver chained from the replay ------------------------------------------------------------------------------------------------------
def _chained_solve(A, rhs, shift, tol, inv_world, limit):
    """INIT, then STEPs until DONE, with expect_* for the vectors and numpy dot products for the scalars"""
    st = C.expect_init(rhs)
    d, r, p = st["d"], st["r"], st["p"]
    sc = np.zeros(C.NSC)
    sc[RHO] = sc[RHS2] = sc[TRUE2] = float(rhs @ rhs)
    while sc[DONE] == 0.0 and sc[ITER] < limit:
        y = (A @ p) / inv_world
        after = sc.copy()
        ap = C.fma_exact(shift, p, y * inv_world)
        after[PAP] = float(p @ ap)
        r2 = C.expect_step(y, d, r, p, sc, after, inv_world, shift)["r"]  # (r' needs PAP' alone)
        after[RHO] = float(r2 @ r2)
        out = C.expect_step(y, d, r, p, sc, after, inv_world, shift)
        assert C.same_bits(out["r"], r2) and C.same_bits(out["y"], ap)
        d, r, p = out["d"], out["r"], out["p"]
        after[ITER] += 1
        after[DONE] = 1.0 if C.within_tol(after[RHO], sc[RHS2], tol) else 0.0
        sc = after
    y = (A @ d) / inv_world
    after = sc.copy()
    res = rhs - C.fma_exact(shift, d, y * inv_world)
    after[TRUE2] = float(res @ res)
    out = C.expect_residual(y, rhs, d, p, sc, after, inv_world, shift, tol)
    assert C.same_bits(out["r"], res)
    return d, int(sc[ITER]), math.sqrt(after[TRUE2] / sc[RHS2])


@pytest.mark.parametrize("inv_world,shift", C.PARAMS)
def test_the_replay_solves_a_system(inv_world, shift):
    n, cond, tol = 200, 100.0, 1e-10
    A = C.spectral(10.0 ** np.linspace(-2.0, 0.0, n), 3)
    rhs = np.random.default_rng(4).standard_normal(n)
    assert np.linalg.cond(A + shift * np.eye(n)) <= cond * (1 + 1e-9)
    d, its, true = _chained_solve(A, rhs, shift, tol, inv_world, 400)
    want = np.linalg.solve(A + shift * np.eye(n), rhs)
    dist = float(np.linalg.norm(d - want) / np.linalg.norm(want))
    print(f"inv_world {inv_world:.3g} shift {shift}: {its} iterations, true residual {true:.2e}, |d - solve| / |solve| {dist:.2e}")
    assert 20 < its < 400 and true <= 2 * tol and dist <= tol * cond


# ---- a model of the kernel, and the mistakes the replay must refuse ------------------------------------------------------------------------
def _kernel_sum(a, b) -> float:
    """sum a_k b_k as the kernel adds it: thread t runs fma over k = t, t + 1024, ..., then a tree over the 1024 threads"""
    n = a.size
    acc = np.zeros(C.BLOCK)
    for k0 in range(0, n, C.BLOCK):
        m = min(C.BLOCK, n - k0)
        acc[:m] = C.fma_exact(a[k0:k0 + m], b[k0:k0 + m], acc[:m])
    w = C.BLOCK // 2
    while w:
        acc[:w] = acc[:w] + acc[w:2 * w]
        w //= 2
    return float(acc[0])


MUTANTS = ("no inv_world", "shift on y", "beta inverted", "alpha from the new rho", "residual keeps p", "residual keeps rho",
           "done step writes y", "done step counts", "loop stops at the last full stride", "loop runs to the next full stride",
           "breakdown updates d")


def _model(mode, st, n, inv_world, shift, tol, mutant=None):
    """One call of the kernel on buffers of 1024 ceil(n / 1024) entries whose tail past n is NaN (the guard words), with one mistake"""
    st = st.copy()
    sc = st.sc
    lim = n
    if mutant == "loop stops at the last full stride":
        lim = n // C.BLOCK * C.BLOCK
    elif mutant == "loop runs to the next full stride":
        lim = -(-n // C.BLOCK) * C.BLOCK
    s = slice(0, lim)
    y, rhs, d, r, p = st.y, st.rhs, st.d, st.r, st.p
    scaled = lambda: y[s] * (1.0 if mutant == "no inv_world" else inv_world)  # noqa: E731
    with np.errstate(all="ignore"):
        if mode == INIT:
            d[s], r[s], p[s] = 0.0, rhs[s], rhs[s]
            rho = _kernel_sum(rhs[s], rhs[s])
            stop = 1.0 if rho == 0.0 else 0.0
            sc[:] = [rho, rho, stop, 0.0, rho, 0.0, stop, 0.0]
        elif mode == STEP:
            if sc[DONE] != 0.0:
                if mutant == "done step writes y":
                    y[s] = C.fma_exact(shift, p[s], scaled())
                if mutant == "done step counts":
                    sc[ITER] += 1.0
                return st
            ap = C.fma_exact(shift, y[s] if mutant == "shift on y" else p[s], scaled())
            y[s] = ap
            pap = _kernel_sum(p[s], ap)
            if not pap > 0.0:
                sc[PAP], sc[DONE], sc[BREAKDOWN] = pap, 1.0, 1.0
                if mutant == "breakdown updates d":
                    d[s] = C.fma_exact(sc[RHO] / pap, p[s], d[s])
                return st
            rho = sc[RHO]
            alpha = np.float64(rho) / np.float64(pap)
            r2 = C.fma_exact(-alpha, ap, r[s])
            rho2 = _kernel_sum(r2, r2)
            d[s] = C.fma_exact(np.float64(rho2) / np.float64(pap) if mutant == "alpha from the new rho" else alpha, p[s], d[s])
            r[s] = r2
            beta = np.float64(rho) / np.float64(rho2) if mutant == "beta inverted" else np.float64(rho2) / np.float64(rho)
            p[s] = C.fma_exact(beta, p[s], r2)
            sc[RHO], sc[PAP] = rho2, pap
            sc[ITER] += 1.0
            if rho2 <= tol * tol * sc[RHS2]:
                sc[DONE] = 1.0
        else:
            rk = rhs[s] - C.fma_exact(shift, d[s], scaled())
            r[s] = rk
            rr = _kernel_sum(rk, rk)
            ok = bool(rr <= tol * tol * sc[RHS2])
            if not ok and mutant != "residual keeps p":
                p[s] = rk
            sc[TRUE2] = rr
            sc[CONVERGED] = sc[DONE] = 1.0 if ok else 0.0
            if not ok and mutant != "residual keeps rho":
                sc[RHO] = rr
    return st


def _padded(n, **vectors):
    L = -(-n // C.BLOCK) * C.BLOCK
    out = {}
    for k in C.VECTORS:
        out[k] = np.full(L, np.nan)
        out[k][:n] = vectors.get(k, 0.0)
    return C.State(sc=np.zeros(C.NSC), **out)


def _head(st, n):
    return C.State(*(getattr(st, k)[:n] for k in C.VECTORS), st.sc)


def _caught(mode, before, after, n, inv_world, shift, tol):
    """the replay's problems with the call, the guard words among them"""
    v = C.verify_call(mode, _head(before, n), _head(after, n), inv_world, shift, tol)
    out = list(v.problems)
    if not all(bool(np.isnan(getattr(after, k)[n:]).all()) for k in C.VECTORS):
        out.append("a guard word was overwritten")
    return out


@pytest.mark.parametrize("inv_world,shift", C.PARAMS, ids=lambda v: f"{v:.3g}")
@pytest.mark.parametrize("n", C.SIZES)
def test_the_replay_accepts_the_kernel_and_refuses_each_mistake(n, inv_world, shift):
    """INIT, three STEPs, RESIDUAL, two STEPs of the GPU test's sequence on the model: every call passes as it stands; each mistake, put
    into the one call where it acts, is refused -- or, where it cannot change anything (inv_world = 1, shift = 0, n a multiple of the
    stride), leaves the faithful call's bits."""
    tol = C.SEQ_TOL
    pb = C.step_problem(n)
    st = _padded(n, rhs=pb.rhs)
    calls = []  # (mode, before, after)
    worst = 0.0

    def run(mode, st):
        if mode != INIT:
            st = st.copy()
            st.y[:n] = pb.product(st.p[:n] if mode == STEP else st.d[:n], inv_world)
        after = _model(mode, st, n, inv_world, shift, tol)
        calls.append((mode, st, after))
        return after

    for mode in (INIT, STEP, STEP, STEP, RESIDUAL, STEP, STEP):
        st = run(mode, st)
        v = C.verify_call(mode, _head(calls[-1][1], n), _head(st, n), inv_world, shift, tol)
        assert _caught(mode, calls[-1][1], st, n, inv_world, shift, tol) == [], (mode, v.problems)
        worst = max(worst, v.worst)
    print(f"np {n} inv_world {inv_world:.3g} shift {shift}: the model's worst scalar error / bound {worst:.3g}")
    if n >= 1023:
        assert st.sc[ITER] == 5.0 and st.sc[DONE] == 0.0 and calls[4][2].sc[CONVERGED] == 0.0  # every call was a live one
    live = [c for c in calls if c[0] == STEP and c[1].sc[DONE] == 0.0]
    assert live
    init, step, resid = calls[0], live[min(2, len(live) - 1)], calls[4]
    done = step[1].copy()
    done.sc[DONE] = 1.0
    broken = step[1].copy()
    broken.y[:n] = -np.abs(broken.y[:n]) * np.sign(broken.p[:n]) - broken.p[:n]  # p.Ap < 0
    restart = resid[1].copy()  # a RESIDUAL that must restart whatever the size: a right-hand side the iterate is far from
    restart.rhs[:n] = restart.rhs[:n] + 1.0
    where = {"no inv_world": [step, resid], "shift on y": [step], "beta inverted": [step], "alpha from the new rho": [step],
             "residual keeps p": [(RESIDUAL, restart, None)], "residual keeps rho": [(RESIDUAL, restart, None)],
             "done step writes y": [(STEP, done, None)], "done step counts": [(STEP, done, None)],
             "loop stops at the last full stride": [init, step, resid], "loop runs to the next full stride": [init, step, resid],
             "breakdown updates d": [(STEP, broken, None)]}
    assert set(where) == set(MUTANTS)
    idle = {"no inv_world": inv_world == 1.0, "shift on y": shift == 0.0, "loop stops at the last full stride": n % C.BLOCK == 0,
            "loop runs to the next full stride": n % C.BLOCK == 0}
    for mutant in MUTANTS:
        for mode, before, _ in where[mutant]:
            good = _model(mode, before, n, inv_world, shift, tol)
            assert _caught(mode, before, good, n, inv_world, shift, tol) == [], (mutant, "the faithful call")
            bad = _model(mode, before, n, inv_world, shift, tol, mutant)
            if idle.get(mutant, False):
                assert all(C.same_bits(getattr(good, k), getattr(bad, k)) for k in C.VECTORS + ("sc",)), mutant
                continue
            found = _caught(mode, before, bad, n, inv_world, shift, tol)
            assert found, f"np {n}: '{mutant}' in mode {mode} went unnoticed"
    # the branches those calls were meant to reach
    assert _model(STEP, broken, n, inv_world, shift, tol).sc[BREAKDOWN] == 1.0
    assert _model(RESIDUAL, restart, n, inv_world, shift, tol).sc[CONVERGED] == 0.0


# ---- what the GPU driver tests rely on, on the float64 replay ----------------------------------------------------------------------------
def test_driver_inputs_meet_their_conditions():
    c = C.driver_case("stagnating")
    r = c.replay()
    print(f"stagnating: {r.iterations} iterations, DONE by the recurrence at {r.done_at}, {r.restarts} restarts, {r.products} products; true "
          f"residuals {[f'{t:.2e}' for _, t in r.true]}")
    assert (c.max_iter, c.check_every, c.shift) == (37, 8, 0.0)
    assert r.iterations == c.max_iter and not r.converged and not r.breakdown
    assert r.restarts >= 2 and r.residuals == r.restarts + 1
    # the true residual misses the tolerance by a factor of four or more at every check: no rounding difference turns it into convergence
    assert all(t >= 4 * c.tol for _, t in r.true) and len(r.true) == r.residuals
    # the recurrence meets the tolerance at the last step of a batch only, and by a wide margin on either side: no product is spent on
    # a step that is a no-op, so products = iterations + RESIDUAL calls
    assert all(k % c.check_every == 0 for k in r.done_at) and len(r.done_at) == r.restarts
    for k, v in enumerate(r.recurrence, 1):
        assert v <= c.tol / 100 if k in r.done_at else v >= 4 * c.tol, (k, v)
    assert r.products == r.iterations + r.residuals <= c.max_iter + r.residuals + 2
    # the spectrum is what driver_case says
    w = np.linalg.eigvalsh(c.A)
    assert abs(w.min() - 3e-6) <= 1e-12 and abs(w.max() - 1.0) <= 1e-12

    c = C.driver_case("convergent")
    r = c.replay()
    print(f"convergent: {r.iterations} of {c.max_iter} iterations, {r.restarts} restarts, {r.products} products, true residual {r.true[-1][1]:.2e}")
    assert r.converged and not r.breakdown and r.iterations + 20 <= c.max_iter and r.true[-1][1] <= c.tol
    want = np.linalg.solve(c.A + c.shift * np.eye(C.ORDER), c.rhs)
    assert float(np.linalg.norm(r.d - want)) <= 1e-8 * float(np.linalg.norm(want))

    for name in ("indefinite", "nan"):
        c = C.driver_case(name)
        r = c.replay()
        print(f"{name}: {r.iterations} iterations, {r.products} products, breakdown {r.breakdown}")
        assert r.breakdown and not r.converged and r.iterations == 0 and r.products <= c.check_every + 1 and r.restarts == 0
        assert name == "nan" or not r.d.any()
    assert int(np.isnan(C.driver_case("nan").rhs).sum()) == 1

    c = C.driver_case("short")
    r = c.replay()
    full = C.driver_case("convergent").replay()
    print(f"short: {r.iterations} iterations, {r.products} products, true residual {r.true[-1][1]:.2e}")
    assert (c.max_iter, c.check_every) == (11, 8) and r.iterations == 11 < full.iterations and not r.converged and r.true[-1][1] >= 4 * c.tol
    assert r.products == 12 and r.done_at == []
