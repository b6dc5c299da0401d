"""Host replay of the conjugate-gradient step kernel behind pynqs_rbm_sr_cg_step (include/pynqs_amd.h, "pynqs_rbm_sr_cg_step";
rbm_sr_cg_kernel in pynqs_amd/csrc/kernels_rbm_sr.hip) and of the driver loop of pynqs_amd.sr._FusedSR.solve.  (No tests here.)

The step kernel does not depend on the operator: y is an input.  Every vector entry it writes is ONE correctly rounded operation (a
product, a difference or a fused multiply-add) of numbers the caller knows -- the input vectors and the kernel's own scalars -- so the
vectors are replayed bit for bit:
    INIT      d = 0,  r = p = rhs
    STEP      Ap_k = fma(shift, p_k, fl(y_k inv_world))  (left in y),   alpha = fl(RHO / PAP'),   d_k' = fma(alpha, p_k, d_k),
              r_k' = fma(-alpha, Ap_k, r_k),   beta = fl(RHO' / RHO),   p_k' = fma(beta, p_k, r_k');
              nothing when DONE is set;  only y when not (PAP' > 0): breakdown
    RESIDUAL  r_k = fl(rhs_k - fma(shift, d_k, fl(y_k inv_world))),   p = r unless TRUE2' <= (tol tol) RHS2
(X: the scalar before the call, X': after it).  The scalars are sums over the kernel's own vectors -- RHO = r.r, PAP = p.Ap,
TRUE2 = r.r, RHS2 = rhs.rhs -- in an order the replay does not restate: thread t of 1024 runs acc = fma(a_k, b_k, acc) over k = t,
t + 1024, ..., then a tree of ten levels over LDS.  Each of the m = ceil(np / 1024) + 10 operations on the way of a term to the result
rounds once, so
    |sum - exact| <= gamma_m sum_k |a_k b_k|,     gamma_m = m u / (1 - m u),   u = 2^-53,
whatever the order inside the tree (sum_bound; derived from the kernel's structure, not measured).  The flags follow exactly from the
kernel's own scalars in float64:
    STEP      DONE' = (RHO' <= (tol tol) RHS2),  ITER' = ITER + 1;   breakdown (not PAP' > 0): DONE' = BREAKDOWN' = 1, RHO and ITER kept
    RESIDUAL  DONE' = CONVERGED' = (TRUE2' <= (tol tol) RHS2),  RHO' = TRUE2' when not; ITER, BREAKDOWN, PAP, RHS2 kept
    INIT      RHO = RHS2 = TRUE2 = rhs.rhs,  DONE = CONVERGED = (that sum == 0),  ITER = PAP = BREAKDOWN = 0.

fma_exact is a*b + c rounded once: Dekker's exact product and Boldo and Melquiond's sum through rounding to odd ("Emulation of FMA and
correctly rounded sums: proved algorithms using rounding to odd", IEEE TC 57, 2008) where no operand is near the ends of the
exponent range, fractions.Fraction entry by entry elsewhere (with the IEEE sign of an exact zero); tests/test_cg_exact.py holds both
paths to float(Fraction(a) * Fraction(b) + Fraction(c)).

cg_replay is a plain float64 conjugate-gradient iteration under the driver's control flow (batches of check_every steps that turn into
no-ops once DONE is set, the true residual when DONE, the restart from it, the forced DONE when max_iter is spent): it serves to choose
the driver tests' operators and to prove on the CPU what they rely on."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

RHO, RHS2, DONE, ITER, TRUE2, PAP, CONVERGED, BREAKDOWN, NSC = range(9)  # include/pynqs_amd.h: PYNQS_SR_*
INIT, STEP, RESIDUAL = 0, 1, 2
BLOCK = 1024  # kSrCgBlock
U = 2.0 ** -53
VECTORS = ("y", "rhs", "d", "r", "p")


# ---- a*b + c, rounded once -------------------------------------------------------------------------------------------------------------
def _fma_fraction(a: float, b: float, c: float) -> float:
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c  # NaN and infinities: no rounding to speak of
    s = Fraction(a) * Fraction(b) + Fraction(c)
    if s == 0:  # IEEE 754, round to nearest: -0 only when the product and c are both -0; an exact cancellation gives +0
        prod_neg = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, b) < 0)
        return -0.0 if (a == 0 or b == 0) and c == 0 and prod_neg and math.copysign(1.0, c) < 0 else 0.0
    return float(s)  # (int / int: correctly rounded, subnormals included)


def _two_sum(x, y):
    s = x + y
    bb = s - x
    return s, (x - (s - bb)) + (y - bb)


def _split(x):
    t = 134217729.0 * x  # 2^27 + 1
    hi = t - (t - x)
    return hi, x - hi


def two_prod(a, b):
    """(h, l) with h + l = a b exactly (Dekker), for operands away from the ends of the exponent range"""
    h = a * b
    a1, a2 = _split(a)
    b1, b2 = _split(b)
    return h, a2 * b2 - (((h - a1 * b1) - a2 * b1) - a1 * b2)


_LO, _HI = 2.0 ** -400, 2.0 ** 400


def _in_range(x):
    ax = np.abs(x)
    return (ax >= _LO) & (ax <= _HI)


def fma_exact(a, b, c) -> np.ndarray:
    """elementwise a*b + c with ONE rounding (float64), operands broadcast against each other"""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    shape = a.shape
    a, b, c = a.reshape(-1), b.reshape(-1), c.reshape(-1)
    fast = _in_range(a) & _in_range(b) & (_in_range(c) | (c == 0))
    out = np.empty(a.shape, dtype=np.float64)
    if fast.any():
        af, bf, cf = a[fast], b[fast], c[fast]
        with np.errstate(all="ignore"):
            uh, ul = two_prod(af, bf)
            th, tl = _two_sum(cf, uh)
            s, e = _two_sum(tl, ul)  # v = tl + ul rounded to odd: when inexact, the neighbour of the sum whose last bit is set
            bits = s.view(np.int64)
            fix = (e != 0) & ((bits & 1) == 0)
            away = (e > 0) == (s > 0)  # the exact sum lies beyond s: one step up in magnitude; else one step down
            v = np.where(fix, (bits + np.where(away, 1, -1)).view(np.float64), s)
            out[fast] = th + v
    easy = ~fast & ((a == 0) | (b == 0)) & np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & (c != 0)  # (+-0) + c = c
    out[easy] = c[easy]
    for k in np.flatnonzero(~fast & ~easy):
        out[k] = _fma_fraction(float(a[k]), float(b[k]), float(c[k]))
    return out.reshape(shape)


# ---- the scalars: exact sums of products and their a-priori bound ------------------------------------------------------------------------
def gamma(m: int) -> float:
    return m * U / (1.0 - m * U)


def sum_bound(a, b):
    """(hi, lo, bound): sum_k a_k b_k = hi + lo to 2^-106 of it (hi its correctly rounded value), and the kernel's a-priori error bound
    gamma_m sum_k |a_k b_k| with m = ceil(np / 1024) + 10.  NaN in, NaN out."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    m = (a.size + BLOCK - 1) // BLOCK + 10
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return math.nan, 0.0, math.nan
    if bool(((_in_range(a) | (a == 0)) & (_in_range(b) | (b == 0))).all()):
        h, l = two_prod(a, b)
        terms = np.concatenate([h, l]).tolist()
        hi = math.fsum(terms)
        lo = math.fsum(terms + [-hi])
        mag = math.fsum(np.abs(h).tolist()) * (1.0 + 2.0 ** -50)  # (|h| is |a b| rounded: 2^-53 of it)
    else:
        fr = [Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, b)]
        ex = sum(fr)
        hi = float(ex)
        lo = float(ex - Fraction(hi))
        mag = float(sum(abs(t) for t in fr)) * (1.0 + 2.0 ** -50)
    return hi, lo, gamma(m) * mag


def scalar_ratio(got: float, a, b) -> float:
    """|got - sum a b| / bound (0 when both vanish; inf when got is off a vanishing bound or not a number)"""
    hi, lo, bound = sum_bound(a, b)
    if math.isnan(hi):
        return 0.0 if math.isnan(got) else math.inf
    if not math.isfinite(got):
        return math.inf
    err = abs((got - hi) - lo)
    return err / bound if bound > 0 else (0.0 if err == 0 else math.inf)


# ---- the vectors -------------------------------------------------------------------------------------------------------------------------
def expect_init(rhs):
    rhs = np.asarray(rhs, dtype=np.float64)
    return {"d": np.zeros_like(rhs), "r": rhs.copy(), "p": rhs.copy()}


def expect_step(y, d, r, p, sc_before, sc_after, inv_world: float, shift: float):
    """{y, d, r, p} after a STEP on these inputs, from the kernel's scalars before and after the call"""
    if sc_before[DONE] != 0.0:
        return {"y": y.copy(), "d": d.copy(), "r": r.copy(), "p": p.copy()}
    ap = fma_exact(shift, p, y * inv_world)
    if not (sc_after[PAP] > 0.0):
        return {"y": ap, "d": d.copy(), "r": r.copy(), "p": p.copy()}
    with np.errstate(all="ignore"):
        alpha = np.float64(sc_before[RHO]) / np.float64(sc_after[PAP])
        beta = np.float64(sc_after[RHO]) / np.float64(sc_before[RHO])
    r2 = fma_exact(-alpha, ap, r)
    return {"y": ap, "d": fma_exact(alpha, p, d), "r": r2, "p": fma_exact(beta, p, r2)}


def within_tol(value: float, rhs2: float, tol: float) -> bool:
    return bool(np.float64(value) <= np.float64(tol) * np.float64(tol) * np.float64(rhs2))


def expect_residual(y, rhs, d, p, sc_before, sc_after, inv_world: float, shift: float, tol: float):
    """{r, p} after a RESIDUAL"""
    r = rhs - fma_exact(shift, d, y * inv_world)
    return {"r": r, "p": p.copy() if within_tol(sc_after[TRUE2], sc_before[RHS2], tol) else r.copy()}


def same_bits(a, b) -> bool:
    """the same float64 bits entry by entry (every NaN counts as the same NaN)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))


@dataclass
class State:
    """the five vectors and the eight scalars of a solve, as host arrays"""
    y: np.ndarray
    rhs: np.ndarray
    d: np.ndarray
    r: np.ndarray
    p: np.ndarray
    sc: np.ndarray

    def copy(self) -> "State":
        return State(*(getattr(self, k).copy() for k in VECTORS + ("sc",)))


@dataclass
class Verdict:
    problems: list = field(default_factory=list)
    ratios: dict = field(default_factory=dict)  # scalar name -> error / bound

    @property
    def worst(self) -> float:
        return max(self.ratios.values(), default=0.0)


def verify_call(mode: int, before: State, after: State, inv_world: float, shift: float, tol: float) -> Verdict:
    """Everything one call of pynqs_rbm_sr_cg_step must have done to `before` to give `after`: the vectors bit for bit (those the mode
    must not touch included), the sums within sum_bound of the exact sums over the vectors in `after`, the flags and the counter
    exactly."""
    v = Verdict()
    b, a = before.sc, after.sc
    keep = lambda *slots: [s for s in range(NSC) if s not in slots]  # noqa: E731
    names = ("RHO", "RHS2", "DONE", "ITER", "TRUE2", "PAP", "CONVERGED", "BREAKDOWN")

    def vectors(want):
        for k in VECTORS:
            w = want.get(k, getattr(before, k))
            if not same_bits(getattr(after, k), w):
                bad = np.flatnonzero(~((getattr(after, k) == w) | (np.isnan(getattr(after, k)) & np.isnan(w))))
                v.problems.append(f"{k}: {bad.size} of {w.size} entries differ, the first at {int(bad[0]) if bad.size else -1}")

    def scalars_kept(slots):
        for s in slots:
            if not same_bits(a[s:s + 1], b[s:s + 1]):
                v.problems.append(f"{names[s]} changed: {b[s]!r} -> {a[s]!r}")

    def flag(slot, want):
        if not (a[slot] == (1.0 if want else 0.0)):
            v.problems.append(f"{names[slot]} is {a[slot]!r}, expected {1.0 if want else 0.0}")

    def total(slot, x, z):
        v.ratios[names[slot]] = q = scalar_ratio(float(a[slot]), x, z)
        if not q <= 1.0:
            v.problems.append(f"{names[slot]} = {a[slot]!r} is {q:.3g} bounds from the exact sum")

    if mode == INIT:
        vectors(expect_init(before.rhs))
        total(RHO, after.r, after.r)
        for s in (RHS2, TRUE2):
            if not same_bits(a[s:s + 1], a[RHO:RHO + 1]):
                v.problems.append(f"{names[s]} is not RHO after INIT")
        zero = bool(a[RHO] == 0.0)
        flag(DONE, zero), flag(CONVERGED, zero), flag(BREAKDOWN, False)
        if not (a[ITER] == 0.0 and a[PAP] == 0.0):
            v.problems.append("ITER or PAP not cleared by INIT")
    elif mode == STEP:
        vectors(expect_step(before.y, before.d, before.r, before.p, b, a, inv_world, shift))
        if b[DONE] != 0.0:
            scalars_kept(range(NSC))
        elif not (a[PAP] > 0.0):
            total(PAP, before.p, after.y)
            scalars_kept(keep(PAP, DONE, BREAKDOWN))
            flag(DONE, True), flag(BREAKDOWN, True)
        else:
            total(PAP, before.p, after.y)
            total(RHO, after.r, after.r)
            scalars_kept(keep(PAP, RHO, DONE, ITER, BREAKDOWN))
            flag(DONE, within_tol(a[RHO], b[RHS2], tol)), flag(BREAKDOWN, b[BREAKDOWN] != 0.0)
            if not (a[ITER] == b[ITER] + 1.0 and a[ITER] == math.floor(a[ITER])):
                v.problems.append(f"ITER {b[ITER]!r} -> {a[ITER]!r}")
    else:
        vectors(expect_residual(before.y, before.rhs, before.d, before.p, b, a, inv_world, shift, tol))
        total(TRUE2, after.r, after.r)
        ok = within_tol(a[TRUE2], b[RHS2], tol)
        flag(DONE, ok), flag(CONVERGED, ok)
        if ok:
            scalars_kept(keep(TRUE2, DONE, CONVERGED))
        else:
            scalars_kept(keep(TRUE2, DONE, CONVERGED, RHO))
            if not same_bits(a[RHO:RHO + 1], a[TRUE2:TRUE2 + 1]):
                v.problems.append(f"RHO = {a[RHO]!r} is not TRUE2 = {a[TRUE2]!r} after a restart")
    return v


# ---- the driver's control flow on a plain float64 iteration --------------------------------------------------------------------------------
@dataclass
class Replay:
    iterations: int
    restarts: int      # RESIDUAL calls that did not end the solve: the iteration went on from the true residual
    residuals: int     # RESIDUAL calls (products with d)
    products: int      # all products, those of steps that were no-ops included
    converged: bool
    breakdown: bool
    recurrence: list   # per iteration: sqrt(rho / |rhs|^2)
    true: list         # per RESIDUAL call: (iterations so far, sqrt(|r|^2 / |rhs|^2))
    done_at: list      # iterations at which the recurrence set DONE
    d: np.ndarray


def cg_replay(A, rhs, shift: float, tol: float, max_iter: int, check_every: int) -> Replay:
    """_FusedSR.solve on one rank with numpy float64 in the place of the kernels"""
    A, rhs = np.asarray(A, dtype=np.float64), np.asarray(rhs, dtype=np.float64)
    d, r, p = np.zeros_like(rhs), rhs.copy(), rhs.copy()
    rho = rhs2 = float(r @ r)
    true2 = rho
    done = conv = rho == 0.0
    bd = False
    it = products = restarts = residuals = used = 0
    rec, true, done_at = [], [], []
    op = lambda v: A @ v + shift * v  # noqa: E731
    while not conv:
        left = max_iter - used
        if done:
            products += 1
            residuals += 1
            r = rhs - op(d)
            true2 = float(r @ r)
            conv = done = true2 <= tol * tol * rhs2
            if not conv:
                p, rho = r.copy(), true2
            true.append((it, math.sqrt(true2 / rhs2) if rhs2 > 0 and true2 == true2 else math.nan))
            if conv or left <= 0 or bd:
                break
            restarts += 1
            continue
        if left <= 0:
            done = True
            continue
        for _ in range(min(check_every, left)):
            products += 1
            if done:
                continue
            ap = op(p)
            pap = float(p @ ap)
            if not pap > 0.0:
                bd = done = True
                continue
            alpha = rho / pap
            d = d + alpha * p
            r = r - alpha * ap
            rho2 = float(r @ r)
            p = r + (rho2 / rho) * p
            rho = rho2
            it += 1
            rec.append(math.sqrt(rho / rhs2))
            if rho <= tol * tol * rhs2:
                done = True
                done_at.append(it)
        used = it
    return Replay(it, restarts, residuals, products, bool(conv), bd, rec, true, done_at, d)


# ---- seeded inputs shared by tests/test_cg_exact.py and tests/test_gpu_sr_cg.py ------------------------------------------------------------
SIZES = (1, 2, 1023, 1024, 1025, 2049, 58320, 100003)  # around the stride of 1024; the largest P_real served; an odd length past it
PARAMS = ((1.0, 0.02), (0.5, 1e-3), (1.0 / 3.0, 0.0))  # (inv_world, shift)
SEQ_TOL = 1e-9  # of the step sequences: not met within their sixteen steps from np = 1023 on


@dataclass
class StepProblem:
    """rhs and a diagonal-plus-rank-one SPD operator A = diag(dg) + u u^T (eigenvalues in 0.1 ... 11) for the step sequences"""
    rhs: np.ndarray
    dg: np.ndarray
    u: np.ndarray

    def product(self, v, inv_world: float) -> np.ndarray:
        """what the step is handed in y: the ranks' SUM of A v (any float64 vector would do)"""
        return (self.dg * v + self.u * float(self.u @ v)) / inv_world


def step_problem(n: int) -> StepProblem:
    g = np.random.default_rng([11, n])
    u = g.standard_normal(n)
    return StepProblem(g.standard_normal(n), 10.0 ** g.uniform(-1.0, 1.0, n), u / math.sqrt(float(u @ u)))


def spectral(lam, seed: int) -> np.ndarray:
    """Q diag(lam) Q^T with a seeded orthogonal Q, symmetric to the last bit"""
    lam = np.asarray(lam, dtype=np.float64)
    Q, _ = np.linalg.qr(np.random.default_rng([13, seed, lam.size]).standard_normal((lam.size, lam.size)))
    A = (Q * lam[None, :]) @ Q.T
    return 0.5 * (A + A.T)


@dataclass
class DriverCase:
    A: np.ndarray
    rhs: np.ndarray
    shift: float
    tol: float
    max_iter: int
    check_every: int

    def replay(self) -> Replay:
        return cg_replay(self.A, self.rhs, self.shift, self.tol, self.max_iter, self.check_every)


ORDER = 300
STAGNATING_EIGENVALUES = (1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 3e-6)


def driver_case(name: str) -> DriverCase:
    """The operators of the driver tests (tests/test_cg_exact.py proves what is claimed here on cg_replay):
      convergent  eigenvalues 0.01 ... 1, shift 0.02, tol 1e-10: converges with iterations to spare
      stagnating  eight distinct eigenvalues, the smallest 3e-6, shift 0: the recurrence meets tol = 2e-12 after sixteen iterations and
                  after every eight from then on -- at the last step of a batch of check_every = 8 --, while the true residual
                  stays near 3e-11 |rhs| (the rounding of d on the smallest eigenvalue): every check restarts
      indefinite  A = -I, shift 0: p.Ap < 0 at the first step
      nan         the convergent operator with one NaN in rhs
      short       the convergent operator with max_iter = 11, check_every = 8: the limit falls inside the second batch"""
    rhs = np.random.default_rng([13, 7]).standard_normal(ORDER)
    if name == "stagnating":
        lam = np.array([STAGNATING_EIGENVALUES[k % 8] for k in range(ORDER)])
        return DriverCase(spectral(lam, 2), rhs, 0.0, 2e-12, 37, 8)
    if name == "indefinite":
        return DriverCase(-np.eye(ORDER), rhs, 0.0, 1e-10, 100, 8)
    A = spectral(10.0 ** np.random.default_rng([13, 5]).uniform(-2.0, 0.0, ORDER), 1)
    if name == "convergent":
        return DriverCase(A, rhs, 0.02, 1e-10, 120, 8)
    if name == "nan":
        bad = rhs.copy()
        bad[ORDER // 3] = np.nan
        return DriverCase(A, bad, 0.02, 1e-10, 120, 8)
    assert name == "short"
    return DriverCase(A, rhs, 0.02, 1e-10, 11, 8)
