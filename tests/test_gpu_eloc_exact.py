"""pynqs_eloc_rbm (flavours "real", "tanh", "pRBM"), pynqs_eloc_crbm (complex parameters and "cos") and pynqs_green_rbm against the exact
yardstick of tests/eloc_exact.py (numpy longdouble from the packed integrals and the parameters): every tolerance is the a-priori
rounding bound derived in that module's docstring,
    |E_got - E_exact| <= u [(t_0 + c_add) a_0 + sum_k a_k ((t_k + kappa_k + c_add + 1) |r_k| + ext_k)]      per walker,
    |g_k - g_k,exact| <= u a_k ((t_k + kappa_k + 2) |r_k| + ext_k)                                           per entry of the Green's row,
and psi(x) as written by these kernels under rbm_exact's amplitude bound.  No walker and no row entry is left out.  The cases are the
smallest shapes at which each structure can go wrong (1, 2 and 3 ONV words, unequal spins, the degenerate classes, H below and beyond
the chunk of eight, resident and windowed kernels, one workgroup per walker and the chunked launch with atomics), in the parameter
regimes of the children tests plus "cross" (rbm_exact.regime_params), where an excitation takes theta through zero.  Which form a case
takes is asked of the library (pynqs_eloc_rbm_form / pynqs_eloc_crbm_form: the launch's own rule).  tests/test_eloc_exact.py checks the
yardstick itself on the CPU and that every case listed here is a finite, well-conditioned, non-vacuous one."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

import eloc_exact as X
import rbm_exact as R
from conftest import golden, rand_occ, synth_integrals

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "kernel kind sorb noA noB H n regime ints form")
# kernel: "rbm" (cx.eloc_rbm), "crbm" (cx.eloc_crbm), "green" (gfmc.green_kernel);  ints: "syn" (conftest.synth_integrals) / "fe2s2";
# form: what the library must report for the launch: resident / windowed, one workgroup per walker / chunked (atomics).
# A walker's tiles are cut over several workgroups only when it has at least 8 tiles of 64 blocks: sorb 12 has one tile and takes one
# workgroup per walker for any n; the chunked launch is reached at sorb 40 (Fe2S2), 66, 128 and 130.
R1, RC, W1, WC = "resident one", "resident chunked", "windowed one", "windowed chunked"

ELOC_CASES = (
    [Case("rbm", "real", 12, 3, 3, 20, 4, reg, "syn", R1) for reg in R.REGIMES_ANY + R.REGIMES_ELOC] + [
        Case("rbm", "real", 12, 3, 3, 20, 1025, "small", "syn", R1),
        Case("rbm", "real", 12, 2, 4, 7, 4, "fe2s2", "syn", R1),
        Case("rbm", "real", 2, 1, 1, 3, 1, "small", "syn", R1), Case("rbm", "real", 4, 1, 0, 6, 2, "small", "syn", R1),
        Case("rbm", "real", 66, 3, 4, 40, 2, "chunk-50", "syn", RC), Case("rbm", "real", 66, 3, 4, 40, 2, "cross", "syn", RC),
        Case("rbm", "real", 130, 3, 2, 64, 2, "chunk-50", "syn", RC), Case("rbm", "real", 130, 3, 2, 64, 2, "cross", "syn", RC),
        Case("rbm", "real", 40, 15, 15, 80, 2, "fe2s2", "fe2s2", RC), Case("rbm", "real", 40, 15, 15, 80, 2, "spread-45", "fe2s2", RC),
        Case("rbm", "tanh", 12, 3, 3, 20, 4, "small", "syn", R1), Case("rbm", "tanh", 12, 3, 3, 20, 4, "cross", "syn", R1),
        Case("rbm", "tanh", 16, 5, 3, 24, 4, "alt30", "syn", R1), Case("rbm", "tanh", 16, 5, 3, 24, 4, "chunk-50", "syn", R1),
        Case("rbm", "tanh", 66, 3, 4, 40, 2, "cross", "syn", RC),
        Case("rbm", "pRBM", 12, 3, 3, 20, 4, "alt30", "syn", R1), Case("rbm", "pRBM", 12, 3, 3, 20, 4, "cross", "syn", R1),
        Case("rbm", "pRBM", 16, 5, 3, 24, 4, "small", "syn", R1), Case("rbm", "pRBM", 16, 5, 3, 24, 4, "chunk-50", "syn", R1),
        Case("rbm", "pRBM", 66, 3, 4, 40, 2, "chunk-50", "syn", RC),
        # windowed: sorb x H beyond the LDS
        Case("rbm", "real", 128, 3, 2, 400, 2, "fe2s2", "syn", WC), Case("rbm", "real", 128, 3, 2, 400, 2, "chunk-50", "syn", WC),
        Case("rbm", "real", 40, 3, 2, 1200, 2, "fe2s2", "syn", W1), Case("rbm", "real", 40, 3, 2, 1200, 2, "chunk-50", "syn", W1),
        Case("rbm", "tanh", 130, 3, 2, 400, 2, "fe2s2", "syn", WC), Case("rbm", "tanh", 130, 3, 2, 400, 2, "chunk-50", "syn", WC)] +
    [Case("crbm", "complex", 12, 3, 3, 20, 4, reg, "syn", R1) for reg in ("small", "fe2s2", "alt30", "chunk-50", "imb50", "imb1000", "cross")] + [
        Case("crbm", "complex", 16, 5, 3, 24, 4, "fe2s2", "syn", R1), Case("crbm", "complex", 16, 5, 3, 24, 4, "imb1000", "syn", R1),
        Case("crbm", "complex", 66, 3, 4, 40, 2, "chunk-50", "syn", RC), Case("crbm", "complex", 66, 3, 4, 40, 2, "cross", "syn", RC),
        Case("crbm", "complex", 66, 3, 4, 160, 2, "fe2s2", "syn", WC),  # windows by itself: 67 x 161 complex rows are 169 KiB
        Case("crbm", "cos", 12, 3, 3, 20, 4, "small", "syn", R1)] +
    # beyond the 30 electrons of Fe2S2: 33 on one word (the order-free fast_single walks 33 terms, fast_diag one lane per electron) and 65
    # on two (fast_diag's lanes come round a second time); the form is what pynqs_eloc_rbm_form / _crbm_form give these shapes
    [Case("rbm", "real", 40, 17, 16, 20, 2, reg, "syn", R1) for reg in ("small", "chunk-50")] +
    [Case("crbm", "complex", 40, 17, 16, 20, 2, reg, "syn", RC) for reg in ("small", "chunk-50")] +
    [Case(k, kind, 72, 33, 32, 20, 2, reg, "syn", RC) for k, kind in (("rbm", "real"), ("crbm", "complex")) for reg in ("small", "chunk-50")])
MANY_ELECTRON = [c for c in ELOC_CASES if c.noA + c.noB > 30]
# (kind "cos": prod_h cos(theta_h) with the real parameters of the regime, through the complex kernel and the complex reference with (i W, i b))

# the complex kernel with a forced window of 6 hidden units: a window boundary INSIDE the saturated chunk of eight (the real kernel's
# windows are multiples of eight and cannot end there)
FORCED_WINDOW_CASE = Case("crbm", "complex", 12, 3, 3, 20, 4, "chunk-50", "syn", W1)
FORCED_WINDOW = "6"

GREEN_CASES = [
    Case("green", "real", 12, 3, 2, 24, 40, "fe2s2", "syn", R1), Case("green", "real", 12, 3, 2, 24, 40, "chunk-50", "syn", R1),
    Case("green", "real", 12, 3, 2, 24, 40, "cross", "syn", R1), Case("green", "real", 66, 3, 4, 70, 4, "cross", "syn", R1),
    Case("green", "real", 128, 3, 2, 400, 3, "chunk-50", "syn", W1),
    Case("green", "tanh", 12, 3, 2, 24, 40, "fe2s2", "syn", R1), Case("green", "tanh", 12, 3, 2, 24, 40, "chunk-50", "syn", R1),
    Case("green", "tanh", 12, 3, 2, 24, 40, "cross", "syn", R1), Case("green", "tanh", 66, 3, 4, 70, 4, "chunk-50", "syn", R1),
    Case("green", "tanh", 128, 3, 2, 400, 3, "fe2s2", "syn", W1)]

# one case per flavour also goes through energy.local_energy (SIMPLE, FUSED_RBM): the dispatcher's choice of table and flavour
ROUTE_CASES = [Case("rbm", "real", 12, 3, 3, 20, 4, "cross", "syn", R1), Case("rbm", "tanh", 12, 3, 3, 20, 4, "cross", "syn", R1),
               Case("rbm", "pRBM", 12, 3, 3, 20, 4, "cross", "syn", R1), Case("crbm", "complex", 12, 3, 3, 20, 4, "cross", "syn", R1),
               Case("crbm", "cos", 12, 3, 3, 20, 4, "small", "syn", R1)]


# seed of rbm_exact.regime_params where seed 0 gives a walker with |tanh(a.x)| < 1e-3 (a condition on the reference: tests/test_eloc_exact.py)
PARAM_SEED = {("tanh", 12, 24, "fe2s2"): 1, ("tanh", 12, 24, "cross"): 1}


def case_id(c):
    return f"{c.kernel}-{c.kind}-{c.sorb}.{c.noA}+{c.noB}-H{c.H}-n{c.n}-{c.regime}-{c.ints}"


@functools.lru_cache(maxsize=None)
def integrals(ints: str, sorb: int):
    if ints == "fe2s2":
        d = golden("fe2s2_inputs.npz")
        assert sorb == 40
        return np.ascontiguousarray(d["h1e"], dtype=np.float64), np.ascontiguousarray(d["h2e"], dtype=np.float64)
    return synth_integrals(sorb)


def _force(occ: np.ndarray, want: dict) -> np.ndarray:
    """occupations with the orbitals of `want` set as asked, the electron numbers of each spin kept (the displaced electron or hole goes to
    the lowest orbital of that spin outside `want`); an orbital whose spin has no room is left as it is"""
    occ = occ.copy()
    for row in occ:
        for o, v in want.items():
            if row[o] == v:
                continue
            other = [p for p in range(o & 1, row.size, 2) if p not in want and row[p] == v]
            if other:
                row[other[0]], row[o] = row[o], v
    return occ


@functools.lru_cache(maxsize=None)
def walkers(sorb: int, noA: int, noB: int, n: int, regime: str) -> np.ndarray:
    """0/1 [n, sorb]: conftest.rand_occ; "cross": every walker occupies p0, p1 and leaves q0, q1 empty (rbm_exact.cross_orbitals);
    "one-338-w": every walker occupies rbm_exact.forced_orbitals(sorb), as test_gpu_rbm_exact.children_case does"""
    occ = rand_occ(n, sorb, noA, noB, seed=7 * sorb + noA)
    if regime == "cross":
        p0, p1, q0, q1 = R.cross_orbitals(sorb)
        occ = _force(occ, {p0: 1, p1: 1, q0: 0, q1: 0})
    elif regime == "one-338-w":
        occ = _force(occ, {o: 1 for o in R.forced_orbitals(sorb)})
    assert occ[:, 0::2].sum(1).tolist() == [noA] * n and occ[:, 1::2].sum(1).tolist() == [noB] * n
    return occ


@functools.lru_cache(maxsize=None)
def params(kind: str, sorb: int, H: int, regime: str):
    """(the reference's Rbm, the real-parameter Rbm the kernel is given for "cos" or None)"""
    if kind == "cos":
        real = R.regime_params(regime, "real", sorb, H, 0)
        return R.make("complex", 1j * real.W, 1j * real.hb, None), real
    return R.regime_params(regime, kind, sorb, H, PARAM_SEED.get((kind, sorb, H, regime), 0)), None


_STRUCT, _WALKER = {}, {}

Ref = namedtuple("Ref", "case rbm real occ walkers psi")


def reference(c: Case) -> Ref:
    """The yardstick of a case: computed once per (integrals, determinant) and once per (parameters, determinant), shared by every test
    and by cases that differ in the kernel only (E_loc and the Green's row of the same walkers)."""
    rbm, real = params(c.kind, c.sorb, c.H, c.regime)
    occ = walkers(c.sorb, c.noA, c.noB, c.n, c.regime)
    h1, h2 = integrals(c.ints, c.sorb)
    ws = []
    for row in occ:
        ks = (c.ints, c.sorb, row.tobytes())
        if ks not in _STRUCT:
            _STRUCT[ks] = X.structure(row, h1, h2)
        kw = (c.kind, c.H, c.regime) + ks
        if kw not in _WALKER:
            _WALKER[kw] = X.walker(rbm, _STRUCT[ks])
        ws.append(_WALKER[kw])
    cat = lambda f: np.concatenate([getattr(w.psi, f) for w in ws])  # noqa: E731
    psi = R.Exact(rbm.kind, cat("re"), cat("im"), cat("vis"), cat("cond"), cat("y"), cat("sech2"))
    return Ref(c, rbm, real, occ, ws, psi)


def form_of(c: Case) -> str:
    """the form the library's own launch rule gives this case"""
    from pynqs_amd import _native as N

    nele = c.noA + c.noB
    if c.kernel == "crbm":
        f = N.lib().pynqs_eloc_crbm_form(c.n, c.sorb, nele, c.noA, c.noB, c.H)
    else:
        f = N.lib().pynqs_eloc_rbm_form(c.n, c.sorb, nele, c.noA, c.noB, c.H, int(c.kernel == "green"))
    assert f >= 0, (case_id(c), "unsupported")
    return ("windowed" if f & 1 else "resident") + (" chunked" if f & 2 else " one")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bra(occ):
    from oracle import oracle

    return oracle.pm01_to_onv(occ, occ.shape[1])


def _report(what, ratio):
    ratio = np.atleast_1d(np.asarray(ratio, dtype=np.float64))
    worst = int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)))
    print(f"{what}: worst error / bound {ratio[worst]:.3g} at {worst} of {ratio.size}; non-finite {int((~np.isfinite(ratio)).sum())}")
    return f"{what}: error / bound {ratio[worst]:.3g} at {worst}, {int((~(ratio <= 1)).sum())} of {ratio.size} outside"


def eloc_ratio(ref: Ref, got: np.ndarray) -> np.ndarray:
    """|E_got - E_exact| / bound per walker; inf where the kernel's value is not finite"""
    got = np.asarray(got)
    assert got.shape == (len(ref.walkers),)
    out = np.empty(got.size)
    for i, w in enumerate(ref.walkers):
        g = complex(got[i])
        err = abs(X.CLD(g) - w.E) if np.isfinite(g.real) and np.isfinite(g.imag) else np.inf
        out[i] = float(err) / w.bound()
    return out


# ln of the largest finite double is 709.78, of the smallest normal one -708.40.  rbm_exact.LN_MAX = 690 holds for every case but the
# windowed shapes the kernels exist for: 400 hidden units with eight at -50 reach 697 (still finite and normal: LN_FINITE), and the
# product of 1200 factors 2cosh(theta) >= 2 is beyond any double: there psi(x) must come out as +inf (the correctly rounded value), while
# every ratio psi(x') / psi(x), and so E_loc, stays finite.  tests/test_eloc_exact.py asserts which of the three a case is.
LN_FINITE, LN_OVERFLOW = 708.0, 711.0


def psi_ratio(ref: Ref, got: np.ndarray) -> np.ndarray:
    c = ref.case
    got = np.asarray(got)
    if c.kind == "cos":  # the kernel returns psi exp(-H ln 2) = prod cos(theta)
        got = got * 2.0 ** c.H
    lnpsi = ref.psi.re.astype(np.float64)
    assert bool(((np.abs(lnpsi) <= LN_FINITE) | (lnpsi >= LN_OVERFLOW)).all())
    over = lnpsi >= LN_OVERFLOW
    if not over.any():
        return R.amp_ratio(ref.rbm, got, ref.psi)
    assert bool(over.all()) and c.kind in ("real", "complex")
    inf = (np.isinf(got.real) | np.isinf(got.imag)) & ~(np.isnan(got.real) | np.isnan(got.imag)) & ((got.real > 0) | (c.kind == "complex"))
    return np.where(inf, 0.0, np.inf)


def run_kernel(c: Case, ref: Ref):
    """(eloc, psi) of the case from the C_extension entry, host arrays"""
    from pynqs_amd import C_extension as cx

    h1, h2 = integrals(c.ints, c.sorb)
    bra = _dev(_bra(ref.occ))
    nele = c.noA + c.noB
    if c.kernel == "rbm":
        tab = cx.RBMTable(_dev(ref.rbm.W), _dev(ref.rbm.hb), None if c.regime == "novb" else _dev(ref.rbm.vb))
        e, p = cx.eloc_rbm(bra, _dev(h1), _dev(h2), tab, c.sorb, nele, c.noA, c.noB, rbm_type=c.kind)
    else:
        cos = c.kind == "cos"
        tab = cx.CRBMTable(_dev(R.pairs(ref.rbm.W)), _dev(R.pairs(ref.rbm.hb)), None if cos else _dev(R.pairs(ref.rbm.vb)))
        e, p = cx.eloc_crbm(bra, _dev(h1), _dev(h2), tab, c.sorb, nele, c.noA, c.noB, log_scale=c.H * np.log(2.0) if cos else 0.0)
    return e.cpu().numpy(), p.cpu().numpy()


def _check(c: Case, what: str, e, p):
    ref = reference(c)
    re_, rp = eloc_ratio(ref, e), psi_ratio(ref, p)
    msg = [_report(f"{what} {case_id(c)} E_loc", re_), _report(f"{what} {case_id(c)} psi(x)", rp)]
    assert bool((re_ <= 1.0).all()) and bool((rp <= 1.0).all()), msg


@pytest.mark.parametrize("case", ELOC_CASES, ids=case_id)
def test_local_energy_meets_the_rounding_bound(case):
    assert form_of(case) == case.form
    if case in MANY_ELECTRON:   # the fused kernel serves the shape: the energy layer would not fall back to the generic path for it
        from pynqs_amd import _native as N

        assert getattr(N.lib(), f"pynqs_eloc_{case.kernel}_supported")(case.sorb, case.noA + case.noB, case.noA, case.noB, case.H) == 1
    _check(case, "eloc", *run_kernel(case, reference(case)))


def test_complex_window_boundary_inside_the_saturated_chunk(monkeypatch):
    c = FORCED_WINDOW_CASE
    monkeypatch.setenv("PYNQS_CRBM_WINDOW", FORCED_WINDOW)
    assert form_of(c) == c.form
    _check(c, f"eloc window {FORCED_WINDOW}", *run_kernel(c, reference(c)))


def _module(c: Case, ref: Ref):
    from pynqs_amd.rbm import ComplexRBM, RealRBM

    if c.kind == "complex":
        return ComplexRBM(_dev(R.pairs(ref.rbm.W)), _dev(R.pairs(ref.rbm.hb)), _dev(R.pairs(ref.rbm.vb))).cuda()
    real = ref.real if c.kind == "cos" else ref.rbm
    return RealRBM(_dev(real.W), _dev(real.hb), _dev(real.vb), rbm_type=c.kind).cuda()


@pytest.mark.parametrize("case", ROUTE_CASES, ids=case_id)
def test_energy_layer_routes_to_the_same_kernel(case):
    """energy.local_energy, SIMPLE method, FUSED_RBM: the dispatcher's table and flavour, under the same bound"""
    from pynqs_amd import energy, public_function as pf

    c, ref = case, reference(case)
    h1, h2 = integrals(c.ints, c.sorb)
    x = _dev(_bra(ref.occ))
    dt = torch.complex128 if c.kind in ("pRBM", "complex") else torch.float64
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    calls = []
    orig = {n: getattr(energy.CX, n) for n in ("eloc_rbm", "eloc_crbm")}
    try:
        for n, f in orig.items():
            setattr(energy.CX, n, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(f, n))
        assert energy.FUSED_RBM
        m = _module(c, ref)
        ab = lambda xx, func: pf.ansatz_batch(func, xx, 100000, c.sorb, x.device, dt)  # noqa: E731
        el, _, ps, _ = energy.local_energy(x, _dev(h1), _dev(h2), m, ab, c.sorb, c.noA + c.noB, c.noA, c.noB, dtype=dt)
    finally:
        for n, f in orig.items():
            setattr(energy.CX, n, f)
        torch.set_default_dtype(old)
    assert calls == ["eloc_" + c.kernel], calls
    _check(c, "local_energy", el.cpu().numpy(), ps.cpu().numpy())


def green_reference(c: Case):
    """(Ref, Lambda, [eloc_exact.Green per walker]): the columns in the order of the oracle's comb, matched by the bits of x'"""
    from oracle import oracle

    ref = reference(c)
    key = ("green",) + tuple(c)
    if key not in _WALKER:
        comb, _ = oracle.comb(_bra(ref.occ), c.sorb, c.noA, c.noB)
        bits = np.unpackbits(comb, axis=-1, bitorder="little")[..., :c.sorb]
        lam = X.lambda_in_largest_gap(ref.walkers)
        _WALKER[key] = (lam, [X.green(w, lam, X.match_columns(w, bits[i])) for i, w in enumerate(ref.walkers)])
    return (ref,) + _WALKER[key]


@pytest.mark.parametrize("case", GREEN_CASES, ids=case_id)
def test_greens_row_meets_the_rounding_bound_per_entry(case):
    from pynqs_amd import gfmc, public_function as pf

    c = case
    assert form_of(c) == c.form and gfmc.FUSED_GREEN
    ref, lam, rows = green_reference(c)
    h1, h2 = integrals(c.ints, c.sorb)
    x = _dev(_bra(ref.occ))
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        m = _module(c, ref)
        ab = lambda xx, func: pf.ansatz_batch(func, xx, 100000, c.sorb, x.device, torch.float64)  # noqa: E731
        eloc, gk, comb, _, neg = gfmc.green_kernel(x, lam, _dev(h1), _dev(h2), m, ab, c.sorb, c.noA + c.noB, c.noA, c.noB)
    finally:
        torch.set_default_dtype(old)
    assert isinstance(comb, gfmc.CombRows), "the row did not come from pynqs_green_rbm"
    gk, neg = gk.cpu().numpy(), neg.cpu().numpy()
    worst, zeros_wrong, unsure = [], 0, 0
    for i, (w, g) in enumerate(zip(ref.walkers, rows)):
        got = gk[i]
        assert got.shape == g.g.shape
        err = np.where(np.isfinite(got), np.abs(got.astype(X.LD) - g.g).astype(np.float64), np.inf)
        # an entry whose |h_k r_k| lies below its own bound may fall on either side of the sign decision
        alt = np.where(g.sure, np.inf, np.abs(got.astype(X.LD) - np.where(g.keep, 0, -w.hr.real[np.concatenate([[0], g.perm])])).astype(np.float64))
        ratio = np.minimum(err, alt) / g.bound
        worst.append(ratio)
        kept, dropped = g.sure & g.keep, g.sure & ~g.keep
        kept[0] = dropped[0] = False
        zeros_wrong += int((got[kept] == 0).sum()) + int((got[dropped] != 0).sum())
        unsure += int((~g.sure).sum())
        assert bool(neg[i]) == g.clamp and (got[0] == 0) == g.clamp, (i, float(g.k0), float(got[0]))
    ratio = np.concatenate(worst)
    msg = [_report(f"green {case_id(c)} row entries (Lambda {lam:.6g}, clamped {int(neg.sum())} of {neg.size}, unsure signs {unsure})", ratio)]
    re_ = eloc_ratio(ref, eloc.cpu().numpy())
    msg.append(_report(f"green {case_id(c)} E_loc", re_))
    assert zeros_wrong == 0, f"{zeros_wrong} entries on the wrong side of the sign decision"
    assert bool((ratio <= 1.0).all()) and bool((re_ <= 1.0).all()), msg
