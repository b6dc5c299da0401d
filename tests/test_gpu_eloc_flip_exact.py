"""The fused spin-flip-projected local energy -- pynqs_eloc_rbm_signed, pynqs_eloc_rbm_flip, pynqs_eloc_jrbm_flip and
energy.local_energy(use_spin_flip=True) on a RealRBM / JastrowRBM -- against the longdouble yardstick of tests/flip_exact.py, which gets
psi(flip x'_k) by flipping the bits of x'_k and evaluating the original parameters (no mirrored table).  Every tolerance is that module's
a-priori bound per walker,
    B_proj = [B + |R| Bbar + |R| |Ebar| (rel + relbar + 2 CM u) + 2 CM u |R| |Ebar|] / extra_norm^2 + 4 CM u |E_proj|,
and for the signed pass alone Bbar and the amplitude bound of psi(flip x).  No walker is left out.
Shapes: sorb 8 (2a2b, the complete space), sorb 12 with 3a2b (flip x leaves the sector) and 1a0b (degenerate classes; no beta electron, so
every sigma_k = +1), sorb 16 with closed-shell walkers only (flip x = x), sorb 66 and 130 (two and three ONV words, the latter with 2a1b: no beta-beta class; the chunked launch),
resident and windowed (sorb x H beyond the LDS: 40 x 520 with one workgroup per walker, 128 / 130 x 160 chunked) forms as the library's own
rule reports them, the theta regimes of test_gpu_eloc_exact.py including "cross" and the saturated ones, eta = +-1, extra_norm as a float
and as a device tensor.  The integrals are random per spin orbital (conftest.synth_integrals): E(flip x) is not Ebar.
tests/test_flip_exact.py checks the yardstick and, per case, that the two wrong variants (sigma = +1; Ebar := E(flip x)) would fail here."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

import eloc_exact as X
import flip_exact as F
import jrbm_exact as J
import rbm_exact as R
import test_gpu_eloc_exact as T
from conftest import golden, rand_occ, synth_integrals

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "entry kind sorb noA noB H n regime form eta norm jreg closed seed", defaults=(None, False, 0))
# entry: "signed" (cx.eloc_rbm_signed on the mirrored table: Ebar, psi(flip x)), "flip" (cx.eloc_rbm_flip), "jflip" (cx.eloc_jrbm_flip);
# norm: a float, or ("tensor", value): extra_norm handed over as a one-element device tensor;  jreg: jrbm_exact.J_REGIMES (Jastrow forms);
# closed: closed-shell walkers only (the beta string is the alpha string)
R1, RC, W1, WC = T.R1, T.RC, T.W1, T.WC
TEN = lambda v: ("tensor", v)  # noqa: E731

FLIP_CASES = (
    # the theta regimes at 3a2b, eta and the form of extra_norm alternating
    [Case("flip", "real", 12, 3, 2, 20, 4, reg, R1, (1.0, -1.0)[i & 1], (1.3, TEN(0.8))[(i >> 1) & 1])
     for i, reg in enumerate(R.REGIMES_ANY + R.REGIMES_ELOC)] + [
        Case("flip", "real", 8, 2, 2, 12, 8, "fe2s2", R1, 1.0, 1.0), Case("flip", "real", 8, 2, 2, 12, 8, "alt30", R1, -1.0, TEN(1.7)),
        Case("flip", "tanh", 8, 2, 2, 12, 8, "small", R1, -1.0, 1.3), Case("flip", "pRBM", 8, 2, 2, 12, 8, "alt30", R1, 1.0, TEN(0.9)),
        Case("flip", "real", 12, 1, 0, 6, 4, "small", R1, -1.0, 1.1), Case("flip", "pRBM", 12, 1, 0, 6, 4, "small", R1, 1.0, 1.1),
        Case("flip", "real", 16, 3, 3, 24, 4, "fe2s2", R1, 1.0, TEN(1.2), closed=True), Case("flip", "real", 16, 3, 3, 24, 4, "chunk-50", R1, -1.0, 1.2, closed=True),
        Case("flip", "tanh", 16, 3, 3, 24, 4, "small", R1, 1.0, 1.2, closed=True), Case("flip", "pRBM", 16, 3, 3, 24, 4, "alt30", R1, -1.0, 1.2, closed=True),
        Case("flip", "tanh", 12, 3, 2, 20, 4, "cross", R1, 1.0, 1.0, seed=1), Case("flip", "tanh", 12, 3, 2, 20, 4, "chunk-50", R1, -1.0, TEN(1.4)),
        Case("flip", "pRBM", 12, 3, 2, 20, 4, "cross", R1, -1.0, 1.0), Case("flip", "pRBM", 12, 3, 2, 20, 4, "chunk-50", R1, 1.0, TEN(1.4)),
        # two and three words: the chunked launch
        Case("flip", "real", 66, 3, 4, 40, 2, "chunk-50", RC, 1.0, 1.3), Case("flip", "real", 66, 3, 4, 40, 2, "cross", RC, -1.0, TEN(1.3)),
        Case("flip", "tanh", 66, 3, 4, 40, 2, "cross", RC, 1.0, 1.3), Case("flip", "pRBM", 66, 3, 4, 40, 2, "chunk-50", RC, -1.0, 1.3),
        Case("flip", "real", 130, 2, 1, 64, 2, "chunk-50", RC, -1.0, 1.3), Case("flip", "real", 130, 2, 1, 64, 1, "cross", RC, 1.0, TEN(1.3)),
        # windowed: sorb x H beyond the LDS
        Case("flip", "real", 40, 3, 2, 520, 2, "fe2s2", W1, -1.0, 1.3), Case("flip", "real", 128, 2, 1, 160, 1, "chunk-50", WC, 1.0, TEN(1.3)),
        Case("flip", "tanh", 130, 2, 1, 160, 1, "fe2s2", WC, -1.0, 1.3), Case("flip", "pRBM", 40, 3, 2, 520, 2, "fe2s2", W1, 1.0, 1.3)])

SIGNED_CASES = [
    Case("signed", "real", 12, 3, 2, 20, 4, "fe2s2", R1, 1.0, 1.0), Case("signed", "real", 12, 3, 2, 20, 4, "cross", R1, 1.0, 1.0),
    Case("signed", "tanh", 8, 2, 2, 12, 8, "small", R1, 1.0, 1.0), Case("signed", "pRBM", 66, 3, 4, 40, 2, "chunk-50", RC, 1.0, 1.0),
    Case("signed", "real", 16, 3, 3, 24, 4, "fe2s2", R1, 1.0, 1.0, closed=True), Case("signed", "real", 40, 3, 2, 520, 2, "fe2s2", W1, 1.0, 1.0)]

JFLIP_CASES = [
    Case("jflip", "real", 8, 2, 2, 12, 8, "fe2s2", R1, 1.0, 1.3, "j-asym"), Case("jflip", "real", 8, 2, 2, 12, 8, "alt30", R1, -1.0, TEN(0.9), "j-strong"),
    Case("jflip", "real", 12, 3, 2, 20, 4, "cross", R1, -1.0, 1.3, "j-strong"), Case("jflip", "real", 12, 3, 2, 20, 4, "chunk-50", R1, 1.0, TEN(1.3), "j-small"),
    Case("jflip", "real", 12, 1, 0, 6, 4, "small", R1, 1.0, 1.1, "j-asym"),
    Case("jflip", "real", 16, 3, 3, 24, 4, "fe2s2", R1, -1.0, 1.2, "j-asym", closed=True),
    Case("jflip", "real", 66, 3, 4, 40, 2, "cross", RC, 1.0, 1.3, "j-asym"), Case("jflip", "real", 130, 2, 1, 64, 1, "chunk-50", RC, -1.0, TEN(1.3), "j-small")]

# through energy.local_energy(use_spin_flip=True), each flavour and the JastrowRBM, without and with use_spin_raising (<S-S+> by the same route
# with a second, independent set of integrals: conftest.synth_integrals(seed = SPIN_SEED))
# (the generic route is held to 1e-8 Ha absolute: a route case must be one where that is a meaningful figure -- yardstick bound <= 1e-9 Ha for
# both sets of integrals, asserted in tests/test_flip_exact.py; "j-strong" with "cross" has |E_loc| ~ 1e11 Ha, one ulp of which is 1e-5)
ROUTE_CASES = [Case("flip", "real", 12, 3, 2, 20, 4, "cross", R1, -1.0, TEN(1.3)), Case("flip", "tanh", 12, 3, 2, 20, 4, "chunk-50", R1, -1.0, TEN(1.4)),
               Case("flip", "pRBM", 12, 3, 2, 20, 4, "cross", R1, -1.0, 1.0), Case("jflip", "real", 12, 3, 2, 20, 4, "cross", R1, -1.0, 1.3, "j-asym")]
SPIN_SEED = 4321

ALL_CASES = FLIP_CASES + SIGNED_CASES + JFLIP_CASES


def case_id(c):
    nrm = f"t{c.norm[1]}" if isinstance(c.norm, tuple) else f"{c.norm}"
    return (f"{c.entry}-{c.kind}-{c.sorb}.{c.noA}+{c.noB}-H{c.H}-n{c.n}-{c.regime}-eta{c.eta:+.0f}-N{nrm}" + (f"-{c.jreg}" if c.jreg else "")
            + ("-closed" if c.closed else ""))


def norm_value(c) -> float:
    return float(c.norm[1]) if isinstance(c.norm, tuple) else float(c.norm)


@functools.lru_cache(maxsize=None)
def walkers(sorb, noA, noB, n, regime, closed, seed) -> np.ndarray:
    occ = rand_occ(n, sorb, noA, noB, seed=7 * sorb + noA + 1000 * seed)
    if closed:
        assert noA == noB
        occ[:, 1::2] = occ[:, 0::2]
    elif regime == "cross":
        p0, p1, q0, q1 = R.cross_orbitals(sorb)
        occ = T._force(occ, {p0: 1, p1: 1, q0: 0, q1: 0})
    assert occ[:, 0::2].sum(1).tolist() == [noA] * n and occ[:, 1::2].sum(1).tolist() == [noB] * n
    return occ


@functools.lru_cache(maxsize=None)
def params(c: Case):
    """(Rbm, M or None)"""
    rbm = R.regime_params(c.regime, c.kind, c.sorb, c.H, c.seed)
    return rbm, (J.jastrow_params(c.jreg, c.sorb) if c.jreg else None)


_STRUCT, _REF = {}, {}
Ref = namedtuple("Ref", "case rbm M occ walkers")


def reference(c: Case, spin: bool = False, wrong: bool = False) -> Ref:
    """The yardstick of a case, computed once (the entries "signed" and "flip" of the same shape share it); spin: with the <S-S+> stand-in
    integrals; wrong: also the variant that needs the structure of the flipped walker (the CPU test's)."""
    key = (c.kind, c.sorb, c.noA, c.noB, c.H, c.n, c.regime, c.eta, norm_value(c), c.jreg, c.closed, c.seed, spin, wrong)
    if key not in _REF:
        rbm, M = params(c)
        occ = walkers(c.sorb, c.noA, c.noB, c.n, c.regime, c.closed, c.seed)
        h1, h2 = synth_integrals(c.sorb, SPIN_SEED) if spin else synth_integrals(c.sorb)
        ws = []
        for row in occ:
            ks = (spin, c.sorb, row.tobytes())
            if ks not in _STRUCT:
                _STRUCT[ks] = X.structure(row, h1, h2)
            ws.append(F.walker(rbm, _STRUCT[ks], c.eta, norm_value(c), M, *((h1, h2) if wrong else ())))
        _REF[key] = Ref(c, rbm, M, occ, ws)
    return _REF[key]


def form_of(c: Case) -> str:
    from pynqs_amd import _native as N

    nele = c.noA + c.noB
    if c.entry == "jflip":
        f = N.lib().pynqs_eloc_jrbm_flip_form(c.n, c.sorb, nele, c.noA, c.noB, c.H)
    else:
        f = N.lib().pynqs_eloc_rbm_flip_form(c.n, c.sorb, nele, c.noA, c.noB, c.H)
        assert f == N.lib().pynqs_eloc_rbm_form(c.n, c.sorb, nele, c.noA, c.noB, c.H, 0)
    assert f >= 0, (case_id(c), "unsupported")
    return ("windowed" if f & 1 else "resident") + (" chunked" if f & 2 else " one")


_dev, _bra, _report = T._dev, T._bra, T._report


def _norm_arg(c):
    return torch.tensor(c.norm[1], dtype=torch.float64, device="cuda") if isinstance(c.norm, tuple) else c.norm


def ratio(got, exact, bounds) -> np.ndarray:
    """|got - exact| / bound per walker; inf where the kernel's value is not finite"""
    got = np.asarray(got)
    out = np.empty(got.size)
    for i, (e, b) in enumerate(zip(exact, bounds)):
        g = complex(got[i])
        out[i] = (float(abs(X.CLD(g) - e)) if np.isfinite(g.real) and np.isfinite(g.imag) else np.inf) / b
    return out


def tables(ref: Ref):
    """(RBMTable, its mirror, JastrowTable or None, its mirror or None) of a case, by the package's own helpers"""
    from pynqs_amd import C_extension as cx

    W, hb, vb = _dev(ref.rbm.W), _dev(ref.rbm.hb), _dev(ref.rbm.vb)
    jt = jm = None
    if ref.M is not None:
        jt, jm = cx.JastrowTable(_dev(ref.M)), cx.mirrored_jastrow_table(_dev(ref.M))
    return cx.RBMTable(W, hb, vb), cx.mirrored_rbm_table(W, hb, vb), jt, jm


def run_kernel(c: Case, ref: Ref):
    from pynqs_amd import C_extension as cx

    h1, h2 = synth_integrals(c.sorb)
    bra, sys_ = _dev(_bra(ref.occ)), (c.sorb, c.noA + c.noB, c.noA, c.noB)
    tab, mir, jt, jm = tables(ref)
    if c.entry == "signed":
        e, p = cx.eloc_rbm_signed(bra, _dev(h1), _dev(h2), mir, *sys_, rbm_type=c.kind)
    elif c.entry == "flip":
        e, p = cx.eloc_rbm_flip(bra, _dev(h1), _dev(h2), tab, mir, *sys_, c.eta, _norm_arg(c), rbm_type=c.kind)
    else:
        e, p = cx.eloc_jrbm_flip(bra, _dev(h1), _dev(h2), tab, jt, mir, jm, *sys_, c.eta, _norm_arg(c))
    return e.cpu().numpy(), p.cpu().numpy()


def psi_ratio(ref: Ref, got, mirrored: bool) -> np.ndarray:
    """psi(x) (mirrored: psi(flip x), which the signed pass writes for the mirrored table) under the amplitude bound"""
    ws = ref.walkers
    rbm, M = (F.mirror_params(ref.rbm, ref.M) if mirrored else (ref.rbm, ref.M))
    cat = lambda f: np.concatenate([getattr((w.wbar if mirrored else w.w).psi, f) for w in ws])  # noqa: E731
    ex = R.Exact(rbm.kind, cat("re"), cat("im"), cat("vis"), cat("cond"), cat("y"), cat("sech2"))
    return J.amp_ratio(rbm, M, got, ex) if M is not None else R.amp_ratio(rbm, np.asarray(got), ex)


def _check(c: Case, what: str, e, p, ref=None):
    ref = ref or reference(c)
    ws = ref.walkers
    if c.entry == "signed":
        re_ = ratio(e, [w.Ebar for w in ws], [w.bound_bar() for w in ws])
    else:
        re_ = ratio(e, [w.E_proj for w in ws], [w.bound() for w in ws])
    rp = psi_ratio(ref, p, c.entry == "signed")
    msg = [_report(f"{what} {case_id(c)} E", re_), _report(f"{what} {case_id(c)} psi", rp)]
    assert bool((re_ <= 1.0).all()) and bool((rp <= 1.0).all()), msg


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_projected_energy_meets_the_rounding_bound(case):
    assert form_of(case) == case.form
    _check(case, case.entry, *run_kernel(case, reference(case)))


def test_abi_symbols_exist():
    from pynqs_amd import _native as N

    for name in ("pynqs_eloc_rbm_signed", "pynqs_eloc_rbm_flip", "pynqs_eloc_rbm_flip_supported", "pynqs_eloc_rbm_flip_form",
                 "pynqs_eloc_jrbm_signed", "pynqs_eloc_jrbm_flip", "pynqs_eloc_jrbm_flip_supported", "pynqs_eloc_jrbm_flip_form"):
        assert hasattr(N.lib(), name), name


def closed_shell_fe2s2(eta: float):
    """(Case, Ref) of two closed-shell Fe2S2 walkers (the fixture's alpha strings on both spins) with the fixture's RBM and the molecule's
    own, spin-symmetric, integrals"""
    d, d0 = golden("fe2s2_inputs.npz"), golden("eloc_e2e_fe2s2.npz")
    c = Case("flip", "real", 40, 15, 15, 80, 2, "fixture", RC, eta, 1.3, closed=True)
    key = ("fe2s2-closed", eta)
    if key not in _REF:
        occ = np.unpackbits(np.ascontiguousarray(d["ci_space"][:2]), axis=1, bitorder="little")[:, :40]
        occ[:, 1::2] = occ[:, 0::2]
        h1, h2 = np.ascontiguousarray(d["h1e"], dtype=np.float64), np.ascontiguousarray(d["h2e"], dtype=np.float64)
        rbm = R.make("real", d0["W"], d0["hb"], d0["vb"])
        _REF[key] = Ref(c, rbm, None, occ, [F.walker(rbm, X.structure(row, h1, h2), eta, 1.3) for row in occ])
    return c, _REF[key]


@pytest.mark.parametrize("eta", [1.0, -1.0])
def test_closed_shell_walkers_have_the_projector_as_a_factor(eta):
    """flip x = x and spin-symmetric integrals (Fe2S2's own): R = 1 and Ebar = E, so E_proj = E (1 + eta eta_m(x)) / extra_norm^2 in
    structure: where eta eta_m(x) = -1 the two passes cancel to their rounding, else E_proj is 2 E / extra_norm^2"""
    from pynqs_amd import C_extension as cx

    c, ref = closed_shell_fe2s2(eta)
    d = golden("fe2s2_inputs.npz")
    h1, h2 = _dev(np.ascontiguousarray(d["h1e"], dtype=np.float64)), _dev(np.ascontiguousarray(d["h2e"], dtype=np.float64))
    bra, sys_ = _dev(_bra(ref.occ)), (40, 30, 15, 15)
    tab, mir, _, _ = tables(ref)
    e, _ = cx.eloc_rbm_flip(bra, h1, h2, tab, mir, *sys_, eta, 1.3)
    e0, _ = cx.eloc_rbm(bra, h1, h2, tab, *sys_)
    e, e0 = e.cpu().numpy(), e0.cpu().numpy()
    for i, w in enumerate(ref.walkers):
        assert not w.open_shell and float(abs(w.R - 1)) == 0.0
        fac = 1 + eta * w.eta_m_x
        want = e0[i] * fac / 1.3 ** 2
        print(f"closed-shell Fe2S2 walker {i}, eta {eta:+.0f}, eta_m {w.eta_m_x:+.0f}: E_proj {e[i]:.3e}, E (1 + eta eta_m) / N^2 {want:.3e}, bound {w.bound():.2e}")
        assert abs(e[i] - want) <= w.bound() + abs(fac) * w.w.bound() / 1.3 ** 2 + float(abs(w.Ebar - w.E)) / 1.3 ** 2, (i, e[i], want)


def test_zero_jastrow_returns_the_bits_of_the_rbm_form():
    """M = 0: every pair factor is exp(0) = 1 and r_o = 0 exactly, so the Jastrow form does the RBM form's arithmetic.  psi(x), summed in
    a fixed order, has the RBM form's bits.  E_loc has no fixed bits from launch to launch in either kernel (the waves pull their tiles
    from a counter, a chunked launch adds with atomics: tests/test_gpu_jrbm.py), so the two energies are held to what the ORDER of the
    additions alone can change: two sums of the same terms are each within c_add u A of the exact sum (eloc_exact: c_add additions on
    A = a_0 + sum a_k |r_k|), in both passes, and the combine repeats exactly on equal inputs: 2 c_add u (A + |R| Abar) / N^2, plus the
    four roundings of the combine on what the order changed."""
    from pynqs_amd import C_extension as cx

    for c in (JFLIP_CASES[0], JFLIP_CASES[2], JFLIP_CASES[6]):
        ref = reference(c)
        h1, h2 = _dev(synth_integrals(c.sorb)[0]), _dev(synth_integrals(c.sorb)[1])
        bra, sys_ = _dev(_bra(ref.occ)), (c.sorb, c.noA + c.noB, c.noA, c.noB)
        tab, mir, _, _ = tables(ref)
        zero = torch.zeros((c.sorb, c.sorb), dtype=torch.float64, device="cuda")
        jt, jm = cx.JastrowTable(zero), cx.mirrored_jastrow_table(zero)
        ej, pj = cx.eloc_jrbm_flip(bra, h1, h2, tab, jt, mir, jm, *sys_, c.eta, _norm_arg(c))
        er, pr = cx.eloc_rbm_flip(bra, h1, h2, tab, mir, *sys_, c.eta, _norm_arg(c))
        assert torch.equal(pj, pr), case_id(c)
        rbm0 = [F.walker(ref.rbm, w.w.st, c.eta, norm_value(c)) for w in ref.walkers]   # (the yardstick without the Jastrow factor)
        tol = np.array([2 * w.w.st.c_add(False) * X.U * (w.w.A + float(abs(w.R)) * w.wbar.A) * (1 + 4 * X.U) / w.norm ** 2 for w in rbm0])
        diff = (ej - er).abs().cpu().numpy()
        print(case_id(c), "M = 0: max |E_J - E_RBM| / order-of-additions bound", float((diff / tol).max()), "identical bits:", int((diff == 0).sum()), "of", diff.size)
        assert bool((diff <= tol).all()), (case_id(c), diff, tol)


def _module(c: Case, ref: Ref):
    from pynqs_amd.rbm import JastrowRBM, RealRBM

    W, hb, vb = _dev(ref.rbm.W), _dev(ref.rbm.hb), _dev(ref.rbm.vb)
    return (JastrowRBM(W, hb, vb, _dev(ref.M)) if ref.M is not None else RealRBM(W, hb, vb, rbm_type=c.kind)).cuda()


def _local_energy(c: Case, ref: Ref, spin_raising: bool, fused_rbm: bool = True, x=None, h=None, module=None, sys_=None, dt=None):
    """energy.local_energy(use_spin_flip=True) on the case's module with SpinProjection.eta = c.eta; (eloc, sloc, psi) as host arrays"""
    from pynqs_amd import energy, public_function as pf

    sorb = c.sorb if sys_ is None else sys_[0]
    sys_ = sys_ or (c.sorb, c.noA + c.noB, c.noA, c.noB)
    x = _dev(_bra(ref.occ)) if x is None else x
    h1, h2 = h or tuple(_dev(a) for a in synth_integrals(c.sorb))
    dt = dt or (torch.complex128 if c.kind == "pRBM" else torch.float64)
    old, old_eta, old_fused = torch.get_default_dtype(), pf.SpinProjection._eta, energy.FUSED_RBM
    torch.set_default_dtype(torch.float64)
    try:
        pf.SpinProjection.init(2 if c.eta < 0 else 4, 0)
        assert pf.SpinProjection.eta == c.eta
        energy.FUSED_RBM = fused_rbm
        m = module if module is not None else _module(c, ref)
        ab = lambda xx, func: pf.ansatz_batch(func, xx, 100000, sorb, x.device, dt)  # noqa: E731
        kw = {}
        if spin_raising:
            hs1, hs2 = (_dev(a) for a in synth_integrals(c.sorb, SPIN_SEED))
            kw = dict(use_spin_raising=True, h1e_spin=hs1, h2e_spin=hs2)
        el, sl, ps, _ = energy.local_energy(x, h1, h2, m, ab, *sys_, dtype=dt, use_spin_flip=True, extra_norm=_norm_arg(c), **kw)
    finally:
        energy.FUSED_RBM = old_fused
        pf.SpinProjection._eta = old_eta
        torch.set_default_dtype(old)
    return el.cpu().numpy(), sl.cpu().numpy(), ps.cpu().numpy()


@pytest.mark.parametrize("spin_raising", [False, True], ids=["eloc", "eloc+sloc"])
@pytest.mark.parametrize("case", ROUTE_CASES, ids=case_id)
def test_energy_layer_runs_the_fused_projected_form(case, spin_raising, monkeypatch):
    """local_energy(use_spin_flip=True): nothing of size nbatch x ncomb is materialised (get_comb_hij_fused raises), E_loc and <S-S+>
    within the bound, psi(x) within the amplitude bound; and with FUSED_RBM off the generic route agrees within its 1e-8"""
    from pynqs_amd import energy

    c, ref = case, reference(case)
    generic = _local_energy(c, ref, spin_raising, fused_rbm=False)

    def boom(*a, **k):
        raise AssertionError("get_comb_hij_fused called: the projected SIMPLE form fell back to the materialising path")

    monkeypatch.setattr(energy, "get_comb_hij_fused", boom)
    el, sl, ps = _local_energy(c, ref, spin_raising)
    _check(c, "local_energy", el, ps, ref)
    if spin_raising:
        sref = reference(c, spin=True)
        rs = ratio(sl, [w.E_proj for w in sref.walkers], [w.bound() for w in sref.walkers])
        assert bool((rs <= 1.0).all()), _report(f"local_energy {case_id(c)} <S-S+>", rs)
    else:
        assert not sl.any()
    for what, got, want in zip(("E_loc", "<S-S+>"), (el, sl), generic):
        print(f"{case_id(c)} {what}: fused - generic {float(np.abs(got - want).max()):.3e} Ha, |value| up to {float(np.abs(want).max()):.3e}")
        assert float(np.abs(got - want).max()) <= 1e-8, (case_id(c), what)
    np.testing.assert_allclose(ps, generic[2], rtol=1e-12)


def test_fe2s2_fixture_through_local_energy(fe2s2, monkeypatch):
    """The reference's own numbers (tests/golden/eloc_flip_multipsi_fe2s2.npz, simple_flip: 32 Fe2S2 walkers) at 1e-8 Ha, fused"""
    from pynqs_amd import energy
    from pynqs_amd.rbm import RealRBM

    d0, d = golden("eloc_e2e_fe2s2.npz"), golden("eloc_flip_multipsi_fe2s2.npz")
    c = Case("flip", "real", 40, 15, 15, 80, 32, "fixture", RC, float(d["eta"]), TEN(float(d["extra_norm"])))

    def boom(*a, **k):
        raise AssertionError("get_comb_hij_fused called")

    monkeypatch.setattr(energy, "get_comb_hij_fused", boom)
    m = RealRBM(_dev(d0["W"]), _dev(d0["hb"]), _dev(d0["vb"])).cuda()
    el, _, ps = _local_energy(c, None, False, x=_dev(d["x"]), h=(_dev(fe2s2["h1e"]), _dev(fe2s2["h2e"])), module=m, sys_=(40, 30, 15, 15))
    np.testing.assert_allclose(ps, d["psi_simple_flip"], rtol=1e-12)
    np.testing.assert_allclose(el, d["eloc_simple_flip"], rtol=0, atol=1e-8)


def test_auto_nbatch_sizes_the_projected_form_as_fused():
    from pynqs_amd import energy, public_function as pf

    c = ROUTE_CASES[0]
    x, h1 = _dev(_bra(reference(c).occ)).repeat(64, 1), _dev(synth_integrals(c.sorb)[0])
    n_sd = pf.get_Num_SinglesDoubles(c.sorb, c.noA, c.noB)
    for case in (ROUTE_CASES[0], ROUTE_CASES[3]):
        m = _module(case, reference(case))
        energy.reset_caches()
        nb = energy.auto_nbatch(x, h1, c.sorb, c.noA + c.noB, c.noA, c.noB, m, None, torch.float64, False, 0, False, False, True, False)
        want = max(1, pf.get_nbatch(c.sorb, x.size(0), n_sd, 64.0, 0.25, x.device, False, torch.double, fused="simple_rbm", eps_sample=0))
        assert [k[4] for k in energy._AUTO_NBATCH] == ["simple_rbm"], "the projected form was not sized as the fused SIMPLE path"
        assert nb == want, (case_id(case), nb, want)
    energy.reset_caches()
