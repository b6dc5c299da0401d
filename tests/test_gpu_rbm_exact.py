"""pynqs_rbm_forward, pynqs_rbm_children_prepare + pynqs_rbm_forward_children and pynqs_rbm_grad against the exact reference of
tests/rbm_exact.py (numpy longdouble straight from the parameters, spot-checked with mpmath at 50 digits): every tolerance is the
a-priori rounding bound derived in that module's docstring, a function of the shapes, the inputs and the reference alone,
    amplitudes   |psi / psi_exact - 1| <= u (sorb + H + 16) cond(x)                              per row,
    gradient     |G_k - G_exact_k|     <= u [4 sum_n a_n |O_nk| + sum_n |f_n| ((40 + n / 128) max(1, |tanh|) + (sorb + 2) S_h |sech^2|)]   per entry,
and no row or entry is left out of a comparison.  The parameter regimes (rbm_exact.regime_params) reach where the kernels' algorithms
differ: |theta| of 30-338 with either sign (the children kernels use exp(-2 theta) with the SIGNED theta), whole chunks of eight
saturated units, Im b up to +-1000 (the argument reduction of sincos_mod), no visible bias, theta ~ 1e-8 (tanh's 1 - e cancellation).
The children are built on the host (rbm_exact.make_children), so that every structure of the kernel is hit on purpose.
tests/test_rbm_exact.py checks on the CPU that every case listed here is a finite, well-conditioned one."""
import numpy as np
import pytest
import torch

import rbm_exact as R

pytestmark = pytest.mark.gpu

# (kind, sorb, H, n, regime): 1, 2 and 3 ONV words, an odd sorb, H around the chunk of eight, n around the workgroup of 256
FORWARD_CASES = [
    ("real", 12, 1, 1, "small"), ("real", 40, 7, 255, "fe2s2"), ("real", 66, 8, 256, "alt30"), ("real", 130, 9, 257, "chunk-50"),
    ("real", 184, 40, 1025, "chunk+50"), ("real", 37, 64, 256, "two-200"), ("real", 40, 65, 257, "one-338"),
    ("real", 40, 80, 1025, "spread-45"), ("real", 66, 40, 255, "novb"),
    ("tanh", 12, 7, 255, "small"), ("tanh", 40, 40, 256, "alt30"), ("tanh", 130, 65, 257, "chunk-50"), ("tanh", 37, 9, 1, "fe2s2"),
    ("tanh", 184, 80, 1025, "spread-45"),
    ("pRBM", 12, 8, 256, "small"), ("pRBM", 40, 40, 257, "alt30"), ("pRBM", 66, 64, 255, "two-200"), ("pRBM", 184, 9, 1025, "one-338"),
    ("pRBM", 130, 1, 1, "novb"),
    ("complex", 12, 1, 1, "small"), ("complex", 40, 40, 1025, "fe2s2"), ("complex", 66, 7, 255, "alt30"), ("complex", 130, 8, 256, "chunk-50"),
    ("complex", 184, 9, 257, "chunk+50"), ("complex", 37, 64, 256, "two-200"), ("complex", 40, 65, 255, "one-338"),
    ("complex", 40, 80, 257, "spread-45"), ("complex", 66, 40, 256, "novb"), ("complex", 40, 40, 1025, "imb50"),
    ("complex", 130, 80, 257, "imb1000"), ("complex", 184, 368, 255, "fe2s2")]

# (kind, sorb, H, regime, form): the factor table in LDS (a thread per row) / beyond 64 KB (a wave per row)
CHILD_CASES = [
    ("complex", 40, 40, "small", "lds"), ("complex", 40, 40, "fe2s2", "lds"), ("complex", 40, 40, "alt30", "lds"),
    ("complex", 40, 40, "chunk+50", "lds"), ("complex", 40, 40, "chunk-50", "lds"), ("complex", 40, 40, "two-200", "lds"),
    ("complex", 40, 40, "one-338", "lds"), ("complex", 40, 40, "one-338-w", "lds"), ("complex", 40, 40, "spread-45", "lds"),
    ("complex", 40, 40, "imb50", "lds"), ("complex", 40, 40, "imb1000", "lds"), ("complex", 40, 40, "novb", "lds"),
    ("complex", 12, 1, "small", "lds"), ("complex", 184, 9, "chunk-50", "lds"),
    ("real", 40, 80, "small", "lds"), ("real", 40, 80, "alt30", "lds"), ("real", 40, 80, "chunk-50", "lds"), ("real", 40, 80, "spread-45", "lds"),
    ("real", 40, 65, "two-200", "lds"), ("real", 40, 9, "one-338", "lds"), ("real", 40, 40, "one-338-w", "lds"), ("real", 12, 1, "chunk-50", "lds"),
    ("real", 66, 40, "chunk-50", "lds"), ("real", 130, 9, "two-200", "lds"), ("real", 130, 8, "fe2s2", "lds"), ("real", 40, 64, "novb", "lds"),
    ("tanh", 12, 7, "small", "lds"), ("tanh", 40, 64, "chunk-50", "lds"), ("tanh", 66, 8, "alt30", "lds"),
    ("pRBM", 40, 40, "chunk-50", "lds"), ("pRBM", 130, 9, "small", "lds"), ("pRBM", 66, 7, "one-338", "lds"),
    ("real", 120, 120, "small", "wave"), ("real", 120, 120, "chunk-50", "wave"), ("real", 120, 120, "two-200", "wave"),
    ("real", 120, 120, "one-338", "wave"), ("real", 120, 120, "one-338-w", "wave"), ("real", 184, 65, "spread-45", "wave"),
    ("complex", 136, 150, "fe2s2", "wave"), ("complex", 136, 150, "chunk-50", "wave"), ("complex", 136, 150, "alt30", "wave"),
    ("complex", 136, 150, "imb1000", "wave"), ("complex", 66, 65, "two-200", "wave"), ("complex", 184, 368, "fe2s2", "wave"),
    ("tanh", 130, 64, "chunk-50", "wave"), ("pRBM", 184, 80, "alt30", "wave")]

# (kind, sorb, H, n, regime, complex eloc, pow, prob with exact zeros): 32 walkers per workgroup
GRAD_CASES = [
    ("real", 40, 80, 1000, "small", False, False, False), ("real", 40, 80, 1000, "fe2s2", True, True, False),
    ("real", 12, 1, 1, "small", False, False, False), ("real", 66, 7, 31, "alt30", False, True, False),
    ("real", 130, 8, 32, "sat40", False, False, True), ("real", 184, 9, 33, "tiny", True, False, False),
    ("real", 40, 40, 1000, "sat40", False, False, False), ("real", 40, 64, 33, "novb", False, False, False),
    ("real", 37, 65, 31, "chunk-50", False, False, True), ("real", 40, 40, 1000, "tiny", False, True, False),
    ("complex", 40, 40, 1000, "fe2s2", True, False, False), ("complex", 40, 37, 1000, "small", True, True, False),
    ("complex", 12, 1, 1, "small", True, False, False), ("complex", 66, 7, 31, "alt30", True, False, True),
    ("complex", 130, 8, 32, "sat40", True, True, False), ("complex", 184, 9, 33, "tiny", True, False, False),
    ("complex", 40, 40, 1000, "tiny", True, False, False), ("complex", 40, 64, 33, "novb", True, False, False),
    ("complex", 40, 65, 32, "imb50", True, False, False), ("complex", 40, 80, 1000, "imb1000", False, False, False),
    ("complex", 40, 40, 1000, "sat40", True, True, True)]

EVEN_CASES = [("real", 40, 80, "alt30"), ("real", 40, 40, "chunk+50"), ("complex", 40, 40, "fe2s2"), ("complex", 40, 40, "spread-45"),
              ("real", 120, 120, "two-200"), ("complex", 136, 150, "alt30"), ("tanh", 40, 64, "chunk-50"), ("pRBM", 40, 40, "chunk-50")]

NW = 24  # parents per children case


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _onv(words):
    return _dev(words.view(np.uint8).reshape(words.shape[0], -1))


def kernel_params(rbm, regime):
    """the parameters as the kernels take them (host arrays): complex as (re, im) pairs, no visible bias in the regime "novb\""""
    c = (lambda z: R.pairs(z)) if rbm.kind == "complex" else (lambda z: np.ascontiguousarray(z))
    return c(rbm.W), c(rbm.hb), None if regime == "novb" else c(rbm.vb)


def _forward(rbm, regime, words):
    from pynqs_amd import C_extension as cx

    W, hb, vb = kernel_params(rbm, regime)
    sorb = rbm.W.shape[1]
    return cx.rbm_forward(_onv(words), _dev(W), _dev(hb), None if vb is None else _dev(vb), sorb, rbm.kind).cpu().numpy()


def _children(rbm, regime, rows, par, parents, **kw):
    from pynqs_amd import C_extension as cx

    W, hb, vb = kernel_params(rbm, regime)
    sorb = rbm.W.shape[1]
    return cx.rbm_forward_children(_onv(rows), _dev(par), _onv(parents), _dev(W), _dev(hb), None if vb is None else _dev(vb), sorb, rbm.kind, **kw)


def _report(what, ratio):
    worst = int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)))
    print(f"{what}: worst error / bound {ratio[worst]:.3g} at {worst} of {ratio.size}; non-finite {int((~np.isfinite(ratio)).sum())}")
    return f"{what}: error / bound {ratio[worst]:.3g} at {worst}, {int((~(ratio <= 1)).sum())} of {ratio.size} outside"


def children_case(kind, sorb, H, regime, nw=NW, seed=0):
    """(rbm, parents, rows, parent index, flips, x of the rows, Exact of the rows): the reference of a children case"""
    parents = R.rand_words(nw, sorb, 11 + seed)
    force = None
    if regime == "one-338-w":  # every parent occupies the orbitals coupled to the saturated unit (theta = -330); children empty 2 and 4 of them
        force = R.forced_orbitals(sorb)
        bits = R.pm1(parents, sorb) > 0
        bits[:, force] = True
        parents = R.pack_bits(bits)
    rows, par, nflip = R.make_children(parents, sorb, 5 + seed, force)
    rbm, x, ex = R.checked_case(kind, sorb, H, regime, rows, seed)
    return rbm, parents, rows, par, nflip, x, ex


@pytest.mark.parametrize("kind,sorb,H,n,regime", FORWARD_CASES)
def test_forward_meets_the_rounding_bound(kind, sorb, H, n, regime):
    words = R.rand_words(n, sorb, 3)
    rbm, x, ex = R.checked_case(kind, sorb, H, regime, words)
    got = _forward(rbm, regime, words)
    assert got.shape == (n,) and got.dtype == (np.float64 if kind in ("real", "tanh") else np.complex128)
    ratio = R.amp_ratio(rbm, got, ex)
    msg = _report(f"forward {kind} {sorb}x{H} n {n} {regime}", ratio)
    assert bool((ratio <= 1.0).all()), msg


@pytest.mark.parametrize("kind,sorb,H,regime,form", CHILD_CASES)
def test_children_meet_the_rounding_bound(kind, sorb, H, regime, form):
    from pynqs_amd import C_extension as cx

    assert R.children_form(sorb, H, kind) == form and cx.rbm_forward_children_supported(sorb, H, kind)
    rbm, parents, rows, par, nflip, x, ex = children_case(kind, sorb, H, regime)
    assert set(nflip.tolist()) >= {0, 2, 4} and len(set(par.tolist())) == NW and bool((np.diff(par) < 0).any())
    got = _children(rbm, regime, rows, par, parents).cpu().numpy()
    ratio = R.amp_ratio(rbm, got, ex)
    msg = _report(f"children {kind} {sorb}x{H} {regime} ({form})", ratio)
    assert bool((ratio <= 1.0).all()), msg
    # the plain forward on the same rows, for the record and under the same bound
    ratio_f = R.amp_ratio(rbm, _forward(rbm, regime, rows), ex)
    assert bool((ratio_f <= 1.0).all()), _report("forward on the children", ratio_f)


@pytest.mark.parametrize("kind,sorb,H,regime", [("complex", 40, 40, "chunk-50"), ("real", 120, 120, "two-200"), ("real", 40, 9, "fe2s2")])
def test_children_count_tail_and_a_single_walker(kind, sorb, H, regime):
    """count_dev smaller than n: the rows before it meet the bound, the tail is left untouched; nwalkers = 1: every row from walker 0."""
    rbm, parents, rows, par, nflip, x, ex = children_case(kind, sorb, H, regime)
    n = rows.shape[0]
    cnt = n - 37
    cplx = kind in ("complex", "pRBM")
    out = torch.full((n,), 7.0, dtype=torch.complex128 if cplx else torch.float64, device="cuda")
    count = torch.tensor([cnt, 0, 0, 0], dtype=torch.int32, device="cuda")
    _children(rbm, regime, rows, par, parents, count=count, out=out)
    got = out.cpu().numpy()
    assert bool((got[cnt:] == 7.0).all())
    ratio = R.amp_ratio(rbm, got, ex)[:cnt]
    assert bool((ratio <= 1.0).all()), _report("counted rows", ratio)
    one = parents[:1]
    rows1, par1, _ = R.make_children(one, sorb, 9)
    rbm1, x1, ex1 = R.checked_case(kind, sorb, H, regime, rows1)
    assert bool((par1 == 0).all())
    ratio1 = R.amp_ratio(rbm1, _children(rbm1, regime, rows1, par1, one).cpu().numpy(), ex1)
    assert bool((ratio1 <= 1.0).all()), _report("one walker", ratio1)


@pytest.mark.parametrize("kind,sorb,H,regime", EVEN_CASES)
def test_amplitudes_are_even_in_the_hidden_units(kind, sorb, H, regime):
    """psi is even under (W_h, b_h) -> (-W_h, -b_h): the forward and the children of the two parameter sets agree within twice the bound
    (which is the same for both: cond(x) is even too), on a random half of the hidden units."""
    rbm, parents, rows, par, nflip, x, ex = children_case(kind, sorb, H, regime)
    units = np.flatnonzero(np.random.default_rng(7).random(H) < 0.5)
    assert 0 < units.size < H
    mir = R.mirrored(rbm, units)
    exm = R.exact_ld(mir, x)
    assert np.allclose(exm.cond, ex.cond, rtol=1e-12) and float(np.abs((exm.re - ex.re).astype(np.float64)).max()) <= 1e-15 * R.LN_MAX
    allowed = 2 * R.amp_bound(sorb, H, ex.cond)
    for name, a, b in (("forward", _forward(rbm, regime, rows), _forward(mir, regime, rows)),
                       ("children", _children(rbm, regime, rows, par, parents).cpu().numpy(), _children(mir, regime, rows, par, parents).cpu().numpy())):
        assert bool(np.isfinite(a.real).all() and np.isfinite(b.real).all()), name
        al, bl = a.astype(R.CLD), b.astype(R.CLD)
        if kind == "pRBM":
            r = al * np.conj(bl)
            d = np.abs(np.arctan2(r.imag, r.real)).astype(np.float64)
        elif kind == "tanh":
            vis = ex.vis.astype(np.float64)
            d = (np.abs(al - bl) / np.exp(ex.re)).astype(np.float64)
            allowed_t = allowed * np.abs(vis) + 2 * R.U * ((sorb + 1) * float(np.abs(rbm.vb).sum()) * (1 - vis * vis) + 1)
            assert bool((d <= allowed_t).all()), (name, float((d / allowed_t).max()))
            continue
        else:
            d = np.abs(al / bl - 1).astype(np.float64)
        assert bool((d <= allowed).all()), (name, float((d / allowed).max()))


@pytest.mark.parametrize("sorb,H,form", [(40, 8, "lds"), (130, 8, "lds"), (136, 16, "wave")])
def test_argument_reduction_with_exact_arguments(sorb, H, form):
    """W = 0 and b in conjugate pairs with Im b up to +-4000: theta, a.x and the total phase are exact, so the generic bound's allowance
    for the rounding of theta (u sorb |b| ~ 1e-11 here, which would hide an inexact reduction of the sine's argument by k pi / 2) is not
    needed: forward and children (LDS and wave form) within rbm_exact.amp_bound_exact_theta, a few hundred u."""
    assert R.children_form(sorb, H, "complex") == form
    rbm, parents, rows, par, nflip, x, ex = children_case("complex", sorb, H, "exact-theta")
    allowed = R.amp_bound_exact_theta(rbm)
    assert allowed <= 0.05 * float(R.amp_bound(sorb, H, ex.cond).min()) and float(np.abs(rbm.hb.imag).max()) > 1000
    for name, got in (("forward", _forward(rbm, "exact-theta", rows)), ("children", _children(rbm, "exact-theta", rows, par, parents).cpu().numpy())):
        err = np.where(np.isfinite(got.real) & np.isfinite(got.imag), np.abs(got.astype(R.CLD) / ex.psi() - 1).astype(np.float64), np.inf)
        print(f"exact theta {sorb}x{H} {name}: worst error / bound {float(err.max() / allowed):.3g} (bound {allowed:.3g})")
        assert bool((err <= allowed).all()), (name, float(err.max()), allowed)


def grad_inputs(kind, sorb, H, n, regime, eloc_cplx, use_pow, zeros, seed=0):
    """(rbm, words, prob, eloc, e_total, pow) of a gradient case, host arrays.  e_total is the float64 sum the caller would pass (an input
    of the kernel and of the reference alike); with one walker it differs from eloc[0], or f = 0 and the case tests nothing."""
    g = np.random.default_rng([seed, sorb, H, n])
    words = R.rand_words(n, sorb, 17)
    rbm = R.regime_params(regime, kind, sorb, H, seed)
    prob = g.random(n)
    if zeros and n > 2:
        prob[g.choice(n, max(1, n // 4), replace=False)] = 0.0
    prob /= prob.sum()
    eloc = g.standard_normal(n) - 100.0
    if eloc_cplx:
        eloc = eloc + 0.1j * g.standard_normal(n)
    e_total = (prob * eloc).sum() if n > 1 else eloc[0] + (0.37 - 0.05j if eloc_cplx else 0.37)
    pw = 0.5 + g.random(n) if use_pow else None
    return rbm, words, prob, eloc, e_total, pw


@pytest.mark.parametrize("kind,sorb,H,n,regime,eloc_cplx,use_pow,zeros", GRAD_CASES)
def test_gradient_meets_the_rounding_bound_per_entry(kind, sorb, H, n, regime, eloc_cplx, use_pow, zeros):
    from pynqs_amd import _native as N

    rbm, words, prob, eloc, e_total, pw = grad_inputs(kind, sorb, H, n, regime, eloc_cplx, use_pow, zeros)
    x = R.pm1(words, sorb)
    ge = R.grad_exact(rbm, x, prob, eloc, e_total, pw)
    assert float(np.abs(ge.f).max()) > 0 and np.isfinite(ge.loss) and bool((ge.bW > 0).all())
    cplx = kind == "complex"
    flav = N.RBM_COMPLEX if cplx else N.RBM_REAL
    W, hb, vb = kernel_params(rbm, regime)
    Wd, hbd, vbd = _dev(W), _dev(hb), None if vb is None else _dev(vb)
    et = np.array([e_total.real, e_total.imag] if eloc_cplx else [float(np.real(e_total))], dtype=np.float64)
    el = R.pairs(eloc) if eloc_cplx else np.ascontiguousarray(eloc.real)
    onv, pd, eld, etd = _onv(words), _dev(prob), _dev(el), _dev(et)
    pwd = None if pw is None else _dev(pw)
    work = torch.empty(max(N.lib().pynqs_rbm_grad_workspace(n, sorb, H, flav) // 8, 1), dtype=torch.float64, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def run():
        gw, ghb = torch.full_like(Wd, 7.0), torch.full_like(hbd, 7.0)
        gvb = None if vbd is None else torch.full_like(vbd, 7.0)
        loss = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
        N.check(N.lib().pynqs_rbm_grad(onv.data_ptr(), n, sorb, Wd.data_ptr(), hbd.data_ptr(), ptr(vbd), H, flav, pd.data_ptr(), eld.data_ptr(),
                                       int(eloc_cplx), etd.data_ptr(), ptr(pwd), gw.data_ptr(), ghb.data_ptr(), ptr(gvb), loss.data_ptr(),
                                       work.data_ptr(), torch.cuda.current_stream().cuda_stream), "pynqs_rbm_grad")
        torch.cuda.synchronize()
        return gw, ghb, gvb, loss

    gw, ghb, gvb, loss = run()
    eW, ehb, evb = R.grad_errors(ge, gw.cpu().numpy(), ghb.cpu().numpy(), None if gvb is None else gvb.cpu().numpy(), cplx)
    msgs = [_report(f"grad {kind} {sorb}x{H} n {n} {regime} {nm}", e.ravel()) for nm, e in (("W", eW), ("hb", ehb), ("vb", evb)) if e.size]
    dl = abs(float(np.longdouble(float(loss)) - np.longdouble(ge.loss)))
    print(f"loss {float(loss)!r} exact {ge.loss!r} error / bound {dl / ge.bloss:.3g}; bound / max|G| {float(ge.bW.max() / np.abs(ge.GW).max()):.3g}")
    assert eW.size == H * sorb and ehb.size == H and evb.size == (0 if vb is None else sorb)
    assert bool((eW <= 1.0).all() and (ehb <= 1.0).all() and (evb <= 1.0).all()), msgs
    assert dl <= ge.bloss, (float(loss), ge.loss, ge.bloss)
    again = run()
    assert all(a is None or torch.equal(a, b) for a, b in zip((gw, ghb, gvb, loss), again))  # fixed order of additions
