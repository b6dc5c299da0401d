"""pynqs_jastrow_grad through the C ABI, pynqs_jastrow_table_build and the layer above them (grad.FusedJastrowRbmGrad) against the exact
yardstick of tests/jrbm_exact.py (numpy longdouble): every tolerance is the a-priori rounding bound derived in that module's docstring,
    grad_M   |got - exact| <= u (n + 8) 2 sum_n |f_n|                               per entry,
    loss     |got - exact| <= u (2 sorb + n + 8) 2 sum_n |f_n| sum_ij |M_ij|,
at the shapes of tests/jastrow_grad_cases.py: one, two and three words with the last bit of each, one to seventeen workgroups with and
without a short last one, the loss as the lone output of a block, exact zeros among the probabilities, c_n.  No entry is left out and a
non-finite value counts as an infinite error.  Workspace, gradient and loss lie between guard words that the call must leave alone.
tests/test_jastrow_grad_cases.py shows on the CPU that a kernel wrong in any of these structures could not stay under the bounds."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

import jastrow_grad_cases as C
import jrbm_exact as J
import rbm_exact as R

pytestmark = pytest.mark.gpu

GUARD = 256  # guard doubles on either side of a region
NAN = float("nan")
U = J.U


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _onv(words):
    return _dev(words.view(np.uint8).reshape(words.shape[0], -1))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """`count` doubles inside a larger tensor filled with NaN, GUARD doubles on either side"""

    def __init__(self, count: int) -> None:
        self.count = count
        self.whole = torch.full((count + 2 * GUARD,), NAN, dtype=torch.float64, device="cuda")
        self.region = self.whole[GUARD:GUARD + count]
        self.nan_bits = int(torch.full((1,), NAN, dtype=torch.float64).view(torch.int64).item())

    def data_ptr(self) -> int:
        return self.region.data_ptr()

    def intact(self) -> bool:
        """every guard word still has its NaN bit pattern"""
        w = self.whole.view(torch.int64)
        return bool((w[:GUARD] == self.nan_bits).all()) and bool((w[GUARD + self.count:] == self.nan_bits).all())

    def untouched(self) -> bool:
        return bool((self.whole.view(torch.int64) == self.nan_bits).all())

    def bits(self) -> np.ndarray:
        return self.region.view(torch.int64).cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def reference(c: C.Case):
    """(inputs, yardstick) of a case, computed once and shared by the tests"""
    inp = C.inputs(c)
    return inp, J.grad_exact(inp.M, inp.x, inp.prob, inp.eloc, inp.e_total, inp.pow)


Device = namedtuple("Device", "onv M prob eloc et pow")


def device_inputs(inp: C.Inputs) -> Device:
    return Device(_onv(inp.words), _dev(inp.M), _dev(inp.prob), _dev(inp.eloc), _dev(np.array([inp.e_total])), None if inp.pow is None else _dev(inp.pow))


def jastrow_grad(n: int, sorb: int, d: Device, grad, loss, work, pow="own") -> int:
    """pynqs_jastrow_grad on the regions given (loss: a region or None for NULL); the return code"""
    from pynqs_amd import _native as N

    rc = N.lib().pynqs_jastrow_grad(_ptr(d.onv), n, sorb, _ptr(d.M), _ptr(d.prob), _ptr(d.eloc), _ptr(d.et), _ptr(d.pow if isinstance(pow, str) else pow),
                                    _ptr(grad), _ptr(loss), _ptr(work), _stream())
    torch.cuda.synchronize()
    return rc


def fresh_buffers(n: int, sorb: int):
    from pynqs_amd import _native as N

    nbytes = N.lib().pynqs_jastrow_grad_workspace(n, sorb)
    assert nbytes == C.groups(n) * (sorb * sorb + 1) * 8
    return Guarded(sorb * sorb), Guarded(1), Guarded(nbytes // 8)


def grad_ratio(ge: J.JGrad, got: np.ndarray) -> np.ndarray:
    """|got - exact| / bound per entry; inf where the kernel's value is not finite"""
    ok = np.isfinite(got)
    return np.where(ok, np.abs(np.where(ok, got, 0).astype(J.LD) - ge.G).astype(np.float64) / ge.bound, np.inf)


def loss_ratio(ge: J.JGrad, got: float, bloss=None, want=None) -> float:
    if not np.isfinite(got):
        return float("inf")
    return abs(float(J.LD(got) - J.LD(ge.loss if want is None else want))) / (ge.bloss if bloss is None else bloss)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_kernel_meets_the_bounds_between_guard_words_and_repeats_its_bits(case):
    from pynqs_amd import _native as N

    n, sorb = case.n, case.sorb
    inp, ge = reference(case)
    d = device_inputs(inp)
    grad, loss, work = fresh_buffers(n, sorb)
    assert jastrow_grad(n, sorb, d, grad, loss, work) == N.OK
    got, got_loss = grad.region.cpu().numpy().reshape(sorb, sorb), float(loss.region[0])
    rg, rl = grad_ratio(ge, got), loss_ratio(ge, got_loss)
    worst = tuple(int(i) for i in np.unravel_index(int(np.argmax(rg)), rg.shape))
    print(f"JGRAD {C.case_id(case)}: gradient worst error / bound {rg.max():.3g} at {worst} of {rg.size}, non-finite {int((~np.isfinite(got)).sum())}; "
          f"loss error / bound {rl:.3g} ({got_loss!r}, exact {ge.loss!r})")
    assert rg.shape == (sorb, sorb) and bool((rg <= 1.0).all()), f"{int((~(rg <= 1.0)).sum())} of {rg.size} entries outside, worst {rg.max():.3g} at {worst}"
    assert rl <= 1.0, (got_loss, ge.loss, ge.bloss)
    assert grad.intact() and loss.intact() and work.intact()
    # the same sum of the same terms: [i][j] and [j][i], and every diagonal entry (2 sum_n f_n in walker order)
    bits = grad.bits().reshape(sorb, sorb)
    assert np.array_equal(bits, bits.T)
    assert bool((np.diag(bits) == bits[0, 0]).all())
    # a second call into the dirty workspace and outputs
    lbits = loss.bits()
    assert jastrow_grad(n, sorb, d, grad, loss, work) == N.OK
    assert np.array_equal(grad.bits().reshape(sorb, sorb), bits) and np.array_equal(loss.bits(), lbits)
    assert grad.intact() and loss.intact() and work.intact()
    # loss = NULL: the same gradient, nothing else written
    grad2, loss2, work2 = fresh_buffers(n, sorb)
    assert jastrow_grad(n, sorb, d, grad2, None, work2) == N.OK
    assert np.array_equal(grad2.bits().reshape(sorb, sorb), bits) and grad2.intact() and work2.intact() and loss2.untouched()
    # pow = NULL is c_n = 1
    if not case.pow:
        grad3, loss3, work3 = fresh_buffers(n, sorb)
        assert jastrow_grad(n, sorb, d, grad3, loss3, work3, pow=torch.ones(n, dtype=torch.float64, device="cuda")) == N.OK
        assert np.array_equal(grad3.bits().reshape(sorb, sorb), bits) and np.array_equal(loss3.bits(), lbits)
        assert grad3.intact() and loss3.intact() and work3.intact()


@pytest.mark.parametrize("sorb", [12, 130])
def test_no_walkers_give_a_zero_gradient_and_a_zero_loss(sorb):
    from pynqs_amd import _native as N

    M = _dev(J.jastrow_params("j-asym", sorb))
    none = Device(None, M, None, None, None, None)
    assert N.lib().pynqs_jastrow_grad_workspace(0, sorb) == 0
    zero = np.zeros(sorb * sorb, dtype=np.int64)  # the bits of +0.0
    for with_loss in (True, False):
        grad, loss = Guarded(sorb * sorb), Guarded(1)
        assert jastrow_grad(0, sorb, none, grad, loss if with_loss else None, None) == N.OK
        assert np.array_equal(grad.bits(), zero) and grad.intact()
        if with_loss:
            assert np.array_equal(loss.bits(), zero[:1]) and loss.intact()


def test_bad_arguments_are_refused_on_the_host():
    """argument checks before any launch: an error code, and the outputs keep their fill"""
    from pynqs_amd import _native as N

    case = C.CASES[1]
    n, sorb = case.n, case.sorb
    inp, _ = reference(case)
    d = device_inputs(inp)
    lib = N.lib()
    assert lib.pynqs_jastrow_grad_workspace(-1, sorb) == -1 and lib.pynqs_jastrow_grad_workspace(n, 0) == -1
    assert lib.pynqs_jastrow_grad_workspace(n, 193) == -1
    for what, args in (("sorb = 0", (n, 0, d)), ("sorb = 193", (n, 193, d)), ("n < 0", (-1, sorb, d)),
                       ("jastrow = NULL", (n, sorb, d._replace(M=None)))):
        grad, loss, work = fresh_buffers(n, sorb)
        rc = jastrow_grad(*args, grad, loss, work)
        assert rc == N.EINVAL, (what, rc)
        assert lib.pynqs_last_error()
        assert grad.untouched() and loss.untouched() and work.untouched(), what
    # and missing inputs with walkers to read
    for what, dd in (("onv", d._replace(onv=None)), ("prob", d._replace(prob=None)), ("eloc", d._replace(eloc=None)), ("e_total", d._replace(et=None))):
        grad, loss, work = fresh_buffers(n, sorb)
        assert jastrow_grad(n, sorb, dd, grad, loss, work) == N.EINVAL, what
        assert grad.untouched() and loss.untouched() and work.untouched(), what
    grad, loss, work = fresh_buffers(n, sorb)
    assert jastrow_grad(n, sorb, d, None, loss, work) == N.EINVAL and jastrow_grad(n, sorb, d, grad, loss, None) == N.EINVAL
    assert grad.untouched() and loss.untouched() and work.untouched()
    assert lib.pynqs_jastrow_table_bytes(0) == -1 and lib.pynqs_jastrow_table_bytes(193) == -1
    tab = Guarded(8)
    assert lib.pynqs_jastrow_table_build(_ptr(d.M), 0, tab.data_ptr(), _stream()) == N.EINVAL
    assert lib.pynqs_jastrow_table_build(_ptr(d.M), 193, tab.data_ptr(), _stream()) == N.EINVAL
    assert lib.pynqs_jastrow_table_build(None, sorb, tab.data_ptr(), _stream()) == N.EINVAL
    assert lib.pynqs_jastrow_table_build(_ptr(d.M), sorb, None, _stream()) == N.EINVAL
    torch.cuda.synchronize()
    assert tab.untouched()


def table_layout(sorb: int):
    """pynqs_amd/csrc/rbm.h, JastrowLayout, restated: S | exp(+4 S) | exp(-4 S) | tr M (| a pad word), in doubles"""
    n2 = sorb * sorb
    return n2, (3 * n2 + 2) & ~1


def exp_error_in_u(got: np.ndarray, S: np.ndarray, sign: int) -> np.ndarray:
    """|got / exp(sign 4 S) - 1| / u against the longdouble exponential of the table's own S (the product 4 S is exact)"""
    want = np.exp(sign * 4 * S.astype(J.LD))
    return np.where(np.isfinite(got), np.abs(got.astype(J.LD) / want - 1).astype(np.float64) / U, np.inf)


@pytest.mark.parametrize("sorb", [2, 16, 66, 192])
def test_table_build_against_the_layout_restated(sorb):
    from pynqs_amd import C_extension as cx, _native as N

    M = J.jastrow_params("j-asym", sorb)
    n2, total = table_layout(sorb)
    assert N.lib().pynqs_jastrow_table_bytes(sorb) == 8 * total
    tab = Guarded(total)
    assert N.lib().pynqs_jastrow_table_build(_dev(M).data_ptr(), sorb, tab.data_ptr(), _stream()) == N.OK
    torch.cuda.synchronize()
    assert tab.intact()
    t = tab.region.cpu().numpy()
    S, E4p, E4m, tr = t[:n2].reshape(sorb, sorb), t[n2:2 * n2].reshape(sorb, sorb), t[2 * n2:3 * n2].reshape(sorb, sorb), float(t[3 * n2])
    # S: IEEE addition is correctly rounded and commutative
    want = M + M.T
    want[np.diag_indices(sorb)] = 0.0
    assert np.array_equal(S.view(np.int64), want.view(np.int64))
    assert bool((np.diag(S).view(np.int64) == 0).all()) and np.array_equal(S.view(np.int64), S.T.copy().view(np.int64))
    dl = np.diag(M).astype(J.LD)
    assert abs(float(J.LD(tr) - dl.sum())) <= (sorb - 1) * U * float(np.abs(np.diag(M)).sum())
    if total > 3 * n2 + 1:
        assert t[3 * n2 + 1:].view(np.int64).tolist() == [0]
    ep, em = exp_error_in_u(E4p, S, +1), exp_error_in_u(E4m, S, -1)
    print(f"JTABLE sorb {sorb}: worst relative error of exp(+4 S) {ep.max():.3f} u, of exp(-4 S) {em.max():.3f} u (u = 2^-53), "
          f"|4 S| up to {4 * np.abs(S).max():.3g}")
    assert float(ep.max()) <= 2.0 and float(em.max()) <= 2.0
    # the layer's table has the same bits
    assert np.array_equal(cx.JastrowTable(_dev(M)).buf.cpu().numpy().view(np.int64), t.view(np.int64))
    # the spin-mirrored table: S of M[i ^ 1][j ^ 1]
    idx = np.arange(sorb) ^ 1
    Mm = np.ascontiguousarray(M[idx][:, idx])
    wantm = Mm + Mm.T
    wantm[np.diag_indices(sorb)] = 0.0
    tm = cx.mirrored_jastrow_table(_dev(M)).buf.cpu().numpy()
    Sm = tm[:n2].reshape(sorb, sorb)
    assert np.array_equal(Sm.view(np.int64), wantm.view(np.int64)) and (sorb == 2 or not np.array_equal(Sm, S))
    assert float(exp_error_in_u(tm[n2:2 * n2].reshape(sorb, sorb), Sm, +1).max()) <= 2.0
    assert float(exp_error_in_u(tm[2 * n2:3 * n2].reshape(sorb, sorb), Sm, -1).max()) <= 2.0


# ---- the layer: grad.FusedJastrowRbmGrad ------------------------------------------------------------------------------------------
L_SORB, L_H = 66, 7
L_NAMES = ("weights", "hidden_bias", "visible_bias", "jastrow")
LayerRef = namedtuple("LayerRef", "words prob eloc e_total pow ge gj")


@functools.lru_cache(maxsize=None)
def layer_params():
    return R.regime_params("fe2s2", "real", L_SORB, L_H, 0), J.jastrow_params("j-asym", L_SORB)


@functools.lru_cache(maxsize=None)
def layer_reference(n: int, use_pow: bool = False) -> LayerRef:
    rbm, M = layer_params()
    g = np.random.default_rng([7, L_SORB, n])
    words = R.rand_words(n, L_SORB, seed=29)
    prob = g.random(n)
    prob /= prob.sum()
    eloc = -100.0 + g.standard_normal(n)
    e_total = float((prob * eloc).sum())
    powc = np.full(n, 0.5) if use_pow else None
    x = R.pm1(words, L_SORB)
    return LayerRef(words, prob, eloc, e_total, powc, R.grad_exact(rbm, x, prob, eloc, e_total, powc), J.grad_exact(M, x, prob, eloc, e_total, powc))


def new_module():
    from pynqs_amd.rbm import JastrowRBM

    rbm, M = layer_params()
    return JastrowRBM(_dev(rbm.W), _dev(rbm.hb), _dev(rbm.vb), _dev(M)).cuda()


def layer_call(fg, ref: LayerRef, **kw):
    """one call of the layer: ({parameter name: gradient bits}, loss bits, gradients, loss)"""
    a = dict(onv=_onv(ref.words), state_prob=_dev(ref.prob), eloc=_dev(ref.eloc), e_total=_dev(np.array(ref.e_total)))
    a.update(kw)
    loss = fg(a.pop("onv"), a.pop("state_prob"), a.pop("eloc"), a.pop("e_total"), **a)
    torch.cuda.synchronize()
    got = {k: getattr(fg.module, k).grad.detach().cpu().numpy().copy() for k in L_NAMES}
    return {k: v.view(np.int64) for k, v in got.items()}, np.array([float(loss)]).view(np.int64), got, float(loss)


def same_bits(a, b) -> bool:
    return all(np.array_equal(a[0][k], b[0][k]) for k in L_NAMES) and np.array_equal(a[1], b[1])


def under_the_bounds(what: str, ref: LayerRef, got, loss: float) -> None:
    errs = R.grad_errors(ref.ge, got["weights"], got["hidden_bias"], got["visible_bias"], False)
    rm = grad_ratio(ref.gj, got["jastrow"])
    rl = loss_ratio(ref.gj, loss, ref.ge.bloss + ref.gj.bloss, ref.ge.loss + ref.gj.loss)
    print(f"JLAYER {what}: worst error / bound W {errs[0].max():.3g}, b {errs[1].max():.3g}, a {errs[2].max():.3g}, M {rm.max():.3g}, loss {rl:.3g}")
    assert errs[0].shape == (L_H, L_SORB) and errs[1].shape == (L_H,) and errs[2].shape == (L_SORB,) and rm.shape == (L_SORB, L_SORB)
    assert all(bool((e <= 1.0).all()) for e in errs) and bool((rm <= 1.0).all()) and rl <= 1.0, what


def test_layer_keeps_one_workspace_over_calls_of_different_sizes():
    """n = 513, 65, 1025 on one object: `work` serves pynqs_rbm_grad and then pynqs_jastrow_grad, is kept while it is large enough (with the
    content of the call before) and re-allocated when it is not; every call has the bits of a fresh object's only call and meets the bounds"""
    from pynqs_amd import _native as N, grad as G

    fg = G.FusedJastrowRbmGrad(new_module(), L_SORB)
    need = lambda n: max(N.lib().pynqs_rbm_grad_workspace(n, L_SORB, L_H, N.RBM_REAL), N.lib().pynqs_jastrow_grad_workspace(n, L_SORB))  # noqa: E731
    assert need(65) < need(513) < need(1025)
    held = []
    for n in (513, 65, 1025):
        ref = layer_reference(n)
        seq = layer_call(fg, ref)
        held.append((fg.work.data_ptr(), fg.work.numel() * 8))
        one = layer_call(G.FusedJastrowRbmGrad(new_module(), L_SORB), ref)
        assert same_bits(seq, one), n
        under_the_bounds(f"sequence n {n}", ref, seq[2], seq[3])
    assert held[1] == held[0] and held[0][1] >= need(513) and held[2][1] >= need(1025) > held[0][1], held


def test_layer_gives_the_same_bits_for_every_form_of_its_arguments():
    from pynqs_amd import grad as G

    n = 65
    ref = layer_reference(n)
    m = new_module()
    fg = G.FusedJastrowRbmGrad(m, L_SORB)
    base = layer_call(fg, ref)
    under_the_bounds(f"forms n {n}", ref, base[2], base[3])
    # <E> as a Python float, a 0-d CPU tensor and a device tensor (torch's default dtype is float32: the float must not pass through it)
    assert float(np.float32(ref.e_total)) != ref.e_total
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float32)
    try:
        assert same_bits(layer_call(fg, ref, e_total=ref.e_total), base)
    finally:
        torch.set_default_dtype(old)
    assert same_bits(layer_call(fg, ref, e_total=torch.tensor(ref.e_total, dtype=torch.float64)), base)
    assert same_bits(layer_call(fg, ref, e_total=_dev(np.array([ref.e_total]))), base)
    # extra_psi_pow = 0.5 against a tensor of 0.5, under the bounds with c_n = 0.5
    refp = layer_reference(n, True)
    half = layer_call(fg, ref, extra_psi_pow=0.5)
    under_the_bounds(f"forms n {n} c = 0.5", refp, half[2], half[3])
    assert same_bits(layer_call(fg, ref, extra_psi_pow=_dev(refp.pow)), half) and not same_bits(half, base)
    assert same_bits(layer_call(fg, ref, extra_psi_pow=1.0), base)
    # a complex state_prob with a zero imaginary part against its real part
    p = _dev(ref.prob)
    assert same_bits(layer_call(fg, ref, state_prob=torch.complex(p, torch.zeros_like(p))), base)
    # a float32 eloc against eloc.double()
    e32 = _dev(ref.eloc).float()
    assert same_bits(layer_call(fg, ref, eloc=e32), layer_call(fg, ref, eloc=e32.double()))
    # a module wrapped in an object with .module (what DistributedDataParallel looks like)
    wrapped = type("Wrapped", (), {"module": m})()
    fw = G.FusedJastrowRbmGrad(wrapped, L_SORB)
    assert fw.module is m and same_bits(layer_call(fw, ref), base)


def test_layer_refuses_what_it_does_not_serve():
    from pynqs_amd import grad as G
    from pynqs_amd.rbm import RealRBM

    n = 65
    ref = layer_reference(n)
    rbm, _ = layer_params()
    m = new_module()
    fg = G.FusedJastrowRbmGrad(m, L_SORB)
    with pytest.raises(ValueError):
        layer_call(fg, ref, eloc=_dev(ref.eloc).to(torch.complex128))
    with pytest.raises(ValueError):
        G.FusedJastrowRbmGrad(m, L_SORB - 2)
    with pytest.raises(ValueError):
        G.FusedJastrowRbmGrad(RealRBM(_dev(rbm.W), _dev(rbm.hb), _dev(rbm.vb)).cuda(), L_SORB)
    with pytest.raises(ValueError):
        G.FusedRbmGrad(m, L_SORB)
