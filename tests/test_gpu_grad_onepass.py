"""pynqs_rbm_grad_loss_form: the one-pass schedule of the gradient's first kernel (the theta chains of 64 hidden units at a time side by
side, W staged in LDS where 64 rows fit, else read from global memory a batch ahead) against the two-pass schedule it replaces, in one
process and bit for bit -- gradient (torch.equal) and loss (as int64) -- for both workgroup sizes; and against the estimator through
autograd at tests/test_gpu_rbm_grad_groups.py's tolerances (1e-11 of the largest gradient entry, the loss to 1e-10).

Shapes: H around the pass of 32 and the super-pass of 64 hidden units (1, 31, 32, 33, 40, 63, 64, 65, 80); sorb 6, 40 and 70 (two words;
at 70 orbitals 64 complex rows of W are 70 KB and take the global-memory path, every other shape the LDS path); walker counts around
the group of 32."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ONEPASS, TWOPASS = 0, 1
HIDDEN = [1, 31, 32, 33, 40, 63, 64, 65, 80]
SYSTEMS = [(6, 2), (40, 15), (70, 20)]
WALKERS = [1, 31, 32, 33, 65]


def _model(kind, H, sorb, dev, seed):
    from pynqs_amd.rbm import ComplexRBM, RealRBM

    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)  # noqa: E731
    if kind == "complex":
        return ComplexRBM(0.3 * r(H, sorb, 2), 0.4 * r(H, 2), 0.2 * r(sorb, 2)).to(dev)
    return RealRBM(0.3 * r(H, sorb), 0.4 * r(H), 0.2 * r(sorb)).to(dev)


def _inputs(n, sorb, no, eloc_cplx, dev, seed):
    import bench as B

    g = torch.Generator().manual_seed(seed)
    x = B.synth_walkers(n, sorb, no, no, 17 + seed).to(dev)
    prob = torch.rand(n, generator=g, dtype=torch.float64)
    prob = (prob / prob.sum()).to(dev)
    eloc = torch.randn(n, generator=g, dtype=torch.float64) - 100.0
    if eloc_cplx:
        eloc = torch.complex(eloc, 0.1 * torch.randn(n, generator=g, dtype=torch.float64))
    eloc = eloc.to(dev)
    return x, prob, eloc, (prob * eloc).sum()


def _run(fg, schedule, block, args):
    fg.schedule, fg.block = schedule, block
    loss = fg(*args)
    return [p.grad.clone() for p in fg.params], loss.clone()


@pytest.mark.parametrize("sorb,no", SYSTEMS)
@pytest.mark.parametrize("H", HIDDEN)
def test_one_pass_equals_two_passes_bit_for_bit(H, sorb, no):
    from pynqs_amd import grad as G

    dev = torch.device("cuda")
    for kind in ("real", "complex"):
        m = _model(kind, H, sorb, dev, 3 + H)
        fg = G.FusedRbmGrad(m, sorb)
        for n in WALKERS:
            for eloc_cplx in (False, True):
                args = _inputs(n, sorb, no, eloc_cplx, dev, n)
                for block in (256, 512):
                    want, loss_want = _run(fg, TWOPASS, block, args)
                    got, loss_got = _run(fg, ONEPASS, block, args)
                    tag = f"{kind} H={H} sorb={sorb} n={n} eloc_cplx={eloc_cplx} B={block}"
                    assert all(torch.equal(a, b) for a, b in zip(got, want)), tag
                    assert torch.equal(loss_got.view(torch.int64), loss_want.view(torch.int64)), tag
                    again, loss_again = _run(fg, ONEPASS, block, args)  # two calls: the same bits
                    assert all(torch.equal(a, b) for a, b in zip(again, got)), tag
                    assert torch.equal(loss_again.view(torch.int64), loss_got.view(torch.int64)), tag


@pytest.mark.parametrize("H", [40, 65])
@pytest.mark.parametrize("kind,eloc_cplx", [("complex", True), ("complex", False), ("real", False), ("real", True)])
def test_one_pass_against_autograd(kind, eloc_cplx, H):
    from pynqs_amd import C_extension as cx, grad as G

    dev = torch.device("cuda")
    sorb, no, n = 40, 15, 65
    m = _model(kind, H, sorb, dev, 11)
    x, prob, eloc, e_tot = _inputs(n, sorb, no, eloc_cplx, dev, 5)
    dtype = torch.complex128 if (kind == "complex" or eloc_cplx) else torch.float64
    states = cx.onv_to_tensor(x, sorb).to(torch.float64)
    for p in m.parameters():
        p.grad = None
    loss_ref = G.grad(m, states, prob, eloc, e_tot, 1.0, dtype)
    want = [p.grad.clone() for p in m.parameters()]
    fg = G.FusedRbmGrad(m, sorb)
    for block in (256, 512):
        got, loss = _run(fg, ONEPASS, block, (x, prob, eloc, e_tot))
        scale = max(float(w.abs().max()) for w in want)
        err = max(float((a - w).abs().max()) for a, w in zip(got, want))
        print(f"{kind} eloc_cplx={eloc_cplx} H={H} B={block}: gradient error {err:.2e} (bound {1e-11 * scale:.2e}), "
              f"loss error {abs(float(loss) - float(loss_ref)):.2e}")
        for a, w in zip(got, want):
            assert a.shape == w.shape
            np.testing.assert_allclose(a.cpu().numpy(), w.cpu().numpy(), rtol=0, atol=1e-11 * scale)
        np.testing.assert_allclose(float(loss), float(loss_ref), rtol=0, atol=1e-10 * max(1.0, abs(float(loss_ref))))


def test_bad_schedule_and_block_are_refused():
    from pynqs_amd import grad as G

    dev = torch.device("cuda")
    m = _model("real", 8, 6, dev, 1)
    fg = G.FusedRbmGrad(m, 6)
    args = _inputs(4, 6, 2, False, dev, 2)
    for schedule, block in ((2, 0), (0, 128)):
        fg.schedule, fg.block = schedule, block
        with pytest.raises(RuntimeError, match="bad schedule / block"):
            fg(*args)
