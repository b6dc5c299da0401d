"""pynqs_rbm_grad_loss with the wider workgroups of its first kernel (32 walkers per workgroup as before, 16 threads per walker instead of
8) and the loss written a second time into a tensor of the caller's: walker counts around 16 and around the group of 32, against the
estimator through autograd at tests/test_gpu_rbm_grad.py's tolerances (1e-11 of the largest gradient entry, the loss to 1e-10)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SORB, NO, H = 40, 15, 37  # two passes of 32 hidden units, the second with 5 live ones


def _case(kind, eloc_cplx, n, dev, seed=0):
    import bench as B
    from pynqs_amd.rbm import ComplexRBM, RealRBM

    g = torch.Generator().manual_seed(3 + seed)
    r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)  # noqa: E731
    m = (ComplexRBM(0.3 * r(H, SORB, 2), 0.4 * r(H, 2), 0.2 * r(SORB, 2)) if kind == "complex" else RealRBM(0.3 * r(H, SORB), 0.4 * r(H), 0.2 * r(SORB))).to(dev)
    x = B.synth_walkers(n, SORB, NO, NO, 17 + seed).to(dev)
    prob = torch.rand(n, generator=g, dtype=torch.float64); prob = (prob / prob.sum()).to(dev)
    eloc = torch.randn(n, generator=g, dtype=torch.float64) - 100.0
    if eloc_cplx:
        eloc = torch.complex(eloc, 0.1 * torch.randn(n, generator=g, dtype=torch.float64))
    eloc = eloc.to(dev)
    return m, x, prob, eloc, (prob * eloc).sum()


@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 33, 65, 8192])
@pytest.mark.parametrize("kind,eloc_cplx", [("complex", True), ("complex", False), ("real", False), ("real", True)])
def test_gradient_and_loss_around_the_group_sizes(kind, eloc_cplx, n):
    from pynqs_amd import C_extension as cx, grad as G

    dev = torch.device("cuda")
    m, x, prob, eloc, e_tot = _case(kind, eloc_cplx, n, dev)
    dtype = torch.complex128 if (kind == "complex" or eloc_cplx) else torch.float64
    states = cx.onv_to_tensor(x, SORB).to(torch.float64)
    for p in m.parameters():
        p.grad = None
    loss_ref = G.grad(m, states, prob, eloc, e_tot, 1.0, dtype)
    want = [p.grad.clone() for p in m.parameters()]
    fg = G.FusedRbmGrad(m, SORB)
    loss = fg(x, prob, eloc, e_tot)
    scale = max(float(w.abs().max()) for w in want)
    err = max(float((p.grad - w).abs().max()) for p, w in zip(m.parameters(), want))
    print(f"{kind} eloc_cplx={eloc_cplx} n={n}: gradient error {err:.2e} (bound {1e-11 * scale:.2e}), loss error {abs(float(loss) - float(loss_ref)):.2e}")
    for p, w in zip(m.parameters(), want):
        assert p.grad.shape == w.shape
        np.testing.assert_allclose(p.grad.cpu().numpy(), w.cpu().numpy(), rtol=0, atol=1e-11 * scale)
    np.testing.assert_allclose(float(loss), float(loss_ref), rtol=0, atol=1e-10 * max(1.0, abs(float(loss_ref))))
    # two runs: the same bits (fixed order of additions), gradient and loss
    first = [p.grad.clone() for p in m.parameters()]
    loss_again = fg(x, prob, eloc, e_tot)
    assert all(torch.equal(a, p.grad) for a, p in zip(first, m.parameters()))
    assert torch.equal(loss.view(torch.int64), loss_again.view(torch.int64))
    # the returned loss is a tensor of its own: a following call (another <E>: another loss, also for one walker) leaves it alone
    assert loss.data_ptr() != loss_again.data_ptr() and loss.data_ptr() != fg.loss.data_ptr() and loss.shape == (1,)
    kept = float(loss)
    other = fg(x, prob, eloc, e_tot + 1.0)
    assert float(loss) == kept and float(fg.loss) == float(other) != kept
