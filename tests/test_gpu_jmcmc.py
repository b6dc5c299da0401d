"""The many-chain Metropolis sampler for the Jastrow-RBM (pynqs_amd.rbm.JastrowRBM -> pynqs_mcmc_jrbm):
 (i) the route: the module is recognised, an opaque wrapper is not; the fused run leaves ln|psi| of the final states;
 (ii) the fused kernel against the generic path (spin_flip_rand -> module forward -> pynqs_mcmc_accept), record for record, 1-3 words;
 (iii) the exact |psi|^2 law at sorb 12, which the law of the RBM without M does not pass;
 (iv) the sampled VMC example.  Every seed is fixed."""
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_mcmc import Opaque, _chi_square, first_det, rand_rbm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mods():
    from pynqs_amd import C_extension, mcmc, rbm

    assert torch.cuda.is_available()
    return C_extension, mcmc, rbm


def rand_jrbm(rbm, sorb, H, seed, amp=0.1, scale=0.2):
    """rand_rbm's real RBM times exp(x^T M x), M a full matrix with entries uniform in +-amp."""
    base = rand_rbm(rbm, sorb, H, "real", seed, scale=scale)
    g = torch.Generator().manual_seed(seed + 1000)
    M = 2 * amp * (torch.rand(sorb, sorb, generator=g, dtype=torch.float64) - 0.5)
    return rbm.JastrowRBM(base.weights.detach(), base.hidden_bias.detach(), base.visible_bias.detach(), M.cuda()).cuda(), base


def test_route(mods):
    cx, mcmc, rbm = mods
    sorb, noA, noB, nch = 40, 5, 5, 512
    model, _ = rand_jrbm(rbm, sorb, 40, 3)
    assert mcmc.mcmc_jrbm_supported(sorb, 40) and not mcmc.mcmc_jrbm_supported(sorb, 513)
    assert mcmc._Fused.applies(model, sorb) and not mcmc._Fused.applies(Opaque(model), sorb)
    assert not mcmc._Fused.applies(model, sorb + 2)  # parameters of another sorb
    x0 = first_det(cx, sorb, noA, noB)
    a = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, 11, x0)
    b = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, 11, x0)
    ua, ca, pa, lut = a.run(model, 10, 40)
    b.run(Opaque(model), 10, 40)
    assert a.lnpsi is not None and b.lnpsi is None
    assert torch.equal(a.states, b.states)
    from pynqs_amd.energy import _jastrow_rbm_params

    W, hb, vb, M = _jastrow_rbm_params(model)
    ref = cx.jrbm_forward(a.states, W, hb, vb, M, sorb).abs().log()
    assert float((a.lnpsi - ref).abs().max()) <= 1e-10
    # psi of the LUT = the ansatz's
    np.testing.assert_allclose(lut.wf_value.cpu().numpy(), model(cx.onv_to_tensor(lut.bra_key, sorb)).detach().cpu().numpy(), rtol=1e-12)
    assert int(ca.sum()) == 40 * nch
    # float32 parameters: the float64 kernel would not make the module's decisions, so the generic path serves
    assert not mcmc._Fused.applies(model.float(), sorb)


@pytest.mark.parametrize("sorb,noA,noB,H,start", [(40, 15, 15, 40, "fe2s2"), (80, 3, 2, 80, None), (130, 2, 3, 16, None)])
def test_fused_equals_generic(mods, fe2s2, sorb, noA, noB, H, start):
    cx, mcmc, rbm = mods
    nch, nsteps, seed = 4096, 300, 54321 + sorb
    model, _ = rand_jrbm(rbm, sorb, H, sorb + 1)
    if start == "fe2s2":
        x0 = torch.from_numpy(np.ascontiguousarray(fe2s2["ci_space"][:nch])).cuda()
    else:
        x0 = first_det(cx, sorb, noA, noB)
    assert mcmc._Fused.applies(model, sorb) and not mcmc._Fused.applies(Opaque(model), sorb)
    a = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, seed, x0)
    b = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, seed, x0)
    a.run(model, 20, nsteps - 20, keep_records=True)
    b.run(Opaque(model), 20, nsteps - 20, keep_records=True)
    assert a.lnpsi is not None and b.lnpsi is None
    assert a.last_records.size(0) == nsteps - 20
    assert torch.equal(a.last_records, b.last_records), "fused and generic records differ"
    assert torch.equal(a.n_accept, b.n_accept)
    assert 0.0 < a.acceptance < 1.0, a.acceptance


def test_stationary_law(mods):
    """65536 chains, 300 steps from one determinant, all 400 determinants of sorb 12: the chains' law is |psi_J|^2 (chi-square at level
    1e-6) and the same counts fail against |psi_RBM|^2, the law with M dropped.  M (entries uniform in +-0.1, seed below) was chosen on
    the CPU: the exact chi-square distance of the two laws, nchains sum (p_J - p_RBM)^2 / p_RBM, is ~9e4 against a critical value of
    ~550, and the law after 300 steps of the exact transition matrix is the stationary one to 1e-20."""
    from scipy.stats import chi2

    cx, mcmc, rbm = mods
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from vmc_rbm_exact_sampling import all_determinants

    sorb, noA, noB = 12, 3, 3
    x_all = cx.tensor_to_onv(torch.from_numpy(all_determinants(sorb, noA, noB)).cuda(), sorb)
    base = rand_rbm(rbm, sorb, 24, "real", 99, scale=0.15)
    g = torch.Generator().manual_seed(5)
    M = 0.2 * (torch.rand(sorb, sorb, generator=g, dtype=torch.float64) - 0.5)
    model = rbm.JastrowRBM(base.weights.detach(), base.hidden_bias.detach(), base.visible_bias.detach(), M.cuda()).cuda()
    assert mcmc._Fused.applies(model, sorb)

    def law(m):
        p = m(cx.onv_to_tensor(x_all, sorb)).detach().abs() ** 2
        return (p / p.sum()).cpu().numpy()

    p_j, p_r = law(model), law(base)
    assert p_j.max() / p_j.min() > 20
    dist = 65536 * float(((p_j - p_r) ** 2 / p_r).sum())
    assert dist > 50 * chi2.isf(1e-6, p_j.size - 1), dist
    _chi_square(mcmc, sorb, noA, noB, x_all, model, p_j)
    with pytest.raises(AssertionError):  # (the same seed, so the same counts)
        _chi_square(mcmc, sorb, noA, noB, x_all, model, p_r)


def test_vmc_example_converges():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import vmc_jrbm_mcmc

    hist, e0 = vmc_jrbm_mcmc.run(log=lambda *a: None)
    final = float(np.mean(hist[-10:]))
    # the bar of test_gpu_mcmc.test_vmc_example_converges: the optimisation on the sampler's own walkers lowers the energy by volts and
    # stays variational
    assert final < hist[0] - 3.0 and final > e0 - 0.05, (final, e0, hist[::10])
