"""Many-chain Metropolis sampler (pynqs_amd.mcmc, pynqs_mcmc_rbm / pynqs_mcmc_accept) against
 (i) a host transliteration of Sampler.MCMC's loop (vmc/sample.py:480-569) with the documented random streams (include/pynqs_amd.h),
 (ii) the generic path (spin_flip_rand -> module forward -> pynqs_mcmc_accept) for every RBM flavour and 1-3 ONV words,
 (iii) the exact |psi|^2 law and energy at sorb 12, and
 (iv) sharding, continuation, argument errors and the VMC example.  Every seed is fixed."""
import math
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

from conftest import synth_integrals
from mcmc_replay import host_r0, host_u

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mods():
    from pynqs_amd import C_extension, mcmc, rbm

    assert torch.cuda.is_available()
    return C_extension, mcmc, rbm


class Opaque(nn.Module):
    """The same amplitude behind a module the sampler does not recognise as an RBM: the generic path."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner(x)


def rand_rbm(rbm, sorb, H, kind, seed, scale=0.2):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: scale * (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)
    if kind == "complex":
        return rbm.ComplexRBM(r(H, sorb, 2), r(H, 2), r(sorb, 2)).cuda()
    return rbm.RealRBM(r(H, sorb), r(H), 4 * r(sorb), kind).cuda()


def first_det(cx, sorb, noA, noB):
    occ = np.zeros((1, sorb), dtype=np.uint8)
    occ[0, 0:2 * noA:2] = 1
    occ[0, 1:2 * noB:2] = 1
    return cx.tensor_to_onv(torch.from_numpy(occ).cuda(), sorb)


def test_matches_host_transliteration(mods):
    cx, mcmc, rbm = mods
    sorb, noA, noB, nch, nsteps, seed = 8, 2, 2, 64, 60, 987654321
    nsd = cx.get_Num_SinglesDoubles(sorb, noA, noB)
    model = rand_rbm(rbm, sorb, 16, "real", 3, scale=1.0)
    x0 = first_det(cx, sorb, noA, noB)
    c = np.arange(nch, dtype=np.uint64)
    # rank r0 - 1 of spin_flip_rand is column r0 of get_comb_tensor
    x = x0.repeat(nch, 1).contiguous()
    comb, _ = cx.get_comb_tensor(x, sorb, noA + noB, noA, noB)
    from pynqs_amd import _native as N

    out = torch.empty_like(x)
    N.check(N.lib().pynqs_spin_flip_rand(x.data_ptr(), nch, sorb, noA, noB, seed, (5 << 32) + 0, out.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "spin_flip_rand")
    r0 = host_r0(seed, 5, c, nsd)
    assert torch.equal(out, comb[torch.arange(nch, device="cuda"), torch.from_numpy(r0).cuda()])
    # the host model: Sampler.MCMC's loop per chain, vectorised over the chains
    state = x0.repeat(nch, 1).contiguous()
    psi = model(cx.onv_to_tensor(state, sorb)).detach().cpu().numpy()
    recs, nacc = [], np.zeros(nch, dtype=np.int64)
    n_therm = 10
    for t in range(nsteps):
        comb, _ = cx.get_comb_tensor(state, sorb, noA + noB, noA, noB)
        r0 = torch.from_numpy(host_r0(seed, t, c, nsd)).cuda()
        prop = comb[torch.arange(nch, device="cuda"), r0].contiguous()
        psi_p = model(cx.onv_to_tensor(prop, sorb)).detach().cpu().numpy()
        b = psi * psi
        acc = (b == 0) | (host_u(seed, t, c) <= (psi_p * psi_p) / b)
        acc_d = torch.from_numpy(acc).cuda()
        state = torch.where(acc_d[:, None], prop, state).contiguous()
        psi = np.where(acc, psi_p, psi)
        if t >= n_therm:
            nacc += acc
            recs.append(state.clone())
    want = torch.stack(recs).view(torch.int64)
    for ansatz in (model, Opaque(model)):
        s = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, seed, x0)
        s.run(ansatz, n_therm, nsteps - n_therm, keep_records=True)
        assert torch.equal(s.last_records.reshape(want.shape), want)
        assert np.array_equal(s.n_accept.cpu().numpy(), nacc)
        assert torch.equal(s.states, state)


def _flavour_cases():
    cases = [(40, 15, 15, kind, "fe2s2") for kind in ("real", "tanh", "pRBM", "complex", "cos")]
    cases += [(80, 3, 2, "real", None), (130, 2, 3, "complex", None), (184, 4, 4, "tanh", None)]
    return cases


@pytest.mark.parametrize("sorb,noA,noB,kind,start", _flavour_cases())
def test_fused_equals_generic(mods, fe2s2, sorb, noA, noB, kind, start):
    cx, mcmc, rbm = mods
    nch, nsteps, seed = 4096, 300, 12345 + sorb
    H = 40 if start == "fe2s2" else sorb
    model = rand_rbm(rbm, sorb, H, kind, sorb + len(kind))
    if start == "fe2s2":
        x0 = torch.from_numpy(np.ascontiguousarray(fe2s2["ci_space"][:nch])).cuda()
    else:
        x0 = first_det(cx, sorb, noA, noB)
    from pynqs_amd.energy import _complex_rbm_params, _real_rbm_params

    assert mcmc._Fused.applies(model, sorb) and not mcmc._Fused.applies(Opaque(model), sorb)
    a = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, seed, x0)
    b = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, seed, x0)
    a.run(model, 20, nsteps - 20, keep_records=True)
    b.run(Opaque(model), 20, nsteps - 20, keep_records=True)
    assert a.last_records.size(0) == nsteps - 20
    assert torch.equal(a.last_records, b.last_records)
    assert torch.equal(a.n_accept, b.n_accept)
    assert 0.0 < a.acceptance <= 1.0
    if kind == "pRBM":
        assert a.acceptance == 1.0
    # the tracked ln|psi| of the final states
    if kind in ("real", "tanh", "pRBM"):
        W, hb, vb, _ = _real_rbm_params(model)
        ref = cx.rbm_forward(a.states, W, hb, vb, sorb, kind).abs().log()
    else:
        W, hb, vb, _, _ = _complex_rbm_params(model)  # (cos: the complex parameters it maps to, constant H ln 2 included)
        ref = cx.rbm_forward(a.states, W, hb, vb, sorb, "complex").abs().log()
    assert float((a.lnpsi - ref).abs().max()) <= 1e-10


def _exact_law(cx, rbm, kind):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from vmc_rbm_exact_sampling import all_determinants

    sorb, noA, noB = 12, 3, 3
    x_all = cx.tensor_to_onv(torch.from_numpy(all_determinants(sorb, noA, noB)).cuda(), sorb)
    model = rand_rbm(rbm, sorb, 24, kind, 99, scale=0.15 if kind == "real" else 0.3)  # |psi|^2 spans 2-3 decades
    psi = model(cx.onv_to_tensor(x_all, sorb)).detach()
    p = psi.abs() ** 2
    return sorb, noA, noB, x_all, model, psi, (p / p.sum()).cpu().numpy()


@pytest.mark.parametrize("kind", ["real", "complex", "tanh", "cos"])
def test_stationary_law(mods, kind):
    cx, mcmc, rbm = mods
    sorb, noA, noB, x_all, model, _, p = _exact_law(cx, rbm, kind)
    assert p.max() / p.min() > 20  # a spread of |psi|^2
    _chi_square(mcmc, sorb, noA, noB, x_all, model, p)


def test_stationary_law_prbm(mods):
    """pRBM: |psi| = 1, so the chains' law is uniform over the space."""
    cx, mcmc, rbm = mods
    sorb, noA, noB, x_all, model, _, p = _exact_law(cx, rbm, "pRBM")
    assert np.allclose(p, 1.0 / p.size, rtol=1e-12, atol=0)
    _chi_square(mcmc, sorb, noA, noB, x_all, model, p)


def _chi_square(mcmc, sorb, noA, noB, x_all, model, p):
    from scipy.stats import chi2

    nch = 65536
    s = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, 2718, x_all[:1].contiguous())
    s.run(model, 300, 0)
    keys = x_all.view(torch.int64).view(-1).cpu().numpy()
    order = np.argsort(keys)
    idx = order[np.searchsorted(keys[order], s.states.view(torch.int64).view(-1).cpu().numpy())]
    assert np.array_equal(keys[idx], s.states.view(torch.int64).view(-1).cpu().numpy())
    obs = np.bincount(idx, minlength=keys.size).astype(np.float64)
    exp_ = nch * p
    small = exp_ < 5
    o = np.append(obs[~small], obs[small].sum()) if small.any() else obs
    e = np.append(exp_[~small], exp_[small].sum()) if small.any() else exp_
    stat = float(((o - e) ** 2 / e).sum())
    assert stat < chi2.isf(1e-6, o.size - 1), (stat, o.size)


@pytest.mark.parametrize("kind", ["real", "complex"])
def test_energy(mods, kind):
    cx, mcmc, rbm = mods
    sorb, noA, noB, x_all, model, psi, p = _exact_law(cx, rbm, kind)
    h1e, h2e = (torch.as_tensor(t).cuda() for t in synth_integrals(sorb))
    from pynqs_amd.energy import _complex_rbm_params, _real_rbm_params

    def eloc(x):
        if kind == "real":
            W, hb, vb, _ = _real_rbm_params(model)
            return cx.eloc_rbm(x, h1e, h2e, cx.RBMTable(W, hb, vb), sorb, noA + noB, noA, noB)[0]
        W, hb, vb, _, _ = _complex_rbm_params(model)
        return cx.eloc_crbm(x, h1e, h2e, cx.CRBMTable(W, hb, vb), sorb, noA + noB, noA, noB)[0]

    e_all = eloc(x_all)
    exact = complex((torch.from_numpy(p).cuda() * e_all).sum())
    nch, nrec = 16384, 40
    s = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, 31415, x_all[:1].contiguous())
    s.run(model, 300, 0)
    u, counts, prob, lut = s.run(model, 0, nrec * 5, every=5, keep_records=True)
    e_u = eloc(u)
    est = complex((prob * e_u).sum())
    # psi of the LUT = the ansatz's
    np.testing.assert_allclose(lut.wf_value.cpu().numpy(), model(cx.onv_to_tensor(lut.bra_key, sorb)).detach().cpu().numpy(), rtol=1e-12)
    # standard error from the per-chain means of the records
    rec = s.last_records.reshape(-1, 1)
    keys = u.view(torch.int64).view(-1)
    pos = torch.searchsorted(keys, rec.view(-1)) if bool((keys[1:] > keys[:-1]).all()) else None
    if pos is None:  # (keys in byte order, not int64 order: look the rows up by sorting)
        order = torch.argsort(keys)
        pos = order[torch.searchsorted(keys[order], rec.view(-1))]
    assert torch.equal(keys[pos], rec.view(-1))
    chain_mean = e_u[pos].reshape(nrec, nch).mean(0).real.double().cpu().numpy()
    se = chain_mean.std(ddof=1) / math.sqrt(nch)
    assert abs(est.real - exact.real) <= 5 * se, (est, exact, se)


def test_sharding_and_continuation(mods):
    cx, mcmc, rbm = mods
    sorb, noA, noB, nch = 40, 15, 15, 2048
    model = rand_rbm(rbm, sorb, 40, "real", 5)
    x0 = first_det(cx, sorb, noA, noB)
    whole = mcmc.MCMCSampler(sorb, 30, 15, 15, nch, 77, x0)
    lo = mcmc.MCMCSampler(sorb, 30, 15, 15, nch // 2, 77, x0, chain_base=0)
    hi = mcmc.MCMCSampler(sorb, 30, 15, 15, nch // 2, 77, x0, chain_base=nch // 2)
    for s in (whole, lo, hi):
        s.run(model, 30, 40, keep_records=True)
    assert torch.equal(torch.cat([lo.last_records, hi.last_records], 1), whole.last_records)
    assert torch.equal(torch.cat([lo.n_accept, hi.n_accept]), whole.n_accept)
    assert torch.equal(torch.cat([lo.states, hi.states]), whole.states)
    # run(n_therm, 2k) == run(n_therm, k) + run(0, k), fused and generic
    for ansatz in (model, Opaque(model)):
        one = mcmc.MCMCSampler(sorb, 30, 15, 15, 512, 78, x0)
        two = mcmc.MCMCSampler(sorb, 30, 15, 15, 512, 78, x0)
        u1, c1, p1, _ = one.run(ansatz, 10, 60, keep_records=True)
        two.run(ansatz, 10, 30, keep_records=True)
        r_a = two.last_records
        two.run(ansatz, 0, 30, keep_records=True)
        assert torch.equal(torch.cat([r_a, two.last_records]), one.last_records)
        assert torch.equal(one.n_accept, two.n_accept) and torch.equal(one.states, two.states)
        assert int(c1.sum()) == 60 * 512 and torch.allclose(p1.sum(), torch.ones((), dtype=torch.float64, device=p1.device))
        flat = one.last_records.reshape(-1, one.len)
        assert u1.size(0) == torch.unique(flat, dim=0).size(0)


def test_errors(mods):
    cx, mcmc, rbm = mods
    from pynqs_amd import _native as N

    x0 = first_det(cx, 40, 15, 15)
    with pytest.raises(RuntimeError):
        mcmc.MCMCSampler(40, 30, 14, 16, 8, 1, x0)  # wrong alpha / beta counts
    with pytest.raises(RuntimeError):
        mcmc.MCMCSampler(40, 30, 15, 15, 8, 1, x0[:, :4].contiguous())  # wrong row length
    s = mcmc.MCMCSampler(40, 30, 15, 15, 8, 1, x0)
    with pytest.raises(RuntimeError):
        s.run(rand_rbm(rbm, 38, 40, "real", 1), 1, 1)  # parameters of another sorb
    tab = cx.RBMTable(*(t.detach() for t in (rand_rbm(rbm, 40, 40, "real", 1).weights, rand_rbm(rbm, 40, 40, "real", 1).hidden_bias)))
    for flav, H in ((3, 40), (99, 40), (N.RBM_REAL, 513)):
        assert N.lib().pynqs_mcmc_rbm_supported(40, H, flav) == 0
        with pytest.raises(RuntimeError):
            N.check(N.lib().pynqs_mcmc_rbm(s._x.data_ptr(), 8, 40, 15, 15, tab.data_ptr(), H, flav, 1, 0, 0, 1, 1, None, None, None,
                                           torch.cuda.current_stream().cuda_stream), "pynqs_mcmc_rbm")
    assert not mcmc.mcmc_rbm_supported(40, 40, "cos")  # (cos reaches the kernel as complex parameters)


def test_vmc_example_converges():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import vmc_rbm_mcmc

    hist, e0 = vmc_rbm_mcmc.run(log=lambda *a: None)
    final = float(np.mean(hist[-10:]))
    # the optimisation with the sampler's own walkers lowers the energy by volts and stays variational (a real, positive RBM cannot
    # carry the sign structure of this random Hamiltonian's ground state, so it does not reach e0 itself)
    assert final < hist[0] - 3.0 and final > e0 - 0.05, (final, e0, hist[::10])
