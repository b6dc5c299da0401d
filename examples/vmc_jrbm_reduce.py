"""The sampled VMC loop of vmc_jrbm_mcmc.py with the REDUCE local energy, the method the package is built around, for the Jastrow-RBM
(pynqs_amd.rbm.JastrowRBM): walkers from many Metropolis chains (pynqs_mcmc_jrbm), local energies from energy.local_energy(reduce_psi=True,
eps, eps_sample) -- the one-launch front end keeps |<x|H|x'>| >= eps and draws eps_sample of the rest, the amplitudes of the distinct x'
come from their parent walkers (pynqs_rbm_forward_children, then the Jastrow factor by pynqs_jastrow_children_apply: no module forward on
the x') and one kernel contracts --, the gradient from pynqs_amd.grad.FusedJastrowRbmGrad, Adam.  Synthetic sorb = 12 problem (3 alpha + 3
beta electrons, 400 determinants: the exact ground state is one eigvalsh away).  The energy falls; with draws it is an unbiased estimate of
the SIMPLE local energy's mean, noisier by the draws.

    python examples/vmc_jrbm_reduce.py [steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vmc_rbm_exact_sampling import all_determinants, synth_integrals  # noqa: E402

from pynqs_amd import C_extension as cx, energy, public_function as pf  # noqa: E402
from pynqs_amd.distributed import get_world_size  # noqa: E402
from pynqs_amd.grad import FusedJastrowRbmGrad  # noqa: E402
from pynqs_amd.mcmc import MCMCSampler  # noqa: E402
from pynqs_amd.rbm import JastrowRBM  # noqa: E402
from pynqs_amd.stats import dist_stats_moments  # noqa: E402


def run(steps=150, sorb=12, noA=3, noB=3, alpha=2, lr=0.02, nchains=8192, n_therm=20, n_sample=20, eps=0.1, eps_sample=20, seed=2024, log=print):
    """(energies per step, exact ground state)"""
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(seed)  # (the draws' seeds come from torch's host generator)
    dev = torch.device("cuda", torch.cuda.current_device())
    h1e, h2e = synth_integrals(sorb)
    # every <x|H|x> moves by -(noA + noB): REDUCE keeps a column only if |<x|H|x'>| >= eps, the diagonal included, and psi(x) is read from
    # the diagonal's record -- a walker whose <x|H|x> happened to lie below eps would have none (the spectrum shifts, nothing else changes)
    h1e = h1e.clone()
    h1e.view(sorb, sorb).diagonal().sub_(1.0)
    h1e, h2e = h1e.to(dev), h2e.to(dev)
    x_all = cx.tensor_to_onv(torch.from_numpy(all_determinants(sorb, noA, noB)).to(dev), sorb)
    g = torch.Generator().manual_seed(7)
    model = JastrowRBM(0.05 * (torch.rand(alpha * sorb, sorb, generator=g) - 0.5), 0.05 * (torch.rand(alpha * sorb, generator=g) - 0.5),
                       0.05 * (torch.rand(sorb, generator=g) - 0.5), torch.zeros(sorb, sorb)).to(dev)
    fused_grad = FusedJastrowRbmGrad(model, sorb)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    ab = lambda xx, func: pf.ansatz_batch(func, xx, 1 << 20, sorb, dev, torch.double)  # noqa: E731
    hmat = cx.get_hij_torch(x_all, x_all, h1e, h2e, sorb, noA + noB)
    e0 = float(torch.linalg.eigvalsh(hmat)[0])
    sampler = MCMCSampler(sorb, noA + noB, noA, noB, nchains, seed, x_all[:1].contiguous())
    sampler.run(model, 200, 0)  # first thermalisation from one determinant
    if sampler.lnpsi is None:
        raise RuntimeError("the sampler did not take the fused Jastrow-RBM chain kernel")
    hist = []
    for it in range(steps):
        x, counts, prob, _ = sampler.run(model, n_therm, n_sample)
        eloc, _, _, _ = energy.local_energy(x, h1e, h2e, model, ab, sorb, noA + noB, noA, noB, reduce_psi=True, eps=eps, eps_sample=eps_sample)
        if not bool(torch.isfinite(eloc).all()):
            raise RuntimeError("a local energy is not finite: eps above some |<x|H|x>|?")
        mean, var, sd, se = dist_stats_moments(eloc, prob, counts=int(counts.sum()), world_size=get_world_size())
        opt.zero_grad()
        fused_grad(x, prob, eloc, mean)
        opt.step()
        hist.append(float(mean))
        if it % 10 == 0 or it == steps - 1:
            log(f"step {it:3d}  <E> = {float(mean):+.8f}  var = {float(var):.3e}  acceptance {sampler.acceptance:.3f}  "
                f"({x.size(0)} distinct)   (exact ground state {e0:+.8f})")
    return hist, e0


if __name__ == "__main__":
    if "RANK" in os.environ:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        torch.distributed.init_process_group("nccl")
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 150)
