"""The loop of vmc_rbm_sr.py for the Jastrow-RBM (pynqs_amd.rbm.JastrowRBM, psi(x) = exp(a.x + x^T M x) prod_h 2cosh(theta_h); the same
seed, M = 0 at the start): synthetic sorb = 12 problem (3 alpha + 3 beta electrons, 400 determinants), local energies from the fused
kernel (pynqs_eloc_jrbm), and the natural-gradient direction d = (S + diag_shift)^-1 F from pynqs_amd.sr.FusedJastrowRbmSR (conjugate
gradients on the matrix-free product pynqs_jrbm_sr_matvec; F from pynqs_rbm_grad + pynqs_jastrow_grad), applied by torch.optim.SGD:
theta <- theta - lr d.  sampling="exact": all determinants with p(x) = |psi(x)|^2 / sum, sharded over the ranks; sampling="mcmc":
walkers from the fused Jastrow-RBM Metropolis chains (pynqs_amd.mcmc.MCMCSampler -> pynqs_mcmc_jrbm), merged across the ranks.  Run
under torchrun for several GPUs.

A float64 dense replay of the exact-sampling loop on the CPU (O[n, P] with the x_i x_j columns, dense S, LAPACK solve) gives, next to
the plain RBM of vmc_rbm_sr.py:

    step   plain RBM    Jastrow-RBM
     10    -5.762 396   -5.556 524
     20                 -6.301 823
     30    -6.611 981   -6.391 214
     39                 -6.420 400        (exact ground state -9.417 487)

The energy never rises (largest step-to-step change -1.97e-3).  Under SR with this shift and step the Jastrow-RBM is ABOVE the plain RBM
at equal step counts; the extra parameters are no shortcut here.

    python examples/vmc_jrbm_sr.py [steps] [exact|mcmc]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vmc_rbm_exact_sampling import all_determinants, synth_integrals  # noqa: E402

from pynqs_amd import C_extension as cx, energy, public_function as pf  # noqa: E402
from pynqs_amd.distributed import get_rank, get_world_size, shard_bounds  # noqa: E402
from pynqs_amd.mcmc import MCMCSampler  # noqa: E402
from pynqs_amd.rbm import JastrowRBM  # noqa: E402
from pynqs_amd.sr import FusedJastrowRbmSR  # noqa: E402
from pynqs_amd.stats import dist_stats_moments  # noqa: E402


def run(steps=40, sorb=12, noA=3, noB=3, alpha=2, lr=0.05, diag_shift=0.02, sampling="exact", tol=1e-6, max_iter=1000, nchains=8192,
        n_therm=20, n_sample=20, seed=2024, log=print):
    """(energies per step, exact ground state)"""
    if sampling not in ("exact", "mcmc"):
        raise ValueError(f"sampling {sampling!r}")
    torch.set_default_dtype(torch.float64)
    dev = torch.device("cuda", torch.cuda.current_device())
    ws = get_world_size()
    h1e, h2e = (t.to(dev) for t in synth_integrals(sorb))
    x_all = cx.tensor_to_onv(torch.from_numpy(all_determinants(sorb, noA, noB)).to(dev), sorb)
    g = torch.Generator().manual_seed(7)
    model = JastrowRBM(0.05 * (torch.rand(alpha * sorb, sorb, generator=g) - 0.5), 0.05 * (torch.rand(alpha * sorb, generator=g) - 0.5),
                       0.05 * (torch.rand(sorb, generator=g) - 0.5), torch.zeros(sorb, sorb)).to(dev)
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    sr = FusedJastrowRbmSR(model, sorb, diag_shift=diag_shift, tol=tol, max_iter=max_iter)
    ab = lambda xx, func: pf.ansatz_batch(func, xx, 1 << 20, sorb, dev, torch.double)  # noqa: E731
    # exact ground state of the same Hamiltonian in the same determinant space, for reference
    hmat = cx.get_hij_torch(x_all, x_all, h1e, h2e, sorb, noA + noB)
    e0 = float(torch.linalg.eigvalsh(hmat)[0])
    if sampling == "mcmc":
        sampler = MCMCSampler(sorb, noA + noB, noA, noB, nchains, seed, x_all[:1].contiguous())
        sampler.run(model, 200, 0)  # first thermalisation from one determinant
        if sampler.lnpsi is None:
            raise RuntimeError("the sampler did not take the fused Jastrow-RBM chain kernel")
    else:
        b, e = shard_bounds(x_all.size(0), ws, get_rank())
        x = x_all[b:e].contiguous()
    hist = []
    for it in range(steps):
        if sampling == "mcmc":
            x, counts, prob, _ = sampler.run(model, n_therm, n_sample)
            eloc, _, _, _ = energy.local_energy(x, h1e, h2e, model, ab, sorb, noA + noB, noA, noB)
            total = int(counts.sum())
        else:
            eloc, _, psi, _ = energy.local_energy(x, h1e, h2e, model, ab, sorb, noA + noB, noA, noB)
            w = psi.abs() ** 2
            norm = w.sum()
            if ws > 1:
                torch.distributed.all_reduce(norm)
            prob = w / norm * ws  # pre-scaled by world_size like vmc/sample.py:772
            total = x_all.size(0)
        mean, var, sd, se = dist_stats_moments(eloc, prob, counts=total, world_size=ws)
        opt.zero_grad()
        sr(x, prob, eloc, mean)
        opt.step()
        hist.append(float(mean))
        if it % 10 == 0 or it == steps - 1:
            log(f"step {it:3d}  <E> = {float(mean):+.8f}  var = {float(var):.3e}  CG {sr.iterations} iterations, residual {sr.residual:.1e}"
                f"   (exact ground state {e0:+.8f})")
    return hist, e0


if __name__ == "__main__":
    if "RANK" in os.environ:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        torch.distributed.init_process_group("nccl")
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 40, sampling=sys.argv[2] if len(sys.argv) > 2 else "exact")
