"""The exact-sampling VMC optimisation of vmc_rbm_exact_sampling.py (sorb = 8, 2 alpha + 2 beta electrons, all 36 determinants with
p(x) = |psi(x)|^2 / sum) for two ansaetze side by side: a real RBM, and the same RBM times a two-body Jastrow factor exp(x^T M x)
(pynqs_amd.rbm.JastrowRBM) with the same hidden units and seed and M = 0 at the start -- so both begin at the same energy.  Both stay on
the fused kernels: local energies from pynqs_amd.energy.local_energy (pynqs_eloc_rbm / pynqs_eloc_jrbm), the gradient from
pynqs_amd.grad.FusedRbmGrad / FusedJastrowRbmGrad (pynqs_rbm_grad, pynqs_jastrow_grad), Adam.  Prints both energy traces and the exact
ground state of the same Hamiltonian.  Run under torchrun for several GPUs (the determinants are sharded over the ranks).

    python examples/vmc_rbm_jastrow.py [steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vmc_rbm_exact_sampling import all_determinants, synth_integrals  # noqa: E402

from pynqs_amd import C_extension as cx, energy, public_function as pf  # noqa: E402
from pynqs_amd.distributed import get_rank, get_world_size, shard_bounds  # noqa: E402
from pynqs_amd.grad import FusedJastrowRbmGrad, FusedRbmGrad  # noqa: E402
from pynqs_amd.rbm import JastrowRBM, RealRBM  # noqa: E402
from pynqs_amd.stats import dist_stats_moments  # noqa: E402


def run(steps=60, sorb=8, noA=2, noB=2, alpha=2, lr=0.05, log=print):
    """(energies of the RBM per step, energies of the Jastrow-RBM per step, exact ground state)"""
    torch.set_default_dtype(torch.float64)
    dev = torch.device("cuda", torch.cuda.current_device())
    ws = get_world_size()
    h1e, h2e = (t.to(dev) for t in synth_integrals(sorb))
    x_all = cx.tensor_to_onv(torch.from_numpy(all_determinants(sorb, noA, noB)).to(dev), sorb)
    b, e = shard_bounds(x_all.size(0), ws, get_rank())
    x = x_all[b:e].contiguous()
    g = torch.Generator().manual_seed(7)
    W, hb, vb = 0.05 * (torch.rand(alpha * sorb, sorb, generator=g) - 0.5), 0.05 * (torch.rand(alpha * sorb, generator=g) - 0.5), \
        0.05 * (torch.rand(sorb, generator=g) - 0.5)
    models = {"RBM": RealRBM(W, hb, vb).to(dev), "Jastrow-RBM": JastrowRBM(W, hb, vb, torch.zeros(sorb, sorb)).to(dev)}
    grads = {"RBM": FusedRbmGrad(models["RBM"], sorb), "Jastrow-RBM": FusedJastrowRbmGrad(models["Jastrow-RBM"], sorb)}
    opts = {k: torch.optim.Adam(m.parameters(), lr=lr) for k, m in models.items()}
    ab = lambda xx, func: pf.ansatz_batch(func, xx, 1 << 20, sorb, dev, torch.double)  # noqa: E731
    # exact ground state of the same Hamiltonian in the same determinant space, for reference
    hmat = cx.get_hij_torch(x_all, x_all, h1e, h2e, sorb, noA + noB)
    e0 = float(torch.linalg.eigvalsh(hmat)[0])
    hist = {k: [] for k in models}
    for it in range(steps):
        for k, model in models.items():
            eloc, _, psi, _ = energy.local_energy(x, h1e, h2e, model, ab, sorb, noA + noB, noA, noB)
            w = psi.abs() ** 2
            norm = w.sum()
            if ws > 1:
                torch.distributed.all_reduce(norm)
            prob = w / norm * ws  # pre-scaled by world_size like vmc/sample.py:772
            mean, var, sd, se = dist_stats_moments(eloc, prob, counts=x_all.size(0), world_size=ws)
            opts[k].zero_grad()
            grads[k](x, prob, eloc, mean)
            opts[k].step()
            hist[k].append(float(mean))
        if it % 10 == 0 or it == steps - 1:
            log(f"step {it:3d}  <E> RBM = {hist['RBM'][-1]:+.8f}   Jastrow-RBM = {hist['Jastrow-RBM'][-1]:+.8f}   (exact ground state {e0:+.8f})")
    lower = min(hist, key=lambda k: hist[k][-1])
    log(f"after {steps} steps the {lower} is lower by {abs(hist['RBM'][-1] - hist['Jastrow-RBM'][-1]):.3e} Ha")
    return hist["RBM"], hist["Jastrow-RBM"], e0


if __name__ == "__main__":
    if "RANK" in os.environ:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        torch.distributed.init_process_group("nccl")
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 60)
