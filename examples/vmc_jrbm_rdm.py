"""The exact-sampling loop of vmc_jrbm_sr.py (synthetic sorb = 12 problem, 3 alpha + 3 beta electrons, 400 determinants, Jastrow-RBM
psi(x) = exp(a.x + x^T M x) prod_h 2cosh(theta_h), stochastic reconfiguration from pynqs_amd.sr.FusedJastrowRbmSR) for a few steps, then
the reduced density matrices of the state it has reached from pynqs_amd.rdm.reduced_density_matrices (the fused kernel pynqs_rdm_jrbm):
the natural occupations, the spin density and the energy dot(h1e, rdm1) + dot(h2e, rdm2) next to the mean of the local energies of the
fused kernel pynqs_eloc_jrbm.  Run under torchrun for several GPUs.

    python examples/vmc_jrbm_rdm.py [steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vmc_rbm_exact_sampling import all_determinants, synth_integrals  # noqa: E402

from pynqs_amd import C_extension as cx, energy, public_function as pf  # noqa: E402
from pynqs_amd.distributed import get_rank, get_world_size, shard_bounds  # noqa: E402
from pynqs_amd.rbm import JastrowRBM  # noqa: E402
from pynqs_amd.rdm import reduced_density_matrices  # noqa: E402
from pynqs_amd.sr import FusedJastrowRbmSR  # noqa: E402
from pynqs_amd.stats import dist_stats_moments  # noqa: E402


def run(steps=10, sorb=12, noA=3, noB=3, alpha=2, lr=0.05, diag_shift=0.02, log=print):
    """(energy from the RDMs, mean local energy, natural occupations, spin density, exact ground state)"""
    torch.set_default_dtype(torch.float64)
    dev = torch.device("cuda", torch.cuda.current_device())
    ws = get_world_size()
    h1e, h2e = (t.to(dev) for t in synth_integrals(sorb))
    x_all = cx.tensor_to_onv(torch.from_numpy(all_determinants(sorb, noA, noB)).to(dev), sorb)
    g = torch.Generator().manual_seed(7)
    model = JastrowRBM(0.05 * (torch.rand(alpha * sorb, sorb, generator=g) - 0.5), 0.05 * (torch.rand(alpha * sorb, generator=g) - 0.5),
                       0.05 * (torch.rand(sorb, generator=g) - 0.5), torch.zeros(sorb, sorb)).to(dev)
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    sr = FusedJastrowRbmSR(model, sorb, diag_shift=diag_shift)
    ab = lambda xx, func: pf.ansatz_batch(func, xx, 1 << 20, sorb, dev, torch.double)  # noqa: E731
    e0 = float(torch.linalg.eigvalsh(cx.get_hij_torch(x_all, x_all, h1e, h2e, sorb, noA + noB))[0])
    b, e = shard_bounds(x_all.size(0), ws, get_rank())
    x = x_all[b:e].contiguous()

    def measure():
        eloc, _, psi, _ = energy.local_energy(x, h1e, h2e, model, ab, sorb, noA + noB, noA, noB)
        w = psi.abs() ** 2
        norm = w.sum()
        if ws > 1:
            torch.distributed.all_reduce(norm)
        prob = w / norm * ws  # pre-scaled by the world size
        mean, var, _, _ = dist_stats_moments(eloc, prob, counts=x_all.size(0), world_size=ws)
        return eloc, prob, mean, var

    for it in range(steps):
        eloc, prob, mean, var = measure()
        opt.zero_grad()
        sr(x, prob, eloc, mean)
        opt.step()
        if it % 5 == 0 or it == steps - 1:
            log(f"step {it:3d}  <E> = {float(mean):+.8f}  var = {float(var):.3e}   (exact ground state {e0:+.8f})")
    eloc, prob, mean, var = measure()
    rdm = reduced_density_matrices(x, prob, model, sorb, noA + noB, noA, noB)
    e_rdm = float(rdm.energy(h1e, h2e))
    occ, spin = rdm.natural_occupations(), rdm.spin_density()
    log(f"final state: <E> = {float(mean):+.10f} from the local energies, {e_rdm:+.10f} from the reduced density matrices"
        f" ({'fused' if rdm.fused else 'generic'} route)")
    log("natural occupations: " + " ".join(f"{v:.5f}" for v in occ))
    log("spin density:        " + " ".join(f"{v:+.5f}" for v in spin))
    return e_rdm, float(mean), occ, spin, e0


if __name__ == "__main__":
    if "RANK" in os.environ:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        torch.distributed.init_process_group("nccl")
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 10)
