"""Fixed-node Green's-function Monte Carlo on the GPU with a Jastrow-RBM trial function, every stage fused: the row of each walker from
pynqs_green_jrbm (pynqs_amd.gfmc.green_kernel recognises pynqs_amd.rbm.JastrowRBM), the move by the column's rank
(pynqs_gfmc_sample_rank), branching by all-gather.  The problem is that of examples/gfmc_rbm_fixed_node.py (sorb = 8, 2 alpha + 2 beta
electrons, synthetic integrals); the trial function is that example's RBM times a two-body Jastrow factor exp(x^T M x).

The Jastrow matrix (seed 4, entries uniform in +-0.05) was picked by diagonalising in the full determinant space (36 determinants, on the
CPU): it lowers both the variational energy of the trial function (+1.747 -> +1.348) and the fixed-node energy (+0.158 -> -0.951; the
exact ground state is -4.577), and leaves E_VMC - E_FN = 2.30, so "GFMC improved on the trial function" is a statement far outside the
statistical error (about 0.015 with 8192 walkers).

    python examples/gfmc_jrbm_fixed_node.py [generations] [walkers]        (also under torchrun: walkers are sharded over the ranks)
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.gfmc_rbm_fixed_node import all_determinants, fixed_node_reference, synth_integrals  # noqa: E402
from pynqs_amd import C_extension as cx, gfmc, public_function as pf  # noqa: E402
from pynqs_amd.distributed import get_rank, get_world_size  # noqa: E402
from pynqs_amd.rbm import JastrowRBM  # noqa: E402

JASTROW_SEED, JASTROW_SCALE = 4, 0.1


def trial_function(sorb, dev):
    g = torch.Generator().manual_seed(7)  # (the RBM of examples/gfmc_rbm_fixed_node.py)
    W, hb, vb = (0.3 * (torch.rand(2 * sorb, sorb, generator=g) - 0.5), 0.3 * (torch.rand(2 * sorb, generator=g) - 0.5),
                 0.3 * (torch.rand(sorb, generator=g) - 0.5))
    M = JASTROW_SCALE * (torch.rand(sorb, sorb, generator=torch.Generator().manual_seed(JASTROW_SEED)) - 0.5)
    return JastrowRBM(W, hb, vb, M).to(dev)


def run(generations=120, walkers=8192, burn_in=40, sorb=8, noA=2, noB=2, seed=3, log=print):
    torch.set_default_dtype(torch.float64)
    dev = torch.device("cuda", torch.cuda.current_device())
    nele = noA + noB
    h1e, h2e = (t.to(dev) for t in synth_integrals(sorb))
    x_all = cx.tensor_to_onv(torch.from_numpy(all_determinants(sorb, noA, noB)).to(dev), sorb)
    trial = trial_function(sorb, dev)
    ab = lambda xx, func: pf.ansatz_batch(func, xx, 1 << 20, sorb, dev, torch.double)  # noqa: E731
    with torch.no_grad():
        psi = ab(x_all, trial)
    hmat = cx.get_hij_torch(x_all, x_all, h1e, h2e, sorb, nele)
    e_exact, e_fn, e_vmc, diag_max = fixed_node_reference(hmat, psi)
    Lambda = diag_max + 0.5  # every diagonal kernel Lambda - H_FN(x, x) stays positive
    # this rank's walkers, drawn from |psi_T|^2
    torch.manual_seed(seed + 1000 * get_rank())
    n = walkers // get_world_size()
    x = x_all[torch.multinomial(psi * psi, n, replacement=True)].contiguous()
    w = torch.ones(n, device=dev)
    num = den = 0.0
    for it in range(generations):
        eloc, gk, comb, _, clamped = gfmc.green_kernel(x, Lambda, h1e, h2e, trial, ab, sorb, nele, noA, noB, torch.double, None, True)
        assert not bool(clamped.any())
        if it >= burn_in:  # mixed estimator on the current population (weights are 1 after the resampling below)
            s = torch.stack([(w * eloc).sum(), w.sum()])
            if get_world_size() > 1:
                torch.distributed.all_reduce(s)
            num, den = num + float(s[0]), den + float(s[1])
        x, w, beta, _ = gfmc.sample_update(x, w, comb, gk)
        x = gfmc.branching(x, w)  # resample in proportion to the weights (all ranks together)
        w = torch.ones(n, device=dev)
        if it % 20 == 0 and get_rank() == 0:
            log(f"generation {it:4d}  <beta> = {float(beta.mean()):.5f}  (Lambda - E_FN = {Lambda - e_fn:.5f})")
    e_gfmc = num / den
    if get_rank() == 0:
        log(f"E_exact = {e_exact:+.6f}   E_FN = {e_fn:+.6f}   E_GFMC = {e_gfmc:+.6f}   E_VMC(psi_T) = {e_vmc:+.6f}")
    return e_exact, e_fn, e_gfmc, e_vmc


if __name__ == "__main__":
    if "RANK" in os.environ:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        torch.distributed.init_process_group("nccl")
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 120, int(sys.argv[2]) if len(sys.argv) > 2 else 8192)
