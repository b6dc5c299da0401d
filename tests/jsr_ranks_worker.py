"""Worker of tests/test_gpu_jrbm_sr.py::test_two_ranks_agree_with_one_rank (no tests here): one rank of a two-rank FusedJastrowRbmSR call,
started by `python -m torch.distributed.run --nproc-per-node 2` as a fresh process; backend gloo, both ranks on device 0 (the arrangement
of tests/sr_ranks_worker.py).  1027 Fe2S2-shaped walkers split by distributed.shard_bounds ("even": 514 + 513) or 1027 + 0 ("empty"),
probabilities pre-scaled by the world size.  Writes <out>_rank<k>.npz: d, F, iterations, converged, n.

    python -m torch.distributed.run --nproc-per-node 2 tests/jsr_ranks_worker.py even|empty <out>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

SORB, NO, H, N, SHIFT, TOL = 40, 15, 40, 1027, 0.02, 1e-10


def inputs():
    import jrbm_sr_exact as JS

    return JS.case_inputs(SORB, NO, H, N)


def main():
    import torch
    import torch.distributed as dist

    from pynqs_amd.distributed import shard_bounds
    from pynqs_amd.rbm import JastrowRBM
    from pynqs_amd.sr import FusedJastrowRbmSR

    split, out = sys.argv[1], sys.argv[2]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, ws = dist.get_rank(), dist.get_world_size()
    rbm, M, words, prob, eloc, e_total = inputs()
    b, e = shard_bounds(N, ws, rank) if split == "even" else ((0, N) if rank == 0 else (N, N))
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    m = JastrowRBM(T(rbm.W), T(rbm.hb), T(rbm.vb), T(M)).cuda()
    sr = FusedJastrowRbmSR(m, SORB, diag_shift=SHIFT, tol=TOL, max_iter=4000)
    onv = T(words.view(np.uint8).reshape(N, -1))[b:e].contiguous()
    sr(onv, T(prob)[b:e] * ws, T(eloc)[b:e], torch.as_tensor(e_total, device="cuda"))
    flat = lambda ts: np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts])  # noqa: E731
    np.savez(f"{out}_rank{rank}.npz", d=flat([p.grad for p in m.parameters()]), F=flat(sr.energy_grad), iterations=sr.iterations,
             converged=sr.converged, n=e - b)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
