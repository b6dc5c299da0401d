"""Worker of tests/test_gpu_rdm.py::test_two_ranks_agree_with_one_rank (no tests here): one rank of a two-rank
pynqs_amd.rdm.reduced_density_matrices call, started by `python -m torch.distributed.run --nproc-per-node 2` as a fresh process; backend
gloo, rank k on device k (modulo the number of devices).  37 walkers of sorb 12 (3 alpha, 2 beta) split by distributed.shard_bounds,
probabilities pre-scaled by the world size.  Writes <out>_rank<k>.npz: flat = (rdm1 | rdm2), n.

    python -m torch.distributed.run --nproc-per-node 2 tests/rdm_ranks_worker.py <out>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

SORB, NOA, NOB, H, N = 12, 3, 2, 8, 37


def inputs():
    import rbm_exact as R
    from conftest import rand_occ

    occ = rand_occ(N, SORB, NOA, NOB, seed=41)
    rbm = R.regime_params("fe2s2", "real", SORB, H, 7)
    w = np.random.default_rng(41).random(N) + 0.1
    return rbm, occ, R.pack_bits(occ.astype(bool)), w / w.sum()


def main():
    import torch
    import torch.distributed as dist

    from pynqs_amd.distributed import shard_bounds
    from pynqs_amd.rbm import RealRBM
    from pynqs_amd.rdm import reduced_density_matrices

    out = sys.argv[1]
    dist.init_process_group("gloo")
    rank, ws = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(rank % torch.cuda.device_count())
    rbm, occ, words, w = inputs()
    b, e = shard_bounds(N, ws, rank)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    m = RealRBM(T(rbm.W), T(rbm.hb), T(rbm.vb)).cuda()
    onv = T(words.view(np.uint8).reshape(N, -1))[b:e].contiguous()
    r = reduced_density_matrices(onv, T(w)[b:e] * ws, m, SORB, NOA + NOB, NOA, NOB, fused=True)
    np.savez(f"{out}_rank{rank}.npz", flat=np.concatenate([r.rdm1.cpu().numpy(), r.rdm2.cpu().numpy()]), n=e - b)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
