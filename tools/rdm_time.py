"""Time of the reduced density matrices (pynqs_amd.rdm) on Fe2S2-shaped inputs (sorb 40, 15 alpha + 15 beta electrons, 80 hidden units,
8192 walkers): the fused call pynqs_rdm_rbm, the scatter call pynqs_rdm_scatter on a ratio row that is already there (its f64 atomic
adds alone: n (nD + nS (nele + 1) + nele (nele + 1) / 2) of them, hence the rate of scattered 8-byte adds), and, alternating in the same
run, pynqs_eloc_rbm on the same walkers -- the comparison value: the same number of amplitude ratios.  Device events around at least
0.2 s of work after a warm-up, twice, to show the spread.

    python tools/rdm_time.py            # the timings
    python tools/rdm_time.py loop       # 20 calls of each, nothing timed: for rocprofv3 --kernel-trace --stats
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402
from pynqs_amd import C_extension as cx  # noqa: E402
from pynqs_amd import rdm as M  # noqa: E402
from pynqs_amd.rbm import RealRBM  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "full"
MIN_SEC = 0.2


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def per_call(fn):
    t = timed(fn, 3)
    return timed(fn, max(3, int(MIN_SEC / max(t, 1e-7)) + 1))


def main():
    sorb, no, H, n = 40, 15, 80, 8192
    nele = 2 * no
    g = torch.Generator().manual_seed(3)
    r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)  # noqa: E731
    m = RealRBM(0.3 * r(H, sorb), 0.4 * r(H), 0.2 * r(sorb)).cuda()
    onv = B.synth_walkers(n, sorb, no, no, 17).cuda().contiguous()
    prob = torch.rand(n, generator=g, dtype=torch.float64)
    prob = (prob / prob.sum()).cuda()
    pair = sorb * (sorb - 1) // 2
    h1e = (r(sorb, sorb) + r(sorb, sorb).t()).reshape(-1).cuda()
    h2e = r(pair * (pair + 1) // 2).cuda()
    table = cx.RBMTable(m.weights.detach(), m.hidden_bias.detach(), m.visible_bias.detach())
    ncomb = cx.get_Num_SinglesDoubles(sorb, no, no) + 1
    nS = 2 * no * (sorb // 2 - no)
    adds = n * ((ncomb - 1 - nS) + nS * nele + nele * (nele + 1) // 2)
    ratio = 0.5 + torch.rand((n, ncomb), generator=g, dtype=torch.float64).cuda()
    out = torch.zeros(sorb * sorb + pair * (pair + 1) // 2, dtype=torch.float64, device="cuda")
    fused = lambda: M.reduced_density_matrices(onv, prob, m, sorb, nele, no, no, fused=True)  # noqa: E731
    scat = lambda: M.scatter(onv, prob, ratio, sorb, nele, no, no, out)  # noqa: E731
    eloc = lambda: cx.eloc_rbm(onv, h1e, h2e, table, sorb, nele, no, no)  # noqa: E731
    tag = f"sorb {sorb} H {H} n {n} (ncomb {ncomb})"
    if mode == "loop":
        for _ in range(20):
            fused(); scat(); eloc()
        torch.cuda.synchronize()
        print(f"{tag}: 20 calls each of the fused path, the scatter kernel and pynqs_eloc_rbm")
        return
    for _ in range(2):
        tf, ts, te = per_call(fused), per_call(scat), per_call(eloc)
        print(f"{tag}: fused {tf * 1e3:8.3f} ms ({tf / te:.2f} x pynqs_eloc_rbm) | scatter on a given ratio row {ts * 1e3:8.3f} ms "
              f"({adds / ts * 1e-9:.2f} G adds / s, {adds * 8 / ts * 1e-12:.3f} TB / s of 8-byte f64 atomic adds) | pynqs_eloc_rbm {te * 1e3:8.3f} ms")


if __name__ == "__main__":
    main()
