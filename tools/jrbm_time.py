"""Time of the fused Jastrow-RBM local energy (pynqs_eloc_jrbm) on Fe2S2-shaped inputs (sorb 40, 15 alpha + 15 beta electrons, 80 hidden
units, 8192 walkers) against its yardstick, pynqs_eloc_rbm on the same walkers and RBM parameters, alternating in the same run; and the
module route for the same JastrowRBM (energy.FUSED_RBM = False: get_comb_tensor plus a module forward on every x').  Device events around
at least 0.2 s of work after a warm-up, twice, to show the spread.  Every GPU step is a child process of its own under a time limit, and
nothing starts after a step that failed.

    python tools/jrbm_time.py            # both steps: "pair" (the two kernels, alternating), then "module"
    python tools/jrbm_time.py pair       # one step, in this process
    python tools/jrbm_time.py loop       # 20 calls of each kernel, nothing timed: for rocprofv3 --kernel-trace --stats
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MIN_SEC = 0.2
LIMITS = {"pair": 180, "module": 300}  # seconds per step


def timed(fn, reps):
    import torch

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


def step(mode):
    import torch

    import bench as B
    from pynqs_amd import C_extension as cx, energy, public_function as pf
    from pynqs_amd.rbm import JastrowRBM

    sorb, no, H, n = 40, 15, 80, 8192
    nele = 2 * no
    g = torch.Generator().manual_seed(3)
    r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)  # noqa: E731
    m = JastrowRBM(0.3 * r(H, sorb), 0.4 * r(H), 0.2 * r(sorb), 0.2 * r(sorb, sorb)).cuda()
    onv = B.synth_walkers(n, sorb, no, no, 17).cuda().contiguous()
    pair = sorb * (sorb - 1) // 2
    h1e = (r(sorb, sorb) + r(sorb, sorb).t()).reshape(-1).cuda()
    h2e = r(pair * (pair + 1) // 2).cuda()
    ncomb = cx.get_Num_SinglesDoubles(sorb, no, no) + 1
    tag = f"sorb {sorb} H {H} n {n} (ncomb {ncomb})"
    if mode in ("pair", "loop"):
        table = cx.RBMTable(m.weights.detach(), m.hidden_bias.detach(), m.visible_bias.detach())
        jtable = cx.JastrowTable(m.jastrow.detach())
        jrbm = lambda: cx.eloc_jrbm(onv, h1e, h2e, table, jtable, sorb, nele, no, no)  # noqa: E731
        rbm = lambda: cx.eloc_rbm(onv, h1e, h2e, table, sorb, nele, no, no)  # noqa: E731
        if mode == "loop":
            for _ in range(20):
                jrbm(); rbm()
            torch.cuda.synchronize()
            print(f"{tag}: 20 calls each of pynqs_eloc_jrbm and pynqs_eloc_rbm")
            return
        for _ in range(2):
            tj, tr = per_call(jrbm), per_call(rbm)
            print(f"{tag}: pynqs_eloc_jrbm {tj * 1e3:8.3f} ms ({n / tj * 1e-6:.2f} M E_loc / s, {tj / tr:.3f} x pynqs_eloc_rbm) | "
                  f"pynqs_eloc_rbm {tr * 1e3:8.3f} ms ({n / tr * 1e-6:.2f} M E_loc / s)")
        return
    assert mode == "module", mode
    torch.set_default_dtype(torch.float64)
    energy.FUSED_RBM = False
    dev = onv.device
    ab = lambda xx, func: pf.ansatz_batch(func, xx, 1 << 20, sorb, dev, torch.double)  # noqa: E731
    chunk = 256  # walkers per call: 256 x ncomb rows of +-1 at a time

    def module():
        for b in range(0, n, chunk):
            energy.local_energy(onv[b:b + chunk], h1e, h2e, m, ab, sorb, nele, no, no)

    for _ in range(2):
        tm = per_call(module)
        print(f"{tag}: the module route (FUSED_RBM = False, {chunk} walkers per call) {tm * 1e3:8.3f} ms ({n / tm * 1e-6:.3f} M E_loc / s)")


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode != "all":
        step(mode)
        return
    for s in ("pair", "module"):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), s], timeout=LIMITS[s]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"step {s!r} ended with status {rc}: nothing further is started")
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
