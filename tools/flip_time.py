"""Time of the fused spin-flip-projected local energy (pynqs_eloc_rbm_flip, pynqs_eloc_jrbm_flip: the plain pass, the signed pass on the
mirrored table, a combine kernel) on 8192 Fe2S2-shaped walkers (sorb 40, 15 alpha + 15 beta electrons, Fe2S2's integrals) with 40 and 80
hidden units, against the plain kernels on the same walkers and parameters (pynqs_eloc_rbm, pynqs_eloc_jrbm), alternating in the same
run; and the generic route of the same form (energy.FUSED_RBM = False: comb_x, its flip and a module forward on 2 x nbatch x ncomb rows)
on 512 walkers, scaled to 8192.  Device events around at least 0.2 s of work after a warm-up, three times, to show the spread.  Every GPU
step is a child process of its own under a time limit, and nothing starts after a step that failed.  The lines go to stdout and to
profiles/flip_time.txt.

    python tools/flip_time.py            # the steps "pair" (RBM), "jpair" (Jastrow-RBM), "generic"
    python tools/flip_time.py pair       # one step, in this process
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "flip_time.txt")
MIN_SEC = 0.2
LIMITS = {"pair": 180, "jpair": 180, "generic": 300}  # seconds per step
HEADER = ("# tools/flip_time.py on one MI355X: sorb 40, 15 + 15 electrons, Fe2S2's integrals, 8192 synthetic walkers; ms per call from device events\n"
          "# around >= 0.2 s of work, three repeats per line group (their spread is the run-to-run spread quoted in the README).\n"
          "# Not measured: hardware counters, a kernel trace, multi-rank runs.\n")


def say(line):
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


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
    import numpy as np
    import torch

    import bench as B
    from pynqs_amd import C_extension as cx, energy, public_function as pf
    from pynqs_amd.rbm import JastrowRBM, RealRBM

    sorb, no, n = 40, 15, 8192
    nele = 2 * no
    d = np.load(os.path.join(ROOT, "tests", "golden", "fe2s2_inputs.npz"))
    h1e = torch.from_numpy(np.ascontiguousarray(d["h1e"], dtype=np.float64)).cuda()
    h2e = torch.from_numpy(np.ascontiguousarray(d["h2e"], dtype=np.float64)).cuda()
    onv = B.synth_walkers(n, sorb, no, no, 17).cuda().contiguous()
    eta, norm = -1.0, torch.tensor(1.3, dtype=torch.float64, device="cuda")
    for H in (40, 80):
        g = torch.Generator().manual_seed(3)
        r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)  # noqa: E731
        W, hb, vb, M = (0.3 * r(H, sorb)).cuda(), (0.4 * r(H)).cuda(), (0.2 * r(sorb)).cuda(), (0.2 * r(sorb, sorb)).cuda()
        tag = f"H {H:3d}"
        table, mirror = cx.RBMTable(W, hb, vb), cx.mirrored_rbm_table(W, hb, vb)
        if mode == "pair":
            flip = lambda: cx.eloc_rbm_flip(onv, h1e, h2e, table, mirror, sorb, nele, no, no, eta, norm)  # noqa: E731
            plain = lambda: cx.eloc_rbm(onv, h1e, h2e, table, sorb, nele, no, no)  # noqa: E731
            for _ in range(3):
                tf, tp = per_call(flip), per_call(plain)
                say(f"{tag} n {n}: pynqs_eloc_rbm_flip  {tf * 1e3:8.3f} ms ({n / tf * 1e-6:.2f} M E_loc / s) = {tf / tp:.3f} x pynqs_eloc_rbm  {tp * 1e3:8.3f} ms "
                    f"({n / tp * 1e-6:.2f} M E_loc / s)")
        elif mode == "jpair":
            jt, jm = cx.JastrowTable(M), cx.mirrored_jastrow_table(M)
            flip = lambda: cx.eloc_jrbm_flip(onv, h1e, h2e, table, jt, mirror, jm, sorb, nele, no, no, eta, norm)  # noqa: E731
            plain = lambda: cx.eloc_jrbm(onv, h1e, h2e, table, jt, sorb, nele, no, no)  # noqa: E731
            for _ in range(3):
                tf, tp = per_call(flip), per_call(plain)
                say(f"{tag} n {n}: pynqs_eloc_jrbm_flip {tf * 1e3:8.3f} ms ({n / tf * 1e-6:.2f} M E_loc / s) = {tf / tp:.3f} x pynqs_eloc_jrbm {tp * 1e3:8.3f} ms "
                    f"({n / tp * 1e-6:.2f} M E_loc / s)")
        else:
            assert mode == "generic", mode
            torch.set_default_dtype(torch.float64)
            pf.SpinProjection.init(2, 0)
            dev, ng, chunk = onv.device, 512, 128  # 128 walkers per call: 2 x 128 x ncomb rows of +-1 at a time
            ab = lambda xx, func: pf.ansatz_batch(func, xx, 1 << 20, sorb, dev, torch.double)  # noqa: E731
            for name, m in (("RealRBM", RealRBM(W, hb, vb).cuda()), ("JastrowRBM", JastrowRBM(W, hb, vb, M).cuda())):
                def run(fused):
                    energy.FUSED_RBM = fused
                    for b in range(0, ng, chunk):
                        energy.local_energy(onv[b:b + chunk], h1e, h2e, m, ab, sorb, nele, no, no, use_spin_flip=True, extra_norm=norm)
                for _ in range(2):
                    tg, tf = per_call(lambda: run(False)), per_call(lambda: run(True))
                    say(f"{tag} {name}: local_energy(use_spin_flip=True) on {ng} walkers, {chunk} per call: generic route {tg * 1e3:9.3f} ms "
                        f"({ng / tg * 1e-6:.4f} M E_loc / s; scaled to {n} walkers {tg * n / ng * 1e3:.1f} ms), fused {tf * 1e3:8.3f} ms")
            energy.FUSED_RBM = True


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode != "all":
        step(mode)
        return
    with open(OUT, "w") as f:
        f.write(HEADER)
    for s in ("pair", "jpair", "generic"):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), s], timeout=LIMITS[s]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"step {s!r} ended with status {rc}: nothing further is started")
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
