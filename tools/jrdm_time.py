"""Time of the fused reduced density matrices of a Jastrow-RBM (pynqs_rdm_jrbm) on Fe2S2-shaped inputs (sorb 40, 15 alpha + 15 beta
electrons, 8192 walkers, 40 and 80 hidden units) against its yardstick, pynqs_rdm_rbm on the same walkers and RBM parameters: single
calls of the two ALTERNATING in the same run, each between device events, the median of REPS calls after a warm-up, twice, to show the
spread; and the generic route of pynqs_amd.rdm for the same JastrowRBM (fused=False: get_comb_tensor, the module's forward on every x',
pynqs_rdm_scatter) on 512 of the walkers, scaled by 16 to the 8192 and labelled as scaled.  Every GPU step is a child process of its own
under a time limit, and nothing starts after a step that failed.

    python tools/jrdm_time.py            # the steps "fused", "generic" in turn
    python tools/jrdm_time.py fused      # one step, in this process
    python tools/jrdm_time.py loop       # 20 calls of each kernel (H = 80), nothing timed: for rocprofv3 --kernel-trace --stats
"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"fused": 180, "generic": 300}  # seconds per step
SORB, NO, N_FUSED, N_GENERIC, REPS = 40, 15, 8192, 512, 31


def problem(H, n):
    """(JastrowRBM, walkers, probabilities)"""
    import torch

    import bench as B
    from pynqs_amd.rbm import JastrowRBM

    g = torch.Generator().manual_seed(3)
    r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)  # noqa: E731
    W, hb, vb, M = 0.3 * r(H, SORB), 0.4 * r(H), 0.2 * r(SORB), 0.2 * r(SORB, SORB)
    onv = B.synth_walkers(n, SORB, NO, NO, 17).cuda().contiguous()
    prob = torch.rand(n, generator=g, dtype=torch.float64)
    return JastrowRBM(W, hb, vb, M).cuda(), onv, (prob / prob.sum()).cuda()


def one_call(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def step(mode):
    import torch

    from pynqs_amd import C_extension as cx, _native as N, rdm

    nele = 2 * NO
    ncomb = cx.get_Num_SinglesDoubles(SORB, NO, NO) + 1
    pair = SORB * (SORB - 1) // 2
    if mode in ("fused", "loop"):
        for H in ((80,) if mode == "loop" else (40, 80)):
            mj, onv, prob = problem(H, N_FUSED)
            n = N_FUSED
            tag = f"sorb {SORB} H {H} n {n} (ncomb {ncomb})"
            table = cx.RBMTable(mj.weights.detach(), mj.hidden_bias.detach(), mj.visible_bias.detach())
            jtable = cx.JastrowTable(mj.jastrow.detach())
            work = torch.empty(N.lib().pynqs_rdm_jrbm_workspace(n, SORB, H) // 8, dtype=torch.float64, device="cuda")
            out = torch.empty(SORB * SORB + pair * (pair + 1) // 2, dtype=torch.float64, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            tail = (H, work.data_ptr(), out.data_ptr(), out[SORB * SORB:].data_ptr(), st)
            jrbm = lambda: N.check(N.lib().pynqs_rdm_jrbm(onv.data_ptr(), n, SORB, nele, NO, NO, prob.data_ptr(), table.data_ptr(), jtable.data_ptr(),  # noqa: E731
                                                          *tail), "pynqs_rdm_jrbm")
            rbm = lambda: N.check(N.lib().pynqs_rdm_rbm(onv.data_ptr(), n, SORB, nele, NO, NO, prob.data_ptr(), table.data_ptr(), *tail), "pynqs_rdm_rbm")  # noqa: E731
            if mode == "loop":
                for _ in range(20):
                    jrbm(); rbm()
                torch.cuda.synchronize()
                print(f"{tag}: 20 calls each of pynqs_rdm_jrbm and pynqs_rdm_rbm")
                return
            for _ in range(3):
                jrbm(); rbm()
            torch.cuda.synchronize()
            for _ in range(2):
                tj, tr = [], []
                for _ in range(REPS):
                    tj.append(one_call(jrbm)); tr.append(one_call(rbm))
                mj_, mr_ = statistics.median(tj), statistics.median(tr)
                print(f"{tag}: pynqs_rdm_jrbm {mj_ * 1e3:8.3f} ms (min {min(tj) * 1e3:.3f}, {n / mj_ * 1e-6:.3f} M walkers / s, {mj_ / mr_:.3f} x pynqs_rdm_rbm) | "
                      f"pynqs_rdm_rbm {mr_ * 1e3:8.3f} ms (min {min(tr) * 1e3:.3f}); medians of {REPS} alternating calls")
            # the same through pynqs_amd.rdm: both tables rebuilt, workspace and result allocated per call
            call = lambda: rdm.reduced_density_matrices(onv, prob, mj, SORB, nele, NO, NO, fused=True)  # noqa: E731
            call()
            torch.cuda.synchronize()
            tp = statistics.median(one_call(call) for _ in range(REPS))
            print(f"{tag}: rdm.reduced_density_matrices(JastrowRBM, fused) {tp * 1e3:8.3f} ms ({n / tp * 1e-6:.3f} M walkers / s), median of {REPS} calls")
        return
    assert mode == "generic", mode
    for H in (40, 80):
        mj, onv, prob = problem(H, N_GENERIC)
        n = N_GENERIC
        call = lambda: rdm.reduced_density_matrices(onv, prob, mj, SORB, nele, NO, NO, fused=False)  # noqa: E731
        call()
        torch.cuda.synchronize()
        for _ in range(2):
            tg = statistics.median(one_call(call) for _ in range(5))
            print(f"sorb {SORB} H {H} n {n} (ncomb {ncomb}): the generic route for the JastrowRBM (fused=False: comb + module forward + pynqs_rdm_scatter) "
                  f"{tg * 1e3:9.3f} ms ({n / tg * 1e-6:.4f} M walkers / s), median of 5 calls; SCALED to {N_FUSED} walkers (x {N_FUSED // n}): "
                  f"{tg * (N_FUSED // n) * 1e3:10.3f} ms")


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode != "all":
        step(mode)
        return
    for s in ("fused", "generic"):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), s], timeout=LIMITS[s]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"step {s!r} ended with status {rc}: nothing further is started")
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
