"""Time of the fused fixed-node Green's row of a Jastrow-RBM trial function (pynqs_green_jrbm) on Fe2S2-shaped inputs (sorb 40, 15 alpha +
15 beta electrons, 8192 walkers, 40 and 80 hidden units) against its yardstick, pynqs_green_rbm on the same walkers and RBM parameters,
alternating in the same run, with the pair factors from the walker's triangle in LDS and from the table in L2 (PYNQS_JRBM_PAIRS); a
complete GFMC step (gfmc.green_kernel + gfmc.sample_update) for both trial functions; and the generic route for the same JastrowRBM
(gfmc.FUSED_GREEN = False: comb + module forward + elementwise row) on 512 walkers, for scale.  Device events around at least 0.2 s of
work after a warm-up, twice, to show the spread.  Every GPU step is a child process of its own under a time limit, and nothing starts
after a step that failed.

    python tools/jrbm_green_time.py            # the steps "pair", "step", "generic" in turn
    python tools/jrbm_green_time.py pair       # one step, in this process
    python tools/jrbm_green_time.py loop       # 20 calls of each kernel (H = 80), nothing timed: for rocprofv3 --kernel-trace --stats
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MIN_SEC = 0.2
LIMITS = {"pair": 180, "step": 180, "generic": 300}  # seconds per step
SORB, NO, N_FUSED, N_GENERIC = 40, 15, 8192, 512


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


def problem(H, n):
    """(JastrowRBM, RealRBM with the same W, b, a, walkers, h1e, h2e, Lambda); the time of a row does not depend on Lambda"""
    import torch

    import bench as B
    from pynqs_amd.rbm import JastrowRBM, RealRBM

    g = torch.Generator().manual_seed(3)
    r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)  # noqa: E731
    W, hb, vb, M = 0.3 * r(H, SORB), 0.4 * r(H), 0.2 * r(SORB), 0.2 * r(SORB, SORB)
    onv = B.synth_walkers(n, SORB, NO, NO, 17).cuda().contiguous()
    pair = SORB * (SORB - 1) // 2
    h1e = (r(SORB, SORB) + r(SORB, SORB).t()).reshape(-1).cuda()
    h2e = r(pair * (pair + 1) // 2).cuda()
    return JastrowRBM(W, hb, vb, M).cuda(), RealRBM(W, hb, vb).cuda(), onv, h1e, h2e, 1.0e3


def step(mode):
    import torch

    from pynqs_amd import C_extension as cx, _native as N, gfmc, public_function as pf

    torch.set_default_dtype(torch.float64)
    nele = 2 * NO
    ncomb = cx.get_Num_SinglesDoubles(SORB, NO, NO) + 1
    dev = torch.device("cuda", torch.cuda.current_device())
    ab = lambda xx, func: pf.ansatz_batch(func, xx, 1 << 20, SORB, dev, torch.double)  # noqa: E731
    if mode in ("pair", "loop"):
        for H in ((80,) if mode == "loop" else (40, 80)):
            mj, mr, onv, h1e, h2e, lam = problem(H, N_FUSED)
            n = N_FUSED
            tag = f"sorb {SORB} H {H} n {n} (ncomb {ncomb})"
            table = cx.RBMTable(mj.weights.detach(), mj.hidden_bias.detach(), mj.visible_bias.detach())
            jtable = cx.JastrowTable(mj.jastrow.detach())
            plan = cx.plan_for(h1e, h2e, SORB, dev)
            eloc = torch.empty(n, device=dev)
            gk = torch.empty((n, ncomb), device=dev)
            neg = torch.empty(n, dtype=torch.uint8, device=dev)
            st = torch.cuda.current_stream().cuda_stream
            jrbm = lambda: N.check(N.lib().pynqs_green_jrbm(onv.data_ptr(), n, SORB, nele, NO, NO, plan.data_ptr(), table.data_ptr(), jtable.data_ptr(), H,  # noqa: E731
                                                            lam, eloc.data_ptr(), None, gk.data_ptr(), neg.data_ptr(), st), "pynqs_green_jrbm")
            rbm = lambda: N.check(N.lib().pynqs_green_rbm(onv.data_ptr(), n, SORB, nele, NO, NO, plan.data_ptr(), table.data_ptr(), H, N.RBM_REAL, lam,  # noqa: E731
                                                          eloc.data_ptr(), None, gk.data_ptr(), neg.data_ptr(), st), "pynqs_green_rbm")
            if mode == "loop":
                for _ in range(20):
                    jrbm(); rbm()
                torch.cuda.synchronize()
                print(f"{tag}: 20 calls each of pynqs_green_jrbm and pynqs_green_rbm")
                return
            for pairs in ("lds", "l2"):
                os.environ["PYNQS_JRBM_PAIRS"] = pairs
                where = "LDS" if N.lib().pynqs_eloc_jrbm_form(n, SORB, nele, NO, NO, H) & 4 else "L2"
                for _ in range(2):
                    tj, tr = per_call(jrbm), per_call(rbm)
                    print(f"{tag}: pynqs_green_jrbm, pairs from {where}, {tj * 1e3:8.3f} ms ({n / tj * 1e-6:.2f} M rows / s, {tj / tr:.3f} x pynqs_green_rbm) | "
                          f"pynqs_green_rbm {tr * 1e3:8.3f} ms ({n / tr * 1e-6:.2f} M rows / s)")
            del os.environ["PYNQS_JRBM_PAIRS"]
        return
    if mode == "step":
        for H in (40, 80):
            mj, mr, onv, h1e, h2e, lam = problem(H, N_FUSED)
            n = N_FUSED
            w = torch.ones(n, device=dev)
            rnd = torch.rand((n, 1), device=dev)

            def move(m):
                _, gk, comb, _, _ = gfmc.green_kernel(onv, lam, h1e, h2e, m, ab, SORB, nele, NO, NO, torch.double, None, True)
                assert isinstance(comb, gfmc.CombRows)
                gfmc.sample_update(onv, w, comb, gk, rnd)

            for _ in range(2):
                tj, tr = per_call(lambda: move(mj)), per_call(lambda: move(mr))
                print(f"sorb {SORB} H {H} n {n}: green_kernel + sample_update, JastrowRBM {tj * 1e3:8.3f} ms ({n / tj * 1e-6:.2f} M walker moves / s, "
                      f"{tj / tr:.3f} x RealRBM) | RealRBM {tr * 1e3:8.3f} ms ({n / tr * 1e-6:.2f} M walker moves / s)")
        return
    assert mode == "generic", mode
    gfmc.FUSED_GREEN = False
    for H in (40, 80):
        mj, _, onv, h1e, h2e, lam = problem(H, N_GENERIC)
        n = N_GENERIC
        w = torch.ones(n, device=dev)
        rnd = torch.rand((n, 1), device=dev)

        def generic():
            _, gk, comb, _, _ = gfmc.green_kernel(onv, lam, h1e, h2e, mj, ab, SORB, nele, NO, NO, torch.double, None, True)
            assert torch.is_tensor(comb)
            gfmc.sample_update(onv, w, comb, gk, rnd)

        for _ in range(2):
            tg = per_call(generic)
            print(f"sorb {SORB} H {H} n {n}: the generic route (FUSED_GREEN = False: comb + module + elementwise row, then the move) {tg * 1e3:8.3f} ms "
                  f"({n / tg * 1e-6:.3f} M walker moves / s)")


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode != "all":
        step(mode)
        return
    for s in ("pair", "step", "generic"):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), s], timeout=LIMITS[s]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"step {s!r} ended with status {rc}: nothing further is started")
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
