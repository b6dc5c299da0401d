"""Time of stochastic reconfiguration for the Jastrow-RBM (pynqs_amd.sr.FusedJastrowRbmSR) next to the plain RBM's (FusedRbmSR) on the
same walkers and the same weights, alternating in the same run: one product (pynqs_jrbm_sr_matvec / pynqs_rbm_sr_matvec = Obar.z + partial
sums + their reduction, three launches), the other parts of an iteration and of a solve (the vector update pynqs_rbm_sr_cg_step on the
longer vector, prepare, the gradient call that supplies F), a whole solve at tol 1e-6 (iterations, milliseconds, host read-backs
included), and the dense torch formulation on the device (O[n, P] with the x_i x_j columns from the module's own theta, S = J^T diag(p) J,
torch.linalg.solve).  Device events around at least 0.2 s of work after a warm-up.  Sizes: the Fe2S2 shape (sorb 40) with 40 and 80
hidden units at 8192 walkers (Z staged in LDS), sorb 120 x 120 hidden units x 4096 walkers (LDS, 57 KiB of it), and sorb 184 x 33
hidden units x 4096 walkers (Z read from global memory; the Jastrow block dominates; no dense solve: S would take 13 GB).

    python tools/jrbm_sr_time.py [quick] > profiles/jrbm_sr_time.txt      # quick: the Fe2S2 shape only
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402
from pynqs_amd.grad import FusedJastrowRbmGrad, FusedRbmGrad  # noqa: E402
from pynqs_amd.rbm import JastrowRBM, RealRBM  # noqa: E402
from pynqs_amd.sr import FusedJastrowRbmSR, FusedRbmSR  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "full"
SIZES = [(40, 15, 40, 8192), (40, 15, 80, 8192)]
if mode != "quick":
    SIZES += [(120, 30, 120, 4096), (184, 46, 33, 4096)]
MIN_SEC = 0.2
DENSE_MAX_P = 30000


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
    """seconds per call over a window of at least MIN_SEC (after a calibration that is also the warm-up)"""
    t = timed(fn, 20)
    return timed(fn, max(20, int(MIN_SEC / max(t, 1e-7)) + 1))


def dense_solve(m, onv, sorb, prob, F, shift):
    from pynqs_amd import C_extension as cx

    x = cx.onv_to_tensor(onv, sorb).to(torch.float64)
    t = torch.tanh(x @ m.weights.detach().t() + m.hidden_bias.detach())
    O = torch.cat([(t[:, :, None] * x[:, None, :]).reshape(x.size(0), -1), t, x, (x[:, :, None] * x[:, None, :]).reshape(x.size(0), -1)], 1)
    J = O - (prob @ O)[None, :]
    S = J.t() @ (prob[:, None] * J)
    S.diagonal().add_(shift)
    return torch.linalg.solve(S, F)


def solve_time(sr, F, reps=3):
    a, c = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        sr.solve(F)
    c.record()
    torch.cuda.synchronize()
    return a.elapsed_time(c) * 1e-3 / reps


def main():
    for sorb, no, H, n in SIZES:
        g = torch.Generator().manual_seed(3)
        r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)  # noqa: E731
        W, hb, vb, M = 0.3 * r(H, sorb), 0.4 * r(H), 0.2 * r(sorb), 0.1 * r(sorb, sorb)
        mj, mr = JastrowRBM(W, hb, vb, M).cuda(), RealRBM(W, hb, vb).cuda()
        onv = B.synth_walkers(n, sorb, no, no, 17).cuda().contiguous()
        g = torch.Generator().manual_seed(5)
        prob = torch.rand(n, generator=g, dtype=torch.float64)
        prob = (prob / prob.sum()).cuda()
        eloc = (torch.randn(n, generator=g, dtype=torch.float64) - 100.0).cuda()
        e_tot = (prob * eloc).sum()
        sj, sp = FusedJastrowRbmSR(mj, sorb, tol=1e-6), FusedRbmSR(mr, sorb, tol=1e-6)
        gj, gp = FusedJastrowRbmGrad(mj, sorb), FusedRbmGrad(mr, sorb)
        sj(onv, prob, eloc, e_tot)  # warm-up; leaves the table, Obar and a search direction
        sp(onv, prob, eloc, e_tot)
        Fj, Fp = sj._rhs.clone(), sp._rhs.clone()
        tag = f"sorb {sorb:3d} H {H:3d} n {n:5d}"
        print(f"{tag}: P {sj.np} (Jastrow-RBM; Z {'staged in LDS' if sorb <= 128 else 'read from global memory'}) / {sp.np} (RBM)")
        # alternating, twice, to show the spread
        for _ in range(2):
            tj = per_call(lambda: sj._product(sj._p, sj._y, False))
            tp = per_call(lambda: sp._product(sp._p, sp._y, False))
            vj = per_call(lambda: sj._cg(2))  # the residual form: two of the step's three passes
            vp = per_call(lambda: sp._cg(2))
            pj = per_call(lambda: sj.prepare(onv, prob))
            pp = per_call(lambda: sp.prepare(onv, prob))
            fj = per_call(lambda: gj(onv, prob, eloc, e_tot))
            fp = per_call(lambda: gp(onv, prob, eloc, e_tot))
            print(f"{tag}: product {tj * 1e6:8.1f} us | RBM {tp * 1e6:8.1f} us (ratio {tj / tp:.2f}) || residual update {vj * 1e6:6.1f} | {vp * 1e6:6.1f} us"
                  f" || prepare {pj * 1e6:7.1f} | {pp * 1e6:7.1f} us || gradient call {fj * 1e6:7.1f} | {fp * 1e6:7.1f} us")
        sj.prepare(onv, prob)
        sp.prepare(onv, prob)
        for _ in range(2):
            for name, s, F in (("Jastrow-RBM", sj, Fj), ("RBM", sp, Fp)):
                t = solve_time(s, F)
                print(f"{tag}: {name:11s} solve tol 1e-6: {s.iterations:4d} iterations, {t * 1e3:8.3f} ms ({t / max(s.iterations, 1) * 1e6:6.1f} us per "
                      f"iteration, read-backs every {s.check_every} included), converged {s.converged}, residual {s.residual:.2e}")
        if sj.np <= DENSE_MAX_P:
            try:
                d = dense_solve(mj, onv, sorb, prob, Fj, sj.diag_shift)  # warm-up
                k = 1 if sj.np > 8000 else 5
                a, c = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(k):
                    d = dense_solve(mj, onv, sorb, prob, Fj, sj.diag_shift)
                c.record()
                torch.cuda.synchronize()
                rel = float((d - sj.d).norm() / d.norm())
                print(f"{tag}: dense torch (build S, torch.linalg.solve), Jastrow-RBM: {a.elapsed_time(c) / k:8.3f} ms; |d_cg - d_dense| / |d| {rel:.2e}")
                del d
            except torch.OutOfMemoryError:
                print(f"{tag}: dense torch: out of memory")
        else:
            print(f"{tag}: dense torch: not run (S alone would take {sj.np ** 2 * 8 / 2 ** 30:.1f} GiB)")
        del sj, sp, gj, gp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
