"""Time of stochastic reconfiguration for RBM amplitudes (pynqs_amd.sr.FusedRbmSR): one conjugate-gradient iteration and its parts
(the product pynqs_rbm_sr_matvec = Obar.z + partial sums + their reduction, three launches; the vector update pynqs_rbm_sr_cg_step), a whole
solve at tol 1e-6 (iterations, milliseconds, host read-backs included), and alongside, alternating in the same run, (a) the gradient
call pynqs_rbm_grad on the same inputs -- the yardstick: a product is expected to cost about one gradient call -- and (b) the dense
torch formulation (O[n, P] from the module's own theta, S = J^H diag(p) J, torch.linalg.solve).  Device events around at least 0.2 s of
work after a warm-up.  Sizes: Fe2S2 (sorb 40; 80 real / 40 complex hidden units) at 8192 and 65536 walkers, and sorb 120 x 240 hidden
units x 4096 walkers.

    python tools/sr_time.py [quick]                 # quick: Fe2S2 at 8192 walkers only
    python tools/sr_time.py loop                    # 60 iterations per size, nothing timed: for rocprofv3 --kernel-trace --stats
    python -m torch.distributed.run --nproc-per-node 2 tools/sr_time.py ranks   # two rehearsal ranks (gloo, both on device 0): the
                                                    # all-reduce of the product per iteration, from events around it
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402
from pynqs_amd.distributed import get_rank, get_world_size, shard_bounds  # noqa: E402
from pynqs_amd.grad import FusedRbmGrad  # noqa: E402
from pynqs_amd.rbm import ComplexRBM, RealRBM  # noqa: E402
from pynqs_amd.sr import FusedRbmSR  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "full"
SIZES = [(40, 15, 80, "real", 8192), (40, 15, 40, "complex", 8192)]
if mode != "quick":
    SIZES += [(40, 15, 80, "real", 65536), (40, 15, 40, "complex", 65536), (120, 30, 240, "real", 4096)]
MIN_SEC = 0.2


def model(kind, sorb, H):
    g = torch.Generator().manual_seed(3)
    r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)  # noqa: E731
    if kind == "complex":
        return ComplexRBM(0.3 * r(H, sorb, 2), 0.4 * r(H, 2), 0.2 * r(sorb, 2)).cuda()
    return RealRBM(0.3 * r(H, sorb), 0.4 * r(H), 0.2 * r(sorb)).cuda()


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


def dense_solve(m, kind, onv, sorb, prob, F, shift):
    from pynqs_amd import C_extension as cx

    x = cx.onv_to_tensor(onv, sorb).to(torch.float64)
    if kind == "complex":
        W, hb = torch.view_as_complex(m.params_weights.detach()), torch.view_as_complex(m.params_hidden_bias.detach())
        xc = x.to(torch.complex128)
        t = torch.tanh(xc @ W.t() + hb)
        O = torch.cat([(t[:, :, None] * xc[:, None, :]).reshape(x.size(0), -1), t, xc], 1)
        J = O - (prob.to(torch.complex128) @ O)[None, :]
        Sc = J.conj().t() @ (prob[:, None] * J)
        P = Sc.size(0)
        S = torch.empty((2 * P, 2 * P), dtype=torch.float64, device=x.device)
        S[0::2, 0::2] = Sc.real
        S[1::2, 1::2] = Sc.real
        S[1::2, 0::2] = Sc.imag
        S[0::2, 1::2] = -Sc.imag
    else:
        t = torch.tanh(x @ m.weights.detach().t() + m.hidden_bias.detach())
        O = torch.cat([(t[:, :, None] * x[:, None, :]).reshape(x.size(0), -1), t, x], 1)
        J = O - (prob @ O)[None, :]
        S = J.t() @ (prob[:, None] * J)
    S.diagonal().add_(shift)
    return torch.linalg.solve(S, F)


def main():
    if "RANK" in os.environ:
        torch.cuda.set_device(0)
        torch.distributed.init_process_group("gloo")
    ws, rank = get_world_size(), get_rank()
    say = print if rank == 0 else (lambda *a, **k: None)
    for sorb, no, H, kind, n in SIZES:
        m = model(kind, sorb, H)
        b, e = shard_bounds(n, ws, rank)
        onv = B.synth_walkers(n, sorb, no, no, 17).cuda()[b:e].contiguous()
        g = torch.Generator().manual_seed(5)
        prob = torch.rand(n, generator=g, dtype=torch.float64)
        prob = (prob / prob.sum()).cuda()[b:e] * ws
        eloc = (torch.randn(n, generator=g, dtype=torch.float64) - 100.0).cuda()[b:e]
        e_tot = torch.as_tensor(-100.0, device="cuda")
        sr = FusedRbmSR(m, sorb, tol=1e-6)
        fg = FusedRbmGrad(m, sorb)
        sr(onv, prob, eloc, e_tot)  # warm-up; leaves the table, Obar and a search direction
        tag = f"sorb {sorb:3d} H {H:3d} {kind:7s} n {n:6d} (P_real {sr.np})"
        F = sr._rhs.clone()
        if mode in ("loop", "ranks"):  # a fixed number of real iterations: a tolerance that is never met
            its = 60 if mode == "loop" else 200
            sr.tol, sr.max_iter = 1e-300, its
            sr.events = [] if mode == "ranks" else None
            a, c = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                torch.cuda.synchronize()
                a.record()
                sr.solve(F)
                c.record()
            if mode == "loop":
                for _ in range(its):
                    fg(onv, prob, eloc, e_tot)
            torch.cuda.synchronize()
            if mode == "loop":
                say(f"{tag}: {sr.iterations} iterations and {its} gradient calls")
            else:
                ar = np.mean([x.elapsed_time(y) for x, y in sr.events]) * 1e-3
                say(f"{tag} ranks {ws}: iteration {a.elapsed_time(c) * 1e-3 / sr.iterations * 1e6:8.1f} us (read-backs and their broadcast every "
                    f"{sr.check_every} included) of which all-reduce of the product (gloo, through the host) {ar * 1e6:8.1f} us")
            continue
        # alternating: product, gradient call, vector update, whole iteration -- twice, to show the spread
        rows = []
        for _ in range(2):
            t_prod = per_call(lambda: sr._product(sr._p, sr._y, False))
            t_grad = per_call(lambda: fg(onv, prob, eloc, e_tot))
            t_vec = per_call(lambda: sr._cg(2))  # the residual form: two of the step's three passes (the step itself: kernel trace)
            t_prep = per_call(lambda: sr.prepare(onv, prob))
            rows.append((t_prod, t_grad, t_vec, t_prep))
        sr.prepare(onv, prob)
        reps = 3
        a, c = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            sr.solve(F)
        c.record()
        torch.cuda.synchronize()
        t_solve = a.elapsed_time(c) * 1e-3 / reps
        for t_prod, t_grad, t_vec, t_prep in rows:
            say(f"{tag}: product {t_prod * 1e6:8.1f} us | pynqs_rbm_grad call {t_grad * 1e6:8.1f} us (product / gradient {t_prod / t_grad:.2f}) | "
                f"residual update {t_vec * 1e6:7.1f} us | prepare {t_prep * 1e6:8.1f} us")
        say(f"{tag}: solve tol 1e-6: {sr.iterations} iterations, {t_solve * 1e3:8.3f} ms ({t_solve / max(sr.iterations, 1) * 1e6:.1f} us per iteration, "
            f"read-backs every {sr.check_every} included), converged {sr.converged}, residual {sr.residual:.2e}")
        try:
            d = dense_solve(m, kind, onv, sorb, prob, F, sr.diag_shift)  # warm-up
            k = 1 if sr.np > 8000 else 5
            torch.cuda.synchronize()
            a.record()
            for _ in range(k):
                d = dense_solve(m, kind, onv, sorb, prob, F, sr.diag_shift)
            c.record()
            torch.cuda.synchronize()
            rel = float((d - sr.d).norm() / d.norm())
            say(f"{tag}: dense torch (build S, torch.linalg.solve): {a.elapsed_time(c) / k:8.3f} ms; |d_cg - d_dense| / |d| {rel:.2e}")
        except torch.OutOfMemoryError:
            say(f"{tag}: dense torch: out of memory")
        del sr, fg
        torch.cuda.empty_cache()
    if ws > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
