"""Chain-steps per second of the many-chain Metropolis sampler for the Jastrow-RBM at the Fe2S2 size (sorb 40, 15 alpha + 15 beta), H = 40
and 80, 8192 and 65536 chains, three routes on the same chains in the same run:
  jrbm    : the fused kernel with the Jastrow ln-ratio, pynqs_mcmc_jrbm;
  rbm     : its yardstick pynqs_mcmc_rbm with the same RBM parameters (M dropped), alternating with jrbm: the ratio is the cost of the
            Jastrow part (the count suggests 1.2-1.5 x: 4 ceil(sorb / G) load + fma pairs per lane and step on top of the hidden units');
  generic : pynqs_spin_flip_rand -> JastrowRBM.forward on +-1 rows -> pynqs_mcmc_accept, what the sampler does for a module it does not
            recognise.
Device events around the launches after a warm-up; no recording (thermalisation launches), so the numbers are the step itself.

    python tools/jrbm_mcmc_time.py [steps] [generic_steps]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pynqs_amd import _native as N  # noqa: E402
from pynqs_amd import mcmc  # noqa: E402
from pynqs_amd.rbm import JastrowRBM, RealRBM  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
gsteps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
ROUNDS = 3  # jrbm and rbm alternate this many times; the median of each is reported
d = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "fe2s2_inputs.npz"))
sorb, noA, noB = 40, 15, 15
x0 = torch.from_numpy(np.ascontiguousarray(d["ci_space"][:1])).cuda()


class Opaque(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner(x)


def models(H):
    g = torch.Generator().manual_seed(11)
    r = lambda *s: 0.1 * (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)  # noqa: E731
    W, hb, vb, M = r(H, sorb), r(H), r(sorb), 2.0 * r(sorb, sorb)
    return JastrowRBM(W, hb, vb, M).cuda(), RealRBM(W, hb, vb, "real").cuda()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


for H in (40, 80):
    mj, mr = models(H)
    form = N.lib().pynqs_mcmc_jrbm_form(sorb, H)
    G = 1
    while 8 * G < H:
        G *= 2
    for nch in (8192, 65536):
        per = max(1, min(mcmc._MAX_STEPS_PER_LAUNCH, mcmc._LAUNCH_WORK // (nch * H)))
        samplers = {k: mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, 5, x0) for k in ("jrbm", "rbm")}
        fused = {"jrbm": mcmc._Fused(mj, sorb), "rbm": mcmc._Fused(mr, sorb)}
        assert fused["jrbm"].jastrow_table is not None and fused["rbm"].jastrow_table is None

        def run(k, n):
            left = n
            while left > 0:
                m = min(per, left)
                samplers[k]._fused_launch(fused[k], m, 1, False)
                left -= m

        for k in ("jrbm", "rbm"):
            run(k, per)  # warm-up
        sec = {"jrbm": [], "rbm": []}
        for _ in range(ROUNDS):
            for k in ("jrbm", "rbm"):
                sec[k].append(timed(lambda: run(k, steps)))
        tj, tr = float(np.median(sec["jrbm"])), float(np.median(sec["rbm"]))
        g = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, 5, x0)
        om = Opaque(mj)
        assert not mcmc._Fused.applies(om, sorb)
        psi = g._forward(om, g._x).clone()
        for _ in range(3):
            g._generic_step(om, psi, False)
        gsec = timed(lambda: [g._generic_step(om, psi, False) for _ in range(gsteps)])
        rj, rr, rg = nch * steps / tj, nch * steps / tr, nch * gsteps / gsec
        print(f"H={H:3d} chains={nch:6d} (G {G}, form {form}, {per} steps/launch): jrbm {rj:.3e} chain-steps/s ({tj / steps * 1e3:.3f} ms/step, "
              f"spread {min(sec['jrbm']) / steps * 1e3:.3f}-{max(sec['jrbm']) / steps * 1e3:.3f}); rbm {rr:.3e} ({tr / steps * 1e3:.3f} ms/step); "
              f"jrbm / rbm time {tj / tr:.3f}x; generic {rg:.3e} chain-steps/s ({gsec / gsteps * 1e3:.3f} ms/step); jrbm / generic "
              f"{rj / rg:.1f}x faster", flush=True)
