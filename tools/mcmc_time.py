"""Chain-steps per second of the many-chain Metropolis sampler at the Fe2S2 size (sorb 40, 15 alpha + 15 beta): the fused RBM kernel
(pynqs_mcmc_rbm) against the generic path (pynqs_spin_flip_rand -> RealRBM / ComplexRBM forward -> pynqs_mcmc_accept) on the same chains.
Device events around the launches after a warm-up; no recording (thermalisation launches), so the numbers are the step itself.

    python tools/mcmc_time.py [steps] [generic_steps]

The fused kernel's f64 operations per chain-step are counted from kernels_mcmc.hip for a double excitation (4 flipped orbitals, the
common case: 7500 of the 7875 Fe2S2 moves), an fma counted as 2: per hidden unit, real 4 x (fma + mul) + add + mul + the |theta| difference
(2) + two (1 + q) products (4) = 20; complex 4 x (2 fma + complex mul 6) + complex mul 6 + |q|^2 3 + add 2 + 2 + two |1 + q|^2 products
(2 x 6) = 65; per chain-step on top, ~60 (log, exp, the visible part).  The excitation itself (integer work) is not counted."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pynqs_amd import _native as N  # noqa: E402
from pynqs_amd import mcmc  # noqa: E402
from pynqs_amd.rbm import ComplexRBM, RealRBM  # noqa: E402

PEAK_F64 = 78.6e12  # vector f64 peak of the MI355X (as bench.py)
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
gsteps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
d = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "fe2s2_inputs.npz"))
sorb, noA, noB = 40, 15, 15
x0 = torch.from_numpy(np.ascontiguousarray(d["ci_space"][:1])).cuda()


class Opaque(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner(x)


def model(H, kind):
    g = torch.Generator().manual_seed(11)
    r = lambda *s: 0.1 * (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)
    return (ComplexRBM(r(H, sorb, 2), r(H, 2), r(sorb, 2)) if kind == "complex" else RealRBM(r(H, sorb), r(H), r(sorb), kind)).cuda()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


for H, kind in ((40, "real"), (80, "real"), (40, "complex")):
    m = model(H, kind)
    flops = (65 if kind == "complex" else 20) * H + 60
    for nch in (8192, 65536):
        s = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, 5, x0)
        f = mcmc._Fused(m, sorb)
        per = max(1, min(mcmc._MAX_STEPS_PER_LAUNCH, mcmc._LAUNCH_WORK // (nch * H)))

        def fused(n):
            left = n
            while left > 0:
                k = min(per, left)
                s._fused_launch(f, k, 1, False)
                left -= k

        fused(per)  # warm-up
        sec = timed(lambda: fused(steps))
        rate = nch * steps / sec
        g = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, 5, x0)
        om = Opaque(m)
        psi = g._forward(om, g._x).clone()
        for _ in range(3):
            g._generic_step(om, psi, False)
        gsec = timed(lambda: [g._generic_step(om, psi, False) for _ in range(gsteps)])
        grate = nch * gsteps / gsec
        print(f"H={H:3d} {kind:7s} chains={nch:6d}: fused {rate:.3e} chain-steps/s ({sec / steps * 1e3:.3f} ms/step, {per} steps/launch, "
              f"{flops} f64 ops/chain-step = {rate * flops / 1e12:.2f} TFLOP/s, {100 * rate * flops / PEAK_F64:.1f} % of f64 peak); "
              f"generic {grate:.3e} chain-steps/s ({gsec / gsteps * 1e3:.3f} ms/step); fused/generic {rate / grate:.0f}x", flush=True)
