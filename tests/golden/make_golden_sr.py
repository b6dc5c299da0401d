#!/usr/bin/env python3
"""Golden vectors of stochastic reconfiguration, captured from the REFERENCE's own Python (development container only; see
make_golden.py / make_golden_r2.py for how the reference is built and imported).

  sr_fe2s2.npz   vmc/grad/sr.py:87-117 (_calculate_sr: dense S = <O* O> - <O*><O>, S + diag_shift, torch.linalg.inv, inv(S).real @ F.real)
                 on the 32 Fe2S2 walkers of grad_fe2s2.npz / eloc_e2e_fe2s2.npz, real RBM, cases "amd -1, pow 0" and "amd 5, pow 1",
                 diag_shift 0.02.  The per-sample derivatives come from the reference module's own analytic_derivate
                 (vmc/ansatz/rbm/rbm.py:213-234), F_p is the reference's gradient already stored in grad_fe2s2.npz.  sr_grad itself cannot
                 be driven end to end on this module (jacobian's "analytic" method hands the module's tuple to torch.func.grad, which
                 wants a scalar), so the capture stops at the function that does the algebra.
                 Stored per case: d per parameter name (weights, hidden_bias, visible_bias) and `dist`, the reference's relative distance
                 |d_ref - d_exact|_2 / |d_exact|_2 from the exact solve of tests/rbm_sr_exact.py (longdouble) on the same inputs.
Only DATA is written: the reference's outputs.

usage: python tests/golden/make_golden_sr.py [--scratch /tmp/refbuild]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_r2 as R2  # noqa: E402

CASES = [(-1, 0), (5, 1)]
DIAG_SHIFT = 0.02


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scratch", default="/tmp/refbuild")
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    R2.harness(a.scratch)
    from vmc.ansatz.rbm.rbm import RBMWavefunction
    from vmc.grad.sr import _calculate_sr

    import rbm_exact as RE
    import rbm_sr_exact as SE

    I = R2.load_inputs()
    sorb = I["sorb"]
    g = np.load(f"{HERE}/grad_fe2s2.npz")
    words = np.ascontiguousarray(I["x"].numpy()).view(np.uint64).reshape(32, -1)
    x = RE.pm1(words, sorb)
    m = RBMWavefunction(sorb, alpha=2, rbm_type="real")
    m.init(I["hb"].clone(), I["W"].clone(), I["vb"].clone())
    (da, db, dw), _ = m.analytic_derivate(torch.from_numpy(x))
    n = x.shape[0]
    per_sample = torch.cat([dw.reshape(n, -1), db.reshape(n, -1), da.reshape(n, -1)], 1)  # weights, hidden_bias, visible_bias
    rbm = RE.make("real", I["W"].numpy(), I["hb"].numpy(), I["vb"].numpy())
    H = rbm.H
    out = {"diag_shift": np.float64(DIAG_SHIFT)}
    for amd, pw in CASES:
        key = f"grad_real_amd{amd}_pow{pw}"
        prob = torch.from_numpy(g[key + "_prob"])
        F = torch.from_numpy(np.concatenate([g[f"{key}_ws1_params_{nm}"].reshape(-1) for nm in ("weights", "hidden_bias", "visible_bias")]))
        d = _calculate_sr(per_sample, F, prob, diag_shift=DIAG_SHIFT, dtype=torch.double).numpy()
        se = SE.sr_exact(rbm, x, prob.numpy())
        dx, last = se.solve(F.numpy(), DIAG_SHIFT)
        assert last <= SE.SOLVE_FLOOR, last
        dist = float(np.sqrt(((d - dx) ** 2).sum()) / np.sqrt((dx ** 2).sum()))
        print(f"{key}: |d| = {np.linalg.norm(d):.6e}  reference to exact {dist:.3e}")
        out[f"sr_real_amd{amd}_pow{pw}_weights"] = d[:H * sorb].reshape(H, sorb)
        out[f"sr_real_amd{amd}_pow{pw}_hidden_bias"] = d[H * sorb:H * sorb + H]
        out[f"sr_real_amd{amd}_pow{pw}_visible_bias"] = d[H * sorb + H:]
        out[f"sr_real_amd{amd}_pow{pw}_dist"] = np.float64(dist)
    np.savez_compressed(f"{a.out}/sr_fe2s2.npz", **out)


if __name__ == "__main__":
    main()
