#!/usr/bin/env python3
"""Golden vectors of stochastic reconfiguration for the Jastrow-RBM, captured from the REFERENCE's own Python (development container only;
see make_golden.py / make_golden_r2.py for how the reference is built and imported, and make_golden_sr.py for the RBM's fixture).

  sr_jrbm_fe2s2.npz   vmc/grad/sr.py:87-117 (_calculate_sr: dense S, S + diag_shift, torch.linalg.inv) on the 32 Fe2S2 walkers of
                      eloc_e2e_fe2s2.npz with per_sample = [the reference RBM module's own analytic_derivate (weights, hidden_bias,
                      visible_bias), x_i x_j] -- d ln psi / d M_ij of the reference's Jastrow (vmc/ansatz/rbm/rbm_other.py) is the product
                      of two inputs, written down here --, the probabilities, local energies and <E> of grad_fe2s2.npz's case "amd -1,
                      pow 0", diag_shift 0.02, and as right-hand side the EXACT energy gradient of tests/jrbm_sr_exact.py (longdouble,
                      rounded to float64; it does not depend on M).
                      Stored: F, d per parameter name (weights, hidden_bias, visible_bias, jastrow), diag_shift and `dist`, the
                      reference's relative distance |d_ref - d_exact|_2 / |d_exact|_2 from the refined exact solve on the same inputs.
Only DATA is written: the reference's outputs and the right-hand side it was given.

usage: python tests/golden/make_golden_sr_jrbm.py [--scratch /tmp/refbuild]
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

KEY = "grad_real_amd-1_pow0"
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

    import jrbm_sr_exact as JS
    import rbm_exact as RE

    I = R2.load_inputs()
    sorb = I["sorb"]
    g = np.load(f"{HERE}/grad_fe2s2.npz")
    words = np.ascontiguousarray(I["x"].numpy()).view(np.uint64).reshape(32, -1)
    x = RE.pm1(words, sorb)
    m = RBMWavefunction(sorb, alpha=2, rbm_type="real")
    m.init(I["hb"].clone(), I["W"].clone(), I["vb"].clone())
    xt = torch.from_numpy(x)
    (da, db, dw), _ = m.analytic_derivate(xt)
    n = x.shape[0]
    per_sample = torch.cat([dw.reshape(n, -1), db.reshape(n, -1), da.reshape(n, -1), (xt[:, :, None] * xt[:, None, :]).reshape(n, -1)], 1)
    rbm = RE.make("real", I["W"].numpy(), I["hb"].numpy(), I["vb"].numpy())
    H = rbm.H
    prob, eloc, e_total = g[KEY + "_prob"], np.asarray(g[KEY + "_eloc"]).real, float(np.asarray(g[KEY + "_e_total"]).real)
    se = JS.sr_exact(rbm, x, prob)
    F = JS.energy_gradient(se, np.zeros((sorb, sorb)), prob, eloc, e_total).astype(np.float64)
    d = _calculate_sr(per_sample, torch.from_numpy(F), torch.from_numpy(prob), diag_shift=DIAG_SHIFT, dtype=torch.double).numpy()
    dx, last = se.solve(F, DIAG_SHIFT)
    assert last <= JS.SOLVE_FLOOR, last
    dist = float(np.sqrt(((d - dx) ** 2).sum()) / np.sqrt((dx ** 2).sum()))
    print(f"{KEY}: P = {se.P}, |d| = {np.linalg.norm(d):.6e}  reference to exact {dist:.3e}")
    nr = se.nrbm
    np.savez_compressed(f"{a.out}/sr_jrbm_fe2s2.npz", diag_shift=np.float64(DIAG_SHIFT), F=F, dist=np.float64(dist),
                        weights=d[:H * sorb].reshape(H, sorb), hidden_bias=d[H * sorb:H * sorb + H], visible_bias=d[H * sorb + H:nr],
                        jastrow=d[nr:].reshape(sorb, sorb))


if __name__ == "__main__":
    main()
