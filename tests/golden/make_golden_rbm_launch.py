#!/usr/bin/env python3
"""Launch decisions of the two fused RBM local-energy kernels (window, chunks, refusal, table sizes), recorded from a build of THIS
project's library: the host-only entry points pynqs_eloc_rbm_form / _supported, pynqs_eloc_crbm_form / _supported and
pynqs_rbm_table_bytes / pynqs_crbm_table_bytes over a grid of systems, hidden-unit counts and batch sizes.  No GPU is needed.

  rbm_launch_forms.json   recorded at commit 73214e5, before the two kernels' host logic was merged into csrc/rbm_tiles.h;
                          tests/test_host_logic.py::test_rbm_launch_decisions_are_unchanged compares every value, with no tolerance.

Re-record only when a launch rule is changed on purpose (PYNQS_AMD_LIB selects the library to record from; the PYNQS_RBM_* /
PYNQS_CRBM_* overrides must be unset).

usage: python tests/golden/make_golden_rbm_launch.py
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SYSTEMS = [(4, 1, 0), (12, 3, 2), (40, 15, 15), (66, 3, 4), (120, 30, 30), (184, 46, 46)]  # (sorb, noA, noB); nele = noA + noB
HIDDEN = [1, 8, 40, 240, 1200, 4000]
NBATCH = [1, 7, 1023, 1024, 8192]


def record(lib) -> dict:
    """Every list runs over SYSTEMS x HIDDEN (x NBATCH (x green 0, 1)), last index fastest."""
    out = {"systems": SYSTEMS, "hidden": HIDDEN, "nbatch": NBATCH, "rbm_table_bytes": [], "crbm_table_bytes": [], "rbm_supported": [],
           "crbm_supported": [], "rbm_form": [], "crbm_form": []}
    for sorb, noA, noB in SYSTEMS:
        nele = noA + noB
        for H in HIDDEN:
            out["rbm_table_bytes"].append(int(lib.pynqs_rbm_table_bytes(sorb, H)))
            out["crbm_table_bytes"].append(int(lib.pynqs_crbm_table_bytes(sorb, H)))
            out["rbm_supported"].append(int(lib.pynqs_eloc_rbm_supported(sorb, nele, noA, noB, H)))
            out["crbm_supported"].append(int(lib.pynqs_eloc_crbm_supported(sorb, nele, noA, noB, H)))
            for n in NBATCH:
                out["crbm_form"].append(int(lib.pynqs_eloc_crbm_form(n, sorb, nele, noA, noB, H)))
                for green in (0, 1):
                    out["rbm_form"].append(int(lib.pynqs_eloc_rbm_form(n, sorb, nele, noA, noB, H, green)))
    return out


def main():
    assert not any(k.startswith(("PYNQS_RBM_", "PYNQS_CRBM_")) for k in os.environ), "unset the PYNQS_RBM_* / PYNQS_CRBM_* overrides"
    from pynqs_amd import _native as N

    with open(os.path.join(HERE, "rbm_launch_forms.json"), "w") as f:
        json.dump(record(N.lib()), f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
