#!/usr/bin/env python3
"""Launch decisions of the two fused RBM local-energy kernels (window, chunks, refusal, table sizes), recorded from a build of THIS
project's library: the host-only entry points pynqs_eloc_rbm_form / _supported, pynqs_eloc_crbm_form / _supported and
pynqs_rbm_table_bytes / pynqs_crbm_table_bytes over a grid of systems, hidden-unit counts and batch sizes.  No GPU is needed.

  rbm_launch_forms.json     recorded at commit 73214e5, before the two kernels' host logic was merged into csrc/rbm_tiles.h;
                            tests/test_host_logic.py::test_rbm_launch_decisions_are_unchanged compares every value, with no tolerance.
  rbm_launch_geometry.json  the whole launch of the real-parameter kernel (pynqs_eloc_rbm_geometry: workgroups, threads, LDS bytes,
                            resident hidden units, chunks, pair factors in LDS) for the four (green, jastrow) combinations, and
                            pynqs_eloc_jrbm_form / _supported, over the same grid.  It is the PARENT's behaviour: recorded at commit
                            e02bd5b plus nothing but that host-only entry, which there was computed from the three launch paths the
                            kernel then had (eloc_rbm_impl, eloc_jrbm_impl, pynqs_green_jrbm), before they became one launcher.  The
                            same test compares every value, with no tolerance.

Re-record only when a launch rule is changed on purpose (PYNQS_AMD_LIB selects the library to record from; the PYNQS_RBM_* /
PYNQS_CRBM_* / PYNQS_JRBM_* overrides must be unset).

usage: python tests/golden/make_golden_rbm_launch.py
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SYSTEMS = [(4, 1, 0), (12, 3, 2), (40, 15, 15), (66, 3, 4), (120, 30, 30), (184, 46, 46)]  # (sorb, noA, noB); nele = noA + noB
HIDDEN = [1, 8, 40, 240, 1200, 4000]
NBATCH = [1, 7, 1023, 1024, 8192]
OVERRIDES = ("PYNQS_RBM_", "PYNQS_CRBM_", "PYNQS_JRBM_")


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


def record_geometry(lib) -> dict:
    """jrbm_supported: SYSTEMS x HIDDEN; jrbm_form: x NBATCH; geometry: x NBATCH x green 0, 1 x jastrow 0, 1, last index fastest, each entry
    [return code, workgroups, threads, LDS bytes, resident hidden units, chunks, pairs in LDS] (zeros behind a return code of -1)."""
    out = {"systems": SYSTEMS, "hidden": HIDDEN, "nbatch": NBATCH, "jrbm_supported": [], "jrbm_form": [], "geometry": []}
    for sorb, noA, noB in SYSTEMS:
        nele = noA + noB
        for H in HIDDEN:
            out["jrbm_supported"].append(int(lib.pynqs_eloc_jrbm_supported(sorb, nele, noA, noB, H)))
            for n in NBATCH:
                out["jrbm_form"].append(int(lib.pynqs_eloc_jrbm_form(n, sorb, nele, noA, noB, H)))
                for green in (0, 1):
                    for jastrow in (0, 1):
                        g = (ctypes.c_int64 * 6)()
                        rc = int(lib.pynqs_eloc_rbm_geometry(n, sorb, nele, noA, noB, H, green, jastrow, g))
                        out["geometry"].append([rc] + [int(v) for v in g])
    return out


def main():
    assert not any(k.startswith(OVERRIDES) for k in os.environ), "unset the PYNQS_RBM_* / PYNQS_CRBM_* / PYNQS_JRBM_* overrides"
    from pynqs_amd import _native as N

    for name, rec in (("rbm_launch_forms.json", record), ("rbm_launch_geometry.json", record_geometry)):
        with open(os.path.join(HERE, name), "w") as f:
            json.dump(rec(N.lib()), f, separators=(",", ":"))
            f.write("\n")


if __name__ == "__main__":
    main()
