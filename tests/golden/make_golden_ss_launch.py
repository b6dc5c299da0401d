#!/usr/bin/env python3
"""Launch decisions of the table-driven SAMPLE_SPACE local-energy kernels, recorded from a build of THIS project's library: the
host-only entry points pynqs_eloc_sample_space_form (column-major: kernel kind, filter levels, workgroup size, sweep / rank scan,
string prefilter, LDS bytes, chunks), pynqs_eloc_sample_space_keys_form (key-major: groups, chunks), pynqs_hash_bytes and
pynqs_reduce_tiles over a grid of systems, table sizes and batch sizes.  No GPU is needed.

  ss_launch_forms.json   recorded from the build in which the launch rules had only just been moved, verbatim, out of
                         eloc_sample_space_impl and launch_keys into ss_form / keys_form (that build differs from commit 05d58d8 by
                         nothing else); tests/test_host_logic.py::test_ss_launch_decisions_are_unchanged compares every value, with
                         no tolerance.

The grid holds every (sorb, noA, noB, nkeys) of tests/test_gpu_ss_exact.py (SHAPES x its tables, but for the two many-electron shapes
added later, whose values are held to tests/ss_exact.py instead), of
tests/test_gpu_energy.py::test_sample_space_kernel_filter_levels (nominal and actual table sizes) and of the benchmark's SAMPLE_SPACE
workloads (Fe2S2 with 18 496 keys; sorb 56, 120, 184 with 65 536), and the sizes around the LDS filter's limit of 2^18 keys.

Re-record only when a launch rule is changed on purpose (PYNQS_AMD_LIB selects the library to record from; the overrides named in
OVERRIDES must be unset).

usage: python tests/golden/make_golden_ss_launch.py
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# (sorb, noA, noB); nele = noA + noB.  test_gpu_ss_exact.SHAPES, test_sample_space_kernel_filter_levels, the bench workloads
SYSTEMS = [(12, 3, 2), (66, 3, 4), (130, 3, 2), (40, 15, 15), (40, 5, 5), (72, 6, 6), (136, 4, 4), (56, 7, 7), (120, 30, 30), (184, 46, 46)]
NKEYS = sorted({0, 1, 1 << 18, (1 << 18) + 1, 1 << 20, 18496, 65536,
                150, 200, 3000, 5000, 300_000,                                  # filter_levels, nominal
                159, 162, 207, 211, 3010, 5010, 300_003,                        # filter_levels, the tables it builds
                1, 43, 74, 210, 332, 598, 600, 19138, 38348, 38350, 43174, 62981, 86326, 86328, 125500})  # test_gpu_ss_exact's tables
NBATCH = [1, 7, 1024, 8192]
OVERRIDES = ("PYNQS_SS_", "PYNQS_FILTER", "PYNQS_KEYS_WG", "PYNQS_WANT_WG", "PYNQS_MIN_CHUNK")


def record(lib) -> dict:
    """Every list runs over SYSTEMS (x NKEYS) (x NBATCH (x hash 0, 1)), last index fastest; keys_form, which no system enters, over
    NKEYS x NBATCH x indexed 0, 1 alone.  A form is its whole out[] array."""
    out = {"systems": SYSTEMS, "nkeys": NKEYS, "nbatch": NBATCH, "hash_bytes": [], "reduce_tiles": [], "ss_form": [], "keys_form": []}
    o8, o3 = (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 3)()
    for sorb, noA, noB in SYSTEMS:
        nele = noA + noB
        for n in NBATCH:
            out["reduce_tiles"].append(int(lib.pynqs_reduce_tiles(n, sorb, nele, noA, noB)))
        for nk in NKEYS:
            out["hash_bytes"].append(int(lib.pynqs_hash_bytes(nk, sorb)))
            for n in NBATCH:
                for flag in (0, 1):
                    assert lib.pynqs_eloc_sample_space_form(n, sorb, nele, noA, noB, nk, flag, o8) == 0
                    out["ss_form"].append(list(o8))
    for nk in NKEYS:
        for n in NBATCH:
            for flag in (0, 1):
                assert lib.pynqs_eloc_sample_space_keys_form(n, SYSTEMS[0][0], nk, flag, o3) == 0
                out["keys_form"].append(list(o3))
    return out


def dump(rec: dict, f) -> None:
    """One line per list of the grid, and per (system, table size) or table size within the lists of forms."""
    per_line = {"ss_form": 2 * len(NBATCH), "keys_form": 2 * len(NBATCH), "hash_bytes": len(NKEYS), "reduce_tiles": len(NBATCH)}
    js = lambda v: json.dumps(v, separators=(",", ":"))
    parts = []
    for k, v in rec.items():
        n = per_line.get(k)
        parts.append(f'"{k}":{js(v)}' if n is None else
                     f'"{k}":[\n' + ",\n".join(",".join(js(e) for e in v[i:i + n]) for i in range(0, len(v), n)) + "\n]")
    f.write("{\n" + ",\n".join(parts) + "\n}\n")


def main():
    assert not any(k.startswith(OVERRIDES) for k in os.environ), f"unset the overrides {OVERRIDES}"
    from pynqs_amd import _native as N

    with open(os.path.join(HERE, "ss_launch_forms.json"), "w") as f:
        dump(record(N.lib()), f)


if __name__ == "__main__":
    main()
