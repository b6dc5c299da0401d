#!/usr/bin/env python3
"""What the one-launch REDUCE front end decides on the host, recorded over a grid of systems, batch sizes, draws, capacities, integral
dtypes, with and without a de-duplication table, under the four settings of pynqs_amd.reduce_front's switches that the tests use.
No GPU is needed: the front ends are built on device "meta".

  reduce_front_parent.npz  (A) what commit 73d51a2 -- the parent of the change that introduced pynqs_reduce_onepass_plan -- answered
                           through its own ReduceFrontEnd (five host queries and a three-step allocation in Python): row_f32_form, the
                           elements of row_f32 / row_cache / tile_scratch / the table (-1: not allocated), segments, fixed slots,
                           chunks, reduce_front.list_capacity with and without table, reduce_front.supported, or the refusal.  Recorded
                           from a checkout of that commit:  python tests/golden/make_golden_reduce_front.py parent --tree <checkout>
                           This recorder touches only what both sides of that change have (the constructor, its buffers, the three
                           module functions and the module switches), so it runs unchanged against either tree and must write the
                           same bytes.
  reduce_front_plans.npz   (B) every field of pynqs_reduce_onepass_plan's answer over the same grid.  Recorded from the FIRST build that
                           had that entry point, in which it only wrapped the unmoved onepass_form() and the allocation sequence ported
                           from ReduceFrontEnd.__init__; nothing had been simplified yet (that build reproduced A byte for
                           byte).  The decision function was restructured only afterwards, against this record.

tests/test_host_logic.py holds the library to both with no tolerance.  Re-record B only when a launch rule is changed on purpose; A never.
The overrides named in OVERRIDES must be unset.

usage: python tests/golden/make_golden_reduce_front.py parent|plans [--tree DIR] [--out DIR]
  --tree: the checkout whose pynqs_amd is recorded (default: this one); --out: where the .npz goes (default: next to this file)
"""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

SYSTEMS = [(12, 3, 2), (24, 4, 4), (40, 15, 15), (56, 7, 7), (66, 3, 3), (80, 20, 20), (120, 30, 30), (130, 2, 2), (136, 4, 4), (184, 46, 46)]
NBATCH = [1, 8, 1024, 8192]
EPS_SAMPLE = [0, 100, 1000, 3000, 4000, 20000]
CAPS = [0, 64, 600, 1100, 3097, 1 << 20]      # + per system and draw count the four values around the list limits: caps()
SWITCHES = [(True, True, 65536), (False, True, 65536), (False, False, 65536), (False, False, 64)]  # (ROW_F32, ROW_CACHE, TILE_SCRATCH_MIN_ROW)
CAP_UNIQUE = 4096
OVERRIDES = ("PYNQS_OP_", "PYNQS_ROW_F32", "PYNQS_TILE_SCRATCH_MIN_ROW")
IN_COLS = ("sorb", "noA", "noB", "nbatch", "eps_sample", "cap_doubles", "f64", "table", "switch")
A_COLS = ("refused", "row_f32_form", "row_f32", "row_cache", "tile_scratch", "nseg", "fixed", "nchunks", "table_elements",
          "list_capacity", "list_capacity_tableless", "supported")


def caps(fixed: int):
    return CAPS + [c for c in (1024 - fixed, 1024 - fixed + 1, 2048 - fixed, 2048 - fixed + 1) if c > 0]


def grid(RF):
    """the rows of IN_COLS, last index fastest"""
    rows = []
    for sorb, noA, noB in SYSTEMS:
        for n in NBATCH:
            for ns in EPS_SAMPLE:
                fixed = RF.geometry(n, sorb, noA + noB, noA, noB, ns)[1]
                rows += [(sorb, noA, noB, n, ns, cap, f64, tab, sw) for cap in caps(fixed) for f64 in (1, 0) for tab in (1, 0)
                         for sw in range(len(SWITCHES))]
    return np.asarray(rows, dtype=np.int64)


class switches:
    """the module switches of pynqs_amd.reduce_front set to SWITCHES[i] (what the tests do with monkeypatch)"""

    def __init__(self, RF, i):
        self.RF, self.new = RF, SWITCHES[i]

    def __enter__(self):
        RF = self.RF
        self.old = (RF.ROW_F32, RF.ROW_CACHE, RF.TILE_SCRATCH_MIN_ROW)
        RF.ROW_F32, RF.ROW_CACHE, RF.TILE_SCRATCH_MIN_ROW = self.new

    def __exit__(self, *exc):
        RF = self.RF
        RF.ROW_F32, RF.ROW_CACHE, RF.TILE_SCRATCH_MIN_ROW = self.old


def numel(t) -> int:
    return -1 if t is None else int(t.numel())


def record_parent(RF, g) -> np.ndarray:
    import torch

    out = np.full((len(g), len(A_COLS)), -1, dtype=np.int64)
    shared = {}
    for i, (sorb, noA, noB, n, ns, cap, f64, tab, sw) in enumerate(g.tolist()):
        dt = torch.float64 if f64 else torch.float32
        with switches(RF, sw):
            key = (sorb, noA, noB, n, ns, f64, sw)
            if key not in shared:
                sysargs = (n, sorb, noA + noB, noA, noB, ns)
                shared[key] = (RF.list_capacity(*sysargs, dt), RF.list_capacity(*sysargs, dt, without_table=True), int(RF.supported(*sysargs)))
            try:
                fe = RF.ReduceFrontEnd(n, sorb, noA + noB, noA, noB, ns, dt, "meta", cap, CAP_UNIQUE, dedup=bool(tab))
                out[i, :9] = (0, fe.row_f32_form, numel(fe.row_f32), numel(fe.row_cache), numel(fe.tile_scratch), fe.nseg, fe.fixed, fe.nchunks,
                              numel(fe.table))
            except RuntimeError:
                out[i, 0] = 1
            out[i, 9:] = shared[key]
    return out


def record_plans(RF, g):
    """(field names, [points, fields]) of pynqs_reduce_onepass_plan's answers as reduce_front.plan asks for them"""
    import torch

    names = None
    out = []
    for sorb, noA, noB, n, ns, cap, f64, tab, sw in g.tolist():
        with switches(RF, sw):
            p = RF.plan(n, sorb, noA + noB, noA, noB, ns, torch.float64 if f64 else torch.float32, cap, RF._pow2_at_least(2 * CAP_UNIQUE), bool(tab))
        names = names or [f for f, _ in p._fields_]
        out.append([int(getattr(p, f)) for f in names])
    return names, np.asarray(out, dtype=np.int64)


def save(path: str, arrays: dict) -> None:
    """a compressed .npz whose bytes depend on the arrays alone (numpy.savez stamps the time into every member)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def main(argv):
    if any(k.startswith(OVERRIDES) for k in os.environ):
        raise SystemExit(f"unset the overrides {OVERRIDES}")
    what = argv[1] if len(argv) > 1 else ""
    tree = argv[argv.index("--tree") + 1] if "--tree" in argv else ROOT
    out = argv[argv.index("--out") + 1] if "--out" in argv else HERE
    sys.path.insert(0, os.path.abspath(tree))
    from pynqs_amd import reduce_front as RF

    g = grid(RF)
    if what == "parent":
        save(os.path.join(out, "reduce_front_parent.npz"), {"in_cols": np.asarray(IN_COLS), "inputs": g, "cols": np.asarray(A_COLS), "values": record_parent(RF, g)})
    elif what == "plans":
        names, vals = record_plans(RF, g)
        save(os.path.join(out, "reduce_front_plans.npz"), {"in_cols": np.asarray(IN_COLS), "inputs": g, "cols": np.asarray(names), "values": vals})
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main(sys.argv)
