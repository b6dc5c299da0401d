#!/usr/bin/env python3
"""tests/golden/many_electron.npz: the reference's own get_comb_hij_fused on the shapes of tests/many_electron_cases.py that the reference
as shipped supports -- one ONV word and at most 40 electrons (cpp_src/common/default.h): (40,16,16), (40,17,16), (40,20,18) and the full
shell (40,20,20).  The goldens before this one stop at 30 electrons.

The reference is read only through its CPU extension as the project's build() compiles it (oracle/_ref/C_extension.so, MAX_SORB_LEN 1);
run build() first.  Only data lands in tests/golden/: per shape the walkers, a sha256 per row of comb and of Hmat (float64 and float32
integrals), and 64 sampled columns -- column 0, both neighbours of every class boundary, the last column, the rest seeded -- of comb and of
both Hmat.  The integrals are tests/many_electron_cases.integrals (conftest.synth_integrals, seed 4321), the walkers its occupations().

usage: python tests/golden/make_golden_many_electron.py
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NSAMPLE = 64


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def sample(c, M) -> np.ndarray:
    n = M.ncomb(c)
    want = {0, n - 1} | {b + d for b in M.boundaries(c) for d in (-1, 0) if 0 <= b + d < n}
    g = np.random.default_rng(600 + n)
    rest = [int(v) for v in g.permutation(n) if int(v) not in want][: max(0, min(NSAMPLE, n) - len(want))]
    return np.array(sorted(want | set(rest)), dtype=np.int64)


def main() -> None:
    import many_electron_cases as M
    from oracle._ref import C_extension as ref

    assert ref.MAX_SORB_LEN == 1
    out = {}
    for c in M.GOLDEN:
        nele = c.noA + c.noB
        ref.check_sorb(c.sorb, nele)  # the reference accepts the shape
        h1, h2 = (torch.from_numpy(a) for a in M.integrals(c.sorb))
        onv = ref.tensor_to_onv(torch.from_numpy(M.occupations(c)), c.sorb)
        comb, hm = ref.get_comb_hij_fused(onv, h1, h2, c.sorb, nele, c.noA, c.noB)
        comb32, hm32 = ref.get_comb_hij_fused(onv, h1.float(), h2.float(), c.sorb, nele, c.noA, c.noB)
        assert torch.equal(comb, comb32) and comb.shape[1] == M.ncomb(c) and hm32.dtype == torch.float32
        comb, hm, hm32 = comb.numpy(), hm.numpy(), hm32.numpy()
        ranks = sample(c, M)
        key = M.case_id(c)
        out[key + "_onv"] = onv.numpy()
        out[key + "_ranks"] = ranks
        out[key + "_comb"] = comb[:, ranks]
        out[key + "_hmat"] = hm[:, ranks]
        out[key + "_hmat_f32"] = hm32[:, ranks]
        out[key + "_comb_sha"] = np.array([sha(r) for r in comb])
        out[key + "_hmat_sha"] = np.array([sha(r) for r in hm])
        out[key + "_hmat_f32_sha"] = np.array([sha(r) for r in hm32])
        print(f"{key}: {c.n} walkers, {comb.shape[1]} columns, {ranks.size} sampled")
    path = os.path.join(HERE, "many_electron.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
