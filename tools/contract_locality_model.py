#!/usr/bin/env python3
"""CPU model of what the REDUCE contraction (pynqs_reduce_contract_form) reads on the flagship workload: no GPU, no native library.

    python3 tools/contract_locality_model.py [--walkers 8192] [--eps 1e-2] [--draws 1000] [--seed 0] > profiles/contract_locality_model.txt

Records: the oracle's rows (oracle.comb_hij_fused) of the benchmark's walkers (tests/golden/fe2s2_inputs.npz, ci_space in order), the
columns with |H| >= eps kept, `draws` multinomial draws per walker from the others (numpy's generator: the LAW of the front end, not its
stream -- counts move by a few thousand from seed to seed); the distinct x' numbered by first appearance in walker order, as the front
end numbers its rows up to launch timing.  A record links to "another walker's row" when its x' first appeared under another walker.
Locality: psi_u has 16 bytes per row (complex), 8 rows per 128-byte line.  A workgroup serves 4 walkers; workgroup b is on XCD b % 8
(observed, not promised).  Placement "by block": workgroup b serves walker group b.  "by XCD": group j (B >> 3) + min(j, B & 7) + (b >> 3),
j = b & 7 (PYNQS_CONTRACT_BY_XCD).  Per XCD: the distinct lines its walkers' records touch, and the misses of an LRU of --lru-lines lines
fed the gathers in walker order.
Batches: a trip is 64 consecutive slots.  The kept list is laid out as the front end does with one chunk: slot 0 column 0, slot 8 + s
single s, the kept doubles compacted from slot `fixed` = 8 + 16 ceil(singles / 16); the drawn list holds the distinct drawn columns first.
Two-list schedule: ceil(trips / 8) batches per list.  One stream: ceil(live trips of both lists / 8)."""
import argparse
import os
import sys
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402


def group_of(b, B):
    j = b & 7
    return j * (B >> 3) + min(j, B & 7) + (b >> 3)


def lru_misses(lines, cap):
    q, miss = OrderedDict(), 0
    for x in lines.tolist():
        if x in q:
            q.move_to_end(x)
        else:
            miss += 1
            q[x] = None
            if len(q) > cap:
                q.popitem(last=False)
    return miss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=8192)
    ap.add_argument("--eps", type=float, default=1e-2)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lru-lines", type=int, default=16384)
    ap.add_argument("--chunk", type=int, default=256)
    a = ap.parse_args()
    d = np.load(os.path.join(ROOT, "tests", "golden", "fe2s2_inputs.npz"))
    sorb, nele, noA, noB = int(d["sorb"]), int(d["nele"]), int(d["noA"]), int(d["noB"])
    ci = d["ci_space"]
    x = np.ascontiguousarray(ci[np.arange(a.walkers) % ci.shape[0]])
    nsingle = noA * (sorb // 2 - noA) + noB * (sorb // 2 - noB)
    fixed = 8 + 16 * ((nsingle + 15) // 16)
    rng = np.random.default_rng(a.seed)
    keys, walker = [], []
    b_two, b_one, live_kept, live_drawn = [], [], [], []
    for i0 in range(0, a.walkers, a.chunk):
        kets, hm = O.comb_hij_fused(x[i0:i0 + a.chunk], d["h1e"], d["h2e"], sorb, nele, noA, noB)
        k64 = np.ascontiguousarray(kets).view(np.uint64).reshape(hm.shape[0], hm.shape[1], -1)
        assert k64.shape[2] == 1, "one-word determinants"
        for r in range(hm.shape[0]):
            mag = np.abs(hm[r])
            keep = mag >= a.eps
            kc = np.nonzero(keep)[0]
            sub = np.where(keep, 0.0, mag)
            dc = np.nonzero(rng.multinomial(a.draws, sub / sub.sum()))[0] if a.draws and sub.sum() > 0 else np.zeros(0, np.int64)
            cols = np.concatenate([kc, dc])
            keys.append(k64[r, cols, 0])
            walker.append(np.full(cols.size, i0 + r, np.int32))
            # slots of the kept list, trips of both lists
            singles = kc[(kc >= 1) & (kc <= nsingle)]
            ndouble = int((kc > nsingle).sum())
            slots = np.concatenate([np.zeros(int(keep[0]), np.int64), 8 + singles - 1, fixed + np.arange(ndouble)])
            tk = (fixed + ndouble + 63) // 64
            lk = np.unique(slots // 64).size
            td, ld = (a.draws + 63) // 64, (dc.size + 63) // 64
            b_two.append((tk + 7) // 8 + (td + 7) // 8)
            b_one.append((lk + ld + 7) // 8)
            live_kept.append(lk)
            live_drawn.append(ld)
    keys, walker = np.concatenate(keys), np.concatenate(walker)
    _, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")           # distinct keys by first appearance
    rank = np.empty(order.size, np.int64)
    rank[order] = np.arange(order.size)
    row = rank[inv]
    owner = walker[first][inv]                          # the walker under which the record's x' first appeared
    print(f"== contract_locality_model: {a.walkers} Fe2S2 walkers, eps {a.eps:g}, {a.draws} multinomial draws per walker (numpy seed {a.seed}), CPU oracle rows ==")
    print(f"records {keys.size}  distinct x' {order.size}  links into another walker's rows {int((owner != walker).sum())}")
    line = row // 8
    B = (a.walkers + 3) // 4
    block = walker // 4
    inv_group = np.empty(B, np.int64)
    for b in range(B):
        inv_group[group_of(b, B)] = b
    for name, xcd in (("by block (workgroup b serves group b)", block % 8), ("by XCD (PYNQS_CONTRACT_BY_XCD)", inv_group[block] % 8)):
        distinct = [np.unique(line[xcd == j]).size for j in range(8)]
        miss = [lru_misses(line[xcd == j], a.lru_lines) for j in range(8)]
        print(f"placement {name}:")
        print(f"   distinct 128-byte lines of psi_u per XCD {distinct}  sum {sum(distinct)}  = {sum(distinct) * 128 / 1e6:.1f} MB, {sum(distinct) * 128 / 8e6:.1f} MB per XCD")
        print(f"   misses of a {a.lru_lines}-line LRU per XCD, gathers in walker order {miss}  sum {sum(miss)} of {keys.size} gathers")
    for name, v in (("two lists (kept, then drawn)", b_two), ("one stream of live trips", b_one)):
        v = np.asarray(v)
        print(f"batches of 8 trips per walker, {name}: mean {v.mean():.2f}  max {v.max()}  histogram {np.bincount(v).tolist()}")
    lk, ld = np.asarray(live_kept), np.asarray(live_drawn)
    print(f"live trips per walker: kept list {lk.min()} - {lk.max()} (mean {lk.mean():.2f}), drawn list {ld.min()} - {ld.max()} (mean {ld.mean():.2f}), both {np.mean(lk + ld):.2f}")


if __name__ == "__main__":
    main()
