"""Host helpers of the many-walker and size tests of the reduced-density-matrix kernels (tests/test_gpu_rdm_shapes.py; checked on the CPU
by tests/test_rdm_cases.py).  Plain Python and numpy: nothing here is shared with the kernels.

(a) grouped(): the yardstick of rdm_exact.estimator for MANY walkers drawn from a small pool of distinct determinants.  Walker i is pool
entry pick[i] with its own weight w[i].  Every slot value is linear in the weights, so the excitations and the exact amplitudes are
formed once per pool entry and enter with the longdouble sum of that entry's weights; A_t takes the sum of |w| and m_t the NUMBER of
walkers that picked the entry (the kernel adds that many terms into the slot, and rdm_exact's bound (m_t + 2 + kappa) u A_t counts
them; the bound holds for any summation tree of m_t terms, so the addition of the slices' tables is inside it).

(b) Layout: a mirror of the fused kernel's slicing and of its LDS footprint, written from the comments of kernels_rdm.hip and the
documented workspace layout (include/pynqs_amd.h):
    workspace (doubles): theta [n][H] | Dg [nslS][sorb][sorb] | T [nslS][sorb][sorb][sorb + 1] | Daa, Dbb [nslD][npS][npS] |
                         Dab [nslD][K K][K K]                                   (Jastrow flavour: | r [n][sorb] behind them)
    slices: the walkers in chunks of 256; want / owners slices (4096 for the pair kernel with its 2 npS + K K owners, 2048 for the
            singles and diagonal kernels with their sorb owners), at most (16 M doubles) / (one slice's tables), at most one per chunk,
            at least one; every slice takes ceil(chunks / slices) chunks and the slice count is what that leaves.
    LDS (bytes): 8 (sorb Hq + 4 H + 2 x 4 + sorb + [singles] K sorb) + 4 (256 + 4) + [Jastrow] 16 sorb,  Hq = H rounded up to 8, plus 1
    served: even sorb <= 192, K K <= 8 x 256, 1 <= H <= 512, nele = noA + noB, noA, noB <= K, the singles kernel's LDS within 64 KiB.
It also states which walkers qualify for an owner (owner_qualifies) and how they fall onto the four waves of each chunk (wave_counts),
so that a GPU case can assert that it really reaches the regime it is named for."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import rdm_exact as X

LD = np.longdouble
KBLOCK, WAVE = 256, 64
MAX_ITEMS, MAX_HIDDEN, MAX_LDS, MAX_SORB = 8, 512, 64 * 1024, 192
TABLE_CAP = 16 << 20  # doubles of one slice's tables


# ---- (a) the grouped yardstick --------------------------------------------------------------------------------------------------------
def grouped(pool: np.ndarray, pick: np.ndarray, w: np.ndarray, rbm=None, amplitude=None) -> X.Estimate:
    """rdm_exact.Estimate of the walkers pool[pick[i]] with the weights w[i].  pool: 0/1 [npool, sorb]; amplitudes as in
    rdm_exact.estimator (from `rbm`, or amplitude(rows 0/1) -> complex longdouble)."""
    pool = np.asarray(pool)
    npool, sorb = pool.shape
    pick = np.asarray(pick, dtype=np.int64)
    wl = np.asarray(w, dtype=np.float64).astype(LD)
    assert pick.shape == wl.shape and (pick.size == 0 or (0 <= pick.min() and pick.max() < npool))
    n1, n2 = X.sizes(sorb)
    val = [np.zeros(n1, dtype=LD), np.zeros(n2, dtype=LD)]
    A = [np.zeros(n1), np.zeros(n2)]
    m = [np.zeros(n1, dtype=np.int64), np.zeros(n2, dtype=np.int64)]
    km = [np.zeros(n1), np.zeros(n2)]
    H = rbm.H if rbm is not None else 0
    for j in range(npool):
        mine = pick == j
        cnt = int(mine.sum())
        if cnt == 0:
            continue
        ws = wl[mine].sum()                       # longdouble: sum of the entry's weights
        wa = float(np.abs(wl[mine]).sum())        # sum |w|
        o = pool[j]
        occupied = [p for p in range(sorb) if o[p]]
        for p in occupied:
            val[0][p * sorb + p] += ws; A[0][p * sorb + p] += wa; m[0][p * sorb + p] += cnt
        for a, p in enumerate(occupied):
            for q in occupied[:a]:
                t = X.tri(X.pair_index(p, q), X.pair_index(p, q))
                val[1][t] += ws; A[1][t] += wa; m[1][t] += cnt
        ex = X.excitations(o)
        if not ex:
            continue
        rows = np.repeat(np.asarray(o)[None, :].astype(np.int8), len(ex) + 1, 0)
        for k, (flip, _, _) in enumerate(ex):
            rows[k + 1, list(flip)] ^= 1
        if rbm is not None:
            import rbm_exact as R

            e = R.exact_ld(rbm, rows.astype(np.float64) * 2 - 1)
            r = np.exp(e.re[1:] - e.re[0]) * (np.cos(e.im[1:] - e.im[0]) + 1j * np.sin(e.im[1:] - e.im[0]))
            kap = (sorb + H + 16) * (e.cond[1:] + e.cond[0] + 2 * H * np.log(2.0)) + 4
        else:
            psi = amplitude(rows)
            r = psi[1:] / psi[0]
            kap = np.full(len(ex), 2.0)
        for k, (_, s, targets) in enumerate(ex):
            c = ws * r[k].real * s
            ca = wa * float(abs(r[k]))
            for which, t, f in targets:
                val[which - 1][t] += c * f
                A[which - 1][t] += ca
                m[which - 1][t] += cnt
                km[which - 1][t] = max(km[which - 1][t], float(kap[k]))
    return X.Estimate(sorb, val[0], val[1], A[0], A[1], m[0], m[1], km[0], km[1], float(wl.sum()),
                      X.kappa_fused(rbm, sorb) if rbm is not None and rbm.kind == "real" else float("nan"))


def grouped_jastrow(rbm, M: np.ndarray, pool: np.ndarray, pick: np.ndarray, w: np.ndarray):
    """(Estimate of the Jastrow-RBM with kappa_fused = kappa of jrdm_exact's "fused" path, kappa_module): jrdm_exact.estimate, grouped"""
    import jrdm_exact as JX

    seen = []
    est = grouped(pool, pick, w, amplitude=JX.amplitude(rbm, M, seen))
    est.kappa_fused = X.kappa_fused(rbm, pool.shape[1]) + JX.kappa_jastrow(M)
    return est, 2.0 * max(seen, default=0.0) + 4.0


def draw(n: int, npool: int, seed) -> tuple:
    """(pick, w): every pool entry picked at least once (the first npool walkers, shuffled in with the rest), weights in (0.1, 1.1) / sum"""
    g = np.random.default_rng(seed)
    pick = np.concatenate([np.arange(npool), g.integers(0, npool, size=n - npool)]) if n >= npool else g.integers(0, npool, size=n)
    pick = g.permutation(pick)
    w = g.random(n) + 0.1
    return pick.astype(np.int64), w / w.sum()


# ---- (b) the layout of the fused kernel -----------------------------------------------------------------------------------------------
def hq(H: int) -> int:
    return (H + 7) // 8 * 8 + 1


@dataclass(frozen=True)
class Layout:
    n: int
    sorb: int
    H: int
    K: int
    npS: int
    nslD: int      # slices of the pair kernel
    lenD: int      # walkers per slice
    nslS: int      # slices of the singles and diagonal kernels
    lenS: int
    total: int     # doubles of pynqs_rdm_rbm's workspace

    @property
    def chunks(self) -> int:
        return (self.n + KBLOCK - 1) // KBLOCK if self.n > 0 else 1

    def regime(self):
        """((slices, chunks per slice) of the pair kernel, the same of the singles and diagonal kernels)"""
        return (self.nslD, self.lenD // KBLOCK), (self.nslS, self.lenS // KBLOCK)

    def last_slice(self, singles: bool) -> int:
        """walkers of the last slice"""
        nsl, length = (self.nslS, self.lenS) if singles else (self.nslD, self.lenD)
        return self.n - (nsl - 1) * length

    def last_chunk(self) -> int:
        return self.n - (self.chunks - 1) * KBLOCK


def _slices(chunks: int, owners: int, per_slice: int, want: int):
    s = (want + owners - 1) // owners
    s = min(s, TABLE_CAP // max(per_slice, 1), chunks)
    s = max(s, 1)
    per = (chunks + s - 1) // s
    return (chunks + per - 1) // per, per * KBLOCK


def layout(n: int, sorb: int, H: int):
    """Layout, or None where the sizes are refused (odd sorb, sorb outside 2 .. 192, H outside 1 .. 8192, n < 0)"""
    if sorb < 2 or sorb % 2 or sorb > MAX_SORB or n < 0 or H < 1 or H > 8192:
        return None
    K = sorb // 2
    npS = K * (K - 1) // 2
    chunks = (n + KBLOCK - 1) // KBLOCK if n > 0 else 1
    szDg, szT = sorb * sorb, sorb * sorb * (sorb + 1)
    szD = (npS * npS, npS * npS, K ** 4)
    nslD, lenD = _slices(chunks, 2 * npS + K * K, sum(szD), 4096)
    nslS, lenS = _slices(chunks, sorb, szT + szDg, 2048)
    total = n * H + nslS * (szDg + szT) + nslD * sum(szD)
    return Layout(n, sorb, H, K, npS, nslD, lenD, nslS, lenS, total)


def workspace_bytes(n: int, sorb: int, H: int, jastrow: bool = False) -> int:
    L = layout(n, sorb, H)
    if L is None:
        return -1
    return 8 * (L.total + (n * sorb if jastrow else 0))


def lds_bytes(sorb: int, H: int, singles: bool, jastrow: bool = False) -> int:
    K = sorb // 2
    doubles = sorb * hq(H) + 4 * H + 2 * (KBLOCK // WAVE) + sorb + (K * sorb if singles else 0)
    return 8 * doubles + 4 * (KBLOCK + KBLOCK // WAVE) + (16 * sorb if jastrow else 0)


def supported(sorb: int, nele: int, noA: int, noB: int, H: int, jastrow: bool = False) -> bool:
    if layout(0, sorb, H) is None:
        return False
    K = sorb // 2
    if nele != noA + noB or noA < 0 or noB < 0 or noA > K or noB > K:
        return False
    if H > MAX_HIDDEN or sorb > KBLOCK or K * K > MAX_ITEMS * KBLOCK:
        return False
    return lds_bytes(sorb, H, True, jastrow) <= MAX_LDS


def max_hidden(sorb: int, jastrow: bool = False) -> int:
    """the largest H the fused kernel serves at this sorb (0: none)"""
    return max((H for H in range(1, MAX_HIDDEN + 1) if supported(sorb, 2, 1, 1, H, jastrow)), default=0)


def owner_empty(sorb: int, noA: int, noB: int) -> bool:
    """the particle side owns when the shells are more than half full"""
    return noA + noB > sorb // 2


def pair_owners(sorb: int):
    """the owners of the pair kernel: (o0, o1) same-spin pairs o0 > o1 of either spin, then (alpha, beta) pairs"""
    out = []
    for spin in (0, 1):
        out += [(2 * hi + spin, 2 * lo + spin) for hi in range(sorb // 2) for lo in range(hi)]
    return out + [(2 * a, 2 * b + 1) for a in range(sorb // 2) for b in range(sorb // 2)]


def owner_qualifies(occ: np.ndarray, orbitals, empty: bool) -> np.ndarray:
    """bool [n]: the walkers in which every owner orbital is empty (the particle side owns) / occupied"""
    want = 0 if empty else 1
    return np.all(np.asarray(occ)[:, list(orbitals)] == want, axis=1)


def wave_counts(qualifies: np.ndarray) -> np.ndarray:
    """int [chunks, 4]: the qualifying walkers of every wave (64 consecutive walkers) of every chunk of 256"""
    q = np.asarray(qualifies, dtype=np.int64)
    chunks = max(1, (q.size + KBLOCK - 1) // KBLOCK)
    full = np.zeros(chunks * KBLOCK, dtype=np.int64)
    full[:q.size] = q
    return full.reshape(chunks, KBLOCK // WAVE, WAVE).sum(2)


def ballot_regimes(occ: np.ndarray, sorb: int, noA: int, noB: int) -> dict:
    """what the owners of both kernels see in these walkers:
        all_waves     : some owner has qualifying walkers in all four waves of one chunk (every wave offset `before` is in use)
        gap_then_hit  : some owner's ballot is empty in one wave and non-empty in the next wave of the same chunk
        empty_chunk   : some owner sees no qualifying walker in one chunk and some in another"""
    empty = owner_empty(sorb, noA, noB)
    out = {"all_waves": False, "gap_then_hit": False, "empty_chunk": False}
    for orbitals in pair_owners(sorb) + [(o,) for o in range(sorb)]:
        c = wave_counts(owner_qualifies(occ, orbitals, empty))
        out["all_waves"] |= bool((c > 0).all(1).any())
        out["gap_then_hit"] |= bool(((c[:, :-1] == 0) & (c[:, 1:] > 0)).any())
        per_chunk = c.sum(1)
        out["empty_chunk"] |= bool((per_chunk == 0).any() and (per_chunk > 0).any())
        if all(out.values()):
            break
    return out
