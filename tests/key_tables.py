"""Host-side replicas and constructions for the key tables underneath the local-energy kernels (numpy only, no device code):
  * the psi hash table and its three Bloom filters (kernels_hash.hip; detcore.h: hash_of, hash_capacity, zobrist32[b], zobrist_of,
    zobrist_strings, filter_positions, filter2_position, hash_filter_bits, hash_filter2_bits, hash_string_bits[_if] at their default
    environment);
  * the row table of pynqs_unique_first (kernels_unique.hip: slot (hash >> 20) & mask) and the de-duplication table of the REDUCE front
    end (reduce_common.h: slot (hash >> 17) & mask).
The replicas restate the HASHING and FILTER functions only, never the probing: linear probing occupies the same SET of slots in whatever
order the keys arrive (occupied_set), so the device table read back must occupy exactly that set -- which is what validates the replicas
against the device code (tests/test_gpu_key_tables.py) -- and every key must sit in a slot that no empty slot separates from its home.

Constructions (tests/test_key_tables.py asserts their conditions on the CPU):
  chain_table(name, cap)      cap / 4 keys of a shape of test_gpu_ss_exact: the walkers and connected determinants that all home in the
                              last slot(s) of a table of `cap` slots: one run of the non-walker keys that wraps from slot cap - 1 to 0;
  absent_queries(...)         determinants of the same sector that are no keys and home on the first slot of that run (the lookup walks
                              the whole run and ends on an empty slot), inside it, and on an empty slot;
  unique_rows(nslots)         one-, two- and three-word rows that all home in the last four slots of pynqs_unique_first's table;
  reduce_case(name)           walkers, eps of a REDUCE call whose distinct kept determinants fill the de-duplication table to >= 0.4 with a
                              run that wraps."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

U64 = np.uint64
_M1, _M2 = U64(0x9E3779B97F4A7C15), U64(0xBF58476D1CE4E5B9)
FILTER_MAX_BITS = 1 << 18


# ---- determinants as words ---------------------------------------------------------------------------------------------------------
def words_of(bits: np.ndarray) -> np.ndarray:
    """uint64 [n, len] of occupation rows uint8 0/1 [n, sorb] (bit o of word o // 64 = orbital o)"""
    bits = np.ascontiguousarray(bits, dtype=np.uint8)
    n, sorb = bits.shape
    L = (sorb - 1) // 64 + 1
    pad = np.zeros((n, 64 * L), dtype=np.uint8)
    pad[:, :sorb] = bits
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little")).view(U64).reshape(n, L)


def onv_of(words: np.ndarray) -> np.ndarray:
    """packed determinants uint8 [n, 8 len] of their words"""
    w = np.ascontiguousarray(words, dtype=U64)
    return w.view(np.uint8).reshape(w.shape[0], 8 * w.shape[1])


# ---- the hash and the capacities ---------------------------------------------------------------------------------------------------
def hash_of(words: np.ndarray) -> np.ndarray:
    """detcore.h hash_of<LEN>: uint64 [n] of uint64 [n, LEN], LEN = 1, 2, 3 (products modulo 2^64)"""
    w = np.ascontiguousarray(words, dtype=U64)
    h = w[:, 0] * _M1
    for k in range(1, w.shape[1]):
        h = (h ^ (h >> U64(32)) ^ w[:, k]) * _M2
    return h ^ (h >> U64(29))


def hash_capacity(nkeys: int) -> int:
    c = 64
    while c < 4 * max(int(nkeys), 1):
        c <<= 1
    return c


def home(words: np.ndarray, cap: int) -> np.ndarray:
    """home slot in the psi table of `cap` slots, int64 [n]"""
    return (hash_of(words) & U64(cap - 1)).astype(np.int64)


def home_unique(words: np.ndarray, mask: int) -> np.ndarray:
    return ((hash_of(words) >> U64(20)) & U64(mask)).astype(np.int64)


def home_dedup(words: np.ndarray, mask: int) -> np.ndarray:
    return ((hash_of(words) >> U64(17)) & U64(mask)).astype(np.int64)


# ---- Zobrist values and filter positions -------------------------------------------------------------------------------------------
def zobrist32(orbital) -> np.ndarray:
    z = (np.asarray(orbital).astype(np.uint32) + np.uint32(1)) * np.uint32(0x9E3779B1)
    z = (z ^ (z >> np.uint32(15))) * np.uint32(0x85EBCA77)
    z = (z ^ (z >> np.uint32(13))) * np.uint32(0xC2B2AE3D)
    return z ^ (z >> np.uint32(16))


def zobrist32b(orbital) -> np.ndarray:
    z = (np.asarray(orbital).astype(np.uint32) + np.uint32(0x51)) * np.uint32(0x7FEB352D)
    z = (z ^ (z >> np.uint32(16))) * np.uint32(0x846CA68B)
    z = (z ^ (z >> np.uint32(15))) * np.uint32(0x9E3779B1)
    return z ^ (z >> np.uint32(13))


def _xor_of(bits: np.ndarray, values: np.ndarray) -> np.ndarray:
    return np.bitwise_xor.reduce(np.where(bits.astype(bool), values[None, :], np.uint32(0)), axis=1).astype(np.uint32)


def zobrist_of(bits: np.ndarray):
    """(z, z2): the XOR of zobrist32 / zobrist32b over the occupied orbitals; bits uint8 [n, sorb]"""
    o = np.arange(bits.shape[1])
    return _xor_of(bits, zobrist32(o)), _xor_of(bits, zobrist32b(o))


def zobrist_strings(bits: np.ndarray):
    """(za, zb): zobrist32 over the occupied even / odd orbitals"""
    z = zobrist32(np.arange(bits.shape[1]))
    even = (np.arange(bits.shape[1]) & 1) == 0
    return _xor_of(bits, np.where(even, z, np.uint32(0))), _xor_of(bits, np.where(even, np.uint32(0), z))


def filter_positions(z: np.ndarray, fbits: int):
    """(b0, b1): the low and the high log2(fbits) bits of z"""
    k = int(fbits).bit_length() - 1
    assert fbits == 1 << k and 10 <= k <= 22
    z = np.asarray(z, dtype=np.uint32)
    return z & np.uint32(fbits - 1), z >> np.uint32(32 - k)


def filter2_position(z2: np.ndarray, f2bits: int):
    """(word, mask): both bits of a key in one 32-bit word"""
    z2 = np.asarray(z2, dtype=np.uint32)
    one = np.uint32(1)
    return z2 & np.uint32(f2bits // 32 - 1), (one << ((z2 >> np.uint32(22)) & np.uint32(31))) | (one << (z2 >> np.uint32(27)))


def hash_filter_bits(nkeys: int) -> int:
    if nkeys <= 0:
        return 0
    b = 1024
    while 2 * b <= 8 * nkeys and 2 * b <= FILTER_MAX_BITS:
        b <<= 1
    return b if b >= nkeys else 0


def hash_filter2_bits(nkeys: int) -> int:
    if nkeys <= 0:
        return 0
    b = 1 << 15
    while b < 32 * nkeys and b < (1 << 26):
        b <<= 1
    return b


def hash_string_bits(nkeys: int) -> int:
    if nkeys <= 0:
        return 0
    b = 1 << 13
    while b < 16 * nkeys and b < (1 << 22):
        b <<= 1
    return b


def hash_string_bits_if(nkeys: int) -> int:
    return hash_string_bits(nkeys) if hash_filter_bits(nkeys) else 0


def hash_bytes(nkeys: int, sorb: int) -> int:
    """pynqs_hash_bytes"""
    L = (sorb - 1) // 64 + 1
    return hash_capacity(nkeys) * (2 if L == 1 else 4) * 8 + (hash_filter_bits(nkeys) + hash_filter2_bits(nkeys) + 2 * hash_string_bits_if(nkeys)) // 8


def _bloom(nbits: int, *positions) -> np.ndarray:
    f = np.zeros(nbits // 32, dtype=np.uint32)
    for b in positions:
        np.bitwise_or.at(f, (b >> np.uint32(5)).astype(np.int64), np.uint32(1) << (b & np.uint32(31)))
    return f


def filter_regions(bits: np.ndarray):
    """The four filter regions behind the slots as hash_build_kernel writes them, uint32 arrays: (LDS filter [fbits / 32], second level
    [f2bits / 32], alpha strings [sbits / 32], beta strings [sbits / 32]); an absent filter is an empty array."""
    nk = bits.shape[0]
    fbits, f2bits, sbits = hash_filter_bits(nk), hash_filter2_bits(nk), hash_string_bits_if(nk)
    z, z2 = zobrist_of(bits)
    lds = _bloom(fbits, *filter_positions(z, fbits)) if fbits else np.zeros(0, dtype=np.uint32)
    second = np.zeros(f2bits // 32, dtype=np.uint32)
    if f2bits:
        word, mask = filter2_position(z2, f2bits)
        np.bitwise_or.at(second, word.astype(np.int64), mask)
    alpha = beta = np.zeros(0, dtype=np.uint32)
    if sbits:
        za, zb = zobrist_strings(bits)
        alpha, beta = _bloom(sbits, *filter_positions(za, sbits)), _bloom(sbits, *filter_positions(zb, sbits))
    return lds, second, alpha, beta


# ---- what linear probing occupies --------------------------------------------------------------------------------------------------
def occupied_set(homes: np.ndarray, cap: int) -> np.ndarray:
    """bool [cap]: the slots linear probing occupies for keys with these home slots -- the same set for every insertion order.  Keys taken
    in the order of their homes land on p_i = max(h_i, p_(i-1) + 1) = i + max_(j <= i) (h_j - j); the k of them that run past the end
    come back as k keys homing on slot 0, which may push more past the end: k is raised until it reproduces itself."""
    h = np.sort(np.asarray(homes, dtype=np.int64))
    assert h.size < cap and (h.size == 0 or (0 <= h[0] and h[-1] < cap))
    k = 0
    while True:
        hh = np.concatenate([np.zeros(k, dtype=np.int64), h])
        p = np.arange(hh.size) + np.maximum.accumulate(hh - np.arange(hh.size))
        over = int((p >= cap).sum())
        if over == k:
            break
        k = over
    occ = np.zeros(cap, dtype=bool)
    occ[p[p < cap]] = True
    assert int(occ.sum()) == h.size
    return occ


Runs = namedtuple("Runs", "wraps longest first_of_wrapped displacement")


def runs_of(homes: np.ndarray, cap: int) -> Runs:
    """The run structure of occupied_set: wraps: a run crosses cap - 1 -> 0; longest: the longest run; first_of_wrapped: the first slot of
    the run through slot cap - 1 (None if that slot is empty); displacement: the largest distance between a key and its home that EVERY
    insertion order must produce: the keys of a run that home on its first j slots fill at least that many slots from its start, so the
    last of them lies N(j) - j slots or more past its home -- the figure of the keys taken in the order of their homes."""
    occ = occupied_set(homes, cap)
    if not occ.any():
        return Runs(False, 0, None, 0)
    e = int(np.flatnonzero(~occ)[-1])                      # rotate so that an empty slot comes last: no run wraps any more
    h = np.sort((np.asarray(homes, dtype=np.int64) - e - 1) % cap)
    p = np.arange(h.size) + np.maximum.accumulate(h - np.arange(h.size))
    rot = np.zeros(cap, dtype=bool)
    rot[p] = True
    assert np.array_equal(np.roll(rot, e + 1), occ)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], rot.astype(np.int8), [0]])))
    starts, ends = edges[0::2], edges[1::2]
    first = None
    if occ[cap - 1]:
        r = (cap - 1 - e - 1) % cap
        first = int((starts[(starts <= r) & (r < ends)][0] + e + 1) % cap)
    return Runs(bool(occ[0] and occ[cap - 1]), int((ends - starts).max()), first, int((p - h).max()))


def simulate(homes: np.ndarray, cap: int) -> np.ndarray:
    """occupied slots by plain insertion in the given order (the CPU test holds occupied_set against it)"""
    occ = np.zeros(cap, dtype=bool)
    for s in np.asarray(homes, dtype=np.int64).tolist():
        while occ[s]:
            s = (s + 1) & (cap - 1)
        occ[s] = True
    return occ


# ---- engineered psi tables ---------------------------------------------------------------------------------------------------------
CHAIN_CASES = [("fe2s2", 64), ("fe2s2", 256), ("fe2s2", 4096), ("s66", 64), ("s66", 256), ("s66", 4096), ("s130", 64), ("s130", 256),
               ("s12one", 64)]
Chain = namedtuple("Chain", "name cap bits nwalkers slots")   # bits uint8 [cap / 4, sorb], the walkers first; slots: last slots drawn from


@functools.lru_cache(maxsize=None)
def candidates(name: str):
    """(occupation rows of test_gpu_ss_exact.table_keys(name, "all"), their words, the number of distinct walkers in front)"""
    import test_gpu_ss_exact as T

    bits = T.table_keys(name, "all")
    return bits, words_of(bits), T._unique_rows(T.walkers(name)).shape[0]


@functools.lru_cache(maxsize=None)
def chain_table(name: str, cap: int) -> Chain:
    bits, words, nw = candidates(name)
    need = cap // 4 - nw
    assert need > 0
    h = home(words[nw:], cap)
    count = np.bincount(h, minlength=cap)[::-1]            # candidates homing on cap - 1, cap - 2, ...
    r = int(np.searchsorted(np.cumsum(count), need)) + 1   # the fewest last slots that supply `need`
    assert r < cap, "too few candidates"
    take = np.flatnonzero(h > cap - r)                     # all of the last r - 1 slots
    rest = np.flatnonzero(h == cap - r)[: need - take.size]
    pick = np.sort(np.concatenate([take, rest])) + nw
    assert pick.size == need
    return Chain(name, cap, np.ascontiguousarray(np.concatenate([bits[:nw], bits[pick]])), nw, r)


Absent = namedtuple("Absent", "first middle empty")   # occupation rows uint8 [m, sorb] each


@functools.lru_cache(maxsize=None)
def _sector_pool(name: str) -> np.ndarray:
    """determinants of the shape's sector: the candidates that lie in it, then random ones"""
    import test_gpu_ss_exact as T
    from conftest import rand_occ

    s = T.SHAPES[name]
    bits = candidates(name)[0]
    ok = (bits[:, 0::2].sum(1) == s.noA) & (bits[:, 1::2].sum(1) == s.noB)
    return T._unique_rows(np.concatenate([bits[ok], rand_occ(4000, s.sorb, s.noA, s.noB, seed=97)]))


def absent_queries(table_keys: np.ndarray, name: str, cap: int, each: int = 6) -> Absent:
    keys = {r.tobytes() for r in np.ascontiguousarray(table_keys, dtype=np.uint8)}
    pool = _sector_pool(name)
    pool = pool[[r.tobytes() not in keys for r in pool]]
    occ = occupied_set(home(words_of(table_keys), cap), cap)
    first = runs_of(home(words_of(table_keys), cap), cap).first_of_wrapped
    assert first is not None
    h = home(words_of(pool), cap)
    inside = np.zeros(cap, dtype=bool)   # the wrapped run without its first slot
    s = (first + 1) & (cap - 1)
    while occ[s]:
        inside[s] = True
        s = (s + 1) & (cap - 1)
    return Absent(pool[h == first][:each], pool[inside[h]][:each], pool[~occ[h]][:each])


def sector_extremes(name: str) -> np.ndarray:
    """the smallest and the largest determinant of the sector as little-endian integers: the lowest / the highest orbitals occupied"""
    import test_gpu_ss_exact as T

    s = T.SHAPES[name]
    lo, hi = np.zeros(s.sorb, dtype=np.uint8), np.zeros(s.sorb, dtype=np.uint8)
    lo[0:2 * s.noA:2] = 1
    lo[1:2 * s.noB:2] = 1
    hi[s.sorb - 2 * s.noA::2] = 1
    hi[s.sorb - 2 * s.noB + 1::2] = 1
    return np.stack([lo, hi])


# ---- rows for pynqs_unique_first ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unique_rows(nslots: int = 1024):
    """{(len, arrangement): (rows uint64 [n, len], distinct rows uint64 [200, len])}: 200 distinct rows per word count that all home in the
    last four slots of the `nslots`-slot row table, each repeated 1-3 times in a seeded shuffle, n <= nslots / 2 (the table keeps its
    size).  arrangement "late": the last element is the only occurrence of its row; "ends": elements 0 and n - 1 are the same row."""
    out = {}
    for L in (1, 2, 3):
        g = np.random.default_rng(300 + L)
        w = g.integers(0, 1 << 63, size=(120000, L), dtype=np.int64).astype(U64) * U64(2) + g.integers(0, 2, size=(120000, L)).astype(U64)
        w = w[~(w == ~U64(0)).all(1)]
        w = w[home_unique(w, nslots - 1) >= nslots - 4]
        w = w[np.sort(np.unique(w, axis=0, return_index=True)[1])][:200]
        assert w.shape[0] == 200
        reps = g.integers(1, 4, size=199)
        body = np.repeat(np.arange(199), reps)
        for arr in ("late", "ends"):
            order = body[g.permutation(body.size)]
            idx = np.concatenate([order, [199]]) if arr == "late" else np.concatenate([[199], order, [199]])
            assert idx.size <= nslots // 2
            out[(L, arr)] = (np.ascontiguousarray(w[idx]), w)
    return out


def first_occurrence(rows: np.ndarray) -> np.ndarray:
    """first[i] = the smallest j with rows[j] == rows[i], int32 [n]"""
    seen = {}
    return np.array([seen.setdefault(r.tobytes(), i) for i, r in enumerate(np.ascontiguousarray(rows))], dtype=np.int32)


# ---- the de-duplication table at its tightest ----------------------------------------------------------------------------------------
# walkers rand_occ(n, sorb, noA, noB, seed), synthetic integrals, |<x|H|x'>| >= eps kept: found by search_reduce_case (a search on the CPU:
# these are inputs), fixed here.  tests/test_key_tables.py asserts what they were chosen for.
ReduceCase = namedtuple("ReduceCase", "name sorb noA noB n eps seed")
# one-word: 256 distinct kept determinants in 512 slots; two-words: 1024 in 2048 -- exactly half full, what the constructor allows at most;
# one-word-draws: all 256 connected determinants of its 5 walkers (kept or drawn) in 512 slots if every one of them is reached
REDUCE_CASES = {c.name: c for c in (ReduceCase("one-word", 12, 2, 3, 12, 0.31417963988686326, 1),
                                    ReduceCase("two-words", 66, 3, 3, 8, 0.49866978111479165, 1),
                                    ReduceCase("one-word-draws", 12, 2, 3, 5, 0.31417963988686326, 16))}
DRAWS = 4000


def pow2_at_least(v: int) -> int:
    c = 64
    while c < v:
        c <<= 1
    return c


def reduce_rows(sorb: int, noA: int, noB: int, n: int, seed: int):
    """(walkers' occupation rows, packed walkers, comb uint8 [n, ncomb, 8 len], hm float64 [n, ncomb]) from the CPU oracle"""
    from conftest import rand_occ, synth_integrals
    from oracle import oracle as O

    occ = rand_occ(n, sorb, noA, noB, seed=seed)
    x = O.pm01_to_onv(occ, sorb)
    h1, h2 = synth_integrals(sorb)
    comb, hm = O.comb_hij_fused(x, h1, h2, sorb, noA + noB, noA, noB)
    return occ, x, comb, hm


def distinct_words(comb: np.ndarray, keep: np.ndarray) -> np.ndarray:
    """the distinct determinants among comb[keep], uint64 [nu, len]"""
    L = comb.shape[-1] // 8
    return np.unique(np.ascontiguousarray(comb[keep]).view(U64).reshape(-1, L), axis=0)


@functools.lru_cache(maxsize=None)
def reduce_case(name: str):
    """(ReduceCase, packed walkers, comb, hm, distinct kept determinants' words)"""
    c = REDUCE_CASES[name]
    _, x, comb, hm = reduce_rows(c.sorb, c.noA, c.noB, c.n, c.seed)
    return c, x, comb, hm, distinct_words(comb, np.abs(hm) >= c.eps)


def search_reduce_case(sorb: int, noA: int, noB: int, ns, seeds, min_load: float = 0.4, max_kept: int = 300):
    """(n, eps, seed, nu, load) of the first walker batch and eps (a midpoint between two consecutive |h|, so that no element is within
    rounding of it) whose distinct kept determinants load the table to >= min_load with a run that wraps, no walker keeping more than
    max_kept columns."""
    for n in ns:
        for seed in seeds:
            _, _, comb, hm = reduce_rows(sorb, noA, noB, n, seed)
            a = np.abs(hm)
            v = np.unique(a)
            floor = np.sort(a, axis=1)[:, ::-1][:, min(max_kept, a.shape[1] - 1)].max()
            ok = np.flatnonzero((v[:-1] >= floor) & (v[1:] <= a[:, 0].min()) & (np.diff(v) >= 1e-6))  # (<x|H|x> of every walker stays kept)
            for i in ok[np.unique(np.linspace(0, ok.size - 1, 600).astype(int))] if ok.size else ():
                eps = float((v[i] + v[i + 1]) / 2)
                u = distinct_words(comb, a >= eps)
                slots = pow2_at_least(2 * u.shape[0])
                if u.shape[0] / slots >= min_load and runs_of(home_dedup(u, slots - 1), slots).wraps:
                    return n, eps, seed, u.shape[0], u.shape[0] / slots
    return None
