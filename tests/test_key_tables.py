"""The constructions of tests/key_tables.py, on the CPU: every condition tests/test_gpu_key_tables.py relies on is asserted here, from the
replicas alone (conditions on the inputs, not measurements):
  * occupied_set against a plain insertion in two different orders, and the replicas' fixed points (capacities, filter sizes);
  * every chain table: exactly cap / 4 distinct keys, hash_capacity(nkeys) == cap, a run that crosses cap - 1 -> 0, the displacement every
    insertion order must produce, three non-empty groups of absent queries that are what they say;
  * unique_rows: 200 distinct rows in the last four slots of a 1024-slot table, the run wraps, n <= 512, the two arrangements, first[i];
  * the REDUCE cases, from oracle.comb_hij_fused: the distinct kept determinants nu, dedup_slots = pow2 >= 2 nu, load >= 0.4, a run under
    home_dedup that crosses the table end, <x|H|x> of every walker kept, eps well inside a gap of the |h|."""
import time

import numpy as np
import pytest

import key_tables as K

_CLOCK = {}


@pytest.fixture(scope="module", autouse=True)
def _clock():
    _CLOCK["t0"] = time.time()
    yield


def test_replicas_fixed_points():
    assert [K.hash_capacity(n) for n in (0, 1, 16, 17, 64, 65, 1024, 300000)] == [64, 64, 64, 128, 256, 512, 4096, 1 << 21]
    assert [K.hash_filter_bits(n) for n in (0, 1, 16, 64, 1024, 3000, 1 << 18, (1 << 18) + 1, 300000)] == [0, 1024, 1024, 1024, 8192, 16384, 1 << 18, 0, 0]
    assert [K.hash_filter2_bits(n) for n in (0, 1, 1024, 1025, 300000, 1 << 22)] == [0, 1 << 15, 1 << 15, 1 << 16, 1 << 24, 1 << 26]
    assert [K.hash_string_bits(n) for n in (0, 1, 512, 513, 1 << 20)] == [0, 1 << 13, 1 << 13, 1 << 14, 1 << 22]
    assert K.hash_string_bits_if(300000) == 0 and K.hash_string_bits_if(3000) == 1 << 16
    assert K.hash_bytes(16, 40) == 64 * 16 + (1024 + (1 << 15) + 2 * (1 << 13)) // 8 and K.hash_bytes(16, 66) == 64 * 32 + (1024 + (1 << 15) + 2 * (1 << 13)) // 8
    # a determinant's words: orbital o is bit o % 64 of word o // 64
    bits = np.zeros((1, 130), dtype=np.uint8)
    bits[0, [0, 63, 64, 129]] = 1
    assert K.words_of(bits).tolist() == [[1 | 1 << 63, 1, 2]]
    # hash_of in exact integer arithmetic
    M = (1 << 64) - 1
    w = np.array([[3, 5, 1 << 63]], dtype=np.uint64)
    h = (3 * 0x9E3779B97F4A7C15) & M
    for q in (5, 1 << 63):
        h = ((h ^ (h >> 32) ^ q) * 0xBF58476D1CE4E5B9) & M
    assert int(K.hash_of(w)[0]) == h ^ (h >> 29)
    b0, b1 = K.filter_positions(np.array([0xDEADBEEF], dtype=np.uint32), 1 << 12)
    assert (int(b0[0]), int(b1[0])) == (0xEEF, 0xDEA)
    word, mask = K.filter2_position(np.array([0xDEADBEEF], dtype=np.uint32), 1 << 15)
    assert int(word[0]) == 0xDEADBEEF & 1023 and int(mask[0]) == (1 << ((0xDEADBEEF >> 22) & 31)) | (1 << (0xDEADBEEF >> 27))


def test_occupied_set_is_what_any_insertion_order_occupies():
    g = np.random.default_rng(1)
    for cap, n in ((64, 16), (64, 31), (256, 64), (1024, 511), (64, 1), (64, 0)):
        for trial in range(6):
            h = g.integers(0, cap, n) if trial < 3 else (cap - 1 - g.integers(0, 3, n)) % cap   # random / crowded at the table's end
            occ = K.occupied_set(h, cap)
            assert np.array_equal(occ, K.simulate(h, cap)) and np.array_equal(occ, K.simulate(h[::-1], cap))
            r = K.runs_of(h, cap)
            assert r.wraps == bool(occ[0] and occ[cap - 1])
            if trial >= 3 and n > 3:
                assert r.wraps and r.displacement >= n / 3 - 1


@pytest.mark.parametrize("name,cap", K.CHAIN_CASES, ids=lambda v: str(v))
def test_chain_tables(name, cap):
    c = K.chain_table(name, cap)
    words = K.words_of(c.bits)
    nk = c.bits.shape[0]
    assert nk == cap // 4 and np.unique(words, axis=0).shape[0] == nk and K.hash_capacity(nk) == cap
    h = K.home(words, cap)
    others = nk - c.nwalkers
    assert bool((h[c.nwalkers:] >= cap - c.slots).all()) and np.unique(h[c.nwalkers:]).size <= c.slots
    if (name, cap) != ("s12one", 64) and cap <= 256:
        assert c.slots == 1                       # every non-walker key homes on slot cap - 1
    _, cand_words, nw = K.candidates(name)
    hc = K.home(cand_words[nw:], cap)
    assert int((hc >= cap - c.slots).sum()) >= others > int((hc > cap - c.slots).sum())   # the fewest last slots that suffice
    r = K.runs_of(h, cap)
    assert r.wraps and r.first_of_wrapped is not None and r.longest >= others
    assert r.displacement >= others / c.slots - 1
    if c.slots == 1:
        assert r.displacement >= others - 1
    occ = K.occupied_set(h, cap)
    assert np.array_equal(occ, K.simulate(h, cap))
    print(f"chain table {name} cap {cap}: {others} keys homing on the last {c.slots} slot(s), longest run {r.longest}, forced displacement {r.displacement}")
    # the absent queries: same sector, no keys, homes where they should be
    import test_gpu_ss_exact as T

    s = T.SHAPES[name]
    keys = {row.tobytes() for row in c.bits}
    a = K.absent_queries(c.bits, name, cap)
    for group in a:
        assert group.shape[0] >= 1
        assert bool((group[:, 0::2].sum(1) == s.noA).all() and (group[:, 1::2].sum(1) == s.noB).all())
        assert not any(row.tobytes() in keys for row in group)
    assert bool((K.home(K.words_of(a.first), cap) == r.first_of_wrapped).all())
    hm = K.home(K.words_of(a.middle), cap)
    assert bool(occ[hm].all()) and bool((hm != r.first_of_wrapped).all())
    between = lambda s0: bool(occ[np.arange(r.first_of_wrapped, r.first_of_wrapped + ((s0 - r.first_of_wrapped) % cap) + 1) % cap].all())  # noqa: E731
    assert all(between(int(s0)) for s0 in hm)      # (inside THE wrapped run, not another one)
    assert not bool(occ[K.home(K.words_of(a.empty), cap)].any())
    lo, hi = K.words_of(K.sector_extremes(name))
    as_int = lambda w: sum(int(v) << (64 * i) for i, v in enumerate(w))  # noqa: E731
    ints = [as_int(w) for w in words]
    assert as_int(lo) <= min(ints) and as_int(hi) >= max(ints)


def test_unique_rows():
    u = K.unique_rows()
    assert sorted(u) == [(L, a) for L in (1, 2, 3) for a in ("ends", "late")]
    for (L, arr), (rows, distinct) in u.items():
        n = rows.shape[0]
        assert rows.shape[1] == L and n <= 512 and 2 * n <= 1024
        assert np.unique(rows, axis=0).shape[0] == 200 == np.unique(distinct, axis=0).shape[0]
        h = K.home_unique(distinct, 1023)
        assert bool((h >= 1020).all())
        r = K.runs_of(h, 1024)
        assert r.wraps and r.longest >= 200 and r.displacement >= 200 / 4 - 1
        first = K.first_occurrence(rows)
        assert first.dtype == np.int32 and bool((first <= np.arange(n)).all()) and np.array_equal(rows[first], rows)
        assert int((first == np.arange(n)).sum()) == 200
        counts = np.bincount(first, minlength=n)
        assert counts.max() <= 3
        if arr == "late":
            assert first[n - 1] == n - 1              # the last element is the first occurrence of its row
        else:
            assert first[n - 1] == 0                  # one key on both ends


@pytest.mark.parametrize("name", sorted(K.REDUCE_CASES))
def test_reduce_cases(name):
    c, x, comb, hm, uniq = K.reduce_case(name)
    a = np.abs(hm)
    L = (c.sorb - 1) // 64 + 1
    assert uniq.shape[1] == L
    # eps sits well inside a gap of the |h|: float64 on the GPU keeps the same columns
    assert float(np.abs(a - c.eps).min()) >= 4e-7
    if name.endswith("draws"):
        uniq = K.distinct_words(comb, np.ones(hm.shape, dtype=bool))   # every connected determinant: kept or drawn
        assert int((hm == 0).sum()) == 0                                # (none that no draw can reach)
    else:
        assert bool((a[:, 0] >= c.eps).all())                          # psi(x) enters every walker's sum
        assert int((a >= c.eps).sum(1).max()) <= 300
    nu = uniq.shape[0]
    slots = K.pow2_at_least(2 * nu)
    assert slots >= 2 * nu and (slots == 64 or slots < 4 * nu)
    assert nu / slots >= 0.4
    r = K.runs_of(K.home_dedup(uniq, slots - 1), slots)
    assert r.wraps
    print(f"REDUCE case {name}: {nu} distinct determinants in {slots} slots (load {nu / slots:.3f}), longest run {r.longest}, forced displacement {r.displacement}")


def test_the_search_finds_the_committed_one_word_case():
    c = K.REDUCE_CASES["one-word"]
    n, eps, seed, nu, load = K.search_reduce_case(c.sorb, c.noA, c.noB, [c.n], [c.seed])
    assert (n, eps, seed, nu, load) == (c.n, c.eps, c.seed, 256, 0.5)


def test_zz_run_time_stays_in_seconds():
    dt = time.time() - _CLOCK["t0"]
    print(f"tests/test_key_tables.py: {dt:.1f} s")
    assert dt < 60.0
