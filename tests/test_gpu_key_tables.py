"""The lookup machinery underneath the local-energy kernels on inputs built to stress it (tests/key_tables.py; their conditions are asserted
on the CPU by tests/test_key_tables.py): psi tables whose non-walker keys all home on the last slot(s), so that they form one probe chain
of up to a thousand keys that runs past slot cap - 1 into slot 0, queried with every key, with absent determinants that home on the first
slot of that chain, inside it and on an empty slot, and with the smallest and the largest determinant of the sector.
  a. the table as pynqs_hash_build leaves it, read back: every key in one slot with its position in the sorted keys, the occupied slots
     exactly those the host replica of the hash predicts (which validates the replica), no empty slot between a key's home and its slot,
     all other words all-ones, and the four filter regions bit for bit the OR of the keys' positions;
  b. hash_lookup, the binary search and WavefunctionLUT.find against a Python dict;
  c. every SAMPLE_SPACE entry point and the REDUCE front end on the chain tables against tests/ss_exact.py under its bound, psi(x) bit-exact;
  d. the unfiltered hash kernel (PYNQS_FILTER_BITS=0, read once per process: a fresh child, tests/ss_nofilter_worker.py);
  e. pynqs_unique_first on rows that all home in the last four slots of its table;
  f. the de-duplication table of the REDUCE front end exactly half full (cap_unique = the number of distinct determinants), one too small,
     and filled by draws;
  g. the block index on keys that differ inside one block only: the other four blocks are one run of equal values.
No tolerance is new here: the energies are held to the bound of ss_exact.py, everything else is exact."""
import functools
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import key_tables as K
import ss_exact as S
import test_gpu_ss_exact as T
from conftest import rand_occ, synth_integrals

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _lut(bits, sorb):
    from pynqs_amd import public_function as pf

    dev = torch.device("cuda")
    keys = _dev(K.onv_of(K.words_of(bits)))
    return pf.WavefunctionLUT(keys, torch.zeros(keys.size(0), dtype=torch.float64, device=dev), sorb, device=dev)


# ---- the tables ------------------------------------------------------------------------------------------------------------------------
# (kind, shape or sorb, size): chain tables; the first n candidates of fe2s2 at the boundary sizes of hash_capacity (1, 16 -> 64 slots,
# 17 -> 128); 3000 random keys at sorb 136 (orbitals in all three words); 300 000 random keys (no LDS filter, no string filters)
TABLES = [("chain", n, c) for n, c in K.CHAIN_CASES] + [("first", "fe2s2", n) for n in (1, 16, 17)] + [("random", 136, 3000), ("random", 40, 300000)]


@functools.lru_cache(maxsize=None)
def table_bits(kind, what, size):
    """(keys 0/1 [nk, sorb], sorb)"""
    if kind == "chain":
        return K.chain_table(what, size).bits, T.SHAPES[what].sorb
    if kind == "first":
        return K.candidates(what)[0][:size], T.SHAPES[what].sorb
    g = np.random.default_rng(what + size)
    no = 10 if what == 136 else 15
    pick = lambda: np.argsort(g.random((size + size // 8, what // 2)), axis=1)[:, :no]  # noqa: E731
    bits = np.zeros((size + size // 8, what), dtype=np.uint8)
    rows = np.arange(bits.shape[0])[:, None]
    bits[rows, 2 * pick()] = 1
    bits[rows, 2 * pick() + 1] = 1
    bits = bits[np.sort(np.unique(K.words_of(bits), axis=0, return_index=True)[1])][:size]
    assert bits.shape[0] == size
    return bits, what


def _sorted_words(lut):
    k = lut.bra_key.cpu().numpy()
    return np.ascontiguousarray(k).view(np.uint64).reshape(k.shape[0], -1)


def _bits_of_words(words, sorb):
    return T.bits_of(K.onv_of(words), sorb)


@pytest.mark.parametrize("case", TABLES, ids=T.case_id)
def test_table_as_built(case):
    from pynqs_amd import _native as N

    bits, sorb = table_bits(*case)
    lut = _lut(bits, sorb)
    words = _sorted_words(lut)
    nk, L = words.shape
    W = 2 if L == 1 else 4
    cap = K.hash_capacity(nk)
    fbits, f2bits, sbits = K.hash_filter_bits(nk), K.hash_filter2_bits(nk), K.hash_string_bits_if(nk)
    raw = lut.hashtable.table.cpu().numpy().view(np.uint64)
    assert raw.nbytes == N.lib().pynqs_hash_bytes(nk, sorb) == K.hash_bytes(nk, sorb) == cap * W * 8 + (fbits + f2bits + 2 * sbits) // 8
    slots = raw[: cap * W].reshape(cap, W)
    idx = slots[:, W - 1].view(np.int64)
    occ = idx != -1
    # every key in exactly one slot, with its position in the sorted keys
    assert int(occ.sum()) == nk and np.array_equal(np.sort(idx[occ]), np.arange(nk))
    assert np.array_equal(slots[occ][:, :L], words[idx[occ]])
    # all other words are all-ones: the empty slots, and the unused third word of a two-word slot
    assert bool((slots[~occ] == ALL_ONES).all()) and bool((slots[:, L:W - 1] == ALL_ONES).all())
    # the occupied set is the replica's (this is what validates the host hash against the device's)
    home = K.home(words, cap)
    want = K.occupied_set(home, cap)
    assert np.array_equal(occ, want), f"{int((occ != want).sum())} slots differ from the replica's occupied set"
    # no empty slot between a key's home and its slot, cyclically
    at = np.empty(nk, dtype=np.int64)
    at[idx[occ]] = np.flatnonzero(occ)
    dist = (at - home) % cap
    empties = np.concatenate([[0], np.cumsum(~np.concatenate([occ, occ]))])
    assert bool((empties[home + dist + 1] - empties[home] == 0).all())
    r = K.runs_of(home, cap)
    if case[0] == "chain":
        assert r.wraps and bool(occ[0] and occ[cap - 1]) and int(dist.max()) >= r.displacement
    print(f"KT table {T.case_id(case)}: {nk} keys, {cap} slots, longest run {r.longest}, largest displacement {int(dist.max())} (forced: {r.displacement})")
    # the four filter regions, bit for bit
    f = raw[cap * W:].view(np.uint32)
    sizes = [fbits // 32, f2bits // 32, sbits // 32, sbits // 32]
    assert f.size == sum(sizes)
    if case == ("random", 40, 300000):
        assert fbits == 0 and sbits == 0 and f2bits > 0
    if case == ("random", 136, 3000):
        assert bool((words != 0).any(0).all())     # orbitals in all three words
    got = np.split(f, np.cumsum(sizes)[:-1])
    for name, g_, w_ in zip(("LDS filter", "second level", "alpha strings", "beta strings"), got, K.filter_regions(_bits_of_words(words, sorb))):
        assert g_.size == w_.size
        missing, extra = int(np.bitwise_count(w_ & ~g_).sum()) if g_.size else 0, int(np.bitwise_count(g_ & ~w_).sum()) if g_.size else 0
        assert missing == 0 and extra == 0, f"{name}: {missing} bits missing, {extra} bits extra"


# ---- lookups ---------------------------------------------------------------------------------------------------------------------------
def queries(case):
    """(queries 0/1 [m, sorb], what each group is) for a table: every key in a shuffled order, absent determinants, the sector's extremes"""
    bits, sorb = table_bits(*case)
    g = np.random.default_rng(zlib.crc32(repr(case).encode()))
    parts = [bits[g.permutation(bits.shape[0])]]
    if case[0] == "chain":
        parts += list(K.absent_queries(bits, case[1], case[2])) + [K.sector_extremes(case[1])]
    else:
        no = {40: (15, 15), 136: (10, 10)}[sorb]
        parts += [rand_occ(40, sorb, *no, seed=7)]
        if case[0] == "first":
            parts += [K.sector_extremes(case[1]), K.candidates(case[1])[0][case[2]:case[2] + 30]]
    q = np.concatenate(parts)
    if q.shape[0] % 256 == 0:
        q = q[:-1]
    return q


@pytest.mark.parametrize("case", [c for c in TABLES if c[2] < 100000], ids=T.case_id)
def test_lookups(case):
    from pynqs_amd import C_extension as cx

    bits, sorb = table_bits(*case)
    lut = _lut(bits, sorb)
    where = {w.tobytes(): i for i, w in enumerate(_sorted_words(lut))}
    q = queries(case)
    qw = K.words_of(q)
    want = np.array([where.get(w.tobytes(), -1) for w in qw], dtype=np.int64)
    assert q.shape[0] % 256 != 0 and int((want >= 0).sum()) >= bits.shape[0] and int((want < 0).sum()) >= 3
    qd = _dev(K.onv_of(qw))
    for name, (pos, found) in (("hash_lookup", cx.hash_lookup(lut.hashtable, qd)), ("wavefunction_lut", cx.wavefunction_lut(lut.bra_key, qd, sorb)),
                               ("WavefunctionLUT.find", lut.find(qd))):
        np.testing.assert_array_equal(pos.cpu().numpy(), want, err_msg=name)
        np.testing.assert_array_equal(found.cpu().numpy(), want >= 0, err_msg=name)


# ---- energies on the chain tables --------------------------------------------------------------------------------------------------------
VALUES = ("real", "complex")


def chain_mantissas(name, cap, values):
    """amplitudes of the chain table's keys in the order of their construction: moduli in [0.25, 1.25), free signs / phases"""
    nk = cap // 4
    g = np.random.default_rng(zlib.crc32(f"chain {name} {cap} {values}".encode()))
    mod = g.random(nk) + 0.25
    return mod * np.where(g.random(nk) < 0.5, -1.0, 1.0) if values == "real" else mod * np.exp(2j * np.pi * g.random(nk))


@functools.lru_cache(maxsize=None)
def chain_columns(name, cap):
    """([ss_exact.Columns per walker], the same for the flip passes) against the chain table"""
    tab = S.Table(K.chain_table(name, cap).bits)
    cache = {}
    sts = T.structures(name)
    cols = lambda st, flip: cache.setdefault((id(st), flip), S.columns(st, tab, flip))  # noqa: E731
    return [cols(st, False) for st in sts], [cols(st, True) for st in sts]


def chain_yardstick(name, cap, values):
    plain, part = chain_columns(name, cap)
    v = S.as_ld(chain_mantissas(name, cap, values))
    p = [S.table_sum(c, v) for c in plain]
    return p, [S.table_sum(c, v, psi_x=r.psi) for c, r in zip(part, p)]


@functools.lru_cache(maxsize=None)
def chain_device(name, cap):
    return T.Device(name, f"chain{cap}", K.chain_table(name, cap).bits)


def run_forms(d, forms, mant, plain, part, tag):
    """[(form, |E_got - E_exact| / bound per walker)] of the entry points `forms` on the device case d; psi(x) must be the table's bits"""
    psi_want = T.psi_array(plain, mant.dtype)
    vs, vh = d.values(mant)
    out = []
    for f in forms:
        e, p0 = d.run(f, vs, vh, psi_want if f.flip else None)
        np.testing.assert_array_equal(p0, psi_want, err_msg=f"{tag} {f.name}: psi(x)")
        ratio, finite_zero = T.ratios(part if f.flip else plain, e)
        assert finite_zero == 0 and ratio.size == len(plain)   # the walkers are keys: none is left out
        T.report(f"KT {tag} {f.name}", ratio)
        out.append((f.name, ratio))
    return out


def form_kind(name, nkeys):
    """pynqs_eloc_sample_space_form of the shape's walkers against a hash table of nkeys keys: (kind, two levels, workgroup, ...)"""
    import ctypes as C

    from pynqs_amd import _native as N

    s = T.SHAPES[name]
    out = (C.c_int64 * 8)()
    N.check(N.lib().pynqs_eloc_sample_space_form(s.n, s.sorb, s.noA + s.noB, s.noA, s.noB, nkeys, 1, out), "pynqs_eloc_sample_space_form")
    return list(out)


@pytest.mark.parametrize("values", VALUES)
@pytest.mark.parametrize("case", K.CHAIN_CASES, ids=T.case_id)
def test_every_entry_point_on_the_chain_tables(case, values):
    name, cap = case
    d = chain_device(name, cap)
    plain, part = chain_yardstick(name, cap, values)
    assert not any(r.zero for r in plain)
    form = form_kind(name, cap // 4)
    print(f"KT form {T.case_id(case)}: {form}")
    assert form[0] == 2                                            # the filtered kernel (kSsFiltered)
    res = run_forms(d, T.FORMS, chain_mantissas(name, cap, values), plain, part, f"{T.case_id(case)} {values}")
    bad = [f"{n}: error / bound {float(r.max()):.3g}" for n, r in res if not bool((r <= 1.0).all())]
    assert not bad, bad


def test_the_filtered_kernel_is_reached_at_every_word_count():
    assert {(T.SHAPES[n].sorb - 1) // 64 + 1 for n, c in K.CHAIN_CASES if form_kind(n, c // 4)[0] == 2} == {1, 2, 3}


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_reduce_front_end_asks_the_chain_table(cplx):
    """energy.reduce_front with the fe2s2 chain table of 256 slots as the wave-function table: link <= -2 exactly for the records whose
    determinant is a key, with its position; the contraction against ss_exact.reduce_columns"""
    from pynqs_amd import energy

    name, cap = "fe2s2", 256
    c = T.RShape("fe2s2-chain256", name, 4, False, 0, "gap", cap // 4)
    s = T.SHAPES[name]
    h1, h2 = T.integrals(s.ints, s.sorb)
    x = _dev(T._onv(T.walkers(name)[T.reduce_rows(c)], s.sorb))
    eps, _ = T.reduce_eps(c)
    lut = _lut(K.chain_table(name, cap).bits, s.sorb)
    words = _sorted_words(lut)
    where = {w.tobytes(): i for i, w in enumerate(words)}
    energy._FRONTS.clear()
    fe, nu = energy.reduce_front(x, _dev(h1), _dev(h2), s.sorb, s.noA + s.noB, s.noA, s.noB, eps, 0, lut.hashtable, seed=17)
    walker, _, w, link, onv, drawn = fe.records()
    link_h = link.cpu().numpy().astype(np.int64)
    want = np.array([where.get(r.tobytes(), -1) for r in onv.cpu().numpy()], dtype=np.int64)
    assert int((want >= 0).sum()) >= 4 and int((want < 0).sum()) > 0
    np.testing.assert_array_equal(link_h <= -2, want >= 0)
    np.testing.assert_array_equal(-2 - link_h[want >= 0], want[want >= 0])
    g = np.random.default_rng(23)
    mant = g.random(nu + cap // 4) + 0.25
    mant = mant * np.exp(2j * np.pi * g.random(mant.size)) if cplx else mant * np.where(g.random(mant.size) < 0.5, -1.0, 1.0)
    all_bits = np.concatenate([T.bits_of(fe.uniq_onv[:nu].cpu().numpy(), s.sorb), _bits_of_words(words, s.sorb)])
    _, cols = T.reduce_reference(c, all_bits, walker.cpu().numpy(), T.bits_of(onv.cpu().numpy(), s.sorb), w.cpu().numpy(), drawn.cpu().numpy())
    vl = S.as_ld(mant)
    ref = [S.contract(cc.w, cc.dw, cc.wabs, np.where(cc.pos >= 0, vl[np.maximum(cc.pos, 0)], 0), vl[cc.pos[0]], cplx) for cc in cols]
    e, px = fe.contract(_dev(mant[:nu]), _dev(mant[nu:]))
    np.testing.assert_array_equal(px.cpu().numpy(), T.psi_array(ref, mant.dtype))
    ratio, _ = T.ratios(ref, e.cpu().numpy())
    line = T.report(f"KT contract fe2s2-chain256 {'complex' if cplx else 'real'}", ratio)
    assert ratio.size == 4 and bool((ratio <= 1.0).all()), line


# ---- the unfiltered hash kernel ------------------------------------------------------------------------------------------------------------
NOFILTER_CHAINS = [(n, c) for n in ("fe2s2", "s66", "s130") for c in (64, 256)]
NOFILTER_HALF = ["fe2s2", "s66", "s130"]


def test_unfiltered_hash_kernel_in_a_fresh_process():
    """PYNQS_FILTER_BITS=0 is read once per process: a child runs pynqs_eloc_sample_space_hash and _hash_flip without filters (it asserts
    form kind 1 itself) and prints its ratios; it is started once, and a child that dies or runs out of time fails the test"""
    env = dict(os.environ, PYNQS_FILTER_BITS="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ss_nofilter_worker.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(r.stdout[-6000:])
    want = {f"{n}-{t}-{v}-{f}" for n, t in [(n, f"chain{c}") for n, c in NOFILTER_CHAINS] + [(n, "half") for n in NOFILTER_HALF]
            for v in VALUES for f in ("hash", "hash-flip")}
    assert set(out["ratios"]) == want and out["kind"] == [1] * len(out["kind"]) and len(out["kind"]) == len(NOFILTER_CHAINS) + len(NOFILTER_HALF)
    bad = {k: v for k, v in out["ratios"].items() if not (len(v) >= 1 and all(0 <= r_ <= 1.0 for r_ in v))}
    assert not bad, bad


# ---- pynqs_unique_first ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(K.unique_rows()), ids=T.case_id)
def test_unique_first_on_rows_that_collide(case):
    from pynqs_amd import _native as N, public_function as pf

    rows, distinct = K.unique_rows()[case]
    n, L = rows.shape
    want = K.first_occurrence(rows)
    x = _dev(K.onv_of(rows))
    lib = N.lib()
    assert lib.pynqs_unique_workspace(n) == 1024 * 4 + 4 * n      # the table keeps its 1024 slots
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(2):
        ws = torch.empty(lib.pynqs_unique_workspace(n), dtype=torch.uint8, device="cuda")
        first = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        N.check(lib.pynqs_unique_first(x.data_ptr(), n, 64 * L, ws.data_ptr(), first.data_ptr(), st), "pynqs_unique_first")
        np.testing.assert_array_equal(first.cpu().numpy(), want)
        # the table itself: the slots the replica predicts, each holding the first row of its key
        tab = ws.cpu().numpy()[: 1024 * 4].view(np.int32)
        assert np.array_equal(tab >= 0, K.occupied_set(K.home_unique(distinct, 1023), 1024))
        assert np.array_equal(np.sort(tab[tab >= 0]), np.flatnonzero(want == np.arange(n)))
    u, inv = pf.unique_onv(x)
    order = np.flatnonzero(want == np.arange(n))                     # order of first appearance
    np.testing.assert_array_equal(u.cpu().numpy(), K.onv_of(rows[order]))
    assert torch.equal(u[inv], x)


# ---- the de-duplication table at its tightest ------------------------------------------------------------------------------------------------
LAYOUTS = ("list", "look-back", "list, no table")


@functools.lru_cache(maxsize=None)
def _reduce_inputs(name):
    from pynqs_amd import C_extension as cx

    c, x, comb, hm, uniq = K.reduce_case(name)
    h1, h2 = synth_integrals(c.sorb)
    h1e, h2e = _dev(h1), _dev(h2)
    xd = _dev(x)
    return c, xd, h1e, h2e, cx.plan_for(h1e, h2e, c.sorb, xd.device).buf


def _front(name, layout, cap_unique, N=0, seed=7):
    """a front end in the wanted form, as tests/test_gpu_contract_batched.py builds them, with the given capacity of the distinct list"""
    from pynqs_amd import _native as NA, reduce_front as RF

    c, x, h1e, h2e, plan = _reduce_inputs(name)
    ncomb = int(NA.lib().pynqs_num_sd(c.sorb, c.noA, c.noB)) + 1
    dedup = layout != "list, no table"
    cap_list = RF.list_capacity(c.n, c.sorb, c.noA + c.noB, c.noA, c.noB, N, torch.float64, without_table=not dedup)
    assert cap_list > 0
    cap_d = cap_list + 1 if layout == "look-back" else min(cap_list, ncomb)
    fe = RF.ReduceFrontEnd(c.n, c.sorb, c.noA + c.noB, c.noA, c.noB, N, torch.float64, x.device, cap_d, cap_unique, dedup=dedup)
    fe.run(x, plan, c.eps, seed, None)
    return fe, fe.counters_host()


def _table_occupied(fe):
    """bool [dedup_slots]: one-word slots hold the key in their first 64-bit word (empty: all ones), longer ones a state word (ready: 2)"""
    t = fe.table.cpu().numpy().reshape(fe.dedup_slots, fe.slot_i32)
    if fe.L == 1:
        return np.ascontiguousarray(t[:, :2]).view(np.int64)[:, 0] != -1
    assert bool(np.isin(t[:, 0], (-1, 2)).all())
    return t[:, 0] == 2


def _sorted_records(fe):
    walker, col, w, link, onv, drawn = fe.records()
    order = torch.argsort(walker * (1 << 32) + col.long(), stable=True)
    return walker[order], col[order], w[order], onv[order], drawn[order]


def _amp_of(onv):
    """an amplitude per DETERMINANT (the distinct list's order follows the atomics): in [0.5, 1.5), from the packed words"""
    w = onv.cpu().numpy().view(np.uint64).reshape(onv.size(0), -1)
    return _dev(0.5 + (K.hash_of(w) >> np.uint64(11)).astype(np.float64) / 2.0 ** 53)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["one-word", "two-words"])
def test_dedup_table_exactly_half_full(name, layout):
    """cap_unique = nu, the number of distinct kept determinants: dedup_slots = 2 nu, the fullest table the constructor allows (the rows of
    the distinct list are handed out in blocks of exactly what a workgroup inserted, reduce_common.h: no slack is needed).  The table-less
    form gives every record a row of its own: its capacity is the number of records."""
    from pynqs_amd import energy, reduce_front as RF
    from test_gpu_reduce_onepass import _check_distinct

    c, x, h1e, h2e, plan = _reduce_inputs(name)
    uniq = K.reduce_case(name)[4]
    nu = uniq.shape[0]
    energy._FRONTS.clear()
    roomy, nu_roomy = energy.reduce_front(x, h1e, h2e, c.sorb, c.noA + c.noB, c.noA, c.noB, c.eps, 0, None, seed=7)
    assert nu_roomy == nu and roomy.dedup_slots > 2 * nu
    rec_roomy = _sorted_records(roomy)
    nrec = rec_roomy[0].numel()
    dedup = layout != "list, no table"
    cap = nu if dedup else nrec
    fe, cnt = _front(name, layout, cap)
    assert fe.dedup == dedup and not fe.overflowed(cnt) and cnt[1] == 0 and cnt[0] == cap
    rec = _sorted_records(fe)
    for a, b in zip(rec, rec_roomy):
        assert torch.equal(a, b)                                      # the kept records, bit for bit those of the roomy run
    walker, col, w, link, onv, drawn = fe.records()
    if dedup:
        assert fe.dedup_slots == 2 * nu == K.pow2_at_least(2 * nu)
        _check_distinct(fe, nu, walker, onv, link, c.sorb)
        occ = _table_occupied(fe)
        want = K.occupied_set(K.home_dedup(uniq, fe.dedup_slots - 1), fe.dedup_slots)
        assert np.array_equal(occ, want), f"{int((occ != want).sum())} slots differ from the replica's occupied set"
        assert bool(occ[0] and occ[-1])
        print(f"KT dedup {name} {layout}: {nu} determinants in {fe.dedup_slots} slots, load {nu / fe.dedup_slots:.3f}")
    else:
        rows = fe.rows_of(link)
        assert int(rows.min()) >= 0 and int(rows.max()) < nrec and rows.unique().numel() == nrec and torch.equal(fe.uniq_onv[rows], onv)
    e_ok, _ = fe.contract(_amp_of(fe.uniq_onv[:cap]))
    assert bool(torch.isfinite(e_ok).all())
    # one row too few: the call says so, and the contraction poisons walkers instead of returning finite wrong energies
    small, cnt_s = _front(name, layout, cap - 1)
    assert small.dedup_slots == fe.dedup_slots if dedup else True
    assert small.overflowed(cnt_s) and cnt_s[1] & RF.OVERFLOW_UNIQUE and not cnt_s[1] & RF.OVERFLOW_TABLE
    e_bad, _ = small.contract(_amp_of(small.uniq_onv[: cap - 1]))
    fin = torch.isfinite(e_bad)
    assert not bool(fin.all())
    assert torch.equal(e_bad[fin].view(torch.int64), e_ok[fin].view(torch.int64))   # (same slots, same amplitude per determinant: same bits)


DRAW_SEED = 11   # selection data: with it the draws reach the load printed below (>= 0.35 asserted)


def test_dedup_table_filled_by_draws():
    """4000 draws per walker on the one-word shape (probe_k_oneword: four records' probes side by side), cap_unique = the number of distinct
    connected determinants of the walkers"""
    from test_gpu_reduce_onepass import _check_distinct

    name = "one-word-draws"
    c, x, h1e, h2e, plan = _reduce_inputs(name)
    comb, hm = K.reduce_case(name)[2:4]
    every = K.distinct_words(comb, np.ones(hm.shape, dtype=bool))
    cap = every.shape[0]
    fe, cnt = _front(name, "list", cap, N=K.DRAWS, seed=DRAW_SEED)
    nu = cnt[0]
    assert not fe.overflowed(cnt) and cnt[1] == 0 and fe.dedup_slots == K.pow2_at_least(2 * cap)
    load = nu / fe.dedup_slots
    print(f"KT dedup {name}: {nu} of {cap} determinants reached, {fe.dedup_slots} slots, load {load:.3f}")
    assert load >= 0.35
    walker, col, w, link, onv, drawn = fe.records()
    assert bool(drawn.any()) and bool((~drawn).any())
    _check_distinct(fe, nu, walker, onv, link, c.sorb)
    reached = fe.uniq_onv[:nu].cpu().numpy().view(np.uint64).reshape(nu, -1)
    assert np.array_equal(_table_occupied(fe), K.occupied_set(K.home_dedup(reached, fe.dedup_slots - 1), fe.dedup_slots))
    # the kept part is the |h| >= eps of the CPU oracle; every drawn record is a sub-eps column with its determinant
    wk, cl = walker.cpu().numpy(), col.cpu().numpy().astype(np.int64)
    dr = drawn.cpu().numpy()
    keep = np.abs(hm) >= c.eps
    got = np.zeros_like(keep)
    got[wk[~dr], cl[~dr]] = True
    assert np.array_equal(got, keep) and not keep[wk[dr], cl[dr]].any()
    np.testing.assert_array_equal(onv.cpu().numpy(), comb[wk, cl])


# ---- the block index on its longest equal-run ----------------------------------------------------------------------------------------------
BLOCK_CASES = [(56, 1), (184, 3)]   # (sorb, the block the keys differ in): bits [10, 22) of one word; bits [110, 146), across words 1 and 2
BLOCK_NO, BLOCK_KEYS, BLOCK_WALKERS = (3, 2), 200, 3


@functools.lru_cache(maxsize=None)
def block_keys(sorb, block):
    """200 distinct determinants of 3 alpha and 2 beta electrons that all live in one block of the index: one determinant, its single and double
    excitations inside the block in a seeded order, then (sorb 56 has only 104 of those) random determinants of the block"""
    import itertools

    from test_gpu_keys_index import NB

    lo, hi = 2 * ((block * (sorb // 2)) // NB), 2 * (((block + 1) * (sorb // 2)) // NB)
    g = np.random.default_rng(sorb + block)
    ns = (hi - lo) // 2
    base = np.zeros(sorb, dtype=np.uint8)
    base[lo + 2 * g.permutation(ns)[: BLOCK_NO[0]]] = 1
    base[lo + 2 * g.permutation(ns)[: BLOCK_NO[1]] + 1] = 1
    occ, emp = np.flatnonzero(base).tolist(), [o for o in range(lo, hi) if not base[o]]
    exc = []
    for k in (1, 2):
        for holes in itertools.combinations(occ, k):
            for parts in itertools.combinations(emp, k):
                if sorted(o & 1 for o in holes) == sorted(o & 1 for o in parts):   # spin is conserved
                    row = base.copy()
                    row[list(holes)] = 0
                    row[list(parts)] = 1
                    exc.append(row)
    exc = np.array(exc)[g.permutation(len(exc))]
    m = 4 * BLOCK_KEYS
    more = np.zeros((m, sorb), dtype=np.uint8)
    rows = np.arange(m)[:, None]
    more[rows, lo + 2 * np.argsort(g.random((m, ns)), axis=1)[:, : BLOCK_NO[0]]] = 1
    more[rows, lo + 2 * np.argsort(g.random((m, ns)), axis=1)[:, : BLOCK_NO[1]] + 1] = 1
    bits = np.concatenate([base[None, :], exc, more])
    bits = bits[np.sort(np.unique(K.words_of(bits), axis=0, return_index=True)[1])][:BLOCK_KEYS]
    assert bits.shape[0] == BLOCK_KEYS and not bits[:, :lo].any() and not bits[:, hi:].any()
    assert bool((bits[:, 0::2].sum(1) == BLOCK_NO[0]).all() and (bits[:, 1::2].sum(1) == BLOCK_NO[1]).all())
    return bits


@pytest.mark.parametrize("sorb,block", BLOCK_CASES)
def test_block_index_on_one_run_per_block(sorb, block):
    import eloc_exact as X
    from pynqs_amd import C_extension as cx, _native as N
    from test_gpu_keys_index import NB, TOL, _block_values

    bits = block_keys(sorb, block)
    nk = bits.shape[0]
    words = K.words_of(bits)
    keys = _dev(K.onv_of(words))
    ki = cx.keys_index_build(keys, sorb)
    raw = ki.index.cpu().numpy().view(np.uint8)
    svals = raw[: NB * nk * 8].view(np.uint64).reshape(NB, nk)
    perm = raw[NB * nk * 8: NB * nk * 12].view(np.uint32).reshape(NB, nk)
    single = 0
    for b in range(NB):
        v, _ = _block_values(words, sorb, b)
        order = np.argsort(v, kind="stable")
        np.testing.assert_array_equal(perm[b], order.astype(np.uint32))
        np.testing.assert_array_equal(svals[b], v[order] | np.uint64(b << 40))
        single += int(np.unique(v).size == 1)
        assert (np.unique(v).size == 1) == (b != block)
    assert single == 4                                # four blocks are one run of nk equal values
    # energies: the first walkers of the table, streamed and indexed, real and complex
    h1, h2 = synth_integrals(sorb)
    noA, noB = BLOCK_NO
    sts = [X.structure(row, h1, h2) for row in bits[:BLOCK_WALKERS]]
    tab = S.Table(bits)
    cols = [S.columns(st, tab) for st in sts]
    x = keys[:BLOCK_WALKERS].contiguous()
    plan = cx.plan_for(_dev(h1), _dev(h2), sorb, x.device)
    st = torch.cuda.current_stream().cuda_stream
    g = np.random.default_rng(5)
    for cplx in (False, True):
        mant = g.random(nk) + 0.25
        mant = mant * np.exp(2j * np.pi * g.random(nk)) if cplx else mant * np.where(g.random(nk) < 0.5, -1.0, 1.0)
        ref = [S.table_sum(c, S.as_ld(mant)) for c in cols]
        wd = _dev(mant)
        out = {}
        for form in ("streamed", "indexed"):
            e, p0 = torch.full_like(wd[:BLOCK_WALKERS], 7.0), torch.full_like(wd[:BLOCK_WALKERS], 7.0)
            args = (x.data_ptr(), BLOCK_WALKERS, sorb, noA + noB, noA, noB, plan.data_ptr(), keys.data_ptr(), nk)
            if form == "streamed":
                rc = N.lib().pynqs_eloc_sample_space_keys(*args, wd.data_ptr(), int(cplx), 0, e.data_ptr(), p0.data_ptr(), st)
            else:
                rc = N.lib().pynqs_eloc_sample_space_indexed(*args, ki.index.data_ptr(), wd.data_ptr(), int(cplx), 0, e.data_ptr(), p0.data_ptr(), st)
            N.check(rc, form)
            out[form] = e.cpu().numpy()
            np.testing.assert_array_equal(p0.cpu().numpy(), T.psi_array(ref, mant.dtype), err_msg=form)
            ratio, _ = T.ratios(ref, out[form])
            line = T.report(f"KT block index sorb {sorb} {form} {'complex' if cplx else 'real'}", ratio)
            assert ratio.size == BLOCK_WALKERS and bool((ratio <= 1.0).all()), line
        np.testing.assert_allclose(out["indexed"], out["streamed"], rtol=0, atol=TOL)
