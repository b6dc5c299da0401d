"""The determinant kernels from 16 to 129 electrons, on one, two and three ONV words (tests/many_electron_cases.py), against the CPU oracle
bit for bit, with float64 and float32 integrals.  The oracle itself is held to the reference up to 40 electrons
(tests/golden/many_electron.npz) and to longdouble Slater-Condon rules on every shape here (tests/test_many_electron_cases.py).

  * get_comb_hij_fused, plan kernels and direct kernels: singles_tile's lane groups, passes and its gather past lane 63, the rounds of
    diag_wave and diag_phase, rows of one column, a row cut inside its singles;
  * the Hmat-only plan route (get_comb_tensor, then get_hij_torch on that very list) and the generic pair kernel in 3-D mode on a copy;
  * the generic pair kernel in 2-D mode with a wave full of diagonal pairs (diag_by_wave's rounds of 512 terms, its zero-filled
    occupation list when nele exceeds the determinants' electrons, clamped lanes in the last block), and exact zeros;
  * the REDUCE compaction (pynqs_reduce_count / _emit) and the one-launch front end against the thresholded oracle row.

(136,65,64) has 129 electrons, past PYNQS_MAX_NELE = 120, which only pynqs_check_sorb enforces: the kernels are held to the oracle there
too ("Beyond 30 electrons")."""
import functools
import hashlib

import numpy as np
import pytest
import torch

import many_electron_cases as M
from conftest import golden

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
LONG_ROW = 100_000     # columns from which the generic pair kernel sees a sample of the row
NDETS = 130            # 130 x 130 pairs: 66.02 blocks of 256


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def host_integrals(sorb: int):
    """{dtype: (h1e, h2e)}, built once per sorb (168e6 numbers at sorb 192)"""
    h1, h2 = M.integrals(sorb)
    return {dt: (h1.astype(dt), h2.astype(dt)) for dt in DTYPES}


@functools.lru_cache(maxsize=None)
def device_integrals(sorb: int):
    return {dt: (G(h1), G(h2)) for dt, (h1, h2) in host_integrals(sorb).items()}


@functools.lru_cache(maxsize=None)
def reference(case):
    """(onv uint8 [n, 8 len], {dtype: (comb, Hmat) of the oracle}); computed once per case, shared by the tests and left unchanged"""
    from oracle import oracle as O

    onv = O.pm01_to_onv(M.occupations(case), case.sorb)
    out = {dt: O.comb_hij_fused(onv, h1, h2, case.sorb, case.noA + case.noB, case.noA, case.noB) for dt, (h1, h2) in host_integrals(case.sorb).items()}
    for c, h in out.values():
        c.setflags(write=False)
        h.setflags(write=False)
    return onv, out


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for f in (reference, device_integrals, host_integrals, M.integrals):
        f.cache_clear()
    from pynqs_amd import energy

    energy.reset_caches()
    torch.cuda.empty_cache()


@pytest.fixture
def cx():
    from pynqs_amd import C_extension as m
    from pynqs_amd import _native

    _native.lib()  # fail loudly if the HIP library is missing
    assert torch.cuda.is_available()
    old = m.USE_PLAN
    yield m
    m.USE_PLAN = old


def system(c):
    return c.sorb, c.noA + c.noB, c.noA, c.noB


@pytest.mark.parametrize("route", ["plan", "direct"])
@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_fused_enumeration_and_matrix_elements(cx, case, route):
    cx.USE_PLAN = route == "plan"
    onv, ref = reference(case)
    x = G(onv)
    for dt in DTYPES:
        h1, h2 = device_integrals(case.sorb)[dt]
        comb, hm = cx.get_comb_hij_fused(x, h1, h2, *system(case))
        co, ho = ref[dt]
        assert hm.dtype == h1.dtype and np.array_equal(comb.cpu().numpy(), co), (route, dt)
        got = hm.cpu().numpy()
        bad = np.flatnonzero((got.view(np.uint8).reshape(got.shape + (-1,)) != ho.view(np.uint8).reshape(ho.shape + (-1,))).any(-1).reshape(-1))
        assert bad.size == 0, f"{route} {np.dtype(dt).name}: {bad.size} of {got.size} elements differ from the oracle, first at flat index {bad[:8].tolist()}"
    if case in M.GOLDEN:
        d, key = golden("many_electron.npz"), M.case_id(case)
        assert np.array_equal(onv, d[key + "_onv"])
        ranks = d[key + "_ranks"]
        for dt, tag in ((np.float64, "_hmat"), (np.float32, "_hmat_f32")):
            h1, h2 = device_integrals(case.sorb)[dt]
            comb, hm = cx.get_comb_hij_fused(x, h1, h2, *system(case))
            c, h = comb.cpu().numpy(), hm.cpu().numpy()
            assert [sha(r) for r in c] == d[key + "_comb_sha"].tolist() and [sha(r) for r in h] == d[key + tag + "_sha"].tolist(), (route, tag)
            assert np.array_equal(c[:, ranks], d[key + "_comb"]) and np.array_equal(h[:, ranks], d[key + tag]), (route, tag)


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_hmat_only_plan_route_and_generic_pairs_in_3d(cx, case):
    """get_comb_tensor(x), then get_hij_torch(x, comb): that pair of tensors is answered by the plan kernel in its Hmat-only form; a copy
    of the list goes through the generic pair kernel, a whole wave per diagonal pair.  Rows of more than 1e5 columns give the generic
    kernel 4096 of their columns (many_electron_cases.column_sample)."""
    sorb, nele, noA, noB = system(case)
    onv, ref = reference(case)
    x = G(onv)
    long_row = M.ncomb(case) > LONG_ROW
    cols = M.column_sample(case) if long_row else None
    for dt in DTYPES:
        h1, h2 = device_integrals(sorb)[dt]
        co, ho = ref[dt]
        comb, _ = cx.get_comb_tensor(x, sorb, nele, noA, noB)
        assert np.array_equal(comb.cpu().numpy(), co)
        assert cx._is_last_comb(x, comb, sorb, nele) == (noA, noB)
        fast = cx.get_hij_torch(x, comb, h1, h2, sorb, nele)
        assert fast.dtype == h1.dtype and np.array_equal(fast.cpu().numpy().view(np.uint8), ho.view(np.uint8)), dt
        copy = comb[:, G(cols)].contiguous() if long_row else comb.clone()
        assert cx._is_last_comb(x, copy, sorb, nele) is None
        slow = cx.get_hij_torch(x, copy, h1, h2, sorb, nele).cpu().numpy()
        want = np.ascontiguousarray(ho[:, cols]) if long_row else ho
        assert np.array_equal(slow.view(np.uint8), want.view(np.uint8)), dt


def determinants(case) -> np.ndarray:
    """NDETS packed determinants from the first row of comb: the first 64 columns -- a wave of consecutive kets, so that the 64 lanes of a
    wave of the 2-D call hold many diagonal pairs in turn -- and seeded others; distinct.  Rows shorter than that repeat their columns:
    then every pair of equal determinants is one more diagonal lane."""
    _, ref = reference(case)
    row = ref[np.float64][0][0]
    n = row.shape[0]
    if n < NDETS:
        return np.ascontiguousarray(row[np.arange(NDETS) % n])
    g = np.random.default_rng(n)
    idx = np.concatenate([np.arange(64), 64 + np.sort(g.choice(n - 64, NDETS - 64, replace=False))])
    dets = np.ascontiguousarray(row[idx])
    assert len({r.tobytes() for r in dets}) == NDETS
    return dets


def far_kets(case, dets: np.ndarray) -> np.ndarray:
    """kets that no rule connects to dets[0]: 3 and 4 orbitals moved, one and two electrons removed, one added (whatever the
    determinant has room for)"""
    from oracle import oracle as O

    bits = M.bits_of(dets[:1], case.sorb)[0]
    occ, emp = np.flatnonzero(bits == 1), np.flatnonzero(bits == 0)
    rows = []
    for k in (3, 4):
        if occ.size >= k and emp.size >= k:
            b = bits.copy(); b[occ[:k]] = 0; b[emp[-k:]] = 1; rows.append(b)
    for k in (1, 2):
        b = bits.copy(); b[occ[-k:]] = 0; rows.append(b)
    if emp.size:
        b = bits.copy(); b[emp[0]] = 1; rows.append(b)
    return O.pm01_to_onv(np.stack(rows), case.sorb)


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_generic_pairs_in_2d_with_many_diagonal_lanes(cx, case):
    from oracle import oracle as O

    sorb, nele, _, _ = system(case)
    dets = determinants(case)
    far = far_kets(case, dets)
    assert (NDETS * NDETS) % 256 != 0
    d = G(dets)
    for dt in DTYPES:
        h1, h2 = host_integrals(sorb)[dt]
        g1, g2 = device_integrals(sorb)[dt]
        for ne in (nele, nele + 2):   # nele + 2: entries of the occupation list past the determinant's electrons read as orbital 0
            want = O.hij(dets, dets, h1, h2, sorb, ne)
            got = cx.get_hij_torch(d, d, g1, g2, sorb, ne).cpu().numpy()
            assert got.shape == (NDETS, NDETS) and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (dt, ne)
        zero = cx.get_hij_torch(d, G(far), g1, g2, sorb, nele).cpu().numpy()
        assert zero.shape == (NDETS, far.shape[0]) and not zero[0].any() and np.array_equal(zero, O.hij(dets, far, h1, h2, sorb, nele)), dt


def eps_in_largest_gap(h: np.ndarray, lo: float = 0.25, hi: float = 0.75) -> float:
    """the middle of the largest gap between consecutive |h| of the rows h [n, ncomb], among the gaps that begin between the quantiles lo
    and hi of the |h| not above the smallest |<x|H|x>| -- ss_exact.eps_in_largest_gap on the oracle's row, in the row's own type, so
    that the comparison |h| >= eps is the same in the kernel and here"""
    v = np.sort(np.abs(h).reshape(-1))
    v = v[v <= np.abs(h[:, 0]).min()]
    if v.size < 8:
        return float(v[0] / 2)   # (a row of one column: <x|H|x> is kept)
    i0, i1 = int(lo * v.size), int(hi * v.size)
    i = i0 + int(np.argmax(np.diff(v[i0:i1 + 1])))
    eps = ((v[i].astype(np.float64) + v[i + 1].astype(np.float64)) / 2).astype(h.dtype)
    assert v[i] < eps < v[i + 1], (v[i], eps, v[i + 1])
    return float(eps)


def kept(case, dt):
    """(eps, row, col, h, onv) of the oracle's columns with |h| >= eps, rows and columns ascending"""
    _, ref = reference(case)
    co, ho = ref[dt]
    eps = eps_in_largest_gap(ho)
    row, col = np.nonzero(np.abs(ho) >= ho.dtype.type(eps))
    assert (col == 0).sum() == ho.shape[0]
    return eps, row, col, ho[row, col], co[row, col]


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_reduce_compaction_keeps_the_oracles_columns(cx, case):
    from pynqs_amd import energy

    onv, _ = reference(case)
    x = G(onv)
    for dt in DTYPES:
        h1, h2 = device_integrals(case.sorb)[dt]
        eps, wrow, wcol, wh, wonv = kept(case, dt)
        row, col, kets, h, counts = energy.reduce_compact(x, h1, h2, *system(case), eps, sort=True)
        assert np.array_equal(row.cpu().numpy(), wrow) and np.array_equal(col.cpu().numpy(), wcol), dt
        assert h.dtype == h1.dtype and np.array_equal(h.cpu().numpy().view(np.uint8), wh.view(np.uint8)) and np.array_equal(kets.cpu().numpy(), wonv), dt
        assert counts.cpu().numpy().tolist() == np.bincount(wrow, minlength=onv.shape[0]).tolist()
        if M.ncomb(case) > 8:   # some columns are kept, some are not
            assert 0.2 < wh.size / (M.ncomb(case) * onv.shape[0]) < 0.8


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_reduce_front_end_writes_the_oracles_columns(cx, case):
    """The one-launch front end on the same threshold: its LIST forms stage the singles and the diagonal in 256 elements per wave, half
    of what every other caller of singles_tile and diag_wave has."""
    from pynqs_amd import energy, reduce_front as RF

    onv, _ = reference(case)
    x = G(onv)
    sorb, nele, noA, noB = system(case)
    assert RF.supported(onv.shape[0], sorb, nele, noA, noB, 0)
    for dt in DTYPES:
        h1, h2 = device_integrals(sorb)[dt]
        eps, wrow, wcol, wh, wonv = kept(case, dt)
        energy.reset_caches()
        fe, nu = energy.reduce_front(x, h1, h2, sorb, nele, noA, noB, eps, want_pm1=False)
        w, col, h, link, kets, _ = fe.records()
        order = torch.argsort((w.long() << 32) | col.long(), stable=True)
        assert np.array_equal(w[order].cpu().numpy(), wrow) and np.array_equal(col[order].cpu().numpy(), wcol), dt
        assert np.array_equal(h[order].cpu().numpy().view(np.uint8), wh.view(np.uint8)) and np.array_equal(kets[order].cpu().numpy(), wonv), dt
        assert torch.equal(fe.uniq_onv[fe.rows_of(link)], kets)
        distinct = {r.tobytes() for r in wonv}
        assert {r.tobytes() for r in fe.uniq_onv[:nu].cpu().numpy()} == distinct
        # every x' once -- but for the full shell of 64 orbitals: its one word, all ones, is the empty mark of the one-word
        # de-duplication table (reduce_common.h), so each of its walkers (it has no other record) takes a row of its own
        assert nu == len(distinct) or (sorb == 64 and nele == 64 and nu == onv.shape[0])
    energy.reset_caches()
