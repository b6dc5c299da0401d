"""The yardstick of the GFMC move (tests/gfmc_exact.py) on the CPU: the law accepts the exact and the sequential answer (gfmc.sample_update
on CPU tensors: torch cumsum + searchsorted) for every case and every uniform, the boundary cases are not vacuous, and the whole set of
references stays cheap.  tests/test_gpu_gfmc_exact.py holds the kernel to the same law."""
import time

import numpy as np
import pytest
import torch

import gfmc_exact as GX

_SPENT = [0.0]  # seconds in the tests of this file (the last one caps it)


@pytest.fixture(autouse=True)
def _clock():
    t0 = time.time()
    yield
    _SPENT[0] += time.time() - t0


def test_the_five_column_counterexample_admits_columns_2_and_4_and_never_3():
    """[2^-53, 2^-53, 1, 0, 1] with u = 0.5 + 2^-53 (gfmc_exact.COUNTEREXAMPLE): the sequential float64 answer is 2 (torch on the CPU gives it
    too); in exact arithmetic S = 2 + 2^-52 is no double and u S lies 2^-53 S above C_2 = C_3, so the first column to reach it is 4.
    Both are within tau; the zero-weight column 3, which the bracket alone admits, is not acceptable."""
    g, u, sequential, exact = GX.COUNTEREXAMPLE
    r = GX.Row(g)
    assert (sequential, exact) == (2, 4) and GX.exact_index(r, u) == exact
    cum, k = 0.0, None
    for j, v in enumerate(g.tolist()):  # the sequential answer in plain float64
        cum += v
        if k is None and cum >= u * float(g.sum()):
            k = j
    assert k == sequential and float(g.sum()) == 2.0 and u * 2.0 == 1.0 + 2.0 ** -52
    assert r.C[2] == r.C[3] and g[3] == 0  # the bracket of column 3 is that of column 2
    assert [j for j in range(5) if GX.accepts(r, u, j)] == [2, 4]
    assert GX.nearest_boundary(r, u) == 2 and GX.zero_follows(r, 2)
    index, _ = _sequential(GX.Block(r, np.array([u])))
    assert index.tolist() == [sequential]


def test_the_law_on_rows_small_enough_to_enumerate():
    """interior uniforms leave exactly one column, the exact one; a zero-weight column k >= 1 is never acceptable; S = 0 gives 0 alone"""
    rng = np.random.default_rng(3)
    for m in (1, 2, 5, 17):
        for fam in ("dense", "zeros60", "g0-zero", "ladder", "wide", "all-zero"):
            if not GX.applies(fam, m):
                continue
            r = GX.Row(GX.make_row(fam, m, rng))
            for u in np.concatenate([rng.random(20), GX.boundary_uniforms(r), [0.0, GX.ONE_BELOW]]).tolist():
                ok = [k for k in range(m) if GX.accepts(r, u, k)]
                k = GX.exact_index(r, u)
                assert k in ok, (fam, m, u, k, ok)
                assert all(r.g[j] > 0 or j == 0 for j in ok)
                if r.S == 0:
                    assert ok == [0]
                elif min(abs(u - c / r.S) for c in [0] + r.C) > 4 * m * 2.0 ** -52:  # farther than tau from every C_j (twice over)
                    assert ok == [k], (fam, m, u, k, ok)
            assert not GX.accepts(r, 0.5, m) and not GX.accepts(r, 0.5, -1)


def test_beta_bound_is_decided_exactly():
    r = GX.Row(np.array([1.0, 2.0 ** -53, 2.0 ** -53]))  # S = 1 + 2^-52, bound 2 * 2^-53 S
    assert GX.beta_check(r, 1.0 + 2.0 ** -52) == (True, 0.0)
    assert GX.beta_check(r, 1.0)[0] and GX.beta_check(r, 1.0 + 2.0 ** -51)[0]
    assert not GX.beta_check(r, 1.0 + 2.0 ** -50)[0] and not GX.beta_check(r, float("nan"))[0]
    assert GX.beta_check(GX.Row(np.zeros(4)), 0.0) == (True, 0.0) and not GX.beta_check(GX.Row(np.zeros(4)), 1e-300)[0]
    assert GX.beta_check(GX.Row(np.array([3.0])), 3.0)[0] and not GX.beta_check(GX.Row(np.array([3.0])), np.nextafter(3.0, 4.0))[0]


def _sequential(block):
    """gfmc.sample_update on CPU tensors for the block's row replicated over its uniforms: (index, beta)"""
    from pynqs_amd import gfmc

    r, u = block
    n = u.size
    gk = torch.from_numpy(r.g).unsqueeze(0).expand(n, r.m)
    comb = torch.arange(r.m, dtype=torch.int64).unsqueeze(1).contiguous().view(torch.uint8).unsqueeze(0).expand(n, r.m, 8)
    w = torch.ones(n, dtype=torch.float64)
    x_new, w_new, beta, acc = gfmc.sample_update(None, w, comb, gk, torch.from_numpy(u).reshape(n, 1))
    index = x_new.contiguous().view(torch.int64).reshape(n)
    assert acc == int((index != 0).sum()) and torch.equal(w_new, beta.reshape(n))
    return index.numpy(), beta.reshape(n).numpy()


@pytest.mark.parametrize("m", GX.WIDTHS)
def test_the_sequential_answer_obeys_the_law(m):
    """every case of the width, every row, every uniform (none is left out: the count is asserted), the all-zero row included"""
    checked = total = 0
    for c in GX.cases_of(m):
        for b in GX.blocks(c):
            total += b.u.size
            index, beta = _sequential(b)
            bad = GX.check_moves(b.row, b.u, index)
            assert not bad, (GX.case_id(c), len(bad), bad[:5])
            ok, ratio = GX.beta_check(b.row, float(beta[0]))
            assert ok and bool((beta == beta[0]).all()), (GX.case_id(c), ratio)
            checked += index.size
    assert checked == total > 0


def test_boundary_cases_are_not_vacuous():
    """per boundary case: at least 1000 uniforms within 2^-52 S of some C_j, at least 200 of them on a column that a zero-weight column
    follows; the families and widths of the cases; every long width has a boundary uniform too"""
    seen = set()
    for c in GX.CASES:
        near = zero = n = 0
        for b in GX.blocks(c):
            a, z = GX.count_boundary(b.row, b.u)
            near, zero, n = near + a, zero + z, n + b.u.size
            assert b.u.size <= 1024 and (0.0 in b.u.tolist()) == c.u0
        if GX.is_boundary(c):
            print(f"{GX.case_id(c)}: {len(GX.blocks(c))} rows, {n} uniforms, {near} on a boundary, {zero} next to a zero-weight column")
            assert near >= GX.NEAR_MIN and zero >= GX.ZERO_MIN, (GX.case_id(c), near, zero)
            seen.add(c.family)
        elif c.m > GX.LONG and c.family != "all-zero":
            assert n == 8 and near >= 2, (GX.case_id(c), near)
    assert seen == set(GX.BOUNDARY_FAMILIES)
    assert {c.m for c in GX.CASES} == set(GX.WIDTHS) and {c.family for c in GX.CASES} == set(GX.FAMILIES)
    assert any(c.family == "g0-zero" and not c.u0 for c in GX.CASES)
    # the ladders sit at every offset of LADDER_AT over the rows of a case (a row draws one of each overlapping group)
    at = set()
    for b in GX.blocks(GX.Case("ladder", 513, True)):
        at |= {s for s in range(510) if tuple(b.row.g[s:s + 4]) == GX.LADDER}
    assert len(GX.blocks(GX.Case("ladder", 513, True))) >= 8
    assert any(s in (61, 62, 63) for s in at) and any(s in (253, 254, 255) for s in at) and any(s <= 3 for s in at) and any(s >= 508 for s in at), at
    assert at <= set(GX.LADDER_AT)
    # tile-zeros: the first column with weight lies in tile >= 1
    for m in (257, 513, 7877):
        g = GX.make_row("tile-zeros", m, np.random.default_rng(m))
        assert not g[:256].any() and g.any()


def test_zz_the_references_stay_cheap():
    dt = _SPENT[0]
    print(f"tests/test_gfmc_exact.py: {dt:.1f} s")
    assert dt < 60.0
