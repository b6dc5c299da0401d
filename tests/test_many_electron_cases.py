"""The case list of tests/many_electron_cases.py and the oracle it is compared with, on the CPU.

  * the list reaches every regime of the determinant kernels that an ONV word count allows (test_the_list_reaches_every_regime; the
    table is printed with -s);
  * oracle.comb_hij_fused and oracle.hij, float64, against eloc_exact.structure on every case: plain Slater-Condon in longdouble that
    shares no code with the oracle.  Columns are matched by the determinant's bits, never by position, and the match must be a
    bijection.  The bound is a priori: a matrix element is a sum of t_k stored numbers of moduli adding up to a_k, so in any order
        |h_oracle - h_k| <= t_k 2^-53 a_k                                       (the diagonal: t_0, a_0),
    and a double, one stored number, must come out exactly.  Above 40 electrons the reference as shipped does not run, so this is the
    only independent check the oracle has there (up to 40: tests/test_oracle_golden.py::test_many_electron_shapes).
    structure() walks every excitation in plain Python, 12 s for the 1 001 984 of (192,32,0): rows of more than 1e5 columns are checked
    on their first walker only -- that cuts (130,9,8) from 2 walkers to 1; every other long row has one walker anyway.  No shape gives
    up electrons."""
import numpy as np
import pytest

import eloc_exact as X
import many_electron_cases as M

U = 2.0 ** -53


def test_the_list_reaches_every_regime():
    reg = {c: M.regime(c) for c in M.CASES}
    print()
    print(f"{'case':>14} {'n':>2} " + " ".join(f"{f:>9}" for f in M.Regime._fields))
    for c, r in reg.items():
        print(f"{M.case_id(c):>14} {c.n:>2} " + " ".join(f"{str(v):>9}" for v in r))
    assert len(set(M.CASES)) == len(M.CASES)
    for words in (1, 2, 3):
        rs = [r for r in reg.values() if r.words == words]
        singles = [r for r, c in ((reg[c], c) for c in M.CASES) if r.words == words and r.passes512 > 0]   # rows that have singles at all
        have = lambda pred, rows=rs: any(pred(r) for r in rows)  # noqa: E731
        # lane groups of singles_tile: G = 16, 32, 64; one word holds at most 64 electrons, and those fill it (a row of one column)
        assert have(lambda r: r.nele <= 16 and r.G == 16, singles) and have(lambda r: 17 <= r.nele <= 32 and r.G == 32, singles)
        assert have(lambda r: 33 <= r.nele <= 64 and r.G == 64 and not r.gather, singles)
        if words > 1:
            assert have(lambda r: r.gather, singles), words
        # singles per pass.  Three passes at QUARTER 512 take cap <= 7, that is 64 electrons or more: a one-word row of 64 electrons has
        # no singles, so one word reaches three passes only in the QUARTER 256 form
        assert have(lambda r: r.cap512 == 16, singles) and have(lambda r: r.cap512 < 16 and r.passes256 >= 3, singles)
        if words > 1:
            assert have(lambda r: r.cap512 < 16 and r.passes512 >= 3, singles)
            assert have(lambda r: r.cap256 <= 2, singles)   # (85 electrons or more)
        # rounds of the diagonal: 512 terms (diag_wave, diag_by_wave), 2048 terms (diag_phase)
        assert have(lambda r: r.wave >= 2 and r.hij >= 2) and have(lambda r: r.wave >= 5 and r.hij >= 5) and have(lambda r: r.phase >= 2)
        assert have(lambda r: r.ncomb == 1)
        assert have(lambda r: r.empty_same) and have(lambda r: r.empty_opp)
        # a cut inside the singles takes d1 >= 2048 singles: K <= 32 spatial orbitals give at most 512; K <= 64 give 2048 only at
        # (128,32,32), a row of 1 542 657 columns that structure() would walk for 20 s -- left to the three-word (192,32,0)
        if words == 3:
            assert have(lambda r: r.cut)
    # the declared limit and one shape past it
    assert any(r.nele == M.MAX_NELE for r in reg.values()) and any(r.nele > M.MAX_NELE and r.ncomb > 1 for r in reg.values())
    assert all(r.ncomb < 1 << 24 for r in reg.values())


def test_plan_chunks_cuts_the_long_row_at_its_last_single():
    c = M.Case(192, 32, 0, 1)
    assert M.plan_chunks(c.n, M.ncomb(c)) == (490, 2048) and M.classes(c)[:2] == (2048, 0) and M.cut_inside_singles(c)
    assert M.plan_chunks(64, 7876) == (4, 2048) and M.plan_chunks(4096, 7876) == (1, 7936) and M.plan_chunks(3, 190) == (1, 256)
    assert [M.cap(n) for n in (16, 31, 32, 64, 120, 129)] == [16, 16, 15, 7, 4, 3]
    assert [M.cap(n, M.QUARTER_LIST) for n in (32, 64, 120, 129)] == [7, 3, 2, 1]
    assert [M.rounds(n, 512) for n in (31, 32, 64, 120)] == [1, 2, 5, 15] and [M.rounds(n, 2048) for n in (63, 64)] == [1, 2]


_WORST = {}


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_oracle_meets_the_longdouble_slater_condon_rules(case):
    from oracle import oracle as O

    c, nele = case, case.noA + case.noB
    h1, h2 = M.integrals(c.sorb)
    occ = M.occupations(c)
    if M.ncomb(c) > 100_000:
        occ = occ[:1]
    onv = O.pm01_to_onv(occ, c.sorb)
    comb, hm = O.comb_hij_fused(onv, h1, h2, c.sorb, nele, c.noA, c.noB)
    assert comb.shape[:2] == (occ.shape[0], M.ncomb(c)) and bool(np.isfinite(hm).all())
    hp = O.hij(onv, comb, h1, h2, c.sorb, nele)
    worst = 0.0
    for i in range(occ.shape[0]):
        st = X.structure(occ[i], h1, h2)
        bits = M.bits_of(comb[i], c.sorb)
        assert np.array_equal(bits[0], occ[i]) and st.bits.shape[0] == M.ncomb(c) - 1
        index = {row.tobytes(): k for k, row in enumerate(st.bits)}
        assert len(index) == st.bits.shape[0]
        perm = np.array([index[row.tobytes()] for row in bits[1:]], dtype=np.int64)   # (a KeyError: a column that is no excitation of x)
        assert np.array_equal(np.sort(perm), np.arange(st.bits.shape[0]))          # a bijection
        want = np.concatenate([[st.h0], st.h[perm]])
        bound = U * np.concatenate([[st.t0 * st.a0], (st.t * st.a)[perm]])
        assert st.t0 == nele * (nele + 1) // 2 and set(np.unique(st.t).tolist()) <= {1, nele}
        for what, got in (("comb_hij_fused", hm[i]), ("hij", hp[i])):
            err = np.abs(got.astype(X.LD) - want).astype(np.float64)
            assert bool((err[bound == 0] == 0).all()) and bool((err[1:][st.t[perm] == 1] == 0).all()), (M.case_id(c), what)   # doubles: exact
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)
            k = int(np.argmax(ratio))
            worst = max(worst, float(ratio[k]))
            assert ratio[k] <= 1.0, f"{M.case_id(c)} walker {i} {what}: column {k} is off by {err[k]:.3g}, bound {bound[k]:.3g}"
    _WORST[M.case_id(c)] = worst
    print(f"\n{M.case_id(c)}: {occ.shape[0]} walker(s) x {M.ncomb(c)} columns, worst |oracle - longdouble| / bound {worst:.3g}")


def test_zz_worst_ratio_per_case():
    print()
    for k, v in _WORST.items():
        print(f"{k:>14}: {v:.3g}")
    assert _WORST and max(_WORST.values()) <= 1.0
