"""The committed cases of tests/reduce_hier_cases.py on the CPU: the rows meet the conditions the GPU test relies on (coverage of every
column, the pooled-cell cap, lone columns of every kind, the neighbour pair), the case table agrees with the host plan
(reduce_front.plan needs no GPU), and the yardstick refuses every mutant of a hierarchical sampler while it passes the sampler itself."""
import numpy as np
import pytest
import torch

import reduce_hier_cases as HC
import reduce_replay as RR


def _drawable(r):
    return r.sub > 0


def test_family_a_reaches_every_column_and_stays_under_the_pooled_cap():
    """Over all (walker, set) pairs every one of the 1425 columns is drawable at least once and kept at least once -- so every tile edge of
    every form is the first and the last positive width of some draw, whatever its tile size -- every walker has a drawable column, whole
    tiles are empty at the start, in the middle and at the end of rows, and at N = 300 no walker has more than 15 % of its probability in
    the pooled cell."""
    fam = HC.FAMILY_BY_NAME["A"]
    drawable, kept = np.zeros(1425, bool), np.zeros(1425, bool)
    after12, stretch = None, (0, 1425, 0)
    for k, b in enumerate(fam.batches):
        r = HC.rows(b)
        assert r.hm.shape == (1024, 1425) and r.hm.dtype == np.float64
        d, keep = _drawable(r), r.keep
        nd = d.sum(1)
        assert int(nd.min()) >= 1 and 1 <= int(nd.max()) <= 32 and 10 <= float(np.median(nd)) <= 16
        assert bool(((r.hm == 0).sum(1) > 1300).all())                      # every other column an exact zero
        p = r.law
        pooled = np.where(fam.N * p < 5, p, 0.0).sum(1)
        assert float(pooled.max()) <= HC.POOLED_CAP, (b.name, float(pooled.max()))
        # empty stretches before the first, behind the last and between two drawable columns of some walker: a whole tile at the start of the
        # row, two tiles' length (a whole tile of any alignment) at its end and in its middle
        first, last = d.argmax(1), 1424 - d[:, ::-1].argmax(1)
        gap = max(int(np.diff(np.flatnonzero(row)).max(initial=0)) for row in d)
        stretch = (max(stretch[0], int(first.max())), min(stretch[1], int(last.min())), max(stretch[2], gap))
        drawable |= d.any(0)
        kept |= keep.any(0)
        print(f"{b.name}: drawable columns per walker {nd.min()} .. {nd.max()} (median {np.median(nd):.0f}), kept median {np.median(keep.sum(1)):.0f}, "
              f"pooled cell at most {pooled.max():.3f} (mean {pooled.mean():.3f}); so far {drawable.sum()} columns drawable, {kept.sum()} kept")
        if k == 11:
            after12 = (int(drawable.sum()), int(kept.sum()))
    assert after12 == (1420, 1424)      # (why there are more than twelve sets)
    assert bool(drawable.all()) and bool(kept.all())
    assert stretch[0] >= HC.TILE and stretch[1] < 1425 - 2 * HC.TILE and stretch[2] > 2 * HC.TILE, stretch


def test_family_b_keeps_nothing():
    for b in HC.FAMILY_BY_NAME["B"].batches:
        r = HC.rows(b)
        assert not bool(r.keep.any()) and np.array_equal(_drawable(r), r.hm != 0) and bool((r.hm[:, 0] != 0).any())


def test_family_c_has_lone_columns_of_every_kind():
    """eps between the two smallest distinct |H| of the batch: the walkers that hold the minimum have exactly one drawable column, every
    other walker none; over the sets the lone column is the diagonal, a single, a double and the row's last column."""
    kinds, counts = set(), []
    for b in HC.FAMILY_BY_NAME["C"].batches:
        r = HC.rows(b)
        d = _drawable(r)
        nd = d.sum(1)
        assert set(np.unique(nd)) == {0, 1}
        w, c = np.nonzero(d)
        assert np.unique(np.abs(r.hm[w, c])).size == 1
        flipped = np.unpackbits(r.kets[w, c] ^ r.x[w], axis=1).sum(1)     # 0: the diagonal, 2: a single, 4: a double excitation
        kinds |= {int(f) for f in flipped}
        assert bool(((flipped == 0) == (c == 0)).all())
        if bool((c == 1424).any()):
            kinds.add("last")
        counts.append(int(w.size))
        print(f"{b.name}: eps {r.eps!r}, {w.size} walkers with a lone column ({c.min()} .. {c.max()}), {int((nd == 0).sum())} without width")
    assert kinds == {0, 2, 4, "last"} and counts[:4] == [103, 115, 2, 37]


def test_the_picked_walkers_are_what_the_table_says():
    r = HC.rows(HC.FAMILY_BY_NAME["Dmax"].batches[0])
    cols = [np.flatnonzero(d) for d in _drawable(r)]
    assert [c.tolist() for c in cols] == [[1424], [1424], [1424], [1420], [1392], [1292], [], []]
    r = HC.rows(HC.FAMILY_BY_NAME["Dpair"].batches[0])
    cols = [np.flatnonzero(d).tolist() for d in _drawable(r)]
    assert cols == [[124, 125], [122, 159], [98], [132], [], [], [], []]      # 124 = 2 * 62: both halves of one word of 16-bit counts
    r = HC.rows(HC.FAMILY_BY_NAME["Dpair"].batches[1])
    cols = [np.flatnonzero(d).tolist() for d in _drawable(r)]
    assert cols[:4] == [[232, 1231], [232, 1327], [232, 1327], [232, 1231]] and [len(c) for c in cols[4:]] == [1, 1, 0, 0]   # (apart by more than any tile)
    assert 0.2 < float(r.law[0, 232]) < 0.8
    assert max(HC.N_MAX.values()) == 65535 < 65536


def test_float32_rows_compare_in_float32():
    for b in HC.FAMILY_BY_NAME["E32"].batches:
        r = HC.rows(b)
        assert r.hm.dtype == np.float32 and np.array_equal(r.keep, np.abs(r.hm) >= np.float32(r.eps)) and bool(r.keep.any())


def _front_on_meta(monkeypatch, route, b, N, kept):
    from pynqs_amd import reduce_front as RF

    monkeypatch.setattr(RF, "ROW_F32", route.row_f32)
    monkeypatch.setattr(RF, "ROW_CACHE", route.row_cache)
    monkeypatch.setattr(RF, "TILE_SCRATCH_MIN_ROW", route.tile_min_row)
    return RF.ReduceFrontEnd(b.n, b.sorb, b.noA + b.noB, b.noA, b.noB, N, torch.float32 if b.f32 else torch.float64, "meta", route.cap_doubles,
                             b.n * (kept + N) + 64, want_pm1=False, dedup=route.dedup)


@pytest.mark.parametrize("family", [f.name for f in HC.FAMILIES])
def test_the_case_table_agrees_with_the_host_plan(family, monkeypatch):
    """Every launch of the table: the plan names the intended form, with the intended buffers.  Where the table says a form cannot be
    reached (the cached LIST form at N = 1) the plan names another; at N_MAX the plan names the form and at N_MAX + 1 no longer."""
    from pynqs_amd import reduce_front as RF

    fam = HC.FAMILY_BY_NAME[family]
    kept = HC.kept_max(family)
    seen = set()
    for route in HC.ROUTES[1:]:
        for b in fam.batches:
            key = (route.name, b.n, b.sorb, b.f32)
            if key in seen:
                continue
            seen.add(key)
            sp = HC.spec(family, route.name)
            N = sp[0] if sp else (fam.N or HC.N_MAX[route.name])
            assert kept + 8 <= route.cap_doubles
            fe = _front_on_meta(monkeypatch, route, b, N, kept)
            got = (fe.form, bool(fe.plan.tile_sums_global), (fe.row_f32_form, fe.row_cache is not None, fe.tile_scratch is not None))
            if sp is None:
                assert got[:2] != (route.form, route.tile_sums_global), (family, route.name, got)
                continue
            assert got == (route.form, route.tile_sums_global, sp[1]), (family, route.name, N, got)
            assert int(fe.plan.lds_bytes) <= 160 * 1024 - 256
            if fam.N == 0:
                assert N == HC.N_MAX[route.name]
                for more in [N + 1] + list(range(N + 257, 65536, 4099)):
                    try:
                        nxt = _front_on_meta(monkeypatch, route, b, more, kept)
                    except RuntimeError:      # more than 65535 draws
                        assert more == 65536
                        continue
                    assert (nxt.form, bool(nxt.plan.tile_sums_global)) != (route.form, route.tile_sums_global) or route.form == "lookback", (route.name, more)
    assert RF.ROW_F32 in (True, False)


@pytest.fixture(scope="module")
def set0():
    return HC.rows(HC.FAMILY_BY_NAME["A"].batches[0])


def test_the_yardstick_passes_a_correct_hierarchical_sampler(set0):
    rng = np.random.default_rng(7)
    fig = HC.check(set0, HC.host_hier(set0, 300, rng), 300)
    stat, dof, limit = HC.pooled_chi_square([fig.hits], [set0.law], 300)
    hstat, hdof, _ = HC.pooled_chi_square([HC.host_counts(set0, 300, rng)], [set0.law], 300)
    print(f"host hierarchical sampler on set 0: {fig.kept} kept + {fig.drawn} drawn records, chi-square {stat:.1f} [{hstat:.1f}], dof {dof}, threshold {limit:.1f}")
    assert dof == hdof > 9000 and stat < limit and hstat < limit and fig.werr <= 1.0 and fig.serr <= 1.0
    for fam, N in (("Dmax", 65535), ("Dpair", 65535), ("C", 300)):
        r = HC.rows(HC.FAMILY_BY_NAME[fam].batches[-1])
        fig = HC.check(r, HC.host_hier(r, N, rng), N)
        assert fig.lone >= 2 and fig.no_width >= 2


@pytest.mark.parametrize("mutant", list(HC.MUTANTS))
def test_the_yardstick_refuses_every_mutant(mutant, set0):
    """each mutant is one mistake in the numpy hierarchical sampler; HC.MUTANTS names the assertion that refuses it"""
    rng = np.random.default_rng(11)
    why = HC.MUTANTS[mutant]
    if mutant == "carry":
        r, N = HC.rows(HC.FAMILY_BY_NAME["Dmax"].batches[0]), 65535
    else:
        r, N = set0, 300
    if why == "chi-square":
        fig = HC.check(r, HC.host_hier(r, N, rng, mutant), N)       # every record is in order: only the law is wrong
        stat, dof, limit = HC.pooled_chi_square([fig.hits], [r.law], N)
        print(f"{mutant}: chi-square {stat:.1f}, dof {dof}, threshold {limit:.1f}")
        assert stat > limit
    else:
        with pytest.raises(AssertionError, match=why):
            HC.check(r, HC.host_hier(r, N, rng, mutant), N)
