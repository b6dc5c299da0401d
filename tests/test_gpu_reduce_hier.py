"""The hierarchical semi-stochastic REDUCE draws on the GPU, route by route and family by family (tests/reduce_hier_cases.py has the cases,
the bounds and their derivation): the multi-pass energy.reduce_compact_sampled and the front end's flush_row32, flush, lookback,
list_cache and list_redraw forms, the last also with its tile sums in global memory, on sparse rows with whole tiles empty, with nothing
kept, with a lone drawable column or none, at N = 1 and at the largest N of each form, with float32 integrals and with two and three
determinant words.  Every launch: the form the plan names, the kept records bit for bit, every drawn record on a sub-eps column of positive
width with the oracle's ket and sign, whole hit counts adding up to N, weights and row sums within the header's bounds, links, distinct list
and counters.  Every route and family: Pearson's chi-square against the exact |H| / S, threshold chi2.isf(1e-9, dof), with numpy's
multinomial at the same shape in brackets.  One line of figures per route and family: profiles/reduce_hier_exact.txt."""
import functools

import numpy as np
import pytest
import torch

import reduce_hier_cases as HC

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()   # (a copy: the shared rows are read-only)


@functools.lru_cache(maxsize=None)
def _integrals(b: HC.Batch):
    """h1, h2 of a batch on the device: the same tensors for every route and launch, so that the library keeps their plan"""
    r = HC.rows(b)
    return _dev(r.h1), _dev(r.h2)


def _distinct(onv: np.ndarray) -> int:
    return np.unique(np.ascontiguousarray(onv).view(f"V{onv.shape[1]}")).size


@functools.lru_cache(maxsize=None)
def _host_law(family: str, N: int):
    """numpy's multinomial on the exact law at the family's shape: (statistic, dof), computed once"""
    rng = np.random.default_rng(2024)
    rs = [HC.rows(b) for b in HC.FAMILY_BY_NAME[family].batches]
    stat, dof, _ = HC.pooled_chi_square([HC.host_counts(r, N, rng) for r in rs], [r.law for r in rs], N)
    return stat, dof


def _multi(r: HC.Rows, b: HC.Batch, N: int, seed: int) -> HC.Records:
    from pynqs_amd import energy as E

    torch.manual_seed(seed)
    kept, drawn = E.reduce_compact_sampled(_dev(r.x), *_integrals(b), b.sorb, b.noA + b.noB, b.noA, b.noB, r.eps, N, seed=seed)
    k_row, k_col, k_onv, k_h, k_counts = (t.cpu().numpy() for t in kept)
    s_row, s_col, s_onv, s_w, s_counts = (t.cpu().numpy() for t in drawn)
    assert np.array_equal(k_counts, r.keep.sum(1)) and np.array_equal(s_counts, np.bincount(s_row, minlength=b.n)), "counts per walker"
    return HC.Records(k_row, k_col, k_h, k_onv, s_row, s_col, s_w, s_onv)


def _front(route: HC.Route, b: HC.Batch, N: int, kept: int, expect, monkeypatch):
    from pynqs_amd import reduce_front as RF

    monkeypatch.setattr(RF, "ROW_F32", route.row_f32)
    monkeypatch.setattr(RF, "ROW_CACHE", route.row_cache)
    monkeypatch.setattr(RF, "TILE_SCRATCH_MIN_ROW", route.tile_min_row)
    assert kept + 8 <= route.cap_doubles
    fe = RF.ReduceFrontEnd(b.n, b.sorb, b.noA + b.noB, b.noA, b.noB, N, torch.float32 if b.f32 else torch.float64, torch.device("cuda"),
                           route.cap_doubles, b.n * (kept + N) + 64, want_pm1=False, dedup=route.dedup)
    assert (fe.form, bool(fe.plan.tile_sums_global)) == (route.form, route.tile_sums_global)
    assert (fe.row_f32_form, fe.row_cache is not None, fe.tile_scratch is not None) == expect
    return fe


def _front_run(fe, route: HC.Route, r: HC.Rows, b: HC.Batch, N: int, seed: int, prime: bool) -> HC.Records:
    from pynqs_amd import C_extension as cx

    x = _dev(r.x)
    plan = cx.plan_for(*_integrals(b), b.sorb, x.device).buf
    if prime:   # every draw slot and row_sum written by a launch in which every walker has width: what the launch under test must undo
        fe.run(x, plan, 1e3, seed + 1000, None)
        assert int((fe.srec_col[: b.n * N].view(b.n, N) >= 0).any(1).sum()) == b.n and bool((fe.row_sum[: b.n] > 0).all())
    fe.run(x, plan, r.eps, seed, None)
    nu, flags, mx = fe.counters_host()
    assert flags == 0 and not fe.overflowed((nu, flags, mx)), "overflow flags"
    walker, col, w, link, onv, drawn = fe.records()
    own = link >= 0
    assert bool(own.all()), "a record without a row of the distinct list"
    rows_own = fe.rows_of(link).cpu().numpy()
    uniq = fe.uniq_onv.cpu().numpy()
    walker, col, w, onv, drawn = (t.cpu().numpy() for t in (walker, col, w, onv, drawn))
    assert int(rows_own.max()) < nu and np.array_equal(uniq[rows_own], onv), "a link does not lead to its determinant"
    if route.dedup:
        assert _distinct(onv) == nu == _distinct(uniq[:nu]), "the distinct list is not the set of the records' determinants"
    else:
        assert nu == onv.shape[0] and np.unique(rows_own).size == nu, "without the table: one row per record"
    k = ~drawn
    return HC.Records(walker[k], col[k], w[k], onv[k], walker[drawn], col[drawn], w[drawn], onv[drawn],
                      row_sum=fe.row_sum[: b.n].cpu().numpy(), slots=fe.srec_col[: b.n * N].view(b.n, N).cpu().numpy())


# (family A alone goes through fifteen integral sets per route: more plans than the library keeps)
@pytest.mark.filterwarnings("ignore:pynqs_amd. the integral plan:RuntimeWarning")
@pytest.mark.parametrize("family,route", HC.CASE_IDS, ids=[f"{f}-{r}" for f, r in HC.CASE_IDS])
def test_every_launch_of_a_route_on_a_family(family, route, monkeypatch):
    fam, rt = HC.FAMILY_BY_NAME[family], HC.ROUTE_BY_NAME[route]
    N, expect = HC.spec(family, route)
    kept = HC.kept_max(family)
    fe, figs, laws = None, [], []
    for k, b in enumerate(fam.batches):
        r = HC.rows(b)
        if route == "multi":
            rec = _multi(r, b, N, 1 + k)
        else:
            if fe is None or (fe.n, fe.h_dtype) != (b.n, torch.float32 if b.f32 else torch.float64):
                fe = _front(rt, b, N, kept, expect, monkeypatch)
            rec = _front_run(fe, rt, r, b, N, 1 + k, fam.prime)
        figs.append(HC.check(r, rec, N))
        laws.append(r.law)
    stat, dof, limit = HC.pooled_chi_square([f.hits for f in figs], laws, N)
    hstat, hdof = _host_law(family, N)
    print(f"{route:18s} {family:5s} N {N:5d}: records {sum(f.kept for f in figs)} kept + {sum(f.drawn for f in figs)} drawn, lone-column walkers {sum(f.lone for f in figs)}, "
          f"no-width walkers {sum(f.no_width for f in figs)}, dof {dof}, chi-square {stat:.1f} [{hstat:.1f}], threshold {limit:.1f}, "
          f"worst weight error / bound {max(f.werr for f in figs):.3g}, row_sum error / bound {max(f.serr for f in figs):.3g}")
    assert dof == hdof and (dof > 0 or not fam.law)
    if dof:
        assert stat < limit and hstat < limit
