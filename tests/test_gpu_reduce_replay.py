"""Every record of every walker of the short-row semi-stochastic REDUCE form (pynqs_reduce_onepass with io->row_f32, row_f32_form 1:
reduce_draw.h) against the exact host replay of its documented draw law (tests/reduce_replay.py, include/pynqs_amd.h):
  * kept records = the CPU oracle's |H| >= eps, columns, values and determinants bit for bit;
  * drawn columns and hit counts = the replay's, exactly (tests/test_reduce_replay.py asserts that no draw of any case is within the
    rounding margin tau of a CDF boundary: nothing is left to the kernel's rounding);
  * weights within (ncomb + 2) 2^-52 relative of (c / N) sign(H) S in the integral dtype, row_sum within ncomb 2^-52 relative of S
    (S exact in longdouble);
  * links leading to the records' determinants (distinct list, de-duplication slots or the wave-function table).
The hierarchical forms (flushing, look-back, LIST with row cache / re-enumeration / tile sums in global memory, and the multi-pass
reduce_compact_sampled) draw tile first, then column: only their law is contractual.  They get Pearson's chi-square pooled over R = 8
seeds against the exact |H| / S with the derived threshold chi2.isf(1e-9, dof); the host replay passes the same function at the same
shapes, N and R on the CPU (tests/test_reduce_replay.py)."""
import numpy as np
import pytest
import torch

import reduce_replay as RR
from conftest import golden

pytestmark = pytest.mark.gpu
LD = RR.LD


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _compare(case, fe, ref, lut=None):
    """all records of the front end's last run against the replay `ref`; returns the worst (weight error / bound, row_sum error / bound)"""
    n, ncomb = ref.hm.shape
    nu, flags, mx = fe.counters_host()
    assert fe.row_f32_form == 1 and fe.row_f32 is not None and fe.form == "rowout"
    assert flags == 0 and not fe.overflowed((nu, flags, mx))
    walker, col, w, link, onv, drawn = fe.records()
    rows_own = fe.rows_of(link[link >= 0]).cpu().numpy()
    uniq = fe.uniq_onv.cpu().numpy()
    walker, col, w, link, onv, drawn = (t.cpu().numpy() for t in (walker, col, w, link, onv, drawn))
    col = col.astype(np.int64)
    assert w.dtype == ref.hm.dtype
    # kept records: the oracle's |H| >= eps, bit for bit
    k = ~drawn
    order = np.lexsort((col[k], walker[k]))
    kw, kc = np.nonzero(ref.keep)
    assert np.array_equal(walker[k][order], kw) and np.array_equal(col[k][order], kc), "kept set"
    assert np.array_equal(w[k][order], ref.hm[kw, kc]), "kept values"
    # drawn records: walker by walker, ascending columns, the replay's columns and counts
    rw, rc, rh = ref.records()
    assert np.array_equal(walker[drawn], rw) and np.array_equal(col[drawn], rc), "drawn columns differ from the replay"
    rs = fe.row_sum[:n].cpu().numpy().astype(LD)
    sign = np.sign(ref.hm[rw, rc]).astype(LD)
    hits = np.rint((w[drawn].astype(LD) * LD(case.N) / (sign * rs[rw])).astype(np.float64)).astype(np.int64) if rw.size else rh
    assert np.array_equal(hits, rh), "hit counts differ from the replay"
    used = fe.srec_col[: n * case.N].view(n, case.N).cpu().numpy() >= 0
    assert np.array_equal(used.sum(1), (ref.hits > 0).sum(1)) and bool((used[:, :-1] >= used[:, 1:]).all())   # the first slots, nothing behind
    # weights and row sums
    want = ref.weights()
    bound_w, werr = LD(ncomb + 2) * LD(2.0) ** -52, 0.0
    if rw.size:
        if ref.hm.dtype == np.float64:
            rel = np.abs(w[drawn].astype(LD) - want) / np.abs(want)
            werr = float(rel.max() / bound_w)
            assert bool((rel <= bound_w).all()), f"weights: {werr} of the bound"
        else:   # float32: the stored value is the rounding of a number within the bound
            lo, hi = (want - bound_w * np.abs(want)).astype(np.float32), (want + bound_w * np.abs(want)).astype(np.float32)
            assert bool(((lo <= w[drawn]) & (w[drawn] <= hi)).all()), "weights (float32)"
            werr = float((np.abs(w[drawn].astype(LD) - want.astype(np.float32).astype(LD)) / np.abs(want)).max() / bound_w)
    live = ref.S > 0
    assert bool((rs[~live] == 0).all())
    bound_s = LD(ncomb) * LD(2.0) ** -52
    serr = float((np.abs(rs[live] - ref.S[live]) / ref.S[live]).max() / bound_s) if live.any() else 0.0
    assert serr <= 1.0, f"row_sum: {serr} of the bound"
    # determinants and links
    assert np.array_equal(onv, ref.kets[walker, col]), "a record's determinant is not the oracle's x'"
    own = link >= 0
    assert np.array_equal(uniq[rows_own], onv[own]) and int(rows_own.max()) < nu, "links"
    if lut is None:
        assert bool(own.all())
        if case.dedup:
            assert np.unique(onv, axis=0).shape[0] == nu
        else:
            assert nu == onv.shape[0] and np.unique(rows_own).size == nu
    else:
        pos, found = lut.find(_dev(onv))
        assert np.array_equal(found.cpu().numpy(), link <= -2) and bool((link <= -2).any()) and bool((link != -1).all())
        assert np.array_equal(pos[found].cpu().numpy(), -2 - link[link <= -2].astype(np.int64))
    print(f"{case.name}: {int(k.sum())} kept + {rw.size} drawn records equal the replay; worst weight error / bound {werr:.3g}, row_sum error / bound {serr:.3g}")
    return werr, serr


def _front(case, x, eps, ref):
    from pynqs_amd import reduce_front as RF

    kept_max = int(ref.keep.sum(1).max())
    dt = torch.float32 if case.f32 else torch.float64
    return RF.ReduceFrontEnd(case.n, case.sorb, case.noA + case.noB, case.noA, case.noB, case.N, dt, x.device, kept_max + 4,
                             case.n * (kept_max + case.N) + 64, want_pm1=False, dedup=case.dedup)


@pytest.mark.parametrize("case", [c for c in RR.CASES if c.via == "front"], ids=lambda c: c.name)
def test_every_record_equals_the_replay(case, fe2s2):
    from pynqs_amd import C_extension as cx, public_function as pf

    xh, h1, h2, eps = RR.inputs(case.name)
    x, h1g, h2g = _dev(xh), _dev(h1), _dev(h2)
    seed, = RR.kernel_seeds(case)
    ref = RR.reference(case.name, seed)
    assert ref.undecided == 0
    lut = None
    if case.lut:
        g = torch.Generator().manual_seed(3)
        lut = pf.WavefunctionLUT(_dev(fe2s2["ci_space"][:3000]), (torch.rand(3000, generator=g, dtype=torch.float64) + 0.2).cuda(), case.sorb,
                                 device=torch.device("cuda"))
    fe = _front(case, x, eps, ref)
    plan = cx.plan_for(h1g, h2g, case.sorb, x.device).buf
    fe.run(x, plan, eps, seed, lut.hashtable if lut is not None else None)
    _compare(case, fe, ref, lut)
    if case.name == "eps_zero":   # the next seed draws other columns, and the replay follows
        fe.run(x, plan, eps, seed + 1, None)
        nxt = RR.replay_rows(ref.hm, ref.kets, eps, case.N, seed + 1)
        assert nxt.undecided == 0 and not np.array_equal(nxt.hits, ref.hits)
        _compare(case, fe, nxt)


def test_through_energy_reduce_front(fe2s2):
    """energy.reduce_front draws its kernel seed from torch's generator (energy._draw_seed): after torch.manual_seed the records are the
    replay's at that seed -- and the committed fixture's, which tests/test_reduce_replay.py reproduces from the law."""
    from pynqs_amd import energy as E

    case = RR.CASE_BY_NAME["through_energy"]
    xh, h1, h2, eps = RR.inputs(case.name)
    seed, = RR.kernel_seeds(case)
    ref = RR.reference(case.name, seed)
    E._FRONTS.clear()
    torch.manual_seed(case.seed)
    fe, nu = E.reduce_front(_dev(xh), _dev(h1), _dev(h2), case.sorb, case.noA + case.noB, case.noA, case.noB, eps, case.N, None)
    _compare(case, fe, ref)
    g = golden("reduce_draws_fe2s2.npz")
    rw, rc, rh = ref.records()
    assert np.array_equal(rw, g["draw_walker"]) and np.array_equal(rc, g["draw_col"]) and np.array_equal(rh, g["draw_hits"])


def test_every_graph_replay_equals_the_replay_at_its_seed(fe2s2):
    """ReduceStep(graph=True): the launch is replayed with the same arguments, the seed word in device memory is bumped inside the graph.
    The capturing call (two warm-up runs, then the first replay) and three further replays each equal the host replay at
    seed + seed_dev, seed_dev as read before the replay: "every replay draws afresh" as an exact statement."""
    from pynqs_amd import C_extension as cx, reduce_front as RF
    from pynqs_amd.rbm import RealRBM

    case = RR.CASE_BY_NAME["graph_replay"]
    d = golden("eloc_e2e_fe2s2.npz")
    xh, h1, h2, eps = RR.inputs(case.name)
    x = _dev(xh)
    plan = cx.plan_for(_dev(h1), _dev(h2), case.sorb, x.device).buf
    rbm = RealRBM(_dev(d["W"]), _dev(d["hb"]), _dev(d["vb"])).cuda().double()
    fe = RF.ReduceFrontEnd(case.n, case.sorb, case.noA + case.noB, case.noA, case.noB, case.N, torch.float64, x.device, 256, 60000 + 300 * case.n,
                           torch.float64)
    step = RF.ReduceStep(fe, plan, eps, rbm, seed=case.seed, graph=True)
    seeds = RR.kernel_seeds(case)
    for i, seed in enumerate(seeds):
        before = int(fe.seed_dev.item())
        e, _ = step(x)
        torch.cuda.synchronize()
        after = int(fe.seed_dev.item())
        used = before if i else after - 1        # (the capturing call bumps the word in its warm-up runs first)
        assert case.seed + used == seed and after == used + 1
        assert bool(torch.isfinite(e).all())
        _compare(case, fe, RR.reference(case.name, seed))
        step.check()


def _hits_of(w, sign, scale, N):
    c = w * N / (sign * scale)
    assert float((c - c.round()).abs().max()) < 1e-6 and bool((c.round() >= 1).all())
    return c.round().long()


@pytest.mark.parametrize("shape", RR.HIER, ids=lambda h: h.name)
def test_hierarchical_forms_follow_the_law(shape, monkeypatch):
    from pynqs_amd import C_extension as cx, energy as E, reduce_front as RF

    xh, h1, h2 = RR.hier_inputs(shape.name)
    hm = RR.hier_rows(shape.name)
    n, ncomb = hm.shape
    p = RR.exact_law(hm, shape.eps)
    x, h1g, h2g = _dev(xh), _dev(h1), _dev(h2)
    hmg = _dev(hm)
    keep = RR.keep_mask(hm, shape.eps)
    S = _dev(np.where(keep, 0.0, np.abs(hm)).sum(1))
    nele = shape.noA + shape.noB
    counts = torch.zeros((n, ncomb), dtype=torch.long, device="cuda")
    if shape.how != "multi":
        monkeypatch.setattr(RF, "ROW_F32", shape.row_f32)
        monkeypatch.setattr(RF, "ROW_CACHE", shape.row_cache)
        monkeypatch.setattr(RF, "TILE_SCRATCH_MIN_ROW", shape.tile_min_row)
        kept_max = int(keep.sum(1).max())
        assert kept_max + 8 <= shape.cap_doubles
        fe = RF.ReduceFrontEnd(n, shape.sorb, nele, shape.noA, shape.noB, shape.N, torch.float64, x.device, shape.cap_doubles,
                               n * (kept_max + shape.N) + 64, want_pm1=False, dedup=shape.dedup)
        assert (fe.row_f32_form, fe.row_cache is not None, fe.tile_scratch is not None) == shape.expect
        assert (fe.form, bool(fe.plan.tile_sums_global)) == (shape.form, shape.tile_sums_global)
        assert (shape.cap_doubles > RF.list_capacity(n, shape.sorb, nele, shape.noA, shape.noB, shape.N)) == (shape.cap_doubles > 1000)
        plan = cx.plan_for(h1g, h2g, shape.sorb, x.device).buf
    for r in range(1, RR.R_SEEDS + 1):
        if shape.how == "multi":
            torch.manual_seed(r)
            _, (s_row, s_col, _, s_w, _) = E.reduce_compact_sampled(x, h1g, h2g, shape.sorb, nele, shape.noA, shape.noB, shape.eps, shape.N, seed=r)
            s_col = s_col.long()
            scale = S[s_row]
        else:
            fe.run(x, plan, shape.eps, r, None)
            assert fe.counters_host()[1] == 0
            walker, col, w, link, onv, drawn = fe.records()
            assert torch.equal(torch.sort(walker[~drawn] * ncomb + col[~drawn].long()).values, _dev(np.flatnonzero(keep.reshape(-1))))
            s_row, s_col, s_w = walker[drawn], col[drawn].long(), w[drawn]
            scale = fe.row_sum[s_row]
        flat = s_row * ncomb + s_col
        assert flat.unique().numel() == flat.numel()
        hits = _hits_of(s_w, torch.sign(hmg[s_row, s_col]), scale, shape.N)
        assert bool((torch.zeros(n, dtype=torch.long, device="cuda").index_add_(0, s_row, hits) == shape.N).all())
        counts[s_row, s_col] += hits
    stat, dof, limit = RR.chi_square(counts.cpu().numpy(), p, RR.R_SEEDS * shape.N)
    print(f"{shape.name}: chi-square {stat:.1f}, dof {dof}, threshold {limit:.1f}")
    assert dof > 0 and stat < limit
