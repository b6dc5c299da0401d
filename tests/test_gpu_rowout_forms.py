"""The two tile loops of the short-row semi-stochastic REDUCE kernel (pynqs_reduce_onepass_form; ReduceFrontEnd.run(form=...)): form 0 sums
a tile by cross-lane moves of a fixed pattern, forms that sum behind the next tile's gathers and hands a full tile's kept columns to the list
together; form 1 is the earlier loop.  On the
same walkers, seed and capacities every output is the same bit for bit, in slot order: seg_count, rec_col, rec_w, srec_col, srec_w, row_sum,
the float32 row with its padding, the distinct count and the overflow words.  The order of the distinct list follows the launch's atomics, so
the distinct determinants are compared as sets and every record's link by the determinant it leads to.  Form 0 is also held to the exact
host replay (tests/reduce_replay.py), as tests/test_gpu_reduce_replay.py holds the default form.
Two cases overflow the kept list (cap_doubles below the kept count): both forms flag it with the same words.  Which kept columns then find
room follows the atomics under either form, so there only what does not depend on that is compared."""
import numpy as np
import pytest
import torch

import reduce_replay as RR

pytestmark = pytest.mark.gpu
LD = RR.LD

CASES = ["one_segment", "sixteen_columns", "multiple_of_16_plus_1", "five_segments_plus_1", "near_8192", "fe2s2_one_draw", "eps_zero",
         "eps_above_all", "no_width", "sparse", "one_word", "many_walkers"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(case, form, eps, cap_doubles, cap_unique, seed):
    from pynqs_amd import C_extension as cx, reduce_front as RF

    xh, h1, h2, _ = RR.inputs(case.name)
    x = _dev(xh)
    fe = RF.ReduceFrontEnd(case.n, case.sorb, case.noA + case.noB, case.noA, case.noB, case.N, torch.float64, x.device, cap_doubles, cap_unique,
                           want_pm1=False, dedup=case.dedup)
    assert fe.row_f32_form == 1 and fe.row_f32 is not None and fe.form == "rowout", "not the short-row semi-stochastic kernel"
    fe.row_f32.fill_(float("nan"))  # (whatever the kernel does not write shows)
    plan = cx.plan_for(_dev(h1), _dev(h2), case.sorb, x.device).buf
    fe.run(x, plan, eps, seed, None, form=form)
    torch.cuda.synchronize()
    return fe


def _np(t):
    return t.cpu().numpy()


def _same_bits(a, b, what):
    a, b = _np(a), _np(b)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what} differs between the forms"


def _record_kets(fe):
    """per record slot (kept slots, then draw slots): the determinant its link leads to (zeros where there is no record)"""
    out = []
    for col, link in ((fe.rec_col, fe.rec_link), (fe.srec_col, fe.srec_link)):
        live = col >= 0
        k = torch.zeros((col.numel(), fe.uniq_onv.size(1)), dtype=torch.uint8, device=col.device)
        assert bool((link[live] >= 0).all())
        k[live] = fe.uniq_onv[fe.rows_of(link[live])]
        out.append(_np(k))
    return out


def _replay_check(case, fe, ref):
    """form 0 against the host replay: kept records the oracle's, drawn columns and hit counts the replay's, weights and S within their bounds"""
    n, ncomb = ref.hm.shape
    nu, flags, mx = fe.counters_host()
    assert flags == 0 and not fe.overflowed((nu, flags, mx))
    walker, col, w, link, onv, drawn = (_np(t) for t in fe.records())
    col = col.astype(np.int64)
    k = ~drawn
    order = np.lexsort((col[k], walker[k]))
    kw, kc = np.nonzero(ref.keep)
    assert np.array_equal(walker[k][order], kw) and np.array_equal(col[k][order], kc), "kept set"
    assert np.array_equal(w[k][order], ref.hm[kw, kc]), "kept values"
    rw, rc, rh = ref.records()
    assert np.array_equal(walker[drawn], rw) and np.array_equal(col[drawn], rc), "drawn columns differ from the replay"
    rs = _np(fe.row_sum[:n]).astype(LD)
    if rw.size:
        sign = np.sign(ref.hm[rw, rc]).astype(LD)
        hits = np.rint((w[drawn].astype(LD) * LD(case.N) / (sign * rs[rw])).astype(np.float64)).astype(np.int64)
        assert np.array_equal(hits, rh), "hit counts differ from the replay"
        want = ref.weights()
        assert bool((np.abs(w[drawn].astype(LD) - want) <= LD(ncomb + 2) * LD(2.0) ** -52 * np.abs(want)).all()), "weights"
    live = ref.S > 0
    assert bool((rs[~live] == 0).all())
    if live.any():
        assert bool((np.abs(rs[live] - ref.S[live]) <= LD(ncomb) * LD(2.0) ** -52 * ref.S[live]).all()), "row_sum"
    assert np.array_equal(onv, ref.kets[walker, col]), "a record's determinant is not the oracle's x'"
    assert np.unique(onv, axis=0).shape[0] == nu


@pytest.mark.parametrize("name", CASES)
def test_forms_agree_bit_for_bit(name):
    case = RR.CASE_BY_NAME[name]
    assert case.via == "front" and not case.f32 and not case.lut
    seed, = RR.kernel_seeds(case)
    ref = RR.reference(name, seed)
    eps = RR.inputs(name)[3]
    kept_max = int(ref.keep.sum(1).max())
    caps = (kept_max + 4, case.n * (kept_max + case.N) + 64)
    fe0, fe1 = (_run(case, form, eps, *caps, seed) for form in (0, 1))
    for what in ("seg_count", "rec_col", "rec_w", "srec_col", "srec_w", "row_sum", "row_f32"):
        _same_bits(getattr(fe0, what), getattr(fe1, what), what)
    c0, c1 = _np(fe0.counters), _np(fe1.counters)
    assert c0[0] == c1[0] and c0[1] == c1[1] == 0 and c0[2] == c1[2], f"counters {c0} / {c1}"
    u0, u1 = _np(fe0.uniq_onv[: c0[0]]), _np(fe1.uniq_onv[: c1[0]])
    assert np.array_equal(np.unique(u0, axis=0), np.unique(u1, axis=0)) and np.unique(u0, axis=0).shape[0] == c0[0], "distinct determinants"
    for a, b in zip(_record_kets(fe0), _record_kets(fe1)):
        assert np.array_equal(a, b), "a record's link leads to another determinant"
    _replay_check(case, fe0, ref)


@pytest.mark.parametrize("eps, cap_doubles", [(1e-3, 128), (1e-300, 64)], ids=["half_the_kept_fit", "every_column_kept"])
def test_forms_flag_an_overflowing_list_alike(eps, cap_doubles):
    """the flagship's rows (43 tiles, 16 walkers) with room for fewer records than are kept (564 - 735 at eps = 1e-3 against 168 fixed + 128
    slots); with eps = 1e-300 every lane of every full tile keeps all four of its columns (7876 against 168 + 64).  The overflow bit, the
    largest count, seg_count, the row's float32 copy and S do not depend on which columns found room."""
    case = RR.CASE_BY_NAME["fe2s2_one_draw"]
    hm, _ = RR.rows(case.name)
    kept = RR.keep_mask(hm, eps).sum(1)
    fe0, fe1 = (_run(case, form, eps, cap_doubles, case.n * (cap_doubles + 200 + case.N) + 64, 1) for form in (0, 1))
    assert fe0.fixed + cap_doubles < int(kept.min())
    for what in ("seg_count", "row_sum", "row_f32"):
        _same_bits(getattr(fe0, what), getattr(fe1, what), what)
    c0, c1 = _np(fe0.counters), _np(fe1.counters)
    assert (c0[1] & 1) and c0[1] == c1[1] and c0[2] == c1[2] == int(kept.max()) - fe0.fixed, f"counters {c0} / {c1}"
    assert fe0.overflowed() and fe1.overflowed()
    assert np.array_equal(_np(fe0.seg_count[: case.n]), kept - fe0.fixed), "seg_count is the kept count whatever the room"
