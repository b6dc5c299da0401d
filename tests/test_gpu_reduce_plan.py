"""The plan of the one-launch REDUCE front end against its launches (pynqs_reduce_onepass_plan, include/pynqs_amd.h): every kernel family
is asked for by name at the smallest row with several tiles (8 walkers, sorb 24, 4 + 4 electrons: 1425 columns -- the shapes of
tests/reduce_replay.py's HIER; the two deterministic forms at cap_doubles 600 / 1100 without draws), launched -- ReduceFrontEnd hands the
launch its plan's form, and the launch refuses unless it arrives at the same form from the buffers it was given -- and its kept records
compared with the multi-pass energy.reduce_compact bit for bit.  One more case hands the launch a form its buffers do not imply."""
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import reduce_replay as RR

pytestmark = pytest.mark.gpu
SORB, NO, N_WALKERS, EPS = 24, 4, 8, 0.45


@dataclass(frozen=True)
class Case:
    form: str
    N: int
    cap_doubles: int
    dedup: bool = True
    row_f32: bool = True
    row_cache: bool = True
    tile_min_row: int = 65536
    tile_sums_global: bool = False


CASES = [
    Case("lookback", 0, 1100),
    Case("list", 0, 600),
    Case("list_cache", 4000, 600, row_f32=False),
    Case("list_redraw", 4000, 600, row_f32=False, row_cache=False),
    Case("list_redraw", 4000, 600, row_f32=False, row_cache=False, tile_min_row=64, tile_sums_global=True),
    Case("flush", 4000, 1100, dedup=False),
    Case("flush_row32", 3000, 1100, dedup=False),
    Case("rowout", 4000, 600),
    Case("lookback", 4000, 1100),
]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def system():
    """(x, h1, h2, integral plan, the kept records of energy.reduce_compact): computed once, shared, never modified"""
    from pynqs_amd import C_extension as cx, energy as E

    x, h1, h2 = (_dev(a) for a in RR.hier_inputs("lookback"))
    kept = E.reduce_compact(x, h1, h2, SORB, 2 * NO, NO, NO, EPS, sort=True)
    return x, h1, h2, cx.plan_for(h1, h2, SORB, x.device).buf, kept


def _front(case, system, monkeypatch):
    from pynqs_amd import reduce_front as RF

    monkeypatch.setattr(RF, "ROW_F32", case.row_f32)
    monkeypatch.setattr(RF, "ROW_CACHE", case.row_cache)
    monkeypatch.setattr(RF, "TILE_SCRATCH_MIN_ROW", case.tile_min_row)
    x, kept_max = system[0], int(system[4][4].max())
    assert kept_max + 8 <= case.cap_doubles
    return RF.ReduceFrontEnd(N_WALKERS, SORB, 2 * NO, NO, NO, case.N, torch.float64, x.device, case.cap_doubles,
                             N_WALKERS * (kept_max + case.N) + 64, want_pm1=False, dedup=case.dedup)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c.form}-{c.N}" + ("-global" if c.tile_sums_global else ""))
def test_every_form_runs_as_planned(case, system, monkeypatch):
    x, h1, h2, plan, (row, col2, onv2, hval, counts) = system
    fe = _front(case, system, monkeypatch)
    assert (fe.form, bool(fe.plan.tile_sums_global)) == (case.form, case.tile_sums_global)
    fe.run(x, plan, EPS, seed=3)
    cnt = fe.counters_host()
    assert cnt[1] == 0 and not fe.overflowed(cnt)
    w, col, h, link, onv, drawn = fe.records()
    kw, kc, kh, ko = w[~drawn], col[~drawn], h[~drawn], onv[~drawn]
    k1 = torch.argsort((kw << 32) | kc.long(), stable=True)
    assert torch.equal(kw[k1], row) and torch.equal(kc[k1], col2) and torch.equal(kh[k1], hval) and torch.equal(ko[k1], onv2)
    assert bool(drawn.any()) == (case.N > 0)


def test_a_launch_that_disagrees_with_its_plan_is_refused(system, monkeypatch):
    """io->form names another form than the buffers imply: PYNQS_EINVAL from the argument check, before the clear kernel -- the counters
    still hold what the run before left (a run at this eps would have counted other rows)."""
    x, h1, h2, plan, _ = system
    fe = _front(CASES[2], system, monkeypatch)
    assert fe.form == "list_cache"
    fe.run(x, plan, EPS, seed=3)
    before = fe.counters.clone()
    assert int(before[0]) > 0
    fe._io.form = 1 + fe._io.form % 7
    with pytest.raises(RuntimeError, match="plan and buffers disagree"):
        fe.run(x, plan, 0.3, seed=3)
    assert torch.equal(fe.counters, before)
    fe._io.form = 0            # (no plan: the launch decides from the buffers, as a C caller's that ignores the plan)
    fe.run(x, plan, EPS, seed=3)
    assert torch.equal(fe.counters, before)


@pytest.mark.parametrize("N", [0, 100])
def test_no_walkers_clear_and_return(system, N):
    """nbatch = 0, with the plan's form or without: the launch clears the counters and returns; nothing else is enqueued"""
    from pynqs_amd import reduce_front as RF

    x, h1, h2, plan, _ = system
    fe = RF.ReduceFrontEnd(0, SORB, 2 * NO, NO, NO, N, torch.float64, x.device, 600, 128, want_pm1=False)
    for form in (int(fe.plan.form), 0):
        fe._io.form = form
        fe.counters.fill_(7)
        fe.run(x[:0].contiguous(), plan, EPS, seed=3)
        assert fe.counters.tolist() == [0, 0, 0, 0]
