"""The two schedules of the LDS form of pynqs_rbm_forward_children against each other, bit for bit: form 0 (eight hidden units at a time,
H % 8 units left over one by one; with real parameters the next chunk's q_h requested ahead) and form 1 (one hidden unit after the other)
run the same operations on the same operands in the same order, so psi must agree as int64 bit patterns -- a nan or a signed zero counts
-- on the same
inputs and the SAME prepared table (one pynqs_rbm_children_prepare_stamped, then pynqs_rbm_forward_children_stamped_form twice).  The
shapes are the smallest at which the chunked control flow can go wrong: H below, at and above one and two chunks and the flagship's 40;
1 to 1025 rows and a second sweep of the capped grid (its size asked of the library); one and 257 parents in runs and shuffled; the device
count at 0, 1 and n - 1 over a sentinel; strangers inside waves of ordinary rows; overflowed products and the raised flag, whose rows must
still come from scratch.  Whether either schedule is RIGHT is the business of tests/test_gpu_children_shapes.py and
tests/test_gpu_rbm_exact.py, which run form 0 against the exact reference -- and so is everything the two forms share (the staging of
the factor table, the second loop with its marker in psi, write_psi): a mistake there is the same in both and cannot show here."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import children_cases as CC
import rbm_exact as R
import test_gpu_children_shapes as S
import test_gpu_rbm_exact as T

pytestmark = pytest.mark.gpu

_dev, _onv = T._dev, T._onv
NAN_BITS = S.NAN_BITS  # what the output holds before a launch: rows at and past the count must keep it
CHUNKED, PER_UNIT = 0, 1
SMALL_N = (1, 63, 64, 65, 1023, 1025)


def _doubles_per_row(kind):
    return 2 if kind in ("complex", "pRBM") else 1


@functools.lru_cache(maxsize=None)  # (a few hundred rows each)
def _pool(sorb, nw, seed):
    parents = R.rand_words(nw, sorb, 11 + seed)
    pool, ppar, _ = R.make_children(parents, sorb, 5 + seed)
    return parents, pool, ppar


def _inputs(kind, sorb, H, nw, n, order, regime="fe2s2", strangers=False, seed=0):
    """(onv, parent, walkers, W, hb, vb) on the GPU: n rows gathered at random from the children rbm_exact.make_children makes of nw random
    parents (0 to 4 flips, the word edges, four flips in one word), shuffled or in runs per parent; strangers: parents -1, nw and nw + 3
    and a row six flips away from the parent it names, inside the first waves"""
    g = np.random.default_rng([41, seed, sorb, H, nw, n])
    parents, pool, ppar = _pool(sorb, nw, seed)
    idx = g.integers(0, pool.shape[0], n)
    if order == "runs":
        idx = idx[np.argsort(ppar[idx], kind="stable")]
    rows, par = np.ascontiguousarray(pool[idx]), ppar[idx].astype(np.int32)
    if strangers:
        assert n > 200 and sorb >= 6
        par[5], par[70], par[130] = -1, nw, nw + 3
        for i in (10, 64, 191):
            rows[i] = R.flipped(parents[par[i]], [int(o) for o in g.choice(sorb, 6, replace=False)])
    rbm = R.regime_params(regime, kind, sorb, H, seed)
    W, hb, vb = T.kernel_params(rbm, regime)
    return _onv(rows), _dev(par), _onv(parents), _dev(W), _dev(hb), None if vb is None else _dev(vb)


def _both_forms(kind, sorb, H, dev_inputs, count=None):
    """int64 bit patterns [n * doubles per row] of form 0 and form 1 on one prepared table, over a sentinel"""
    from pynqs_amd import C_extension as cx, _native as N

    onv, par, walkers, W, hb, vb = dev_inputs
    flav, n, nw = CC.flavour(kind), onv.size(0), walkers.size(0)
    assert CC.geometry(kind, sorb, H, n)[0] == "lds"
    table = torch.empty(max(N.lib().pynqs_rbm_children_table_bytes(nw, sorb, H, flav) // 8, 1), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    vbp = None if vb is None else vb.data_ptr()
    stamp = next(cx._CHILDREN_STAMP)
    N.check(N.lib().pynqs_rbm_children_prepare_stamped(walkers.data_ptr(), nw, sorb, W.data_ptr(), hb.data_ptr(), vbp, H, flav, stamp,
                                                       table.data_ptr(), st), "pynqs_rbm_children_prepare_stamped")
    cnt = None if count is None else torch.tensor([count, 0, 0, 0], dtype=torch.int32, device="cuda")
    out = []
    for form in (CHUNKED, PER_UNIT):
        raw = torch.full((n * _doubles_per_row(kind),), NAN_BITS, dtype=torch.int64, device="cuda")
        N.check(N.lib().pynqs_rbm_forward_children_stamped_form(onv.data_ptr(), n, None if cnt is None else cnt.data_ptr(), par.data_ptr(),
                                                                walkers.data_ptr(), nw, table.data_ptr(), sorb, W.data_ptr(), hb.data_ptr(),
                                                                vbp, H, flav, stamp, form, raw.data_ptr(), st),
                "pynqs_rbm_forward_children_stamped_form")
        out.append(raw)
    torch.cuda.synchronize()
    return out


def _same_bits(what, a, b):
    bad = int((a != b).sum())
    assert bad == 0, f"{what}: {bad} of {a.numel()} words differ between the chunked and the per-unit schedule"
    assert bool((a != NAN_BITS).all()), f"{what}: rows left unwritten"


def _counts(what, kind, sorb, H, dev_inputs, full):
    """count_dev 0, 1 and n - 1: the rows below carry the full run's bits, the rows from the count on keep the sentinel, in both forms"""
    n, c = dev_inputs[0].size(0), _doubles_per_row(kind)
    for v in sorted({0, 1, n - 1}):
        for form, got in zip(("chunked", "per-unit"), _both_forms(kind, sorb, H, dev_inputs, count=v)):
            assert torch.equal(got[:v * c], full[:v * c]), f"{what}, count {v}, {form}: rows below the count"
            assert bool((got[v * c:] == NAN_BITS).all()), f"{what}, count {v}, {form}: rows from the count on"


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("H", [1, 7, 8, 9, 15, 16, 17, 40])
def test_every_chunk_count_and_remainder(kind, H):
    """sorb 12; H: no full chunk, exactly one, a remainder of one and of seven, two chunks, the flagship's five -- each on 1 to 1025 rows,
    from one and from 257 parents, in runs and shuffled, and under the device count"""
    sorb = 12
    for nw in (1, 257):
        for order in CC.ORDERS:
            for n in SMALL_N:
                what = f"{kind} {sorb}x{H}, nw {nw}, n {n}, {order}"
                inp = _inputs(kind, sorb, H, nw, n, order)
                a, b = _both_forms(kind, sorb, H, inp)
                _same_bits(what, a, b)
                if n in (65, 1025) and order == "shuffled":
                    _counts(what, kind, sorb, H, inp, a)


@pytest.mark.parametrize("kind,H", [("real", 17), ("complex", 9), ("complex", 40)])
def test_a_second_sweep_of_the_capped_grid(kind, H):
    """one sweep of the capped grid (the library's own number) plus 1025 rows: every workgroup strides on, the last one row"""
    sorb = 12
    n = CC.geometry(kind, sorb, H, 1 << 30)[2] + 1025
    assert CC.geometry(kind, sorb, H, n)[2] < n
    inp = _inputs(kind, sorb, H, 257, n, "runs")
    a, b = _both_forms(kind, sorb, H, inp)
    _same_bits(f"{kind} {sorb}x{H}, n {n}", a, b)
    _counts(f"{kind} {sorb}x{H}, n {n}", kind, sorb, H, inp, a)


@pytest.mark.parametrize("kind,sorb,H", [("tanh", 12, 17), ("pRBM", 12, 17), ("real", 70, 5), ("real", 70, 9), ("complex", 130, 3), ("complex", 130, 9)])
def test_the_other_flavours_and_word_counts(kind, sorb, H):
    """TANH and PHASE, and determinants of two and three words (flips at the word edges and spread over the words)"""
    for n in (65, 1025):
        inp = _inputs(kind, sorb, H, 257, n, "shuffled", regime="small")
        a, b = _both_forms(kind, sorb, H, inp)
        _same_bits(f"{kind} {sorb}x{H}, n {n}", a, b)
    _counts(f"{kind} {sorb}x{H}", kind, sorb, H, inp, a)


@pytest.mark.parametrize("kind,H", [("real", 9), ("complex", 9), ("complex", 40)])
def test_strangers_among_ordinary_rows(kind, H):
    """parents -1, nw and nw + 3 and rows six flips from their parent in waves whose other rows are ordinary ones: both schedules send them
    from scratch (pynqs_rbm_forward's bits) and leave the others alone"""
    from pynqs_amd import C_extension as cx

    sorb, n = 12, 1025
    inp = _inputs(kind, sorb, H, 257, n, "shuffled", strangers=True)
    a, b = _both_forms(kind, sorb, H, inp)
    _same_bits(f"{kind} {sorb}x{H} with strangers", a, b)
    onv, _, _, W, hb, vb = inp
    c = _doubles_per_row(kind)
    fwd = S._bits(cx.rbm_forward(onv, W, hb, vb, sorb, kind)).view(-1, c)
    at = torch.tensor([5, 70, 130, 10, 64, 191], device="cuda")
    assert torch.equal(a.view(-1, c)[at], fwd[at])
    clean = _both_forms(kind, sorb, H, _inputs(kind, sorb, H, 257, n, "shuffled"))[0].view(-1, c)
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[at] = False
    assert torch.equal(a.view(-1, c)[keep], clean[keep])


@pytest.mark.parametrize("name", ["lds-strangers", "lds-strangers-three-words", "lds-overflow-one-338-w", "lds-overflow-chunk-50"])
def test_the_pinned_strangers_and_overflow_cases(name):
    """the stranger and overflow cases of tests/children_cases.py (an overflowed product is a row for the from-scratch route: were it not
    taken, psi would be inf or nan): the same bits, all of them finite numbers"""
    c = CC.case(name)
    a, b = _both_forms(c.kind, c.sorb, c.H, S._device(name))
    _same_bits(name, a, b)
    assert bool(torch.isfinite(a.view(torch.float64)).all())


def test_the_raised_flag():
    """lds-second-sweep-raised: one parent out of range, every row from scratch over two rounds -- pynqs_rbm_forward's bits in both forms"""
    name = "lds-second-sweep-raised"
    c = CC.case(name)
    a, b = _both_forms(c.kind, c.sorb, c.H, S._device(name))
    _same_bits(name, a, b)
    assert torch.equal(a, S._bits(S._forward(name)).view(-1))
    _counts(name, c.kind, c.sorb, c.H, S._device(name), a)


def test_the_wrapper_passes_the_form_through(monkeypatch):
    """C_extension.rbm_forward_children(form=...) with its own one-launch prepare per call, PYNQS_RBM_CHILDREN_FORM for form=None, and a
    form that does not exist"""
    from pynqs_amd import C_extension as cx, _native as N

    kind, sorb, H = "complex", 12, 40
    onv, par, walkers, W, hb, vb = _inputs(kind, sorb, H, 257, 1025, "runs")
    got = {f: S._bits(cx.rbm_forward_children(onv, par, walkers, W, hb, vb, sorb, kind, form=f)) for f in (None, CHUNKED, PER_UNIT)}
    monkeypatch.setenv("PYNQS_RBM_CHILDREN_FORM", "1")
    got["env"] = S._bits(cx.rbm_forward_children(onv, par, walkers, W, hb, vb, sorb, kind))
    for k in (CHUNKED, PER_UNIT, "env"):
        assert torch.equal(got[None], got[k]), k
    with pytest.raises(RuntimeError):
        cx.rbm_forward_children(onv, par, walkers, W, hb, vb, sorb, kind, form=2)
    assert (N.CHILDREN_CHUNKED, N.CHILDREN_PER_UNIT) == (CHUNKED, PER_UNIT)
    out = (ctypes.c_int64 * 4)()
    assert N.lib().pynqs_rbm_forward_children_geometry(1 << 30, sorb, H, CC.flavour(kind), out) == 0 and out[2] == out[1] * CC.LDS_GROUP
