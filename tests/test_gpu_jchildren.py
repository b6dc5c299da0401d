"""pynqs_jastrow_children_prepare + pynqs_jastrow_children_apply behind pynqs_rbm_forward_children, through the C ABI between nan guard
words and through C_extension.jrbm_forward_children, against jrbm_exact.exact_ld (x'^T M x' formed directly from the +-1 rows in
longdouble) under the a-priori per-row bound of tests/jchildren_exact.py: error / bound <= 1 on every row, no row left out, no other
tolerance.  The cases, the bound with its count of roundings and the proof that a dropped pair term, a wrong sign, a neighbour's parent,
a truncated or a clamped stranger could not pass are in tests/jchildren_exact.py and tests/test_jchildren_cases.py.  The apply kernel's
grid is not capped (a thread per row, include/pynqs_amd.h), so there is no sweep to step past."""
import functools

import numpy as np
import pytest
import torch

import children_cases as CC
import jchildren_exact as JC
import jrbm_exact as J
import test_gpu_rbm_exact as T

pytestmark = pytest.mark.gpu

_dev, _onv, _report = T._dev, T._onv, T._report
NAN_BITS = 0x7FF80000DEADBEEF  # the pattern of the buffers a count must leave alone: a quiet nan with a payload
GUARD = 64


@functools.lru_cache(maxsize=2)
def _device(name):
    """the case's inputs on the GPU: (onv, parent, walkers, W, hb, vb, M)"""
    b = JC.build(name)
    W, hb, vb = T.kernel_params(b.rbm, b.case.regime)
    return _onv(b.rows), _dev(b.parent.copy()), _onv(b.parents.copy()), _dev(W), _dev(hb), _dev(vb), _dev(b.M)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _nan(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _rbm(name, parent=None):
    """psi_RBM of the rows from pynqs_rbm_forward_children, as the Jastrow pass finds it"""
    from pynqs_amd import C_extension as cx

    onv, par, walkers, W, hb, vb, _ = _device(name)
    return cx.rbm_forward_children(onv, par if parent is None else parent, walkers, W, hb, vb, JC.case(name).sorb, "real", out=_nan(onv.size(0)))


def _wrapper(name, count=None, out=None, table=None, parent=None):
    from pynqs_amd import C_extension as cx

    onv, par, walkers, W, hb, vb, M = _device(name)
    if out is None:
        out = _nan(onv.size(0))
    return cx.jrbm_forward_children(onv, par if parent is None else parent, walkers, W, hb, vb, M, JC.case(name).sorb, count=count, out=out,
                                    jastrow_table=table)


def _abi(name, psi_rbm, count=None):
    """(raw int64 words [GUARD + n + GUARD], n) of prepare + apply through the C ABI on a copy of psi_rbm between nan guard words; the tables
    are filled with 7.0 beforehand (a stale word read in place of a written one would show)"""
    from pynqs_amd import C_extension as cx, _native as N

    c = JC.case(name)
    onv, par, walkers, _, _, _, M = _device(name)
    n, nw = onv.size(0), walkers.size(0)
    jt = cx.JastrowTable(M)
    nbytes = N.lib().pynqs_jastrow_children_table_bytes(nw, c.sorb)
    assert nbytes == nw * (c.sorb + 1) * 8
    table = torch.full((nbytes // 8 + GUARD,), 7.0, dtype=torch.float64, device="cuda")
    raw = torch.full((n + 2 * GUARD,), NAN_BITS, dtype=torch.int64, device="cuda")
    psi = raw.view(torch.float64)[GUARD:GUARD + n]
    m = n if count is None else min(max(int(count[0]), 0), n)
    psi[:m] = psi_rbm[:m]
    st = torch.cuda.current_stream().cuda_stream
    N.check(N.lib().pynqs_jastrow_children_prepare(walkers.data_ptr(), nw, c.sorb, jt.data_ptr(), table.data_ptr(), st), "pynqs_jastrow_children_prepare")
    N.check(N.lib().pynqs_jastrow_children_apply(onv.data_ptr(), n, None if count is None else count.data_ptr(), par.data_ptr(), walkers.data_ptr(), nw,
                                                 table.data_ptr(), jt.data_ptr(), c.sorb, psi.data_ptr(), st), "pynqs_jastrow_children_apply")
    torch.cuda.synchronize()
    assert bool((table[nbytes // 8:] == 7.0).all()), "prepare wrote past its table"
    return raw, n


def _within_bound(name, what, got):
    b = JC.build(name)
    assert got.shape == (b.n,)
    ratio = b.ratio(got.cpu().numpy())
    c = b.case
    msg = _report(f"{what} {name} ({c.sorb}x{c.H} {c.regime} {c.jregime}, nw {c.nw}, n {b.n})", ratio)
    assert bool((ratio <= 1.0).all()), msg


def _both_routes(name):
    """the C ABI between guard words and the wrapper: the same bits, every row within the bound, the guard words untouched"""
    got = _wrapper(name)
    _within_bound(name, "jastrow children", got)
    raw, n = _abi(name, _rbm(name))
    assert torch.equal(raw[GUARD:GUARD + n], _bits(got)), int((raw[GUARD:GUARD + n] != _bits(got)).sum())
    assert bool((raw[:GUARD] == NAN_BITS).all()) and bool((raw[GUARD + n:] == NAN_BITS).all())
    return got


@pytest.mark.parametrize("name", JC.WORD_CASES + JC.CHUNK_CASES)
def test_word_counts_and_bit_edges(name):
    """one, two and three words, the last bit of a word, flips at every word edge, four in one word and spread over all words; "chunk-50":
    rows the RBM kernel recomputes from scratch.  The no-flip child: psi = psi_RBM exp(q0), Delta exactly 0 -- the bits of the product of
    the RBM kernel's value with exp of the parent's own q0, which the same kernels give for a list of the parents themselves"""
    from pynqs_amd import C_extension as cx

    got = _both_routes(name)
    b = JC.build(name)
    onv, par, walkers, W, hb, vb, M = _device(name)
    same = np.flatnonzero((b.nflip == 0) & (b.stranger == 0))
    assert same.size >= 1
    # the parents as their own children, each named by its own index, and then by rows in another order: Delta = 0 either way
    nw = walkers.size(0)
    own = cx.jrbm_forward_children(walkers, torch.arange(nw, dtype=torch.int32, device="cuda"), walkers, W, hb, vb, M, b.case.sorb, out=_nan(nw))
    want = own[_dev(b.parent[same].astype(np.int64))]
    assert torch.equal(_bits(got[_dev(same)]), _bits(want))


@pytest.mark.parametrize("name", JC.ROW_CASES)
def test_row_counts_around_the_wave_and_the_workgroup(name):
    _both_routes(name)


@pytest.mark.parametrize("name", JC.PARENT_CASES)
def test_many_parents_in_both_orders(name):
    _both_routes(name)


@pytest.mark.parametrize("name", JC.STRANGER_CASES)
def test_strangers_lane_by_lane(name):
    """parents -1, nw, nw + 5 and rows 5, 6 and sorb flips away from the parent they name, in whole waves, in the first, a middle and the
    last lane: every row within the bound; the rows that are no strangers carry the bits they have without any stranger around"""
    got = _both_routes(name)
    b = JC.build(name)
    named = _dev(np.where(b.stranger != 0, b.true_parent, b.parent).astype(np.int32))
    clean = _wrapper(name, parent=named)
    keep = _dev(b.stranger == 0)
    assert torch.equal(_bits(clean[keep]), _bits(got[keep]))


def test_the_device_count_at_every_edge():
    """count_dev at 0, 1, 63, 64, 65, n - 1, n and n + 5 in a nan-filled psi: rows below the count carry the bits of the full run, rows at
    and past the count and the guard words keep their bits -- through the C ABI and through the wrapper"""
    name = JC.COUNT_CASE
    full = _wrapper(name)
    _within_bound(name, "jastrow children (no count)", full)
    psi_rbm = _rbm(name)
    n = full.size(0)
    bad = []
    for v in (-3, 0, 1, 63, 64, 65, JC.WORKGROUP, n - 1, n, n + 5):
        cnt = min(max(v, 0), n)
        count = torch.tensor([v, 0, 0, 0], dtype=torch.int32, device="cuda")
        raw, _ = _abi(name, psi_rbm, count=count)
        raw2 = torch.full((n + 2 * GUARD,), NAN_BITS, dtype=torch.int64, device="cuda")
        _wrapper(name, count=count, out=raw2.view(torch.float64)[GUARD:GUARD + n])
        torch.cuda.synchronize()
        for what, r in (("abi", raw), ("wrapper", raw2)):
            if not torch.equal(r[GUARD:GUARD + cnt], _bits(full[:cnt])):
                bad.append((v, what, "rows below the count"))
            if not (bool((r[:GUARD] == NAN_BITS).all()) and bool((r[GUARD + cnt:] == NAN_BITS).all())):
                bad.append((v, what, "rows from the count on / guard words"))
    assert not bad, bad


def test_exact_identities():
    """M = 0 returns the bits of rbm_forward_children (exp(0) = 1, the product by 1 is exact); a purely diagonal M multiplies every row by
    exp(tr M) within the bound"""
    zero = _wrapper("zero")
    assert torch.equal(_bits(zero), _bits(_rbm("zero")))
    _within_bound("zero", "jastrow children", zero)
    diag = _both_routes("diag")
    b = JC.build("diag")
    f = (diag / _rbm("diag")).cpu().numpy()
    assert np.abs(f / np.exp(np.trace(b.M)) - 1).max() <= float((b.bound / J.U).max()) * J.U


@pytest.mark.parametrize("name", ["sorb66", "strangers-three-words", "chunk-50"])
def test_reproducible_and_in_step_with_the_from_scratch_kernel(name):
    """two calls give the same bits (a reused JastrowTable too), and the result agrees with jrbm_forward on the same rows within the sum of
    the two bounds"""
    from pynqs_amd import C_extension as cx

    b = JC.build(name)
    onv, _, _, W, hb, vb, M = _device(name)
    a1 = _wrapper(name)
    a2 = _wrapper(name, table=cx.JastrowTable(M))
    assert torch.equal(_bits(a1), _bits(a2))
    scratch = cx.jrbm_forward(onv, W, hb, vb, M, b.case.sorb).cpu().numpy()
    r2 = J.amp_ratio(b.rbm, b.M, scratch, b.ex)
    assert bool((r2 <= 1.0).all()), _report(f"jrbm_forward {name}", r2)
    both = b.bound + J.amp_bound(b.rbm, b.M, b.ex.cond)
    rel = np.abs(a1.cpu().numpy() / scratch - 1)
    assert bool((rel <= both * (1 + 1e-9)).all()), float((rel / both).max())
