"""pynqs_rbm_forward_children where its control flow depends on the sizes, against the exact reference of tests/rbm_exact.py under the
a-priori bound |psi / psi_exact - 1| <= u (sorb + H + 16) cond(x) per row (rbm_exact.amp_ratio <= 1, no row left out, no other
tolerance): a second sweep of the capped, strided grid in both forms (the LDS form's is where the headline workload lives), the last
workgroup with one row and the last group of sixteen with five, factor tables at the edge of the LDS, every flavour across several
workgroups, 1 to 5000 parents in both orders, the device count at every edge, strangers placed lane by lane, the raised flag over two
rounds, and the front end's own list.  The cases, their reference and the proof that a wrapped index, a neighbour's parent, a truncated
or a clamped stranger could not pass are in tests/children_cases.py and tests/test_children_cases.py; every sweep size is asked of the
library (pynqs_rbm_forward_children_geometry), so a changed cap moves the cases with it."""
import functools

import numpy as np
import pytest
import torch

import children_cases as CC
import rbm_exact as R
import test_gpu_rbm_exact as T

pytestmark = pytest.mark.gpu

_dev, _onv, _report = T._dev, T._onv, T._report
NAN_BITS = 0x7FF80000DEADBEEF  # the pattern of the buffers a count must leave alone: a quiet nan with a payload
GUARD = 64


@functools.lru_cache(maxsize=2)
def _device(name):
    """the case's inputs on the GPU: (onv, parent, walkers, W, hb, vb)"""
    b = CC.build(name)
    W, hb, vb = T.kernel_params(b.rbm, b.case.regime)
    # (copies: the builder's arrays are read-only, shared by the tests)
    return _onv(b.rows), _dev(b.parent.copy()), _onv(b.parents.copy()), _dev(W), _dev(hb), None if vb is None else _dev(vb)


def _bits(t):
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int64)


def _stamped(name, count=None, out=None):
    from pynqs_amd import C_extension as cx

    c = CC.case(name)
    onv, par, walkers, W, hb, vb = _device(name)
    if out is None:  # (nan, not torch.empty: a row the kernel skipped must not inherit an earlier call's value from the allocator)
        out = _nan(onv.size(0), c.kind)
    return cx.rbm_forward_children(onv, par, walkers, W, hb, vb, c.sorb, c.kind, count=count, out=out)


def _nan(n, kind):
    return torch.full((n,), float("nan"), dtype=torch.float64 if kind in ("real", "tanh") else torch.complex128, device="cuda")


def _unstamped(name):
    """(psi, flag word) of pynqs_rbm_children_prepare + pynqs_rbm_forward_children through the C ABI"""
    from pynqs_amd import _native as N

    c = CC.case(name)
    onv, par, walkers, W, hb, vb = _device(name)
    flav, n, nw = CC.flavour(c.kind), onv.size(0), walkers.size(0)
    table = torch.full((N.lib().pynqs_rbm_children_table_bytes(nw, c.sorb, c.H, flav) // 8,), 7.0, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    vbp = None if vb is None else vb.data_ptr()
    N.check(N.lib().pynqs_rbm_children_prepare(walkers.data_ptr(), nw, c.sorb, W.data_ptr(), hb.data_ptr(), vbp, c.H, flav, table.data_ptr(), st),
            "pynqs_rbm_children_prepare")
    psi = _nan(n, c.kind)
    N.check(N.lib().pynqs_rbm_forward_children(onv.data_ptr(), n, None, par.data_ptr(), walkers.data_ptr(), nw, table.data_ptr(), c.sorb, W.data_ptr(),
                                               hb.data_ptr(), vbp, c.H, flav, psi.data_ptr(), st), "pynqs_rbm_forward_children")
    torch.cuda.synchronize()
    return psi, float(table[-1])


def _forward(name):
    from pynqs_amd import C_extension as cx

    c = CC.case(name)
    onv, _, _, W, hb, vb = _device(name)
    return cx.rbm_forward(onv, W, hb, vb, c.sorb, c.kind)


def _within_bound(name, what, got):
    b = CC.build(name)
    assert got.shape == (b.n,)
    ratio = R.amp_ratio(b.rbm, got.cpu().numpy(), b.exact())
    msg = _report(f"{what} {name} ({b.case.kind} {b.case.sorb}x{b.case.H} {b.case.regime}, nw {b.case.nw}, n {b.n})", ratio)
    assert bool((ratio <= 1.0).all()), msg


@pytest.mark.parametrize("name", CC.SHAPE_CASES)
def test_every_row_meets_the_rounding_bound(name):
    _within_bound(name, "children", _stamped(name))
    _within_bound(name, "forward on the children", _forward(name))  # the plain forward on the same rows, under the same bound


@pytest.mark.parametrize("name", CC.PARENT_CASES)
def test_many_parents_in_both_orders(name):
    """1, 257 and 5000 parents (the last one in use), the rows shuffled or in runs per parent: every row within the bound, and the two-launch
    prepare + plain entry give the bits of the one-launch stamped pair the wrapper uses"""
    got = _stamped(name)
    _within_bound(name, "children", got)
    plain, flag = _unstamped(name)
    assert flag == 0.0 and torch.equal(_bits(plain), _bits(got))
    _within_bound(name, "forward on the children", _forward(name))


@pytest.mark.parametrize("name", CC.COUNT_CASES)
def test_the_device_count_at_every_edge(name):
    """count_dev around 0, the wave, the workgroup, the sweep and n: the rows below the count carry the bits of the full run (which is held
    to the bound here), the rows from the count on and the guard words on both sides keep their bits"""
    b = CC.build(name)
    n, sweep = b.n, CC.sweep_of(b.case, b.n)
    full = _stamped(name)
    _within_bound(name, "children (no count)", full)
    cplx = full.is_complex()
    values = sorted({v for v in (-3, 0, 1, 63, 64, 65, 1023, 1024, 1025, sweep - 1, sweep, sweep + 1, n - 1, n, n + 5) if v <= n + 5})
    assert {-3, 0, 1, 1025, n - 1, n, n + 5} <= set(values) and (n <= sweep or {sweep - 1, sweep, sweep + 1} <= set(values))
    C = 2 if cplx else 1
    bad = []
    for v in values:
        raw = torch.full(((n + 2 * GUARD) * C,), NAN_BITS, dtype=torch.int64, device="cuda")
        buf = torch.view_as_complex(raw.view(torch.float64).view(-1, 2)) if cplx else raw.view(torch.float64)
        out = buf[GUARD:GUARD + n]
        _stamped(name, count=torch.tensor([v, 0, 0, 0], dtype=torch.int32, device="cuda"), out=out)
        torch.cuda.synchronize()
        cnt = min(max(v, 0), n)
        lo, hi = GUARD * C, (GUARD + cnt) * C
        if not torch.equal(raw[lo:hi], _bits(full[:cnt]).view(-1)):
            bad.append((v, "rows below the count", int((raw[lo:hi] != _bits(full[:cnt]).view(-1)).sum())))
        if not (bool((raw[:lo] == NAN_BITS).all()) and bool((raw[hi:] == NAN_BITS).all())):
            bad.append((v, "rows from the count on / guard words", int((raw[:lo] != NAN_BITS).sum()) + int((raw[hi:] != NAN_BITS).sum())))
    assert not bad, bad


@pytest.mark.parametrize("name", CC.RAISED_CASES)
def test_the_raised_flag_over_two_rounds(name):
    """one parent out of range (tests/test_children_cases.py): every row from scratch, in two rounds of a thread per row -- pynqs_rbm_forward's
    bits, as include/pynqs_amd.h says, stamped and unstamped, and within the bound"""
    want = _forward(name)
    got = _stamped(name)
    assert torch.equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())
    plain, flag = _unstamped(name)
    assert flag == 1.0
    assert torch.equal(_bits(plain), _bits(want)), int((_bits(plain) != _bits(want)).sum())
    _within_bound(name, "children from scratch", got)


@pytest.mark.parametrize("name", CC.STRANGER_CASES)
def test_strangers_lane_by_lane(name):
    """parents -1, nw, nw + 5 and rows 5, 6 and sorb flips away from the parent they name, in whole waves / groups, in the first, a middle
    and the last lane, alone in the last workgroup: every row, stranger or not, within the bound; the rows that are no strangers carry the
    bits they have without any stranger around"""
    b = CC.build(name)
    got = _stamped(name)
    _within_bound(name, "children", got)
    plain, _ = _unstamped(name)
    assert torch.equal(_bits(plain), _bits(got))
    from pynqs_amd import C_extension as cx

    onv, par, walkers, W, hb, vb = _device(name)
    named = _dev(np.where(b.stranger != 0, b.pool_parent[b.idx], b.parent).astype(np.int32))  # index strangers get their true parent back
    clean = cx.rbm_forward_children(onv, named, walkers, W, hb, vb, b.case.sorb, b.case.kind, out=_nan(b.n, b.case.kind))
    keep = _dev(b.stranger == 0)
    assert torch.equal(_bits(clean[keep]), _bits(got[keep]))


@pytest.mark.parametrize("kind,H,regime", [("complex", 9, "fe2s2"), ("real", 7, "small")])
def test_the_front_ends_own_list(kind, H, regime):
    """the distinct x' of a REDUCE front end on 96 walkers (0.31 M rows), through count = its counters and its full-capacity buffers: every
    distinct row within the bound, the tail untouched.  (Few hidden units: the host reference of that many rows is the cost of the test.)"""
    import bench as B
    from pynqs_amd import C_extension as cx, energy as E

    dev = torch.device("cuda")
    sorb, no, n = 40, 15, 96
    x = B.synth_walkers(n, sorb, no, no, 3).to(dev)
    h1, h2 = B.synth_integrals(sorb)
    fe, nu = E.reduce_front(x, h1.to(dev), h2.to(dev), sorb, 2 * no, no, no, 0.3, 40, None, seed=5, pm1_dtype=torch.float64)
    assert n < nu < fe.cap_unique and int(fe.counters[0]) == nu
    words = np.ascontiguousarray(fe.uniq_onv[:nu].cpu().numpy()).view(np.uint64).reshape(nu, -1)
    rbm, _, ex = R.checked_case(kind, sorb, H, regime, words)
    W, hb, vb = (_dev(a) for a in T.kernel_params(rbm, regime))
    cplx = kind == "complex"
    C = 2 if cplx else 1
    raw = torch.full((fe.cap_unique * C,), NAN_BITS, dtype=torch.int64, device=dev)
    out = torch.view_as_complex(raw.view(torch.float64).view(-1, 2)) if cplx else raw.view(torch.float64)
    cx.rbm_forward_children(fe.uniq_onv, fe.uniq_parent, x, W, hb, vb, sorb, kind, count=fe.counters, out=out)
    torch.cuda.synchronize()
    assert bool((raw[nu * C:] == NAN_BITS).all())
    ratio = R.amp_ratio(rbm, out[:nu].cpu().numpy(), ex)
    msg = _report(f"children front-end-list ({kind} {sorb}x{H} {regime}, nw {n}, n {nu})", ratio)
    assert bool((ratio <= 1.0).all()), msg
