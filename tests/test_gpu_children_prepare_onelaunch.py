"""pynqs_rbm_children_prepare_stamped: the table of pynqs_rbm_forward_children from ONE launch (parent chunks, sums blocks and factor blocks in
one grid) against the two-launch pynqs_rbm_children_prepare, bit for bit -- parents and factors -- and the per-call stamp that replaces the
"reset, then maybe raised" flag: a stamp of the call is read as raised, a stale one of an earlier call into the same buffer is not."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(6, 3), (40, 40), (70, 5), (130, 5)]  # one, two and three words; H % 4 != 0: the tail of the last chunk of four hidden units


def _params(kind, sorb, H, dev, seed, with_vb=True):
    g = torch.Generator().manual_seed(seed)
    c = (2,) if kind == "complex" else ()
    r = lambda *s: (torch.rand(*s, *c, generator=g, dtype=torch.float64) - 0.5)  # noqa: E731
    W, hb, vb = 0.3 * r(H, sorb), 0.4 * r(H), 0.2 * r(sorb)
    return W.to(dev), hb.to(dev), (vb.to(dev) if with_vb else None)


def _walkers(n, sorb, seed):
    import bench as B

    no = max(1, sorb // 4)
    return B.synth_walkers(n, sorb, no, no, seed)


def _prepare(kind, x, sorb, W, hb, vb, stamp, table=None, fill=7.0):
    """(table, parents part, factors part, flag word): stamp None = the two launches"""
    from pynqs_amd import _native as N

    flav = N.RBM_COMPLEX if kind == "complex" else N.RBM_REAL
    H, nw, C = W.size(0), x.size(0), 2 if kind == "complex" else 1
    nbytes = N.lib().pynqs_rbm_children_table_bytes(nw, sorb, H, flav)
    if table is None:
        table = torch.full((nbytes // 8,), fill, dtype=torch.float64, device=x.device)
    st = torch.cuda.current_stream(x.device).cuda_stream
    vbp = vb.data_ptr() if vb is not None else None
    if stamp is None:
        N.check(N.lib().pynqs_rbm_children_prepare(x.data_ptr(), nw, sorb, W.data_ptr(), hb.data_ptr(), vbp, H, flav, table.data_ptr(), st), "prepare")
    else:
        N.check(N.lib().pynqs_rbm_children_prepare_stamped(x.data_ptr(), nw, sorb, W.data_ptr(), hb.data_ptr(), vbp, H, flav, stamp, table.data_ptr(), st),
                "prepare_stamped")
    npar = nw * (H + 2) * C
    return table, table[:npar], table[npar:-1], table[-1:]


def _bits(t):
    return t.view(torch.int64)


@pytest.mark.parametrize("nw", [1, 255, 256, 257])
@pytest.mark.parametrize("sorb,H", SHAPES)
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_one_launch_table_is_bitwise_the_two_launch_table(kind, sorb, H, nw):
    dev = torch.device("cuda")
    x = _walkers(nw, sorb, 3).to(dev)
    for with_vb in (True, False):
        W, hb, vb = _params(kind, sorb, H, dev, 11, with_vb)
        _, par2, fac2, flag2 = _prepare(kind, x, sorb, W, hb, vb, None)
        _, par1, fac1, flag1 = _prepare(kind, x, sorb, W, hb, vb, 5)
        assert torch.equal(_bits(fac1), _bits(fac2)), "factor table"
        assert torch.equal(_bits(par1), _bits(par2)), "parents (q_h, sum_h theta_h, a.x)"
        assert bool(torch.isfinite(par1).all()) and not bool((fac1 == 7.0).all())
        # ordinary parameters: the two-launch form resets the flag, the one-launch form leaves the word alone
        assert float(flag2) == 0.0 and float(flag1) == 7.0


def _children(kind, rows, par, x, sorb, W, hb, vb, table, stamp):
    from pynqs_amd import _native as N

    flav = N.RBM_COMPLEX if kind == "complex" else N.RBM_REAL
    n = rows.size(0)
    psi = torch.zeros(n, dtype=torch.complex128 if kind == "complex" else torch.float64, device=x.device)
    N.check(N.lib().pynqs_rbm_forward_children_stamped(rows.data_ptr(), n, None, par.data_ptr(), x.data_ptr(), x.size(0), table.data_ptr(), sorb,
                                                       W.data_ptr(), hb.data_ptr(), vb.data_ptr(), W.size(0), flav, stamp, psi.data_ptr(),
                                                       torch.cuda.current_stream(x.device).cuda_stream), "forward_children_stamped")
    return psi


@pytest.mark.parametrize("kind", ["real", "complex"])
def test_a_stale_stamp_is_not_current_and_a_current_one_is(kind):
    """Two calls into the SAME table buffer.  Call 1 (stamp 41): a hidden unit with Re theta_h < -340 on every parent -- the flag word takes
    the stamp and the children are pynqs_rbm_forward's from scratch, bit for bit.  Call 2 (stamp 42), ordinary parameters: the word still
    holds 41, the children take the table path and agree with pynqs_rbm_forward within twice its rounding bound
    2^-53 (sorb + H + 16) cond (include/pynqs_amd.h; cond <= 1 + sum_h (|b_h| + sum_o |W_ho|) + sum_o |a_o| as |tanh| <= 1).  Reading the
    same table with the stale stamp 41 sends the rows from scratch instead: the comparison, not the word's being non-zero, decides."""
    import rbm_exact as R
    from pynqs_amd import C_extension as cx

    dev = torch.device("cuda")
    sorb, H, nw = 12, 5, 24
    x = _walkers(nw, sorb, 9)
    L = x.size(1) // 8
    rows_np, par_np, _ = R.make_children(x.numpy().view(np.uint64).reshape(nw, L), sorb, 2)
    rows = torch.from_numpy(rows_np.view(np.uint8).reshape(-1, 8 * L)).to(dev)
    par = torch.from_numpy(par_np).to(dev)
    x = x.to(dev)
    W, hb, vb = _params(kind, sorb, H, dev, 21)
    hb_low = hb.clone()
    hb_low.view(-1)[0] = -400.0  # Re b_0: theta_0 <= -400 + sum_o |W_0o| < -340 for every walker
    table, _, _, flag = _prepare(kind, x, sorb, W, hb_low, vb, 41)
    assert float(flag) == 41.0
    got = _children(kind, rows, par, x, sorb, W, hb_low, vb, table, 41)
    want = cx.rbm_forward(rows, W, hb_low, vb, sorb, kind)
    assert bool(torch.isfinite(torch.view_as_real(want) if want.is_complex() else want).all())
    assert torch.equal(torch.view_as_real(got) if got.is_complex() else got, torch.view_as_real(want) if want.is_complex() else want)
    # the second call, same buffer
    _prepare(kind, x, sorb, W, hb, vb, 42, table=table)
    assert float(flag) == 41.0  # stale
    got2 = _children(kind, rows, par, x, sorb, W, hb, vb, table, 42)
    want2 = cx.rbm_forward(rows, W, hb, vb, sorb, kind)
    mod = lambda t: (t.abs().reshape(t.size(0), -1).sum(1) if t.dim() > 1 else t.abs())  # noqa: E731  (|re| + |im| >= |z|)
    cond = 1.0 + float((mod(hb.reshape(H, -1)) + W.abs().reshape(H, -1).sum(1)).sum()) + float(vb.abs().sum())
    bound = 2.0 * 2.0**-53 * (sorb + H + 16) * cond
    rel = float(((got2 - want2).abs() / want2.abs()).max())
    print(f"table path against from scratch: {rel:.2e} (bound {bound:.2e})")
    assert rel <= bound
    assert not torch.equal(torch.view_as_real(got2) if got2.is_complex() else got2, torch.view_as_real(want2) if want2.is_complex() else want2), \
        "the table path rounds differently from the from-scratch path on some row: identical bits mean it was not taken"
    stale = _children(kind, rows, par, x, sorb, W, hb, vb, table, 41)  # the word equals THIS stamp: every row from scratch
    assert torch.equal(torch.view_as_real(stale) if stale.is_complex() else stale, torch.view_as_real(want2) if want2.is_complex() else want2)


def test_the_python_entry_point_stamps_every_call():
    from pynqs_amd import C_extension as cx

    a, b = next(cx._CHILDREN_STAMP), next(cx._CHILDREN_STAMP)
    assert 1 <= a < b
