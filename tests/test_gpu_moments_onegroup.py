"""pynqs_weighted_moments_form: the single-workgroup form of the weighted moments (one workgroup of 1024 threads plays the waves of the
multi-block form; no ticket, no fence, no read-back) against the multi-block form, both forced through the `form` argument: the four
moments, the blocks' partial sums behind them and the five outputs of the closing arithmetic bit for bit, the ticket word left at zero,
called twice on one workspace.  Sizes: below a wave, a wave, around one and four blocks of 256, the flagship's 8192, and the size at
which pynqs_weighted_moments changes form (and the next one: beyond what the single workgroup holds, it is refused there and the entry
points that choose by n take the blocks).  The entry points that choose by n give the same bits on both sides."""
import pytest
import torch

pytestmark = pytest.mark.gpu

AUTO, BLOCKS, ONEGROUP = 0, 1, 2


def _threshold():
    from pynqs_amd import _native as N

    return int(N.lib().pynqs_moments_onegroup_max())


def _sizes():
    t = _threshold()
    return sorted({1, 63, 64, 255, 256, 257, 1023, 1024, 1025, 8192, t, t + 1})


def _inputs(n, cplx, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(n, generator=g, dtype=torch.float64) + 0.1
    p = p / p.sum()
    x = torch.randn(n, generator=g, dtype=torch.float64) - 100.0
    if cplx:
        x = torch.complex(x, 0.3 * torch.randn(n, generator=g, dtype=torch.float64))
    return x, p


def _call(x, p, form, finish, ws=None):
    from pynqs_amd import _native as N

    dev = x.device
    if ws is None:
        ws = torch.zeros(N.lib().pynqs_moments_workspace() // 8, dtype=torch.float64, device=dev)
    out = torch.zeros(6, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.lib().pynqs_weighted_moments_form(x.data_ptr(), int(x.is_complex()), p.data_ptr(), x.numel(), ws.data_ptr(), 1.0, float(x.numel()),
                                                out.data_ptr() if finish else None, form, st), "pynqs_weighted_moments_form")
    return ws, out


def test_sizes_cover_the_threshold():
    t = _threshold()
    assert 8192 <= t <= 32768 and t in _sizes() and t + 1 in _sizes()


@pytest.mark.parametrize("n", [1, 63, 64, 255, 256, 257, 1023, 1024, 1025, 8192, "threshold", "threshold + 1"])
@pytest.mark.parametrize("cplx", [False, True])
def test_one_workgroup_equals_the_blocks_bit_for_bit(cplx, n):
    from pynqs_amd import _native as N

    t = _threshold()
    n = t if n == "threshold" else t + 1 if n == "threshold + 1" else n
    dev = torch.device("cuda")
    x, p = _inputs(n, cplx, 100 + n)
    xd, pd = x.to(dev), p.to(dev)
    nblocks = min((n + 255) // 256, 128)
    for finish in (False, True):
        want_ws, want_out = _call(xd, pd, BLOCKS, finish)
        ws = None
        if n > 32768:  # more than 128 blocks x 256 threads with one element each
            with pytest.raises(RuntimeError, match="bad form"):
                _call(xd, pd, ONEGROUP, finish)
        for _ in range(2 if n <= 32768 else 0):  # (twice on one workspace: nothing is left behind that the next call trips over)
            ws, out = _call(xd, pd, ONEGROUP, finish, ws)
            got, want = ws.view(torch.int64), want_ws.view(torch.int64)
            assert torch.equal(got[:4], want[:4]), "moments"
            assert torch.equal(got[4:4 * (1 + nblocks)], want[4:4 * (1 + nblocks)]), "the blocks' partial sums"
            assert int(got[4 * 129]) == 0 and int(want[4 * 129]) == 0, "ticket word"
            assert torch.equal(out.view(torch.int64), want_out.view(torch.int64)), "mean, var, sd, se"
        # the same workspace serves the multi-block form afterwards (the ticket is where it expects it)
        ws, out = _call(xd, pd, BLOCKS, finish, ws)
        assert torch.equal(ws.view(torch.int64)[:4], want_ws.view(torch.int64)[:4]) and torch.equal(out.view(torch.int64), want_out.view(torch.int64))
        # the form chosen by n
        ws_a, out_a = _call(xd, pd, AUTO, finish)
        assert torch.equal(ws_a.view(torch.int64)[:4], want_ws.view(torch.int64)[:4]) and torch.equal(out_a.view(torch.int64), want_out.view(torch.int64))
    # the plain entry points
    ws2 = torch.zeros_like(want_ws)
    out2 = torch.zeros(6, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.lib().pynqs_weighted_moments_finish(xd.data_ptr(), int(cplx), pd.data_ptr(), n, ws2.data_ptr(), 1.0, float(n), out2.data_ptr(), st), "finish")
    assert torch.equal(ws2.view(torch.int64)[:4], want_ws.view(torch.int64)[:4]) and torch.equal(out2.view(torch.int64), want_out.view(torch.int64))


def test_the_single_workgroup_form_refuses_what_it_cannot_hold():
    dev = torch.device("cuda")
    x, p = _inputs(32769, False, 1)
    with pytest.raises(RuntimeError, match="bad form"):
        _call(x.to(dev), p.to(dev), ONEGROUP, True)
    xd, pd = x[:32768].to(dev).contiguous(), p[:32768].to(dev).contiguous()  # the largest it takes: four batches per wave
    ws, out = _call(xd, pd, ONEGROUP, True)
    want_ws, want_out = _call(xd, pd, BLOCKS, True)
    assert torch.equal(ws.view(torch.int64), want_ws.view(torch.int64)) and torch.equal(out.view(torch.int64), want_out.view(torch.int64))
