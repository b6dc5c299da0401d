"""pynqs_weighted_moments_finish: the weighted moments AND the closing arithmetic of the statistics in one launch (one rank) against
pynqs_weighted_moments followed by pynqs_stats_finish, bit for bit, and both against a numpy longdouble evaluation.

Bounds (u = 2^-52, n terms, fixed-order float64 sums): a sum of n products errs by at most n u sum |terms|, so with S1 = sum p |x|,
S2 = sum p |x|^2, P = sum p:  sum p Re x, sum p Im x: n u S1;  sum p |x|^2: n u S2;  sum p: n u P.  var = m2 - |mean|^2 (2 - P) with
|mean| <= S1 and 2 - P <= 2:  n u (S2 + 8 S1^2)  (m2's n u S2; |mean|^2 errs by 2 sqrt(2) |mean| n u S1, times 2; P's error times
|mean|^2 <= S1^2 for P <= 1)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# 1, 63, 64: less than a wave, a wave; 257: two blocks; 8192: the flagship's; 40000: beyond 128 blocks x 256 threads, the grid-stride loop
SIZES = [1, 63, 64, 257, 8192, 40000]


def _inputs(n, cplx, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(n, generator=g, dtype=torch.float64) + 0.1
    p = p / p.sum()
    x = torch.randn(n, generator=g, dtype=torch.float64) - 100.0
    if cplx:
        x = torch.complex(x, 0.3 * torch.randn(n, generator=g, dtype=torch.float64))
    return x, p


def _two_launches(x, p, counts):
    from pynqs_amd import _native as N

    dev = x.device
    ws = torch.zeros(N.lib().pynqs_moments_workspace() // 8, dtype=torch.float64, device=dev)
    out = torch.zeros(6, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.lib().pynqs_weighted_moments(x.data_ptr(), int(x.is_complex()), p.data_ptr(), x.numel(), ws.data_ptr(), st), "moments")
    N.check(N.lib().pynqs_stats_finish(ws.data_ptr(), 1.0, float(counts), out.data_ptr(), st), "finish")
    return ws[:4].clone(), out[:5].clone()


def _one_launch(x, p, counts):
    from pynqs_amd import _native as N

    dev = x.device
    ws = torch.zeros(N.lib().pynqs_moments_workspace() // 8, dtype=torch.float64, device=dev)
    out = torch.zeros(6, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for _ in range(2):  # (twice: the ticket counter must be back at zero after a call)
        N.check(N.lib().pynqs_weighted_moments_finish(x.data_ptr(), int(x.is_complex()), p.data_ptr(), x.numel(), ws.data_ptr(), 1.0, float(counts),
                                                      out.data_ptr(), st), "moments_finish")
    return ws[:4].clone(), out[:5].clone()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cplx", [False, True])
def test_one_launch_equals_two_launches_and_the_longdouble_sums(cplx, n):
    dev = torch.device("cuda")
    x, p = _inputs(n, cplx, 100 + n)
    xd, pd = x.to(dev), p.to(dev)
    m2l, o2l = _two_launches(xd, pd, n)
    m1l, o1l = _one_launch(xd, pd, n)
    assert torch.equal(m1l.view(torch.int64), m2l.view(torch.int64)), "moments"
    assert torch.equal(o1l.view(torch.int64), o2l.view(torch.int64)), "mean, var, sd, se"
    ld = np.longdouble
    xr, xi, pl = x.real.numpy().astype(ld), (x.imag.numpy() if cplx else np.zeros(n)).astype(ld), p.numpy().astype(ld)
    ax2 = xr * xr + xi * xi
    S1, S2, P = float((pl * np.sqrt(ax2)).sum()), float((pl * ax2).sum()), float(pl.sum())
    want_m = np.array([(pl * xr).sum(), (pl * xi).sum(), (pl * ax2).sum(), pl.sum()], dtype=ld)
    u = n * 2.0**-52
    tol_m = np.array([u * S1, u * S1, u * S2, u * P])
    err_m = np.abs(m1l.cpu().numpy().astype(ld) - want_m).astype(np.float64)
    print(f"n={n} cplx={cplx}: moment errors {err_m} (bounds {tol_m})")
    assert (err_m <= tol_m).all()
    want_var = max(want_m[2] - (want_m[0] ** 2 + want_m[1] ** 2) * (2 - want_m[3]), ld(0))
    o = o1l.cpu().numpy()
    assert abs(float(o[0] - want_m[0])) <= u * S1 and abs(float(o[1] - want_m[1])) <= u * S1
    assert abs(float(o[2] - want_var)) <= u * (S2 + 8.0 * S1 * S1)
    # sd = sqrt(var), se = sd / sqrt(n): one rounding, then two more
    assert abs(o[3] - np.sqrt(o[2])) <= 2.0**-52 * o[3] and abs(o[4] - o[3] / np.sqrt(float(n))) <= 2.0**-51 * o[4]


@pytest.mark.parametrize("cplx", [False, True])
def test_dist_stats_moments_takes_the_one_launch_form_on_one_rank(cplx):
    from pynqs_amd import stats

    dev = torch.device("cuda")
    n = 777
    x, p = _inputs(n, cplx, 5)
    xd, pd = x.to(dev), p.to(dev)
    mean, var, sd, se = stats.dist_stats_moments(xd, pd, None, 1)
    _, o = _two_launches(xd, pd, n)
    got = torch.stack([mean.real if cplx else mean, mean.imag if cplx else torch.zeros_like(var), var, sd, se])
    assert torch.equal(got.view(torch.int64), o.view(torch.int64))
    assert mean.is_complex() == cplx
