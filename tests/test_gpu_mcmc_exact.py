"""The many-chain Metropolis kernels against the accept rule evaluated exactly (include/pynqs_amd.h, "many-chain Metropolis sampling";
tests/mcmc_replay.py):
 (i) every step of the fused kernel pynqs_mcmc_rbm, replayed from its own records with proposals of the CPU oracle and ln|psi| from
     the float64 parameters in longdouble / mpmath, for every flavour, 1-3 ONV words, 1-64 lanes per chain, the table in LDS and in L2,
     and parameter regimes where the kernel's special cases run (|Re theta| past the 1e-290 switch and the exp underflow, Re theta
     changing sign or exactly 0, |q| = 1, imaginary parts in the hundreds); 4096-step launches through the C ABI; a chain that starts
     at amplitude zero;
 (ii) the generic step pynqs_mcmc_accept on hand-made amplitudes (zero, subnormal, 1e+-200, the largest double, non-finite), decided
     in exact rational arithmetic, and fused against generic where the squares of the amplitudes leave the range of a double.
Every seed is fixed.  The replay cases print one line each (steps, ties, max |lnpsi - exact| / tau, lanes, table place, words)."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch
from torch import nn

import mcmc_replay as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from oracle import oracle
    from pynqs_amd import C_extension, _native, mcmc, rbm

    assert torch.cuda.is_available()
    assert np.finfo(np.longdouble).eps < 1e-18, "the replay needs an extended longdouble"
    return C_extension, mcmc, rbm, _native, oracle


class Opaque(nn.Module):
    """The same amplitude behind a module the sampler does not recognise as an RBM: the generic path."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner(x)


def first_det(sorb, noA, noB):
    """uint64 [1, len] words of the determinant with the lowest alpha and beta orbitals occupied."""
    w = np.zeros((1, (sorb - 1) // 64 + 1), dtype=np.uint64)
    for o in list(range(0, 2 * noA, 2)) + list(range(1, 2 * noB, 2)):
        w[0, o // 64] |= np.uint64(1) << np.uint64(o % 64)
    return w


# ---- parameters of the regimes ---------------------------------------------------------------------------------------------------------
# typical: uniform in +-scale / 2.  saturated: NPAIR pairs of hidden units theta = S + h, S - h with S = w.x of large weights (spread 150
# over the states) and h = 330: |theta| + |theta'| is constant while |S| < h, so the chains wander there while |Re theta| of these units
# travels between 0 and 660 (past the 1e-290 switch at ~334 and the exp(-2 |theta|) underflow at ~372), and may change sign where
# |S| > h.  churn: no hidden bias and integer weights +-1..3 (Re theta changes sign on most moves and is exactly 0 on some).  cos: the
# cos flavour (Re theta = 0, |q| = 1), hidden biases up to +-1.5.  imag: complex with imaginary parts of theta in the hundreds.
# return: hidden unit 0 has theta_0 = 202 + 100 (x_6 - x_0) in {2, 202, 402} (visible biases cancel its slope), so that it falls from
# past the exp(-2 |theta|) underflow back to 2 without a sign change -- through 202, as one move 402 -> 2 would need exp(+-4 W) products
# beyond the range of a double; there q = 0 must be recomputed, not carried on as 0 * E.
NPAIR = 2
RETURN_W, RETURN_C = 100.0, 202.0


def _random_dets(g, n, sorb, noA, noB):
    x = -np.ones((n, sorb))
    for i in range(n):
        x[i, 2 * g.permutation(sorb // 2)[:noA]] = 1.0
        x[i, 2 * g.permutation(sorb // 2)[:noB] + 1] = 1.0
    return x


def make_params(kind, regime, sorb, H, seed, noA=0, noB=0):
    g = np.random.default_rng(seed)
    U = lambda s, *shape: s * (g.random(shape) - 0.5)  # noqa: E731
    sc = 1.0 if sorb <= 40 else 0.5
    if regime == "churn":
        W = g.integers(1, 4, (H, sorb)) * g.choice([-1.0, 1.0], (H, sorb))
        return W.astype(np.float64), np.zeros(H), U(1.0, sorb)
    if regime == "saturated":
        W, hb, vb = U(sc, H, sorb), U(sc, H), U(sc, sorb)
        x = _random_dets(g, 2000, sorb, noA, noB)
        for p in range(NPAIR):
            w = U(1.0, sorb)
            S = x @ w
            w = w * (150.0 / S.std())
            W[2 * p] = W[2 * p + 1] = w
            hb[2 * p], hb[2 * p + 1] = 330.0 - (x @ w).mean(), -330.0 - (x @ w).mean()
        if kind == "complex":
            return W + 1j * U(sc, H, sorb), hb + 1j * U(sc, H), vb + 1j * U(sc, sorb)
        return W, hb, vb
    if regime == "return":
        W, hb, vb = U(sc, H, sorb), U(sc, H), U(sc, sorb)
        W[0] = 0.0
        W[0, 0], W[0, 6], hb[0] = -RETURN_W, RETURN_W, RETURN_C
        vb[0], vb[6] = RETURN_W, -RETURN_W
        if kind == "complex":
            return W + 1j * U(sc, H, sorb), hb + 1j * U(sc, H), vb + 1j * U(sc, sorb)
        return W, hb, vb
    if regime == "imag":
        return (U(sc, H, sorb) + 1j * U(60.0, H, sorb), U(sc, H) + 1j * U(600.0, H), U(sc, sorb) + 1j * U(sc, sorb))
    if regime == "cos":
        return U(1.0, H, sorb), U(3.0, H), np.zeros(sorb)
    if kind == "complex":
        return U(sc, H, sorb) + 1j * U(sc, H, sorb), U(sc, H) + 1j * U(sc, H), U(sc, sorb) + 1j * U(sc, sorb)
    return U(sc, H, sorb), U(sc, H), U(4.0 * sc if kind == "tanh" else sc, sorb)


def module_of(rbm, kind, W, hb, vb):
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    if kind == "complex":
        pair = lambda a: T(np.stack([a.real, a.imag], -1))  # noqa: E731
        return rbm.ComplexRBM(pair(W), pair(hb), pair(vb)).cuda()
    return rbm.RealRBM(T(W), T(hb), T(vb), kind).cuda()


def table_of(cx, kind, W, hb, vb):
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    if kind in ("complex", "cos"):
        if kind == "cos":  # (the complex parameters i W, i b the sampler hands the kernel for cos)
            W, hb, vb = 1j * W, 1j * hb, None
        pair = lambda a: T(np.stack([a.real, a.imag], -1))  # noqa: E731
        return cx.CRBMTable(pair(W), pair(hb), pair(vb) if vb is not None else None)
    return cx.RBMTable(T(W), T(hb), T(vb))


#        id                  kind       sorb noA noB  H   regime       chains steps
CASES = [("real-12-8",       "real",     12, 3, 3,   8, "typical",    256, 256),
         ("tanh-12-9",       "tanh",     12, 3, 3,   9, "typical",    256, 256),
         ("complex-12-1",    "complex",  12, 3, 3,   1, "typical",    256, 256),
         ("cos-12-64",       "cos",      12, 3, 3,  64, "cos",        128, 256),
         ("real-40-64",      "real",     40, 5, 5,  64, "typical",     64, 256),
         ("real-40-65",      "real",     40, 5, 5,  65, "typical",     64, 256),
         ("complex-40-32",   "complex",  40, 5, 5,  32, "imag",        64, 256),
         ("complex-40-33",   "complex",  40, 5, 5,  33, "imag",        64, 256),
         ("real-66-16-sat",  "real",     66, 3, 3,  16, "saturated",  128, 256),
         ("complex-12-9-sat", "complex", 12, 3, 3,   9, "saturated",  256, 256),
         ("real-24-16-sat",  "real",     24, 3, 3,  16, "saturated",  128, 256),
         ("real-8-8-return", "real",      8, 2, 2,   8, "return",     256, 256),
         ("complex-8-9-return", "complex", 8, 2, 2,  9, "return",     256, 256),
         ("real-40-16-churn", "real",    40, 5, 5,  16, "churn",      128, 256),
         ("tanh-66-24",      "tanh",     66, 4, 4,  24, "typical",     64, 256),
         ("pRBM-130-65",     "pRBM",    130, 2, 3,  65, "typical",     64, 256),
         ("complex-130-40",  "complex", 130, 3, 2,  40, "typical",     32, 128),
         ("real-192-257",    "real",    192, 2, 2, 257, "typical",     32, 128),
         ("tanh-130-512",    "tanh",    130, 2, 2, 512, "typical",     32, 128)]


def shape_of(case):
    _, kind, sorb, _, _, H, _, _, _ = case
    return R.mcmc_group(H), R.table_doubles(kind, sorb, H) * 8 <= R.LDS_BYTES, (sorb - 1) // 64 + 1


def test_case_coverage(mods):
    """The cases reach every flavour, word count, lane count and regime, and both sides of the LDS switch (sizes from the C ABI)."""
    _, _, _, N, _ = mods
    for case in CASES:
        _, kind, sorb, _, _, H, _, _, _ = case
        nb = N.lib().pynqs_crbm_table_bytes(sorb, H) if kind in ("complex", "cos") else N.lib().pynqs_rbm_table_bytes(sorb, H)
        assert nb == R.table_doubles(kind, sorb, H) * 8, case
    shapes = [shape_of(c) for c in CASES]
    assert {c[1] for c in CASES} == {"real", "tanh", "pRBM", "complex", "cos"}
    assert {s[2] for s in shapes} == {1, 2, 3}
    assert {1, 8, 9, 64, 65, 257, 512} <= {c[5] for c in CASES}
    assert {1, 2, 8, 16, 64} <= {s[0] for s in shapes}
    assert {c[6] for c in CASES} == {"typical", "saturated", "churn", "cos", "imag", "return"}
    # the 64 KB switch at one shape (sorb 40): one hidden unit more moves the table from LDS to L2, real and complex
    by = {c[0]: s for c, s in zip(CASES, shapes)}
    assert by["real-40-64"][1] and not by["real-40-65"][1]
    assert by["complex-40-32"][1] and not by["complex-40-33"][1]
    assert any(s[1] for c, s in zip(CASES, shapes) if c[1] != "pRBM") and any(not s[1] for s in shapes)


def thetas(kind, W, hb, words, sorb):
    x = R.pm1(words, sorb)
    if kind == "cos":
        return np.zeros((x.shape[0], W.shape[0])), x @ W.T + hb
    th = x @ W.T + hb
    return np.real(th), np.imag(th)


def report(tag, rep, extra=""):
    print(f"\n[mcmc-exact] {tag}: {rep.steps} steps, {rep.ties} ties, accepted {int(rep.accepted.sum())}, "
          f"max |lnpsi - exact| / tau = {rep.lnpsi_err:.3g}, ln|psi| by {rep.source}{extra}")


def check(rep, n_accept=None):
    assert rep.mismatches == 0, f"{rep.mismatches} steps against the rule; first: {rep.first_bad}"
    assert rep.ties <= 1e-4 * rep.steps, rep.ties
    if n_accept is not None:
        assert np.array_equal(n_accept, rep.accepted), (n_accept[:8], rep.accepted[:8])
    assert rep.lnpsi_err <= 1.0, rep.lnpsi_err


def regime_coverage(kind, regime, W, hb, rep, sorb):
    """The regime's special cases happened: asserted on the states the chains visited (accepted moves) and the proposals."""
    T, nch, L = rep.prev.shape
    if kind == "pRBM":
        return ""
    re_p, im_p = thetas(kind, W, hb, rep.prev.reshape(-1, L), sorb)
    re_q, _ = thetas(kind, W, hb, rep.prop.reshape(-1, L), sorb)
    if regime == "saturated":
        nb = 2 * NPAIR
        a = np.abs(re_p[:, :nb]).reshape(T, nch, nb)
        lo, hi = a.min(0), a.max(0)
        n = int(((lo < 20.0) & (hi > 400.0)).sum())
        assert n > 0, "no hidden unit travelled between |Re theta| < 20 and > 400 within the launch"
        sg = (re_p[:, :nb] < 0).reshape(T, nch, nb)
        flips = int((sg[1:] != sg[:-1]).sum())
        return f", {n} (chain, unit) pairs travelled |Re theta| < 20 <-> > 400, {flips} sign changes of those units"
    if regime == "churn":
        moved = (rep.prev.reshape(-1, L) != rep.prop.reshape(-1, L)).any(1)
        flips = ((re_p < 0) != (re_q < 0)).any(1)[moved].mean()
        zeros = int((re_q == 0).sum())
        assert flips > 0.5 and zeros > 0, (flips, zeros)
        return f", sign change in {100 * flips:.0f} % of the moves, {zeros} units at Re theta = 0"
    if regime == "return":
        # a chain at theta_0 > 373 (q_0 = 0) that later, with no sign change and through a state in between, reached theta_0 < 5
        th = re_p[:, 0].reshape(T, nch)
        n = 0
        for c in range(nch):
            hi = np.flatnonzero(th[:, c] > 373.0)
            if hi.size:
                t1 = hi[0]
                lo = np.flatnonzero(th[t1:, c] < 5.0)
                if lo.size and (th[t1:t1 + lo[0], c] > 0).all() and ((th[t1:t1 + lo[0], c] > 5) & (th[t1:t1 + lo[0], c] < 373)).any():
                    n += 1
        assert n > 0, "no chain fell from theta_0 > 373 to < 5 without a sign change"
        return f", {n} chains fell from theta_0 > 373 to < 5 without a sign change"
    if regime == "cos":
        # q = exp(-2i theta) went around the unit circle, and some proposals came near a zero of cos (1 + q ~ 0)
        spread = float((im_p.max(0) - im_p.min(0)).max())
        _, im_q = thetas(kind, W, hb, rep.prop.reshape(-1, L), sorb)
        near = int((np.abs(np.cos(im_q)) < 1e-2).sum())
        assert spread > np.pi and near > 0, (spread, near)
        return f", theta spread {spread:.2f}, {near} proposed units with |cos theta| < 0.01"
    if regime == "imag":
        m = float(np.abs(im_p).max())
        assert m > 300, m
        return f", max |Im theta| {m:.0f}"
    return ""


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_replay_fused(mods, case):
    cx, mcmc, rbm, N, oracle = mods
    name, kind, sorb, noA, noB, H, regime, nch, nsteps = case
    seed = 1000 + CASES.index(case)
    W, hb, vb = make_params(kind, regime, sorb, H, seed, noA, noB)
    model = module_of(rbm, kind, W, hb, vb)
    f = mcmc._Fused(model, sorb)
    G, lds, L = shape_of(case)
    assert f.nhidden == H and f.table.buf.numel() * 8 == R.table_doubles(kind, sorb, H) * 8
    x0 = first_det(sorb, noA, noB)
    s = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, seed, torch.from_numpy(x0.view(np.uint8)).cuda())
    s.run(model, 0, nsteps, keep_records=True)
    rec = s.last_records.cpu().numpy().view(np.uint64)
    assert rec.shape == (nsteps, nch, L)
    rep = R.replay(oracle, R.Rbm(kind, W, hb, vb), sorb, noA, noB, seed, 0, 0, np.repeat(x0, nch, 0), rec, s.lnpsi.cpu().numpy())
    extra = regime_coverage(kind, regime, W, hb, rep, sorb)
    report(f"{name} (G {G}, table in {'LDS' if lds else 'L2'}, {L} word{'s' if L > 1 else ''}, {regime})", rep, extra)
    check(rep, s.n_accept.cpu().numpy())
    if kind == "pRBM":
        assert int(rep.accepted.sum()) == rep.steps


def direct_launch(cx, N, kind, W, hb, vb, sorb, noA, noB, x0, nsteps, seed, chain_base=0, t0=0):
    """One pynqs_mcmc_rbm launch of nsteps steps with records (every = 1), past the Python layer's 256 steps per launch."""
    flav = {"real": N.RBM_REAL, "tanh": N.RBM_TANH, "pRBM": N.RBM_PHASE, "complex": N.RBM_COMPLEX, "cos": N.RBM_COMPLEX}[kind]
    tab = table_of(cx, kind, W, hb, vb)
    nch, L = x0.shape
    st = torch.from_numpy(x0.view(np.int64).copy()).cuda()
    rec = torch.empty((nsteps, nch, L), dtype=torch.int64, device="cuda")
    nacc = torch.zeros(nch, dtype=torch.int64, device="cuda")
    lnpsi = torch.empty(nch, dtype=torch.float64, device="cuda")
    N.check(N.lib().pynqs_mcmc_rbm(st.data_ptr(), nch, sorb, noA, noB, tab.data_ptr(), W.shape[0], flav, seed, chain_base, t0, nsteps,
                                   1, rec.data_ptr(), nacc.data_ptr(), lnpsi.data_ptr(), torch.cuda.current_stream().cuda_stream),
            "pynqs_mcmc_rbm")
    torch.cuda.synchronize()
    rec = rec.cpu().numpy().view(np.uint64)
    assert np.array_equal(st.cpu().numpy().view(np.uint64), rec[-1])
    return rec, nacc.cpu().numpy(), lnpsi.cpu().numpy()


@pytest.mark.parametrize("kind,sorb,noA,noB,H,regime", [("real", 12, 3, 3, 9, "typical"), ("real", 24, 3, 3, 16, "churn"),
                                                        ("complex", 12, 3, 3, 9, "typical")])
def test_long_launch(mods, kind, sorb, noA, noB, H, regime):
    """4096 steps in one launch: the incremental state (theta, q, ln|psi|) must not drift from the exact one over a long launch."""
    cx, _, _, N, oracle = mods
    nch, nsteps, seed, base, t0 = 64, 4096, 4242 + sorb + H, 96, 1 << 20
    W, hb, vb = make_params(kind, regime, sorb, H, seed, noA, noB)
    x0 = np.repeat(first_det(sorb, noA, noB), nch, 0)
    rec, nacc, lnpsi = direct_launch(cx, N, kind, W, hb, vb, sorb, noA, noB, x0, nsteps, seed, base, t0)
    rep = R.replay(oracle, R.Rbm(kind, W, hb, vb), sorb, noA, noB, seed, base, t0, x0, rec, lnpsi)
    extra = regime_coverage(kind, regime, W, hb, rep, sorb)
    report(f"long {kind}-{sorb}-{H} {regime} (G {R.mcmc_group(H)}, one launch of {nsteps} steps)", rep, extra)
    check(rep, nacc)
    assert (rep.accepted > 0).all()


def test_zero_amplitude_start(mods):
    """tanh with a.x0 = 0 exactly (dyadic visible biases): the first state has amplitude zero, and so have many others.  The fused
    kernel, the generic path and the exact rule agree record for record; ln|psi| of the final states is their own."""
    cx, mcmc, rbm, N, oracle = mods
    sorb, noA, noB, H, nch, nsteps, seed = 8, 2, 2, 16, 256, 200, 31337
    W, hb, _ = make_params("real", "typical", sorb, H, seed)
    vb = np.array([0.5, 0.25, 0.25, 0.5, 0.5, 0.5, 0.25, 0.25])
    model = module_of(rbm, "tanh", W, hb, vb)
    x0 = first_det(sorb, noA, noB)
    assert float(R.pm1(x0, sorb)[0] @ vb) == 0.0
    x0_t = torch.from_numpy(x0.view(np.uint8)).cuda()
    assert float(model(cx.onv_to_tensor(x0_t, sorb))[0]) == 0.0
    a = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, seed, x0_t)
    b = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, seed, x0_t)
    a.run(model, 0, nsteps, keep_records=True)
    b.run(Opaque(model), 0, nsteps, keep_records=True)
    rec = a.last_records.cpu().numpy().view(np.uint64)
    rep = R.replay(oracle, R.Rbm("tanh", W, hb, vb), sorb, noA, noB, seed, 0, 0, np.repeat(x0, nch, 0), rec, a.lnpsi.cpu().numpy())
    zero_visits = sum(1 for k in R._keys(rep.prev.reshape(-1, 1)) if np.isneginf(rep.exact[bytes(k)][0]))
    report("tanh-8-16 zero-amplitude start (G 2, LDS, 1 word)", rep, f", {zero_visits} chain-steps from a state of amplitude 0")
    assert zero_visits > nch
    check(rep, a.n_accept.cpu().numpy())
    assert rep.ties == 0
    assert torch.equal(a.last_records, b.last_records), "fused and generic records differ"
    assert torch.equal(a.n_accept, b.n_accept)
    assert bool(torch.isfinite(a.lnpsi).any()) and not bool(torch.isnan(a.lnpsi).any())


@pytest.mark.parametrize("shift", [-30.0, 30.0], ids=["tiny", "huge"])
def test_fused_equals_generic_extreme_amplitudes(mods, fe2s2, shift):
    """A real RBM with |psi| ~ 1e-250 (visible biases ~ -30) or ~ 1e+250 (~ +30) at every state: the squares of the amplitudes leave the
    range of a double, their ratios do not.  The generic path must make the fused kernel's decisions."""
    cx, mcmc, rbm, N, _ = mods
    sorb, noA, noB, H, nch, nsteps, seed = 40, 15, 15, 40, 1024, 120, 2024
    W, hb, vb = make_params("real", "typical", sorb, H, seed)
    vb = vb + shift
    model = module_of(rbm, "real", W, hb, vb)
    x0 = torch.from_numpy(np.ascontiguousarray(fe2s2["ci_space"][:nch])).cuda()
    a = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, seed, x0)
    b = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, seed, x0)
    a.run(model, 0, nsteps, keep_records=True)
    b.run(Opaque(model), 0, nsteps, keep_records=True)
    lp = a.lnpsi.cpu().numpy()
    assert (np.abs(lp) > 373).all(), np.abs(lp).min()  # |psi|^2 under- or overflows at every final state
    assert 0.05 < a.acceptance < 0.95, a.acceptance
    assert torch.equal(a.last_records, b.last_records), "fused and generic records differ"
    assert torch.equal(a.n_accept, b.n_accept)


# ---- the generic step on hand-made amplitudes ------------------------------------------------------------------------------------------
MAXD = np.finfo(np.float64).max
TINY = 5e-324


def _exact_accept(u, cur, prop):
    """The documented rule in exact arithmetic: (accept, tie) for amplitudes cur, prop (complex) and the draw u."""
    if not (math.isfinite(prop.real) and math.isfinite(prop.imag)):
        return False, False
    if not (math.isfinite(cur.real) and math.isfinite(cur.imag)) or cur == 0:
        return True, False
    F = Fraction
    ratio = (F(prop.real) ** 2 + F(prop.imag) ** 2) / (F(cur.real) ** 2 + F(cur.imag) ** 2)
    return F(u) <= ratio, abs(ratio - F(u)) <= F(u) * F(1, 10 ** 12)


def _amplitudes(u, cplx, rng):
    """(current, proposed) amplitude pairs: fixed edge cases, then pairs whose ratio lies within 1e-9 of u on either side."""
    nan, inf = float("nan"), float("inf")
    fixed = [(0.0, 1.0), (0.0, 0.0), (0.0, TINY), (1.0, 0.0), (TINY, 0.0), (TINY, 2 * TINY), (3 * TINY, TINY), (-TINY, 1e-310),
             (1e-310, -3e-310), (1e-200, 3e-200), (-1e-200, 1e-201), (1e200, -4e200), (1e200, 1e199), (MAXD, -MAXD / 2),
             (MAXD / 4, MAXD), (-MAXD, MAXD), (1e-300, 1e300), (1e300, -1e-300), (TINY, MAXD), (MAXD, TINY), (1e-170, 1e-170),
             (1e160, 1e160), (1.0, inf), (1.0, -inf), (1.0, nan), (0.0, nan), (inf, 1.0), (nan, 2.0), (-inf, 0.0), (nan, nan),
             (inf, inf), (1e-320, 1e-150)]
    if cplx:
        fixed = [complex(c * math.cos(p), c * math.sin(p)) if math.isfinite(c) else complex(c, 0.0) for c, p in
                 zip([a for a, _ in fixed], rng.uniform(-math.pi, math.pi, len(fixed)))], [
                 complex(d * math.cos(p), -d * math.sin(p)) if math.isfinite(d) else complex(0.0, d) for d, p in
                 zip([b for _, b in fixed], rng.uniform(-math.pi, math.pi, len(fixed)))]
        fixed = list(zip(*fixed)) + [(complex(MAXD, MAXD), complex(MAXD / 2, -MAXD / 2)), (complex(-MAXD, MAXD), complex(MAXD, -MAXD)),
                                     (complex(TINY, -TINY), complex(0.0, 2 * TINY)), (complex(0.0, 1e-200), complex(-1e-200, 1e-200))]
    pairs = [(complex(c), complex(p)) for c, p in fixed]
    for k in range(len(pairs), u.size):
        mag = 10.0 ** rng.uniform(-300, 300)
        r = math.sqrt(u[k]) * (1.0 + (1e-9 if k % 2 else -1e-9))
        if cplx:
            pc, pp = rng.uniform(-math.pi, math.pi, 2)
            pairs.append((mag * complex(math.cos(pc), math.sin(pc)), mag * r * complex(math.cos(pp), math.sin(pp))))
        else:
            pairs.append((complex(mag * rng.choice([-1, 1])), complex(mag * r * rng.choice([-1, 1]))))
    return pairs


@pytest.mark.parametrize("cplx,sorb", [(False, 40), (True, 40), (False, 130), (True, 190)])
def test_accept_kernel_exact(mods, cplx, sorb):
    """pynqs_mcmc_accept: decisions, states, psi (changed only where a move is accepted), record_row and n_accept against the rule
    evaluated in fractions.Fraction of the given doubles; non-finite amplitudes as include/pynqs_amd.h documents them."""
    _, _, _, N, _ = mods
    nch, seed, base, t = 192, 777 + sorb, 1000, 7
    L = (sorb - 1) // 64 + 1
    rng = np.random.default_rng(sorb + cplx)
    u = R.host_u(seed, t, np.uint64(base) + np.arange(nch, dtype=np.uint64))
    pairs = _amplitudes(u, cplx, rng)
    mask = np.array([(1 << min(64, sorb - 64 * w)) - 1 for w in range(L)], dtype=np.uint64)
    words = lambda: (rng.integers(0, 2 ** 63, (nch, L), dtype=np.uint64) * np.uint64(2) + np.uint64(1)) & mask  # noqa: E731
    st0, prop = words(), words()
    cur = np.array([c for c, _ in pairs]); new = np.array([p for _, p in pairs])
    want = [_exact_accept(u[k], cur[k], new[k]) for k in range(nch)]
    acc = np.array([w for w, _ in want])
    assert not any(tie for _, tie in want)
    assert 0.2 < acc.mean() < 0.8
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    as_dbl = (lambda a: np.stack([a.real, a.imag], -1)) if cplx else (lambda a: a.real.copy())
    st, psi, pr, psi_p = T(st0.view(np.int64)), T(as_dbl(cur)), T(prop.view(np.int64)), T(as_dbl(new))
    row = torch.full_like(st, -1)
    nacc0 = rng.integers(0, 50, nch)
    nacc = T(nacc0)
    N.check(N.lib().pynqs_mcmc_accept(st.data_ptr(), psi.data_ptr(), pr.data_ptr(), psi_p.data_ptr(), nch, sorb, int(cplx), seed, base, t,
                                      row.data_ptr(), nacc.data_ptr(), torch.cuda.current_stream().cuda_stream), "pynqs_mcmc_accept")
    torch.cuda.synchronize()
    got = (st.cpu().numpy().view(np.uint64) == prop).all(1)
    bad = np.flatnonzero(got != acc)
    assert bad.size == 0, [(int(k), cur[k], new[k], float(u[k]), bool(acc[k])) for k in bad[:6]]
    want_st = np.where(acc[:, None], prop, st0)
    assert np.array_equal(st.cpu().numpy().view(np.uint64), want_st)
    assert np.array_equal(row.cpu().numpy().view(np.uint64), want_st)
    assert np.array_equal(nacc.cpu().numpy(), nacc0 + acc)
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)  # noqa: E731
    want_psi = np.where(acc[:, None] if cplx else acc, as_dbl(new), as_dbl(cur))
    assert np.array_equal(bits(psi.cpu().numpy()), bits(want_psi))
    # without record_row and n_accept
    st2, psi2 = T(st0.view(np.int64)), T(as_dbl(cur))
    N.check(N.lib().pynqs_mcmc_accept(st2.data_ptr(), psi2.data_ptr(), pr.data_ptr(), psi_p.data_ptr(), nch, sorb, int(cplx), seed, base,
                                      t, None, None, torch.cuda.current_stream().cuda_stream), "pynqs_mcmc_accept")
    assert torch.equal(st2, st) and np.array_equal(bits(psi2.cpu().numpy()), bits(want_psi))
