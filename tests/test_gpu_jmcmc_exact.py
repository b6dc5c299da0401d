"""The fused Jastrow-RBM chain kernel pynqs_mcmc_jrbm against the accept rule evaluated exactly (include/pynqs_amd.h, "many-chain
Metropolis sampling"; tests/mcmc_replay.py with the amplitude of tests/jmcmc_replay.py):
 (i) every step replayed from the kernel's own records, proposals of the CPU oracle, ln|psi| = ln|psi_RBM| + x^T M x from the float64
     parameters in longdouble / mpmath: 1-3 ONV words, 1-64 lanes per chain, the three places of the two tables (both in LDS, the RBM
     table only, neither), M typical / asymmetric with a diagonal / strong enough to decide most steps, and the RBM's saturated regime;
 (ii) the same records replayed with M dropped must NOT follow the rule (the replay sees the Jastrow factor);
 (iii) M = 0: records, accept counts and ln|psi| of pynqs_mcmc_jrbm equal pynqs_mcmc_rbm's bit for bit;
 (iv) a 4096-step launch through the C ABI, and the argument errors.
Every seed is fixed.  The replay cases print one line each."""
import numpy as np
import pytest
import torch

import jmcmc_replay as JR
import mcmc_replay as R
import test_gpu_mcmc_exact as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from oracle import oracle
    from pynqs_amd import C_extension, _native, mcmc, rbm

    assert torch.cuda.is_available()
    assert np.finfo(np.longdouble).eps < 1e-18, "the replay needs an extended longdouble"
    return C_extension, mcmc, rbm, _native, oracle


# M regimes: every entry uniform in +-amp, a full matrix (asymmetric, non-zero diagonal)
M_AMP = {"typical": 0.1, "asym": 0.25, "strong": 3.0, "zero": 0.0}

#        id               sorb noA noB  H   RBM regime   M regime  chains steps  form
CASES = [("j-4-1",          4, 1, 1,   1, "typical",   "typical", 256, 256, None),
         ("j-12-9",        12, 3, 3,   9, "typical",   "asym",    256, 256, None),
         ("j-12-8-strong", 12, 3, 3,   8, "typical",   "strong",  256, 256, None),
         ("j-40-40",       40, 5, 5,  40, "typical",   "typical",  64, 256, 3),
         ("j-40-64",       40, 5, 5,  64, "typical",   "typical",  64, 256, 1),
         ("j-40-65",       40, 5, 5,  65, "typical",   "typical",  64, 256, 0),
         ("j-66-16",       66, 3, 3,  16, "typical",   "typical", 128, 256, None),
         ("j-130-16",     130, 2, 3,  16, "typical",   "typical",  64, 256, 1),
         ("j-8-260",        8, 2, 2, 260, "typical",   "typical", 256, 256, None),
         ("j-24-16-sat",   24, 3, 3,  16, "saturated", "typical", 128, 256, None)]
IDS = [c[0] for c in CASES]


def make_case(case):
    name, sorb, noA, noB, H, regime, mreg, nch, nsteps, _ = case
    seed = 2000 + IDS.index(name)
    W, hb, vb = E.make_params("real", regime, sorb, H, seed, noA, noB)
    g = np.random.default_rng(seed + 500)
    M = 2.0 * M_AMP[mreg] * (g.random((sorb, sorb)) - 0.5)
    return seed, W, hb, vb, M


def jmodule(rbm, W, hb, vb, M):
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return rbm.JastrowRBM(T(W), T(hb), T(vb), T(M)).cuda()


def test_case_coverage(mods):
    """The cases reach the three forms, 1-3 words and 1, 2, 8, 64 lanes; the form follows from the table sizes the C ABI reports."""
    _, _, _, N, _ = mods
    lib = N.lib()
    forms, groups, words = set(), set(), set()
    for case in CASES:
        name, sorb, _, _, H, _, _, _, _, want = case
        form = lib.pynqs_mcmc_jrbm_form(sorb, H)
        assert lib.pynqs_mcmc_jrbm_supported(sorb, H) == 1, name
        rb, sb = lib.pynqs_rbm_table_bytes(sorb, H), 8 * sorb * sorb  # (S: the table's first block of sorb^2 doubles)
        assert 3 * sb < lib.pynqs_jastrow_table_bytes(sorb) <= 3 * sb + 16
        assert form == (1 if rb <= R.LDS_BYTES else 0) + (2 if rb + sb <= R.LDS_BYTES else 0), (name, form, rb, sb)
        assert want is None or form == want, (name, form)
        forms.add(form); groups.add(R.mcmc_group(H)); words.add((sorb - 1) // 64 + 1)
    assert forms == {0, 1, 3}
    assert {1, 2, 8, 64} <= groups
    assert words == {1, 2, 3}
    assert 8 * 130 * 130 > R.LDS_BYTES  # j-130-16: S alone is past the LDS bound
    assert lib.pynqs_mcmc_jrbm_form(40, 513) == -1 and lib.pynqs_mcmc_jrbm_supported(193, 8) == 0


def moved_counts(rep, rec):
    """(accepted, rejected) among the proposals that differ from the state."""
    T, nch, L = rep.prev.shape
    moved = (rep.prev != rep.prop).any(2)
    took = (rec.reshape(T, nch, L) == rep.prop).all(2)
    return int((moved & took).sum()), int((moved & ~took).sum())


def check_power(oracle, case, seed, W, hb, vb, M, x0, rec, base=0, t0=0):
    """The same records against the RBM alone (M dropped): the replay must report steps against the rule."""
    _, sorb, noA, noB = case[:4]
    rep0 = R.replay(oracle, R.Rbm("real", W, hb, vb), sorb, noA, noB, seed, base, t0, x0, rec)
    assert rep0.mismatches > 0, "the replay without M follows the records too: it does not see the Jastrow factor"
    return rep0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_replay_fused(mods, case):
    cx, mcmc, rbm, N, oracle = mods
    name, sorb, noA, noB, H, regime, mreg, nch, nsteps, _ = case
    seed, W, hb, vb, M = make_case(case)
    model = jmodule(rbm, W, hb, vb, M)
    assert mcmc._Fused.applies(model, sorb)
    f = mcmc._Fused(model, sorb)
    assert f.jastrow_table is not None and f.nhidden == H
    L = (sorb - 1) // 64 + 1
    x0 = E.first_det(sorb, noA, noB)
    s = mcmc.MCMCSampler(sorb, noA + noB, noA, noB, nch, seed, torch.from_numpy(x0.view(np.uint8)).cuda())
    s.run(model, 0, nsteps, keep_records=True)
    assert s.lnpsi is not None, "the sampler took the generic path"
    rec = s.last_records.cpu().numpy().view(np.uint64)
    assert rec.shape == (nsteps, nch, L)
    x0n = np.repeat(x0, nch, 0)
    amp = JR.JRbm(W, hb, vb, M)
    rep = R.replay(oracle, amp, sorb, noA, noB, seed, 0, 0, x0n, rec, s.lnpsi.cpu().numpy())
    extra = E.regime_coverage("real", regime, W, hb, rep, sorb)
    acc, rej = moved_counts(rep, rec)
    form = N.lib().pynqs_mcmc_jrbm_form(sorb, H)
    E.report(f"{name} (G {R.mcmc_group(H)}, form {form}, {L} word{'s' if L > 1 else ''}, RBM {regime}, M {mreg}, Jastrow scale "
             f"{amp.jastrow_scale:.3g})", rep, f", moves accepted {acc} / rejected {rej}{extra}")
    E.check(rep, s.n_accept.cpu().numpy())
    assert acc > 0 and rej > 0, (acc, rej)
    rep0 = check_power(oracle, case, seed, W, hb, vb, M, x0n, rec)
    print(f"[jmcmc-exact] {name}: without M {rep0.mismatches} of {rep0.steps} steps are against the rule")
    if mreg == "strong":
        # the Jastrow part of 2 (ln|psi'| - ln|psi|) against the RBM part, over the proposals that move
        T = rep.prev.shape[0]
        moved = (rep.prev != rep.prop).any(2).reshape(-1)
        xp, xq = R.pm1(rep.prev.reshape(-1, L)[moved], sorb), R.pm1(rep.prop.reshape(-1, L)[moved], sorb)
        dj = 2 * (((xq @ M) * xq).sum(1) - ((xp @ M) * xp).sum(1))
        lr_q, _ = R.Rbm("real", W, hb, vb).lnabs_ld(xq)
        lr_p, _ = R.Rbm("real", W, hb, vb).lnabs_ld(xp)
        dr = 2 * (lr_q - lr_p).astype(np.float64)
        frac = float((np.abs(dj) > np.abs(dr)).mean())
        print(f"[jmcmc-exact] {name}: |Jastrow part| > |RBM part| in {100 * frac:.1f} % of {moved.sum()} moving proposals ({T} steps)")
        assert frac > 0.5, frac


def launch(cx, N, W, hb, vb, M, sorb, noA, noB, x0, nsteps, seed, chain_base=0, t0=0):
    """One launch of nsteps steps with records (every = 1): pynqs_mcmc_jrbm, or pynqs_mcmc_rbm where M is None."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tab = cx.RBMTable(T(W), T(hb), T(vb))
    nch, L = x0.shape
    st = torch.from_numpy(x0.view(np.int64).copy()).cuda()
    rec = torch.empty((nsteps, nch, L), dtype=torch.int64, device="cuda")
    nacc = torch.zeros(nch, dtype=torch.int64, device="cuda")
    lnpsi = torch.empty(nch, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if M is None:
        N.check(N.lib().pynqs_mcmc_rbm(st.data_ptr(), nch, sorb, noA, noB, tab.data_ptr(), W.shape[0], N.RBM_REAL, seed, chain_base, t0,
                                       nsteps, 1, rec.data_ptr(), nacc.data_ptr(), lnpsi.data_ptr(), stream), "pynqs_mcmc_rbm")
    else:
        jt = cx.JastrowTable(T(M))
        N.check(N.lib().pynqs_mcmc_jrbm(st.data_ptr(), nch, sorb, noA, noB, tab.data_ptr(), jt.data_ptr(), W.shape[0], seed, chain_base,
                                        t0, nsteps, 1, rec.data_ptr(), nacc.data_ptr(), lnpsi.data_ptr(), stream), "pynqs_mcmc_jrbm")
    torch.cuda.synchronize()
    rec = rec.cpu().numpy().view(np.uint64)
    assert np.array_equal(st.cpu().numpy().view(np.uint64), rec[-1])
    return rec, nacc.cpu().numpy(), lnpsi.cpu().numpy()


@pytest.mark.parametrize("name", ["j-12-9", "j-40-40"])
def test_zero_jastrow_is_the_rbm_kernel(mods, name):
    """M = 0: the Jastrow terms are sums of exact zeros, so one pynqs_mcmc_jrbm launch and one pynqs_mcmc_rbm launch with the same seed
    and t0 give identical records, identical n_accept and ln|psi| equal bit for bit."""
    cx, _, _, N, _ = mods
    case = CASES[IDS.index(name)]
    _, sorb, noA, noB, H, _, _, nch, nsteps, _ = case
    seed, W, hb, vb, _ = make_case(case)
    x0 = np.repeat(E.first_det(sorb, noA, noB), nch, 0)
    a = launch(cx, N, W, hb, vb, np.zeros((sorb, sorb)), sorb, noA, noB, x0, nsteps, seed, 7, 1000)
    b = launch(cx, N, W, hb, vb, None, sorb, noA, noB, x0, nsteps, seed, 7, 1000)
    assert np.array_equal(a[0], b[0]), "records differ"
    assert np.array_equal(a[1], b[1]) and 0 < a[1].sum() < nch * nsteps
    assert np.array_equal(a[2].view(np.int64), b[2].view(np.int64)), np.abs(a[2] - b[2]).max()


def test_long_launch(mods):
    """4096 steps in one launch: ln|psi|, which alone carries the Jastrow factor from step to step, must not drift from the exact one."""
    cx, _, _, N, oracle = mods
    sorb, noA, noB, H, nch, nsteps, seed, base, t0 = 12, 3, 3, 9, 64, 4096, 4242, 96, 1 << 20
    W, hb, vb = E.make_params("real", "typical", sorb, H, seed, noA, noB)
    M = 2.0 * M_AMP["typical"] * (np.random.default_rng(seed + 500).random((sorb, sorb)) - 0.5)
    x0 = np.repeat(E.first_det(sorb, noA, noB), nch, 0)
    rec, nacc, lnpsi = launch(cx, N, W, hb, vb, M, sorb, noA, noB, x0, nsteps, seed, base, t0)
    rep = R.replay(oracle, JR.JRbm(W, hb, vb, M), sorb, noA, noB, seed, base, t0, x0, rec, lnpsi)
    E.report(f"long j-{sorb}-{H} (G {R.mcmc_group(H)}, one launch of {nsteps} steps)", rep)
    E.check(rep, nacc)
    assert (rep.accepted > 0).all()
    rep0 = R.replay(oracle, R.Rbm("real", W, hb, vb), sorb, noA, noB, seed, base, t0, x0, rec)
    assert rep0.mismatches > 0


def test_errors(mods):
    cx, mcmc, rbm, N, _ = mods
    sorb, noA, noB, H = 40, 5, 5, 40
    W, hb, vb = E.make_params("real", "typical", sorb, H, 1)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tab, jt = cx.RBMTable(T(W), T(hb), T(vb)), cx.JastrowTable(T(np.zeros((sorb, sorb))))
    st = torch.from_numpy(np.repeat(E.first_det(sorb, noA, noB), 8, 0).view(np.int64).copy()).cuda()
    before = st.clone()
    stream = torch.cuda.current_stream().cuda_stream

    def call(jas, nh, base):
        return N.lib().pynqs_mcmc_jrbm(st.data_ptr(), 8, sorb, noA, noB, tab.data_ptr(), jas, nh, 1, base, 0, 1, 1, None, None, None, stream)

    for jas, nh, base in ((None, H, 0), (jt.data_ptr(), 513, 0), (jt.data_ptr(), 0, 0), (jt.data_ptr(), H, 2 ** 32 - 4)):
        with pytest.raises(RuntimeError):
            N.check(call(jas, nh, base), "pynqs_mcmc_jrbm")
    assert N.lib().pynqs_mcmc_jrbm_supported(sorb, 513) == 0 and not mcmc.mcmc_jrbm_supported(sorb, 513)
    assert mcmc.mcmc_jrbm_supported(sorb, H)
    torch.cuda.synchronize()
    assert torch.equal(st, before)
    N.check(call(jt.data_ptr(), H, 2 ** 32 - 8), "pynqs_mcmc_jrbm")  # the last 8 chain indices below 2^32 are fine
