"""The host-side caches in front of the kernels over SEQUENCES of calls, the way a VMC run makes them: integral plans (content key, LRU,
in-place edits), the REDUCE front-end workspaces and their table / no-table decision, total_energy's call token for the multi-psi table,
the keys index of the sample space, and the parameters the gradient objects read.  Every call is checked against a cold computation --
the CPU oracle, or the same entry point on fresh objects -- so a cache that hits when it should miss fails here.
Tolerance: 1e-8 Ha per determinant."""
import numpy as np
import pytest
import torch

from conftest import golden, rand_occ, synth_integrals

pytestmark = pytest.mark.gpu
TOL = 1e-8
DEV = torch.device("cuda")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rbm(sorb, nh, seed, scale=0.05):
    g = np.random.default_rng(seed)
    return scale * (g.random((nh, sorb)) - 0.5), scale * (g.random(nh) - 0.5), scale * (g.random(sorb) - 0.5)


def _module(W, hb, vb):
    from pynqs_amd.rbm import RealRBM

    return RealRBM(*(torch.from_numpy(np.ascontiguousarray(a)) for a in (W, hb, vb))).to(DEV)


def _ab(sorb):
    from pynqs_amd import public_function as pf

    return lambda xx, func: pf.ansatz_batch(func, xx, 1 << 20, sorb, DEV, torch.float64)


def _simple(x, h1, h2, m, sorb, noa, nob):
    from pynqs_amd import energy as E

    return E.local_energy(x, h1, h2, m, _ab(sorb), sorb, noa + nob, noa, nob)[0].cpu().numpy()


def _reduce(x, h1, h2, m, sorb, noa, nob, eps):
    from pynqs_amd import energy as E

    return E.local_energy(x, h1, h2, m, _ab(sorb), sorb, noa + nob, noa, nob, reduce_psi=True, eps=eps)[0].cpu().numpy()


def _reduce_oracle(x, h1, h2, sorb, noa, nob, W, hb, vb, eps):
    """sum over |<x|H|x'>| >= eps of H psi(x') / psi(x) on the oracle's row with the oracle's RBM amplitudes; NaN where the diagonal
    itself is dropped (as the reference)"""
    from oracle import oracle as O

    co, ho = O.comb_hij_fused(np.ascontiguousarray(x), h1, h2, sorb, noa + nob, noa, nob)
    psi = O.rbm_real_psi(co.reshape(-1, co.shape[-1]), sorb, W, hb, vb).reshape(ho.shape)
    e = (np.where(np.abs(ho) >= eps, ho, 0.0) * psi).sum(1) / psi[:, 0]
    return np.where(np.abs(ho[:, 0]) >= eps, e, np.nan)


def _close(got, want, tol=TOL):
    ok = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), ok), "a walker is finite in one result and not in the other"
    assert ok.any()
    np.testing.assert_allclose(got[ok], want[ok], rtol=0, atol=tol)


def _fresh_front_caches(monkeypatch):
    from pynqs_amd import energy as E

    for name, val in (("_FRONT_DENSE", set()), ("_FRONTS", {}), ("_FRONT_NODEDUP", {}), ("_FRONT_NODEDUP_CALLS", {})):
        monkeypatch.setattr(E, name, val)


def test_relabelled_system_is_not_served_the_plan_of_the_original(monkeypatch):
    """The spin orbitals of synth_integrals(40) reversed: the same physics with other labels (alpha <-> beta), the packed h2e a permutation of
    the same values.  Walkers, RBM columns and visible bias relabelled alike, noA and noB swapped.  Every call matches the oracle on its own
    inputs, and the relabelled E_loc reproduces the first system's walker for walker (only the order of the sums differs)."""
    from oracle import oracle as O
    from pynqs_amd import C_extension as cx

    _fresh_front_caches(monkeypatch)
    sorb, noa, nob, n, eps = 40, 7, 5, 64, 1e-3
    h1, h2 = synth_integrals(sorb, 77)
    a, b = O.decompress_h1e_h2e(h1, h2, sorb)
    p = np.arange(sorb)[::-1]
    r1, r2 = O.compress_h1e_h2e(a[np.ix_(p, p)], b[np.ix_(p, p, p, p)], sorb)
    occ = rand_occ(n, sorb, noa, nob, 3)
    W, hb, vb = _rbm(sorb, 24, 5)
    runs = [(h1, h2, O.pm01_to_onv(occ, sorb), W, vb, noa, nob), (r1, r2, O.pm01_to_onv(occ[:, p], sorb), W[:, p], vb[p], nob, noa)]
    first, plans = None, []
    for h1_, h2_, x_, W_, vb_, na, nb in runs:
        H1, H2, X = T(h1_), T(h2_), T(x_)
        comb, hm = cx.get_comb_hij_fused(X, H1, H2, sorb, na + nb, na, nb)
        co, ho = O.comb_hij_fused(x_, h1_, h2_, sorb, na + nb, na, nb)
        assert np.array_equal(comb.cpu().numpy(), co) and np.array_equal(hm.cpu().numpy(), ho)
        plans.append(cx.plan_for(H1, H2, sorb, DEV))
        m = _module(W_, hb, vb_)
        es = _simple(X, H1, H2, m, sorb, na, nb)
        np.testing.assert_allclose(es, O.eloc_simple_rbm(x_, h1_, h2_, sorb, na + nb, na, nb, W_, hb, vb_)[0], rtol=0, atol=TOL)
        er = _reduce(X, H1, H2, m, sorb, na, nb, eps)
        _close(er, _reduce_oracle(x_, h1_, h2_, sorb, na, nb, W_, hb, vb_, eps))
        if first is None:
            first = es, er
        else:
            np.testing.assert_allclose(es, first[0], rtol=0, atol=TOL)
            _close(er, first[1])
    assert plans[0] is not plans[1] and not torch.equal(plans[0].buf, plans[1].buf)


def test_plan_lru_over_more_systems_than_it_holds():
    """_MAX_PLANS + 1 systems of one shape and a float32 copy of one of them, alternated over two rounds, each through the same tensor
    objects (identity hits) and through fresh equal copies (content hits): every call matches the oracle, equal content still shares a plan."""
    from oracle import oracle as O
    from pynqs_amd import C_extension as cx

    sorb, no, n = 12, 3, 24
    systems = [synth_integrals(sorb, 100 + k) for k in range(cx._MAX_PLANS + 1)]
    x = O.pm01_to_onv(rand_occ(n, sorb, no, no, 1), sorb)
    W, hb, vb = _rbm(sorb, 6, 2, scale=0.5)
    m = _module(W, hb, vb)
    want = [O.eloc_simple_rbm(x, a, b, sorb, 2 * no, no, no, W, hb, vb)[0] for a, b in systems]
    f32 = tuple(t.astype(np.float32) for t in systems[2])
    want_f32 = O.eloc_simple_rbm(x, f32[0].astype(np.float64), f32[1].astype(np.float64), sorb, 2 * no, no, no, W, hb, vb)[0]
    assert np.abs(want_f32 - want[2]).max() > 10 * TOL   # (the float32 copy is another system: a plan mix-up shows)
    kept = [(T(a), T(b)) for a, b in systems]
    X = T(x)
    for _ in range(2):
        for k, (a, b) in enumerate(systems):
            pk = cx.plan_for(*kept[k], sorb, DEV)
            assert cx.plan_for(T(a), T(b), sorb, DEV) is pk   # (equal content in fresh tensors: the same plan)
            for H1, H2 in (kept[k], (T(a), T(b))):
                np.testing.assert_allclose(_simple(X, H1, H2, m, sorb, no, no), want[k], rtol=0, atol=TOL)
                hm = cx.get_comb_hij_fused(X, H1, H2, sorb, 2 * no, no, no)[1]
                assert np.array_equal(hm.cpu().numpy(), O.comb_hij_fused(x, a, b, sorb, 2 * no, no, no)[1])
            np.testing.assert_allclose(_simple(X, T(f32[0]), T(f32[1]), m, sorb, no, no), want_f32, rtol=0, atol=TOL)
    p0 = cx.plan_for(*kept[0], sorb, DEV)
    assert cx.plan_for(T(systems[0][0]), T(systems[0][1]), sorb, DEV) is p0
    assert cx.plan_for(*kept[1], sorb, DEV) is not p0


def test_in_place_edits_of_the_integrals_give_new_plans():
    """copy_ under no_grad, an edit through a view, mul_ on a slice: each bumps the version counter the views share -> a new plan, and the
    energies of the edited integrals."""
    from oracle import oracle as O
    from pynqs_amd import C_extension as cx

    sorb, no, n = 12, 3, 24
    x = O.pm01_to_onv(rand_occ(n, sorb, no, no, 4), sorb)
    W, hb, vb = _rbm(sorb, 6, 3, scale=0.5)
    m = _module(W, hb, vb)
    X = T(x)
    H1, H2 = (T(a) for a in synth_integrals(sorb, 31))
    other = synth_integrals(sorb, 32)

    def edit_copy():
        with torch.no_grad():
            H2.copy_(T(other[1]))

    def edit_view():
        v = H1.view(sorb, sorb)
        v[1, 4] += 0.25
        v[4, 1] += 0.25   # (kept symmetric)

    def edit_slice():
        H2[100:400].mul_(1.5)

    plans = [cx.plan_for(H1, H2, sorb, DEV)]
    for edit in (None, edit_copy, edit_view, edit_slice):
        if edit is not None:
            edit()
            pl = cx.plan_for(H1, H2, sorb, DEV)
            assert all(pl is not q for q in plans), edit.__name__
            plans.append(pl)
        h1, h2 = H1.cpu().numpy(), H2.cpu().numpy()
        np.testing.assert_allclose(_simple(X, H1, H2, m, sorb, no, no), O.eloc_simple_rbm(x, h1, h2, sorb, 2 * no, no, no, W, hb, vb)[0],
                                   rtol=0, atol=TOL)
        assert np.array_equal(cx.get_comb_hij_fused(X, H1, H2, sorb, 2 * no, no, no)[1].cpu().numpy(),
                              O.comb_hij_fused(x, h1, h2, sorb, 2 * no, no, no)[1])


def _record_fronts(monkeypatch):
    from pynqs_amd import energy as E

    seen = []
    finish = E.reduce_front_finish

    def rec(t):
        out = finish(t)
        seen.append(out[0].dedup)
        return out

    monkeypatch.setattr(E, "reduce_front_finish", rec)
    return seen


def test_same_shape_other_walkers_with_the_table(monkeypatch, fe2s2):
    """REDUCE on walkers A, then B of the same batch size, then A again, with the de-duplication table: the cached workspace and its table
    carry nothing over -- every call matches the oracle walker for walker."""
    from pynqs_amd import energy as E

    _fresh_front_caches(monkeypatch)
    monkeypatch.setattr(E, "FRONT_NODEDUP_RATIO", 2.0)   # (never drop the table)
    sorb, no, n, eps = 40, 15, 128, 1e-3
    ci = np.ascontiguousarray(fe2s2["ci_space"])
    A, B = ci[:n], ci[n:2 * n]
    h1, h2 = fe2s2["h1e"], fe2s2["h2e"]
    H1, H2 = T(h1), T(h2)
    W, hb, vb = _rbm(sorb, 40, 6)
    m = _module(W, hb, vb)
    seen = _record_fronts(monkeypatch)
    want = {"A": _reduce_oracle(A, h1, h2, sorb, no, no, W, hb, vb, eps), "B": _reduce_oracle(B, h1, h2, sorb, no, no, W, hb, vb, eps)}
    for name in "ABA":
        _close(_reduce(T(A if name == "A" else B), H1, H2, m, sorb, no, no, eps), want[name])
    assert seen == [True, True, True] and len(E._FRONTS) == 1
    assert list(E._FRONT_NODEDUP.values()) == [None]


def _long_rows(seed, n=320, sorb=80, no=20):
    import bench as B

    return B.synth_walkers(n, sorb, no, no, seed).to(DEV)


def _long_row_system():
    sorb = 80
    h1, h2 = (t.numpy() for t in __import__("bench").synth_integrals(sorb))
    W, hb, vb = _rbm(sorb, sorb // 2, 1)
    return sorb, 20, h1, h2, T(h1), T(h2), (W, hb, vb), _module(W, hb, vb)


def test_same_shape_other_walkers_without_the_table(monkeypatch):
    """Long rows (sorb 80) where nearly every x' is distinct: the first call drops the table, the later ones run table-less on ONE cached
    workspace.  A, B, A, B: each call equals a cold call on fresh caches walker for walker, and the oracle on the first walkers."""
    from pynqs_amd import energy as E

    sorb, no, h1, h2, H1, H2, prm, m = _long_row_system()
    eps = 0.3
    A, B = _long_rows(99), _long_rows(98)
    _fresh_front_caches(monkeypatch)
    cold_B = _reduce(B, H1, H2, m, sorb, no, no, eps)
    _fresh_front_caches(monkeypatch)
    seen = _record_fronts(monkeypatch)
    cold_A = _reduce(A, H1, H2, m, sorb, no, no, eps)
    assert seen == [True] and list(E._FRONT_NODEDUP.values())[0] is not None   # (decided: no table from now on)
    for x, cold in ((B, cold_B), (A, cold_A), (B, cold_B)):
        _close(_reduce(x, H1, H2, m, sorb, no, no, eps), cold, 1e-10)
    assert seen == [True, False, False, False] and len(E._FRONTS) == 1
    for x, cold in ((A, cold_A), (B, cold_B)):
        idx = np.flatnonzero(np.isfinite(cold))[:3]
        _close(cold[idx], _reduce_oracle(x[idx].cpu().numpy(), h1, h2, sorb, no, no, *prm, eps))


def test_table_decision_is_measured_again(monkeypatch):
    """FRONT_NODEDUP_RECHECK calls after the table was dropped for all-distinct walkers, the decision is measured again: once the walkers
    have concentrated (one determinant repeated, same batch size) a call runs WITH the table, records the new decision, and the table stays."""
    from pynqs_amd import energy as E

    sorb, no, h1, h2, H1, H2, prm, m = _long_row_system()
    eps, recheck = 0.3, 2
    monkeypatch.setattr(E, "FRONT_NODEDUP_RECHECK", recheck)
    _fresh_front_caches(monkeypatch)
    seen = _record_fronts(monkeypatch)
    A = _long_rows(99)
    eA = _reduce(A, H1, H2, m, sorb, no, no, eps)
    (nk, caps), = E._FRONT_NODEDUP.items()
    assert caps is not None and seen == [True]
    i0 = int(np.flatnonzero(np.isfinite(eA))[0])
    one = _reduce_oracle(A[i0:i0 + 1].cpu().numpy(), h1, h2, sorb, no, no, *prm, eps)
    _close(eA[i0:i0 + 1], one)
    xr = A[i0:i0 + 1].repeat(A.size(0), 1).contiguous()
    for _ in range(recheck + 1):
        _close(_reduce(xr, H1, H2, m, sorb, no, no, eps), np.repeat(one, xr.size(0)))
    assert any(seen[1:]), f"no call ran with the table after the walkers concentrated: {seen}"
    assert E._FRONT_NODEDUP[nk] is None   # (measured again: keep the table)
    _close(_reduce(xr, H1, H2, m, sorb, no, no, eps), np.repeat(one, xr.size(0)))
    assert seen[-1]


class _Holder:
    """ansatz.module.sample / ansatz.module.extra, as the reference's multi-psi code dereferences a DDP-wrapped model."""

    def __init__(self, sample, extra):
        import types

        self.module = types.SimpleNamespace(sample=sample, extra=extra)


def test_call_token_after_an_exception(monkeypatch, fe2s2):
    """total_energy (multi-psi, sample space) raises in its second chunk after the first stored f on the table's keys under its call token.
    After the reference's GD step on f's parameters (p.data.add_, no version bump) a direct local_energy call on the same table must use
    the new f: equal to a cold call on a fresh table object and to the oracle."""
    from oracle import oracle as O
    from pynqs_amd import energy as E, public_function as pf

    d0, d = golden("eloc_e2e_fe2s2.npz"), golden("eloc_flip_multipsi_fe2s2.npz")
    sorb, nele, no = 40, 30, 15
    old_dtype = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        rbm, extra = _module(d0["W"], d0["hb"], d0["vb"]), _module(d["W2"], d["hb2"], d["vb2"])
        holder = _Holder(rbm, extra)
        keys, wf = T(d["lut_keys"]), T(d["lut_wf"])
        lut = pf.WavefunctionLUT(keys, wf, sorb, device=DEV)
        h1, h2 = fe2s2["h1e"], fe2s2["h2e"]
        H1, H2, X = T(h1), T(h2), T(d["x"])
        enm = torch.tensor(float(d["extra_norm_multi"]), dtype=torch.float64, device=DEV)
        kw = dict(WF_LUT=lut, use_sample_space=True, use_multi_psi=True, extra_norm=enm)
        calls = []
        real = E.local_energy

        def flaky(*a, **k):
            calls.append(1)
            if len(calls) == 2:
                raise RuntimeError("ansatz failed in chunk 2")
            return real(*a, **k)

        monkeypatch.setattr(E, "local_energy", flaky)
        with pytest.raises(RuntimeError, match="chunk 2"):
            E.total_energy(X, X.size(0) // 2, -1, H1, H2, holder, sorb, nele, no, no, **kw)
        monkeypatch.setattr(E, "local_energy", real)
        assert len(calls) == 2 and getattr(lut, "_pynqs_f_keys", None) is not None   # (chunk 1 stored f under the call's token)
        with torch.no_grad():
            for q in extra.parameters():
                q.data.add_(0.02)
        ab = lambda xx, func: pf.ansatz_batch(func, xx, 100000, sorb, DEV, torch.float64)  # noqa: E731
        e_direct = E.local_energy(X, H1, H2, holder, ab, sorb, nele, no, no, **kw)[0].cpu().numpy()
        kw["WF_LUT"] = pf.WavefunctionLUT(keys, wf, sorb, device=DEV)
        e_cold = E.local_energy(X, H1, H2, holder, ab, sorb, nele, no, no, **kw)[0].cpu().numpy()
        np.testing.assert_allclose(e_direct, e_cold, rtol=0, atol=TOL)
        # the oracle: E_loc = |f(x)|^2 / N^2 * sum_k H_k (f psi)(x'_k) / (f psi)(x), (f psi) a table over the sample space
        W2, hb2, vb2 = (q.detach().cpu().numpy() for q in (extra.weights, extra.hidden_bias, extra.visible_bias))
        ks, ws = lut.bra_key.cpu().numpy(), lut.wf_value.cpu().numpy()
        x = d["x"]
        e_t, _ = O.eloc_sample_space(x, h1, h2, sorb, nele, no, no, ks, ws * O.rbm_real_psi(ks, sorb, W2, hb2, vb2))
        _, found = O.wavefunction_lut(ks, x, sorb)
        want = e_t * O.rbm_real_psi(x, sorb, W2, hb2, vb2) ** 2 / float(d["extra_norm_multi"]) ** 2
        assert found.any()
        np.testing.assert_allclose(e_direct[found], want[found], rtol=0, atol=TOL)
        assert E._call_token() is None
    finally:
        torch.set_default_dtype(old_dtype)


def test_keys_index_after_the_keys_are_rewritten_in_place(monkeypatch, fe2s2):
    """The indexed key-major sample-space kernel; then WF_LUT.bra_key is rewritten IN PLACE with another sorted key set of the same size
    (same tensor, same address) and its values updated: the energies are the oracle's on the new keys."""
    from oracle import oracle as O
    from pynqs_amd import energy as E, public_function as pf

    monkeypatch.setattr(E, "SS_KEYS", True)
    monkeypatch.setattr(E, "SS_INDEX", True)
    sorb, nele, no, n, nk = 40, 30, 15, 64, 3000
    ci = np.ascontiguousarray(fe2s2["ci_space"])
    h1, h2 = fe2s2["h1e"], fe2s2["h2e"]
    H1, H2 = T(h1), T(h2)
    x = ci[:n]
    g = np.random.default_rng(8)
    sets = [ci[:nk], np.concatenate([ci[:n], ci[nk:2 * nk - n]])]   # (both hold the walkers)
    luts = [pf.WavefunctionLUT(T(k), T(g.random(nk) + 0.25), sorb, device=DEV) for k in sets]
    lut = luts[0]
    key_obj = lut.bra_key
    for step, src in enumerate(luts):
        if step:
            lut.bra_key.copy_(src.bra_key)
            lut.wf_value.copy_(src.wf_value)
            assert lut.bra_key is key_obj
        e = E.local_energy(T(x), H1, H2, None, None, sorb, nele, no, no, WF_LUT=lut, use_sample_space=True)[0].cpu().numpy()
        assert getattr(lut, "_keys_index", None) is not None   # (the indexed form ran)
        want, _ = O.eloc_sample_space(x, h1, h2, sorb, nele, no, no, src.bra_key.cpu().numpy(), src.wf_value.cpu().numpy())
        np.testing.assert_allclose(e, want, rtol=0, atol=TOL)


def _grad_inputs(sorb, n, seed, cplx=False):
    import bench as B
    from pynqs_amd import C_extension as cx

    x = B.synth_walkers(n, sorb, 15, 15, seed).to(DEV)
    g = torch.Generator().manual_seed(seed)
    prob = torch.rand(n, generator=g, dtype=torch.float64)
    prob = (prob / prob.sum()).to(DEV)
    eloc = torch.randn(n, generator=g, dtype=torch.float64) - 100.0
    if cplx:
        eloc = torch.complex(eloc, 0.1 * torch.randn(n, generator=g, dtype=torch.float64))
    eloc = eloc.to(DEV)
    return x, cx.onv_to_tensor(x, sorb).to(torch.float64), prob, eloc, (prob * eloc).sum()


@pytest.mark.parametrize("kind", ["real", "complex"])
def test_fused_gradient_follows_replaced_parameters(kind):
    """FusedRbmGrad after load_state_dict(..., assign=True) and after assigning a new nn.Parameter: the gradient is autograd's at the
    CURRENT parameters and lands on the current parameters' .grad."""
    from pynqs_amd import grad as G
    from pynqs_amd.rbm import ComplexRBM, RealRBM

    sorb, H, n = 40, 24, 300
    g = torch.Generator().manual_seed(3)
    r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)  # noqa: E731
    m = (ComplexRBM(0.3 * r(H, sorb, 2), 0.4 * r(H, 2), 0.2 * r(sorb, 2)) if kind == "complex" else
         RealRBM(0.3 * r(H, sorb), 0.4 * r(H), 0.2 * r(sorb))).to(DEV)
    dtype = torch.complex128 if kind == "complex" else torch.float64
    x, states, prob, eloc, e_tot = _grad_inputs(sorb, n, 17, kind == "complex")
    fg = G.FusedRbmGrad(m, sorb)

    def check():
        for p in m.parameters():
            p.grad = None
        fg(x, prob, eloc, e_tot)
        got = [p.grad for p in m.parameters()]
        assert all(q is not None for q in got), "the gradient did not land on the module's current parameters"
        got = [q.clone() for q in got]
        for p in m.parameters():
            p.grad = None
        G.grad(m, states, prob, eloc, e_tot, 1.0, dtype)
        want = [p.grad for p in m.parameters()]
        scale = max(float(w.abs().max()) for w in want)
        for a, w in zip(got, want):
            np.testing.assert_allclose(a.cpu().numpy(), w.cpu().numpy(), rtol=0, atol=1e-11 * scale)

    check()
    sd = {k: v.detach().clone() * 1.1 + 0.01 for k, v in m.state_dict().items()}
    m.load_state_dict(sd, assign=True)
    check()
    name = next(iter(dict(m.named_parameters())))
    setattr(m, name, torch.nn.Parameter(getattr(m, name).detach() * 0.9))
    check()


def test_graphed_gradient_refuses_reallocated_parameters():
    """GraphedGrad replays the addresses it captured: after p.data = p.data.clone() a call raises instead of reading the old storage."""
    from pynqs_amd import grad as G
    from pynqs_amd.rbm import RealRBM

    sorb, H, n = 40, 16, 64
    g = torch.Generator().manual_seed(4)
    r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)  # noqa: E731
    m = RealRBM(0.3 * r(H, sorb), 0.4 * r(H), 0.2 * r(sorb)).to(DEV)
    _, states, prob, eloc, e_tot = _grad_inputs(sorb, n, 5)
    gg = G.GraphedGrad(m, n, sorb, torch.double, DEV)
    gg(states, prob, eloc, e_tot)
    old = [p.data for p in m.parameters()]   # (kept alive: whatever the replay reads stays valid memory)
    for p in m.parameters():
        p.data = p.data.clone()
    with pytest.raises(RuntimeError, match="re-allocated"):
        gg(states, prob, eloc, e_tot)
    m2 = RealRBM(0.3 * r(H, sorb), 0.4 * r(H), 0.2 * r(sorb)).to(DEV)
    gg2 = G.GraphedGrad(m2, n, sorb, torch.double, DEV)
    m2.weights = torch.nn.Parameter(m2.weights.detach().clone())
    with pytest.raises(RuntimeError, match="replaced"):
        gg2(states, prob, eloc, e_tot)
    del old
