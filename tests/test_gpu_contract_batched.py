"""pynqs_reduce_contract_form: the batched contraction kernel (a slot's column first, weight and link of live slots only, the loads of
eight slots per lane in flight together) against the kernel that visits a lane's slots one at a time, bit for bit on E_loc and psi(x),
on front ends built by ReduceFrontEnd: the LIST form (live prefixes), the look-back form (fixed slots with holes) and the table-less
LIST form, without draws and with 7, 64, 65 and 1000 of them (below, at and above a wave's 64 slots, and more than one batch), 5, 64 and
65 walkers, one- and two-word determinants, real and complex psi, with and without the division, with links into a wave-function table,
with an out-of-range link (NaN for that walker only) and with column 0 absent (psi(x) = 0).

And against numpy longdouble on the same records: a lane adds its products with fma, the lanes meet in a butterfly -- some tree over
the m records of a walker, each partial sum rounded once: |error| <= m 2^-52 sum |w psi| (complex psi: per component, |Re|, |Im| <= | |)."""
import numpy as np
import pytest
import torch

from conftest import rand_occ, synth_integrals

pytestmark = pytest.mark.gpu

BATCHED, SERIAL = 0, 1
# eps None: chosen per batch of walkers so that no walker keeps more than 300 columns (a row of the two-word system has ~9000; with
# draws it is one segment, and the LDS list of the LIST form holds 1024)
SYSTEMS = {"one word": (12, 3, 3, 0.3), "two words": (66, 3, 3, None)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_SETUP = {}


def _setup(system, n):
    """walkers, integrals and the plan of a system (computed once, shared, never written)"""
    from pynqs_amd import C_extension as cx

    key = (system, n)
    if key not in _SETUP:
        sorb, noA, noB, eps = SYSTEMS[system]
        h1, h2 = synth_integrals(sorb)
        h1e, h2e = _dev(h1), _dev(h2)
        x = cx.tensor_to_onv(_dev(rand_occ(n, sorb, noA, noB, seed=sorb + n)), sorb)
        if eps is None:
            _, hm = cx.get_comb_hij_fused(x, h1e, h2e, sorb, noA + noB, noA, noB)
            eps = float(hm.abs().sort(dim=1, descending=True).values[:, 300].max())  # |H| >= eps: at most 300 per walker
        _SETUP[key] = (x, h1e, h2e, cx.plan_for(h1e, h2e, sorb, x.device).buf, eps)
    return _SETUP[key]


def _front(system, n, N, layout, lut=None):
    """a front end run in the wanted form: cap_doubles within the LDS list's capacity (LIST, with or without the table) or beyond it"""
    from pynqs_amd import _native as NA, reduce_front as RF

    sorb, noA, noB, _ = SYSTEMS[system]
    x, h1e, h2e, plan, eps = _setup(system, n)
    ncomb = int(NA.lib().pynqs_num_sd(sorb, noA, noB)) + 1
    dedup = layout != "list, no table"
    cap_list = RF.list_capacity(n, sorb, noA + noB, noA, noB, N, torch.float64, without_table=not dedup)
    assert cap_list > 0
    cap_d = cap_list + 1 if layout == "look-back" else min(cap_list, ncomb)
    fe = RF.ReduceFrontEnd(n, sorb, noA + noB, noA, noB, N, torch.float64, x.device, cap_d, n * ncomb + 64, want_pm1=False, dedup=dedup)
    fe.run(x, plan, eps, 7, lut)
    cnt = fe.counters_host()
    assert not fe.overflowed(cnt)
    return fe, cnt[0]


def _amps(nu, cplx, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(nu, generator=g, dtype=torch.float64) + 0.5
    a = a * torch.where(torch.rand(nu, generator=g) < 0.3, -1.0, 1.0).double()
    if cplx:
        a = a * torch.exp(1j * 6.0 * torch.rand(nu, generator=g, dtype=torch.float64))
    return a.cuda()


def _bits(t):
    return torch.view_as_real(t).view(torch.int64) if t.is_complex() else t.view(torch.int64)


def _both(fe, amp, table=None, divide=True):
    e1, p1 = fe.contract(amp, table, divide=divide, form=SERIAL)
    e0, p0 = fe.contract(amp, table, divide=divide, form=BATCHED)
    return (e0, p0), (e1, p1)


def _longdouble_check(fe, amp, table, e_nodiv, tag):
    """sum_records w psi per walker in longdouble against the kernel's undivided sum"""
    walker, col, w, link, _, _ = fe.records()
    own = link >= 0
    psi = torch.zeros(link.numel(), dtype=amp.dtype, device=amp.device)
    psi[own] = amp[fe.rows_of(link[own])]
    if table is not None:
        psi[link <= -2] = table.to(amp.dtype)[(-2 - link[link <= -2]).long()]
    wk, wn, pn = walker.cpu().numpy(), w.cpu().numpy().astype(np.longdouble), psi.cpu().numpy()
    n = fe.n
    m = np.bincount(wk, minlength=n).astype(np.float64)
    mag = np.zeros(n, dtype=np.longdouble)
    np.add.at(mag, wk, np.abs(wn) * np.abs(pn).astype(np.longdouble))
    bound = (m * 2.0**-52 * mag).astype(np.float64)
    got = e_nodiv.cpu().numpy()
    worst = 0.0
    for part in ("real", "imag") if amp.is_complex() else ("real",):
        want = np.zeros(n, dtype=np.longdouble)
        np.add.at(want, wk, wn * getattr(pn, part).astype(np.longdouble))
        err = np.abs(getattr(got, part).astype(np.longdouble) - want).astype(np.float64)
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
        worst = max(worst, ratio)
        assert (err <= bound).all(), f"{tag} {part}: error / bound {ratio:.3f}"
    print(f"{tag}: {int(m.max())} records per walker at most, error / bound {worst:.3f}")


CASES = [("one word", n, N, layout) for n in (5, 64, 65) for N in (0, 7, 64, 65, 1000) for layout in ("list", "look-back", "list, no table")]
CASES += [("two words", 65, N, layout) for N in (0, 7, 64, 65, 1000) for layout in ("list", "look-back", "list, no table")]


@pytest.mark.parametrize("system,n,N,layout", CASES)
def test_batched_equals_serial_bit_for_bit(system, n, N, layout):
    fe, nu = _front(system, n, N, layout)
    for cplx in (False, True):
        amp = _amps(nu, cplx, 3 + n + N)
        for divide in (True, False):
            (e0, p0), (e1, p1) = _both(fe, amp, divide=divide)
            tag = f"{system} n={n} N={N} {layout} cplx={cplx} divide={divide}"
            assert torch.equal(_bits(e0), _bits(e1)), tag
            assert torch.equal(_bits(p0), _bits(p1)), tag
            if not divide:  # (divided, a walker whose column 0 was not kept is x / 0)
                assert bool(torch.isfinite(torch.view_as_real(e0) if cplx else e0).all()), tag
                _longdouble_check(fe, amp, None, e0, tag)


@pytest.mark.parametrize("N", [0, 65])
@pytest.mark.parametrize("layout", ["list", "look-back"])
def test_links_into_a_wavefunction_table(layout, N):
    from pynqs_amd import C_extension as cx, public_function as pf

    system, n = "one word", 65
    sorb, noA, noB, _ = SYSTEMS[system]
    x, h1e, h2e, _, _ = _setup(system, n)
    comb, _ = cx.get_comb_hij_fused(x, h1e, h2e, sorb, noA + noB, noA, noB)
    keys = torch.unique(comb.reshape(-1, comb.shape[-1]), dim=0)[::2].contiguous()
    g = torch.Generator().manual_seed(3)
    wf = (torch.rand(keys.size(0), generator=g, dtype=torch.float64) + 0.2).cuda()
    lut = pf.WavefunctionLUT(keys, wf, sorb, device=torch.device("cuda"))
    fe, nu = _front(system, n, N, layout, lut.hashtable)
    link = fe.records()[3]
    assert bool((link <= -2).any()) and bool((link >= 0).any())
    for cplx in (False, True):
        amp = _amps(max(nu, 1), cplx, 9)
        tab = lut.wf_value.to(amp.dtype)
        for divide in (True, False):
            (e0, p0), (e1, p1) = _both(fe, amp, tab, divide)
            assert torch.equal(_bits(e0), _bits(e1)) and torch.equal(_bits(p0), _bits(p1))
            if not divide:
                _longdouble_check(fe, amp, tab, e0, f"table {layout} N={N} cplx={cplx}")


@pytest.mark.parametrize("layout", ["list", "look-back", "list, no table"])
def test_an_out_of_range_link_poisons_its_walker_only(layout):
    n, bad_walker = 65, 37
    fe, nu = _front("one word", n, 65, layout)
    fe = _copy_records(fe)
    seg = fe.rec_col.view(fe.nseg, fe.stride)[bad_walker * fe.nchunks]
    read = fe.fixed + min(int(fe.seg_count[bad_walker * fe.nchunks]), fe.cap_doubles)  # the slots the kernels visit
    slot = int(torch.nonzero(seg[:read] >= 0)[0])
    fe.rec_link.view(fe.nseg, fe.stride)[bad_walker * fe.nchunks, slot] = (1 << 30) + fe.cap_unique + 3
    fe._io = fe._make_io()
    for cplx in (False, True):
        amp = _amps(nu, cplx, 4)
        for divide in (True, False):
            for e, _ in _both(fe, amp, divide=divide):
                nan = torch.isnan(torch.view_as_real(e)).any(-1) if cplx else torch.isnan(e)
                want = torch.zeros(n, dtype=torch.bool, device=e.device)
                want[bad_walker] = True
                # (divided, a walker whose column 0 was neither kept nor drawn is x / 0, which may be nan as well)
                assert torch.equal(nan, want) if not divide else bool(nan[bad_walker])
            (e0, p0), (e1, p1) = _both(fe, amp, divide=divide)
            keep = torch.arange(n, device=e0.device) != bad_walker
            assert torch.equal(_bits(e0)[keep], _bits(e1)[keep]) and torch.equal(_bits(p0), _bits(p1))


@pytest.mark.parametrize("layout", ["list", "look-back"])
def test_column_zero_absent(layout):
    n = 64
    fe, nu = _front("one word", n, 7, layout)
    fe = _copy_records(fe)
    fe.rec_col[fe.rec_col == 0] = -1
    fe.srec_col[fe.srec_col == 0] = -1
    fe._io = fe._make_io()
    for cplx in (False, True):
        amp = _amps(nu, cplx, 6)
        (e0, p0), (e1, p1) = _both(fe, amp, divide=False)
        assert torch.equal(_bits(e0), _bits(e1)) and torch.equal(_bits(p0), _bits(p1))
        assert bool((p0 == 0).all()) and bool(torch.isfinite(torch.view_as_real(e0) if cplx else e0).all())
        (d0, _), (d1, _) = _both(fe, amp, divide=True)  # x / 0: inf or nan on both sides, the same ones
        f0, f1 = (torch.view_as_real(d0), torch.view_as_real(d1)) if cplx else (d0, d1)
        assert torch.equal(torch.isnan(f0), torch.isnan(f1)) and torch.equal(f0[~torch.isnan(f0)], f1[~torch.isnan(f1)])


def _copy_records(fe):
    """the front end with its record arrays replaced by copies (the test writes into them)"""
    for name in ("rec_col", "rec_link", "srec_col", "srec_link"):
        setattr(fe, name, getattr(fe, name).clone())
    return fe


def test_bad_form_is_refused():
    fe, nu = _front("one word", 5, 0, "list")
    with pytest.raises(RuntimeError, match="bad form"):
        fe.contract(_amps(nu, False, 1), form=2)
