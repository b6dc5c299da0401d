"""pynqs_reduce_contract_form's placement flag PYNQS_CONTRACT_BY_XCD (workgroup b serves walker group pynqs_reduce_contract_group(b, B)),
on the batched and on the slot-at-a-time kernel, against the slot-at-a-time kernel without it: bit for bit on E_loc and psi(x).  (The
one-stream form this file was first written for -- batches of a walker's next eight live trips across its lists -- passed every case
here and was slower than the batched kernel on the flagship: it is not in the tree; profiles/contract_stream_trace.txt.)

Front ends built by ReduceFrontEnd: the LIST form (live prefixes), the look-back form (fixed slots with holes) and the table-less LIST
form; 12 orbitals (one word) and 66 orbitals (two words); 0, 1, 7, 64, 65, 449, 512, 513 and 1000 draws (the drawn list ends below, at
and above a batch of 8 trips of 64 slots); eps at which the walkers' kept counts lie on both sides of 64 (one trip) and of 512 (one
batch); 1, 3, 4, 5, 29, 32, 33, 36 and 259 walkers (1, 2, 8, 9 and 65 workgroups of 4) and 9 - 25 walkers (3 - 7 workgroups, the other
remainders mod 8); real and complex psi, a different amplitude on every row, so that a skipped or doubled walker cannot pass; with and
without the division; links into a wave-function table; an out-of-range link (NaN for that walker only); column 0 absent; and record
lists with holes punched anywhere, whole trips included."""
import numpy as np
import pytest
import torch

from conftest import rand_occ, synth_integrals

pytestmark = pytest.mark.gpu

BATCHED, SERIAL, BY_XCD = 0, 1, 0x100
FORMS = {"batched by xcd": BATCHED | BY_XCD, "serial by xcd": SERIAL | BY_XCD, "the default": None}
# (sorb, alpha, beta, the kept count the walkers' counts straddle)
SYSTEMS = {"one word, 64 kept": (12, 3, 3, 64), "two words, 64 kept": (66, 3, 3, 64), "two words, 512 kept": (66, 3, 3, 512)}
WALKERS = (1, 3, 4, 5, 29, 32, 33, 36, 259)
DRAWS = (0, 1, 7, 64, 65, 449, 512, 513, 1000)
LAYOUTS = ("list", "look-back", "list, no table")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_SETUP = {}


def _setup(system, n):
    """walkers, integrals, plan and eps of a system (computed once, shared, never written): eps is the median over the walkers of the
    (kept + 1)-th largest |H| of the row -- half the walkers keep more than `kept` columns, half fewer --, raised where a walker would
    keep more than 900 (the LDS list of the LIST form holds 1024)"""
    from pynqs_amd import C_extension as cx

    key = (system, n)
    if key not in _SETUP:
        sorb, noA, noB, kept = SYSTEMS[system]
        h1, h2 = synth_integrals(sorb)
        h1e, h2e = _dev(h1), _dev(h2)
        x = cx.tensor_to_onv(_dev(rand_occ(n, sorb, noA, noB, seed=sorb + n)), sorb)
        _, hm = cx.get_comb_hij_fused(x, h1e, h2e, sorb, noA + noB, noA, noB)
        mag = hm.abs().sort(dim=1, descending=True).values
        eps = float(mag[:, kept].median())
        if mag.shape[1] > 900:
            eps = max(eps, float(mag[:, 900].max()))
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
    assert torch.unique(torch.view_as_real(a) if cplx else a, dim=0).shape[0] == nu  # a different amplitude on every row
    return a.cuda()


def _bits(t):
    return torch.view_as_real(t).view(torch.int64) if t.is_complex() else t.view(torch.int64)


def _same_as_serial(fe, amp, table=None, divide=True, tag="", keep=None, forms=FORMS):
    """every form in `forms` against SERIAL, bit for bit (keep: the walkers compared on E_loc); returns SERIAL's (E_loc, psi(x))"""
    e1, p1 = fe.contract(amp, table, divide=divide, form=SERIAL)
    for name, form in forms.items():
        e, p = fe.contract(amp, table, divide=divide, form=form)
        be, b1 = _bits(e), _bits(e1)
        if keep is not None:
            be, b1 = be[keep], b1[keep]
        assert torch.equal(be, b1), f"{tag} {name}: E_loc"
        assert torch.equal(_bits(p), _bits(p1)), f"{tag} {name}: psi(x)"
    return e1, p1


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N", DRAWS)
@pytest.mark.parametrize("system", list(SYSTEMS))
def test_placement_equals_serial_bit_for_bit(system, N, layout):
    want = SYSTEMS[system][3]
    for n in WALKERS:
        fe, nu = _front(system, n, N, layout)
        if n >= 29:  # the kept counts straddle the wanted one
            kept = torch.bincount(fe.records()[0][~fe.records()[5]], minlength=n)
            assert int(kept.min()) < want < int(kept.max()), f"{system} n={n}: kept {int(kept.min())} .. {int(kept.max())}"
        for cplx in (False, True):
            amp = _amps(nu, cplx, 3 + n + N)
            for divide in (True, False):
                tag = f"{system} n={n} N={N} {layout} cplx={cplx} divide={divide}"
                e1, _ = _same_as_serial(fe, amp, divide=divide, tag=tag)
                if not divide:  # (divided, a walker whose column 0 was not kept is x / 0)
                    assert bool(torch.isfinite(torch.view_as_real(e1) if cplx else e1).all()), tag


@pytest.mark.parametrize("n", [9, 13, 17, 21, 25])
def test_every_remainder_of_the_workgroup_count(n):
    fe, nu = _front("one word, 64 kept", n, 65, "list")
    for cplx in (False, True):
        _same_as_serial(fe, _amps(nu, cplx, n), tag=f"n={n} cplx={cplx}")


@pytest.mark.parametrize("N", [0, 65, 513])
@pytest.mark.parametrize("layout", ["list", "look-back"])
def test_links_into_a_wavefunction_table(layout, N):
    from pynqs_amd import C_extension as cx, public_function as pf

    system, n = "one word, 64 kept", 33
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
            _same_as_serial(fe, amp, tab, divide, tag=f"table {layout} N={N} cplx={cplx} divide={divide}")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_an_out_of_range_link_poisons_its_walker_only(layout):
    n, bad_walker = 33, 21
    fe, nu = _front("one word, 64 kept", n, 65, layout)
    fe = _copy_records(fe)
    seg = fe.rec_col.view(fe.nseg, fe.stride)[bad_walker * fe.nchunks]
    read = fe.fixed + min(int(fe.seg_count[bad_walker * fe.nchunks]), fe.cap_doubles)  # the slots the kernels visit
    slot = int(torch.nonzero(seg[:read] >= 0)[0])
    fe.rec_link.view(fe.nseg, fe.stride)[bad_walker * fe.nchunks, slot] = (1 << 30) + fe.cap_unique + 3
    fe._io = fe._make_io()
    keep = torch.arange(n, device="cuda") != bad_walker
    for cplx in (False, True):
        amp = _amps(nu, cplx, 4)
        for name, form in FORMS.items():
            e, _ = fe.contract(amp, divide=False, form=form)
            nan = torch.isnan(torch.view_as_real(e)).any(-1) if cplx else torch.isnan(e)
            assert torch.equal(nan, ~keep), f"{layout} {name} cplx={cplx}"
        for divide in (True, False):
            _same_as_serial(fe, amp, divide=divide, tag=f"bad link {layout} cplx={cplx} divide={divide}", keep=keep)


@pytest.mark.parametrize("layout", ["list", "look-back"])
def test_column_zero_absent(layout):
    n = 32
    fe, nu = _front("one word, 64 kept", n, 7, layout)
    fe = _copy_records(fe)
    fe.rec_col[fe.rec_col == 0] = -1
    fe.srec_col[fe.srec_col == 0] = -1
    fe._io = fe._make_io()
    for cplx in (False, True):
        amp = _amps(nu, cplx, 6)
        e1, p1 = _same_as_serial(fe, amp, divide=False, tag=f"no column 0 {layout} cplx={cplx}")
        assert bool((p1 == 0).all()) and bool(torch.isfinite(torch.view_as_real(e1) if cplx else e1).all())
        d1, _ = fe.contract(amp, divide=True, form=SERIAL)  # x / 0: inf or nan on both sides, the same ones
        f1 = torch.view_as_real(d1) if cplx else d1
        for name, form in FORMS.items():
            d, _ = fe.contract(amp, divide=True, form=form)
            f = torch.view_as_real(d) if cplx else d
            assert torch.equal(torch.isnan(f), torch.isnan(f1)) and torch.equal(f[~torch.isnan(f)], f1[~torch.isnan(f1)]), name


@pytest.mark.parametrize("system,N", [("one word, 64 kept", 1000), ("two words, 512 kept", 513), ("two words, 64 kept", 0)])
@pytest.mark.parametrize("layout", ["list", "look-back"])
def test_holes_anywhere(system, N, layout):
    """records struck out at random, slot by slot and whole runs of 64 - 256 slots (dead trips between live ones, in the kept and in the
    drawn list): where the live slots are is read off the columns, not assumed"""
    n = 36
    fe, nu = _front(system, n, N, layout)
    fe = _copy_records(fe)
    g = torch.Generator().manual_seed(N + len(layout))
    for name in ("rec_col", "srec_col"):
        col = getattr(fe, name)
        hole = torch.rand(col.numel(), generator=g) < 0.3
        for at in torch.randint(0, max(col.numel(), 1), (max(col.numel() // 300, 4),), generator=g).tolist():
            hole[at: at + 64 * (1 + at % 4)] = True
        col[hole.cuda()] = -1
    fe._io = fe._make_io()
    for cplx in (False, True):
        _same_as_serial(fe, _amps(nu, cplx, 8), divide=False, tag=f"holes {system} N={N} {layout} cplx={cplx}")


def _copy_records(fe):
    """the front end with its record arrays replaced by copies (the test writes into them)"""
    for name in ("rec_col", "rec_link", "srec_col", "srec_link"):
        setattr(fe, name, getattr(fe, name).clone())
    return fe
