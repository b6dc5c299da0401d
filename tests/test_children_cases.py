"""The cases of tests/children_cases.py, on the CPU: every case is finite and well conditioned (rbm_exact.checked_case, inside the builder),
takes the form it names -- by rbm_exact.children_form and by the library's own query, pynqs_rbm_forward_children_geometry, which loads
without a GPU -- and its n stands where the list says relative to the sweeps.  And the mistakes the cases are there for cannot pass: each
is evaluated WITH THE REFERENCE ONLY (the exact psi of the row a wrong kernel would have computed, rounded to double) and must move at
least one row of the region it concerns by more than ten bounds."""
import numpy as np
import pytest

import children_cases as CC
import rbm_exact as R


def test_the_query_is_the_launch_rule():
    """form, workgroups and rows per sweep for both forms: one row is one workgroup, the caps hold from some n on, and the rows per sweep
    are workgroups x rows per workgroup (LDS: a thread per row on both routes; wave: 4 waves x 16 rows, or 256 threads from scratch)"""
    for kind, sorb, H in (("real", 64, 60), ("complex", 184, 9), ("real", 64, 62), ("complex", 32, 62)):
        form = R.children_form(sorb, H, kind)
        per_table, per_scratch = (CC.LDS_GROUP, CC.LDS_GROUP) if form == "lds" else (4 * CC.WAVE_GROUP, 256)
        assert CC.geometry(kind, sorb, H, 0) == (form, 0, 0, 0)
        assert CC.geometry(kind, sorb, H, 1) == (form, 1, per_table, per_scratch)
        assert CC.geometry(kind, sorb, H, per_table + 1) == (form, 2, 2 * per_table, 2 * per_scratch)
        f, wg, table, scratch = CC.geometry(kind, sorb, H, 1 << 30)
        assert f == form and table == wg * per_table and scratch == wg * per_scratch
        assert CC.geometry(kind, sorb, H, table) == CC.geometry(kind, sorb, H, table + 1) == (form, wg, table, scratch)
        assert CC.geometry(kind, sorb, H, table - per_table)[1] == wg - 1
    from pynqs_amd import _native as N
    import ctypes

    out = (ctypes.c_int64 * 4)()
    assert N.lib().pynqs_rbm_forward_children_geometry(-1, 12, 3, N.RBM_REAL, out) != 0
    assert N.lib().pynqs_rbm_forward_children_geometry(1, 12, 3, 3, out) != 0
    assert N.lib().pynqs_rbm_forward_children_geometry(1, 12, 3, N.RBM_REAL, None) != 0


def test_the_table_sizes_are_the_ones_the_cases_name():
    size = lambda kind, sorb, H: (2 * sorb + 1) * ((H + 2) | 1) * (16 if kind == "complex" else 8)  # noqa: E731
    assert size("real", 64, 60) == 65016 and size("real", 64, 62) == 67080 and size("complex", 184, 9) == 64944 and size("complex", 32, 62) == 67600
    assert size("real", 64, 61) == 65016 and size("real", 65, 60) > 65536  # (H 61 pads to the same 63 entries; one more orbital is too many)


def _region(b):
    """the rows the case is about: those of the second sweep where n reaches it, else the last partial workgroup / group of sixteen"""
    sweep = CC.sweep_of(b.case, b.n)
    if b.n > sweep:
        return np.arange(sweep, b.n)
    group = CC.LDS_GROUP if b.case.form == "lds" else CC.WAVE_GROUP
    return np.arange((b.n - 1) // group * group, b.n)


def _moved(b, sel, wrong_words=None, wrong_psi=None):
    """error / bound of the rows `sel` if the kernel had computed the rows `wrong_words` instead (or returned `wrong_psi`)"""
    if wrong_psi is None:
        wrong_psi = CC.as_double(b.case.kind, R.exact_ld(b.rbm, R.pm1(wrong_words, b.case.sorb)).psi())
    return R.amp_ratio(b.rbm, wrong_psi, b.exact(sel))


@pytest.mark.parametrize("name", CC.ALL_CASES)
def test_case_is_what_its_name_says(name):
    b = CC.build(name)
    c = b.case
    form, wg, table, scratch = CC.geometry(c.kind, c.sorb, c.H, b.n)
    assert form == c.form == R.children_form(c.sorb, c.H, c.kind)
    group = CC.LDS_GROUP if form == "lds" else CC.WAVE_GROUP
    assert table == wg * (CC.LDS_GROUP if form == "lds" else 4 * CC.WAVE_GROUP)
    rows, par = b.rows, b.parent
    assert rows.shape == (b.n, (c.sorb - 1) // 64 + 1) and par.shape == (b.n,) and par.dtype == np.int32 and b.parents.shape[0] == c.nw
    ok = b.stranger == 0
    nflip = np.unpackbits((rows[ok] ^ b.parents[par[ok]]).view(np.uint8), axis=1).sum(1)
    assert int(nflip.max()) <= 4 and set(nflip.tolist()) >= {0, 2, 4} and int(par[ok].min()) >= 0
    assert int(par[ok].max()) == c.nw - 1, "the last parent is in use"
    if c.order == "runs":
        assert bool((np.diff(par[ok]) >= 0).all())
    elif c.nw > 1:
        assert bool((np.diff(par[ok]) < 0).any())
    # where n stands relative to the sweeps
    sweep = CC.sweep_of(c, b.n)
    if not isinstance(c.n, int):
        assert sweep == CC.full_sweeps(c)[1 if c.raised else 0] and b.n == sweep + c.n[1] and 0 < c.n[1] < sweep
    else:
        assert b.n <= sweep
    tail = (b.n - 1) % group + 1
    expect = {"lds-second-sweep": 1, "lds-three-workgroups": 1, "lds-largest-real-table": 1, "lds-complex-near-the-limit": 1,
              "wave-second-sweep": 5, "wave-complex": 7, "lds-second-sweep-raised": 1}
    if name in expect:
        assert tail == expect[name], (tail, group)
    if name == "lds-three-workgroups":
        assert wg == 3
    if name in ("lds-tanh", "lds-prbm", "lds-overflow-one-338-w", "lds-overflow-chunk-50"):
        assert wg >= 3
    if name == "wave-h129-one-parent":
        assert c.H % 64 == 1 and c.H // 64 == 2  # lane 0 has three hidden units, the others two
    if name == "wave-raised":
        assert (b.n - sweep) == 300 and scratch == wg * 256
    # the rounding of the exact values to double is far inside the bound
    some = np.unique(np.concatenate([np.arange(min(b.n, 2048)), _region(b)]))
    r = R.amp_ratio(b.rbm, CC.as_double(c.kind, b.exact(some).psi()), b.exact(some))
    assert float(r.max()) <= 0.02, float(r.max())


@pytest.mark.parametrize("name", CC.RAISED_CASES)
def test_raised_cases_raise_the_flag_with_the_last_parent_alone(name):
    b = CC.build(name)
    th = CC.parent_theta(b.rbm, b.parents, b.case.sorb)
    assert bool((th[-1] < -340).any()) and int((th[-1] < -340).sum()) == 1
    assert bool((th[:-1] >= -330).all()), float(th[:-1].min())
    assert int(b.parent.max()) == b.case.nw - 1


@pytest.mark.parametrize("name", ["lds-overflow-one-338-w", "lds-overflow-chunk-50"])
def test_overflow_cases_have_overflow_rows_in_several_workgroups(name):
    """rows whose product of 1 + q_h (or whose q_h after the flips) leaves the range of a double while the parents stay above -340: from
    the reference, sum_h max(0, -2 Re theta_h(row)) > 709 or some -2 Re theta_h(row) > 709"""
    b = CC.build(name)
    x = R.pm1(b.pool, b.case.sorb).astype(R.LD)
    th = b.rbm.hb.astype(R.LD) + x @ b.rbm.W.T.astype(R.LD)
    over = (np.maximum(-2 * th, 0).sum(1) > 709.8)[b.idx]
    assert bool((CC.parent_theta(b.rbm, b.parents, b.case.sorb) > -340).all())
    groups = set((np.flatnonzero(over) // CC.LDS_GROUP).tolist())
    assert len(groups) >= 3 and 0 < int(over.sum()), (int(over.sum()), groups)


@pytest.mark.parametrize("name", CC.STRANGER_CASES)
def test_strangers_sit_where_the_layout_says(name):
    b = CC.build(name)
    c, s = b.case, b.stranger != 0
    assert set(b.stranger[s].tolist()) == set(range(1, 1 + len(CC.STRANGER_KINDS)))
    waves = s[: b.n // 64 * 64].reshape(-1, 64)
    assert bool(waves.all(1).any()) and bool((~waves.any(1)).any())
    assert bool(((waves.sum(1) == 1) & waves[:, 0]).any()) and bool(((waves.sum(1) == 1) & waves[:, -1]).any())
    groups = s[: b.n // 16 * 16].reshape(-1, 16)
    assert bool(groups.all(1).any()) and bool((groups[:, 0] & groups[:, 7] & groups[:, 15] & (groups.sum(1) == 3)).any())
    assert bool(s[CC.LDS_GROUP:].any()) and bool(s[-1])
    par, rows = b.parent, b.rows
    for k, kname in enumerate(CC.STRANGER_KINDS, 1):
        at = np.flatnonzero(b.stranger == k)
        if k <= 3:
            assert bool((par[at] == (-1, c.nw, c.nw + 5)[k - 1]).all())
            continue
        assert bool(((par[at] >= 0) & (par[at] < c.nw)).all())
        d = rows[at] ^ b.parents[par[at]]
        nflip = np.unpackbits(d.view(np.uint8), axis=1).sum(1)
        assert bool((nflip == (c.sorb if kname == "fall" else int(kname[1]))).all())
        if kname[0] == "s" and d.shape[1] > 1:
            assert bool((np.unpackbits(d[:, :1].view(np.uint8), axis=1).sum(1) == 4).all()) and bool((d[:, -1] != 0).all())


@pytest.mark.parametrize("name", CC.ALL_CASES)
def test_mistakes_cannot_pass(name):
    b = CC.build(name)
    c = b.case
    rows, par = b.rows, b.parent
    sweep = CC.sweep_of(c, b.n)
    if b.n > sweep:  # a row of a later sweep taken as row i mod sweep
        late = np.arange(sweep, b.n)
        r = _moved(b, late, wrong_psi=CC.as_double(c.kind, b.exact(late % sweep).psi()))
        assert float(r.max()) > 10.0, ("i mod sweep", float(r.max()))
    reg = _region(b)
    reg = reg[b.stranger[reg] == 0]
    if c.nw > 1 and not c.raised and reg.size:  # the neighbour's row of the parent table with this row's flips
        for off in (1, -1):
            wrong = b.parents[(par[reg] + off) % c.nw] ^ (rows[reg] ^ b.parents[par[reg]])
            r = _moved(b, reg, wrong)
            assert float(r.max()) > 10.0, ("parent off by one", off, float(r.max()))
    if reg.size > 1:  # the row before / after (an index off by one in the last group)
        r = _moved(b, reg[1:], wrong_psi=CC.as_double(c.kind, b.exact(reg[:-1]).psi()))
        assert float(r.max()) > 10.0, ("row off by one", float(r.max()))
    if c.strangers:
        far = np.flatnonzero(b.stranger > 3)
        wrong = b.parents[par[far]] ^ CC.lowest_four(rows[far] ^ b.parents[par[far]])
        r = _moved(b, far, wrong)
        for k in range(4, 1 + len(CC.STRANGER_KINDS)):  # every kind of them
            assert float(r[b.stranger[far] == k].max()) > 10.0, ("truncated to four flips", CC.STRANGER_KINDS[k - 1], float(r[b.stranger[far] == k].max()))
        out = np.flatnonzero((b.stranger > 0) & (b.stranger <= 3))
        wrong = b.parents[0] ^ CC.lowest_four(rows[out] ^ b.parents[0])
        r = _moved(b, out, wrong)
        for k in (1, 2, 3):
            assert float(r[b.stranger[out] == k].max()) > 10.0, ("clamped to walker 0", CC.STRANGER_KINDS[k - 1], float(r[b.stranger[out] == k].max()))


def test_lowest_four():
    d = np.array([[0b101101, 0], [0b11, 0b1110], [0, 1 << 63], [0, 0]], dtype=np.uint64)
    want = np.array([[0b101101, 0], [0b11, 0b0110], [0, 1 << 63], [0, 0]], dtype=np.uint64)
    assert np.array_equal(CC.lowest_four(d), want)
    d = np.array([[0xFF, 0xF]], dtype=np.uint64)
    assert np.array_equal(CC.lowest_four(d), np.array([[0xF, 0]], dtype=np.uint64))
