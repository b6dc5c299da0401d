"""tests/jchildren_exact.py on the CPU: a float64 host mirror of the formula pynqs_jastrow_children_apply evaluates (written apart from the
kernel, in numpy) stays under the a-priori bound on every case, and each mistake such a kernel could make misses the bound by more than
ten bounds on some row of every case it is tried on -- so a GPU test that passes on these cases has excluded it.  No GPU, no library."""
import numpy as np
import pytest

import children_cases as CC
import jchildren_exact as JC
import rbm_exact as R

MISTAKES = ("pair-dropped", "sign-of-r", "q0-dropped", "diagonal-left-in", "x-of-the-child", "parent+1", "parent-1", "upper-triangle-of-M")
STRANGER_MISTAKES = ("truncated-to-four", "clamped-to-walker-0")


def _words_to_flips(d: np.ndarray, sorb: int) -> np.ndarray:
    """orbitals of the set bits of uint64 [m, len] words, int [m, 4] padded with -1 (at most four bits set per row)"""
    bits = R.pm1(d, sorb) > 0
    out = np.full((d.shape[0], 4), -1, dtype=np.int64)
    for k, row in enumerate(bits):
        o = np.flatnonzero(row)
        assert o.size <= 4
        out[k, :o.size] = o
    return out


def mirror(b: JC.Built, mistake: str = "") -> np.ndarray:
    """psi of the rows in float64: psi_RBM (the exact value rounded to a double) times exp(q0[p] + Delta), strangers from scratch"""
    sorb, M = b.case.sorb, b.M
    S = M + M.T
    if mistake == "upper-triangle-of-M":
        S = np.triu(M, 1) + np.triu(M, 1).T
    Sr = S.copy()
    if mistake != "diagonal-left-in":
        np.fill_diagonal(Sr, 0.0)
    np.fill_diagonal(S, 0.0)
    tr = float(np.trace(M))
    xp = R.pm1(b.parents, sorb)
    r = xp @ Sr
    q0 = tr + 0.5 * (xp * r).sum(1)
    xc = R.pm1(b.rows, sorb)
    nw = b.parents.shape[0]
    par = b.parent.astype(np.int64)
    inside = (par >= 0) & (par < nw)
    d = b.rows ^ b.parents[np.where(inside, par, 0)]
    nflip = (R.pm1(d, sorb) > 0).sum(1)
    stranger = ~inside | (nflip > 4)
    if mistake == "truncated-to-four":
        trunc = inside & (nflip > 4)
        d = np.where(trunc[:, None], CC.lowest_four(d), d)
        stranger = ~inside
    if mistake == "clamped-to-walker-0":
        d = np.where(inside[:, None], d, CC.lowest_four(b.rows ^ b.parents[0]))
        par = np.where(inside, par, 0)
        stranger = inside & (nflip > 4)
    e = np.empty(b.n)
    s = np.flatnonzero(stranger)
    e[s] = tr + 0.5 * ((xc[s] @ S) * xc[s]).sum(1)
    c = np.flatnonzero(~stranger)
    F = _words_to_flips(d[c], sorb)
    on = F >= 0
    Fz = np.where(on, F, 0)
    p = par[c]
    tp = p  # the parent whose table row is read
    if mistake in ("parent+1", "parent-1"):
        tp = (p + (1 if mistake == "parent+1" else -1)) % nw
    src = xc[c] if mistake == "x-of-the-child" else xp[p]
    xs = np.where(on, np.take_along_axis(src, Fz, 1), 0.0)
    lin = (xs * np.take_along_axis(r[tp], Fz, 1)).sum(1)
    pair = np.zeros(c.size)
    if mistake != "pair-dropped":
        for i in range(4):
            for j in range(i + 1, 4):
                pair += S[Fz[:, i], Fz[:, j]] * xs[:, i] * xs[:, j]
    delta = (2.0 if mistake == "sign-of-r" else -2.0) * lin + 4.0 * pair
    e[c] = (0.0 if mistake == "q0-dropped" else q0[tp]) + delta
    return np.exp(b.ex_rbm.re).astype(np.float64) * np.exp(e)


@pytest.mark.parametrize("name", JC.ALL_CASES)
def test_the_mirror_meets_the_bound_and_the_case_is_what_its_name_says(name):
    b = JC.build(name)
    c = b.case
    assert b.rows.shape == (c.n, (c.sorb - 1) // 64 + 1) and b.n == c.n
    ratio = b.ratio(mirror(b))
    print(f"{name}: worst error / bound {ratio.max():.3g}")
    assert bool((ratio <= 1.0).all()), (name, float(ratio.max()), int(ratio.argmax()))
    if c.n >= 8:
        assert {0, 2}.issubset(set(b.nflip[b.stranger == 0].tolist())) and (c.sorb < 4 or 4 in b.nflip[b.stranger == 0])
    if c.n > 1:
        assert int(b.true_parent.max()) == c.nw - 1  # the last parent is in use
    if c.order == "runs":
        assert bool((np.diff(b.true_parent) >= 0).all())
    if c.strangers:
        assert set(b.stranger.tolist()) == set(range(len(CC.STRANGER_KINDS) + 1))
        assert bool(((b.parent < 0) | (b.parent >= c.nw)).sum() >= 3)
    # every edge orbital that exists is flipped by some row
    edges = {o for o in (0, 63, 64, 127, 128, c.sorb - 1) if o < c.sorb}
    if c.n >= 1025:
        assert edges <= set(b.flips[b.flips >= 0].tolist())


@pytest.mark.parametrize("name", JC.MISTAKE_CASES)
def test_mistakes_cannot_pass(name):
    b = JC.build(name)
    tried = MISTAKES + (STRANGER_MISTAKES if b.case.strangers else ())
    for m in tried:
        if m.startswith("parent") and b.case.nw == 1:
            continue
        ratio = b.ratio(mirror(b, m))
        assert float(np.nanmax(ratio)) > 10.0, (name, m, float(np.nanmax(ratio)))

