"""gfmc_sample_kernel -- the GFMC move behind pynqs_gfmc_sample and pynqs_gfmc_sample_rank -- against the law of include/pynqs_amd.h held in
exact integer arithmetic by tests/gfmc_exact.py:
    index = k only if  C_{k-1} - tau < u S <= C_k + tau  and  (G_k > 0 or k = 0),  tau = m 2^-52 S;   S = 0 gives index 0;
    |beta - S| <= (m - 1) 2^-53 S, bit-equal for equal rows and across the two entry points;   x_new = column `index` of the comb.
Every walker of every case is checked; the uniforms sit on the CDF boundaries of the rows (fl(C_j / S) and -1, +1, +2 ulp), where the
scan's additions decide, next to random ones, u = 0 and 1 - 2^-53.  tests/test_gfmc_exact.py checks on the CPU that the boundary cases
are not vacuous and that the sequential answer obeys the same law.

Before the move selected among columns with weight only, the tile and column searches took the first running sum to reach the target:
the Hillis-Steele scan adds lane k and lane k - 1 in different trees, so across a zero-weight column the sum can rise by an ulp and a
target between the two selected that column -- in fixed-node GFMC a move across the node.
"""
import numpy as np
import pytest
import torch

import eloc_exact as X
import gfmc_exact as GX
import test_gpu_eloc_exact as E

pytestmark = pytest.mark.gpu

_dev, _bra = E._dev, E._bra
SLAB = 1024
SHAPES = {"12.3+2": (12, 3, 2), "16.4+4": (16, 4, 4), "66.2+1": (66, 2, 1), "130.2+1": (130, 2, 1), "fe2s2": (40, 15, 15)}
RANK_SHAPES = {"4.1+0": (4, 1, 0), "8.2+2": (8, 2, 2), "12.3+2": (12, 3, 2), "16.4+4": (16, 4, 4), "66.1+1": (66, 1, 1), "66.2+1": (66, 2, 1),
               "130.1+1": (130, 1, 1), "130.2+1": (130, 2, 1), "fe2s2": (40, 15, 15)}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sample(gk, u, comb):
    """pynqs_gfmc_sample on device tensors gk [n, m], u [n], comb uint8 [n, m, 8 L]: (index, beta, x_new)"""
    from pynqs_amd import _native as N

    n, m = gk.shape
    L = comb.size(-1) // 8
    assert gk.is_contiguous() and comb.is_contiguous() and u.is_contiguous() and comb.shape == (n, m, 8 * L)
    index = torch.full((n,), -7, dtype=torch.int64, device=gk.device)
    beta = torch.full((n,), -7.0, dtype=torch.float64, device=gk.device)
    x_new = torch.full((n, 8 * L), 0xEE, dtype=torch.uint8, device=gk.device)
    N.check(N.lib().pynqs_gfmc_sample(gk.data_ptr(), n, m, u.data_ptr(), comb.data_ptr(), 64 * L, index.data_ptr(), beta.data_ptr(), x_new.data_ptr(),
                                      _stream()), "pynqs_gfmc_sample")
    return index, beta, x_new


def _sample_rank(gk, u, bra, sorb, noA, noB):
    """pynqs_gfmc_sample_rank on device tensors gk [n, nsd + 1], u [n], bra uint8 [n, 8 L]"""
    from pynqs_amd import _native as N

    n = gk.size(0)
    assert gk.is_contiguous() and bra.is_contiguous() and u.is_contiguous() and bra.size(0) == n
    index = torch.full((n,), -7, dtype=torch.int64, device=gk.device)
    beta = torch.full((n,), -7.0, dtype=torch.float64, device=gk.device)
    x_new = torch.full_like(bra, 0xEE)
    N.check(N.lib().pynqs_gfmc_sample_rank(gk.data_ptr(), n, u.data_ptr(), bra.data_ptr(), sorb, noA + noB, noA, noB, index.data_ptr(), beta.data_ptr(),
                                           x_new.data_ptr(), _stream()), "pynqs_gfmc_sample_rank")
    return index, beta, x_new


def _laid_out(c):
    """the case on the device: rows [R, m], the row of every walker, the uniforms"""
    bl = GX.blocks(c)
    rows = _dev(np.stack([b.row.g for b in bl]))
    which = np.concatenate([np.full(b.u.size, i) for i, b in enumerate(bl)])
    u = np.concatenate([b.u for b in bl])
    return bl, rows, which, u


class Tally:
    """what the README's tests cell quotes, per case: boundary uniforms, how they resolved, the worst |beta - S| / bound"""

    def __init__(self):
        self.n = self.near = self.lower = self.upper = 0
        self.beta = 0.0

    def line(self, what):
        return (f"{what}: {self.n} walkers, {self.near} boundary uniforms ({self.lower} to the lower, {self.upper} to the upper neighbour), "
                f"worst |beta - S| / bound {self.beta:.3g}")


def _check_case(c, bl, which, u, index, beta, tally):
    """every walker: the law; beta within its bound and bit-equal over the walkers of a row.  Returns the failures."""
    bad, o = [], 0
    for i, b in enumerate(bl):
        n = b.u.size
        assert bool((which[o:o + n] == i).all())
        idx, be = index[o:o + n], beta[o:o + n]
        for w in GX.check_moves(b.row, b.u, idx):
            bad.append((GX.case_id(c), "row", i) + w)
        ok, ratio = GX.beta_check(b.row, float(be[0]))
        tally.beta = max(tally.beta, ratio)
        assert ok, (GX.case_id(c), i, float(be[0]), ratio)
        assert bool((be.view(np.uint64) == be.view(np.uint64)[0]).all()), (GX.case_id(c), i, "beta differs between walkers of one row")
        for x, k in zip(b.u.tolist(), idx.tolist()):
            j = GX.nearest_boundary(b.row, x)
            if j >= 0:
                tally.near += 1
                tally.lower += int(k == j)
                tally.upper += int(k > j)
        tally.n += n
        o += n
    assert o == u.size == index.size
    return bad


def _report(bad, what):
    """the failures per case: walkers outside the law (of them on a zero-weight column)"""
    per = {}
    for w in bad:
        a = per.setdefault(w[0], [0, 0])
        a[0] += 1
        a[1] += int(w[5] > 0 and w[-1] == 0.0)
    counts = ", ".join(f"{k} {v[0]} ({v[1]})" for k, v in per.items())
    return f"{what}: {len(bad)} walkers outside the law (on a zero-weight column), per case: {counts}; first: {bad[:3]}"


@pytest.mark.parametrize("m", [m for m in GX.WIDTHS if m <= 2048])
def test_materialised_move_obeys_the_law_at_the_cdf_boundaries(m):
    """pynqs_gfmc_sample, every case of the width, comb of random bytes with L = 1, 2, 3 words (one index for all three); through
    gfmc.sample_update: w_new = fl(w beta) and the accepted count"""
    from pynqs_amd import gfmc

    gen = torch.Generator(device="cuda").manual_seed(m)
    bad = []
    for c in GX.cases_of(m):
        bl, rows, which, u = _laid_out(c)
        tally, first = Tally(), None
        for L in (1, 2, 3):
            index, beta = np.empty(u.size, dtype=np.int64), np.empty(u.size)
            for o in range(0, u.size, SLAB):
                w_ = torch.from_numpy(which[o:o + SLAB]).cuda()
                gk, uu = rows[w_].contiguous(), _dev(u[o:o + SLAB])
                comb = torch.randint(0, 256, (gk.size(0), m, 8 * L), generator=gen, dtype=torch.uint8, device="cuda")
                i_, b_, x_ = _sample(gk, uu, comb)
                assert bool(((i_ >= 0) & (i_ < m)).all()), (GX.case_id(c), "index out of range")
                assert torch.equal(x_, comb[torch.arange(gk.size(0), device="cuda"), i_]), (GX.case_id(c), L, "x_new is not the comb row of index")
                index[o:o + SLAB], beta[o:o + SLAB] = i_.cpu().numpy(), b_.cpu().numpy()
                if L == 1:
                    wgt = torch.rand(gk.size(0), generator=gen, dtype=torch.float64, device="cuda") + 0.5
                    x2, w_new, beta2, acc = gfmc.sample_update(None, wgt, comb, gk, uu.reshape(-1, 1))
                    assert torch.equal(x2, x_) and torch.equal(beta2.reshape(-1), b_)
                    assert np.array_equal(w_new.cpu().numpy(), wgt.cpu().numpy() * b_.cpu().numpy()) and acc == int((i_ != 0).sum())
            if first is None:
                first = (index, beta)
                bad += _check_case(c, bl, which, u, index, beta, tally)
                print(tally.line(GX.case_id(c)))
            else:
                assert np.array_equal(index, first[0]) and np.array_equal(beta.view(np.uint64), first[1].view(np.uint64)), (GX.case_id(c), L)
    assert not bad, _report(bad, f"m = {m}")


@pytest.mark.parametrize("m", GX.LONG_WIDTHS)
def test_long_rows_obey_the_law(m):
    """262 144 columns are exactly 1024 tiles of 256, 262 145 the first width with tiles of 512; eight walkers per row"""
    gen = torch.Generator(device="cuda").manual_seed(m)
    bad = []
    for c in GX.cases_of(m):
        bl, rows, which, u = _laid_out(c)
        assert u.size == 8 and len(bl) == 1
        gk, uu = rows[torch.from_numpy(which).cuda()].contiguous(), _dev(u)
        tally, first = Tally(), None
        for L in (1, 2, 3):
            comb = torch.randint(0, 256, (8, m, 8 * L), generator=gen, dtype=torch.uint8, device="cuda")
            i_, b_, x_ = _sample(gk, uu, comb)
            assert bool(((i_ >= 0) & (i_ < m)).all())
            assert torch.equal(x_, comb[torch.arange(8, device="cuda"), i_]), (GX.case_id(c), L)
            if first is None:
                first = (i_, b_)
                bad += _check_case(c, bl, which, u, i_.cpu().numpy(), b_.cpu().numpy(), tally)
                print(tally.line(GX.case_id(c)))
            else:
                assert torch.equal(i_, first[0]) and torch.equal(b_, first[1])
    assert not bad, _report(bad, f"m = {m}")


def _comb_of(occ, sorb, noA, noB):
    from oracle import oracle

    return oracle.comb(_bra(occ), sorb, noA, noB)[0]


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_rank_move_obeys_the_law_and_is_the_materialised_move_bit_for_bit(shape):
    """pynqs_gfmc_sample_rank on rows of the width a shape has, four walkers in turn: the law, x_new = the oracle's comb row of index, and
    index, beta, x_new equal to pynqs_gfmc_sample's on the materialised comb"""
    from pynqs_amd import public_function as pf

    sorb, noA, noB = SHAPES[shape]
    m = pf.get_Num_SinglesDoubles(sorb, noA, noB) + 1
    occ = E.rand_occ(4, sorb, noA, noB, seed=sorb)
    comb_h = _comb_of(occ, sorb, noA, noB)
    assert comb_h.shape[:2] == (4, m)
    comb_d, bra_d = _dev(comb_h), _dev(_bra(occ))
    slab = int(max(8, min(SLAB, 2 ** 27 // (m * comb_h.shape[2]))))
    bad = []
    for c in GX.cases_of(m):
        bl, rows, which, u = _laid_out(c)
        index, beta = np.empty(u.size, dtype=np.int64), np.empty(u.size)
        for o in range(0, u.size, slab):
            w_ = torch.from_numpy(which[o:o + slab]).cuda()
            gk, uu = rows[w_].contiguous(), _dev(u[o:o + slab])
            who = (torch.arange(o, o + gk.size(0), device="cuda") % 4)
            i_, b_, x_ = _sample_rank(gk, uu, bra_d[who].contiguous(), sorb, noA, noB)
            assert bool(((i_ >= 0) & (i_ < m)).all()), (GX.case_id(c), "index out of range")
            assert torch.equal(x_, comb_d[who, i_]), (GX.case_id(c), "x_new is not the excitation of rank index - 1")
            i2, b2, x2 = _sample(gk, uu, comb_d[who].contiguous())
            assert torch.equal(i_, i2) and torch.equal(b_, b2) and torch.equal(x_, x2), (GX.case_id(c), "the two entry points differ")
            index[o:o + slab], beta[o:o + slab] = i_.cpu().numpy(), b_.cpu().numpy()
        tally = Tally()
        bad += _check_case(c, bl, which, u, index, beta, tally)
        print(tally.line(f"{shape} {GX.case_id(c)}"))
    assert not bad, _report(bad, shape)


@pytest.mark.parametrize("shape", list(RANK_SHAPES), ids=list(RANK_SHAPES))
def test_every_rank_gives_the_oracles_comb_row(shape):
    """one-hot rows: row i has weight at column i alone (every other tile is empty), any u in (0, 1) gives index i and the comb row i"""
    from pynqs_amd import public_function as pf

    sorb, noA, noB = RANK_SHAPES[shape]
    m = pf.get_Num_SinglesDoubles(sorb, noA, noB) + 1
    occ = E.rand_occ(1, sorb, noA, noB, seed=3 * sorb + 1)
    comb_d, bra_d = _dev(_comb_of(occ, sorb, noA, noB)[0]), _dev(_bra(occ))
    assert comb_d.size(0) == m
    gen = torch.Generator(device="cuda").manual_seed(sorb)
    for o in range(0, m, 2048):
        n = min(2048, m - o)
        col = torch.arange(o, o + n, device="cuda")
        wgt = torch.rand(n, generator=gen, dtype=torch.float64, device="cuda") * 3.0 + 2.0 ** -30
        gk = torch.zeros((n, m), dtype=torch.float64, device="cuda")
        gk[torch.arange(n, device="cuda"), col] = wgt
        u = torch.rand(n, generator=gen, dtype=torch.float64, device="cuda") * 0.998 + 0.001
        i_, b_, x_ = _sample_rank(gk, u, bra_d.expand(n, -1).contiguous(), sorb, noA, noB)
        assert torch.equal(i_, col), (shape, o, int((i_ != col).sum()))
        assert torch.equal(b_, wgt) and torch.equal(x_, comb_d[col])


def test_the_empty_row_and_u_zero():
    """S = 0: index 0, beta = 0, x_new = x (both entry points).  u = 0: index 0 where G_0 > 0; where G_0 = 0, index 0 or the first column
    with weight and nothing else -- also behind leading empty tiles"""
    sorb, noA, noB = 12, 3, 2
    occ = E.rand_occ(1, sorb, noA, noB, seed=5)
    comb_h = _comb_of(occ, sorb, noA, noB)
    m = comb_h.shape[1]
    bra = _dev(_bra(occ)).expand(6, -1).contiguous()
    u = _dev(np.array([0.0, 0.25, 0.5, 0.75, GX.ONE_BELOW, 2.0 ** -1074]))
    gk = torch.zeros((6, m), dtype=torch.float64, device="cuda")
    i_, b_, x_ = _sample_rank(gk, u, bra, sorb, noA, noB)
    assert i_.tolist() == [0] * 6 and b_.tolist() == [0.0] * 6 and torch.equal(x_, bra)
    for width in (1, 5, 256, 257, 513, 7877, 262_145):
        gk = torch.zeros((6, width), dtype=torch.float64, device="cuda")
        comb = torch.randint(0, 256, (6, width, 16), dtype=torch.uint8, device="cuda")
        i_, b_, x_ = _sample(gk, u, comb)
        assert i_.tolist() == [0] * 6 and b_.tolist() == [0.0] * 6 and torch.equal(x_, comb[:, 0]), width
    zero = _dev(np.zeros(4))
    for width in (5, 257, 513, 7877, 262_145):
        for first in sorted({1, 3, min(width - 1, 255), min(width - 1, 256), min(width - 1, 300), width - 1}):
            g = np.zeros((4, width))
            g[0, first] = 2.0
            g[1, first:] = 0.5
            g[2, first::7] = 1.0
            g[3, 0], g[3, first] = 1e-300, 1.0
            comb = torch.randint(0, 256, (4, width, 8), dtype=torch.uint8, device="cuda")
            i_, _, x_ = _sample(_dev(g), zero, comb)
            assert i_[3].item() == 0 and all(k in (0, first) for k in i_[:3].tolist()), (width, first, i_.tolist())
            assert torch.equal(x_, comb[torch.arange(4, device="cuda"), i_])
            assert all(GX.accepts(g[r], 0.0, k) for r, k in enumerate(i_.tolist()))


def test_no_walkers_is_ok_and_writes_nothing():
    from pynqs_amd import _native as N

    index = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    beta = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    x_new = torch.full((4, 8), 0xEE, dtype=torch.uint8, device="cuda")
    gk, u = torch.ones((4, 5), dtype=torch.float64, device="cuda"), torch.full((4,), 0.5, dtype=torch.float64, device="cuda")
    comb = torch.zeros((4, 5, 8), dtype=torch.uint8, device="cuda")
    assert N.lib().pynqs_gfmc_sample(gk.data_ptr(), 0, 5, u.data_ptr(), comb.data_ptr(), 12, index.data_ptr(), beta.data_ptr(), x_new.data_ptr(),
                                     _stream()) == N.OK
    assert N.lib().pynqs_gfmc_sample(None, 0, 5, None, None, 12, None, None, None, _stream()) == N.OK
    assert N.lib().pynqs_gfmc_sample_rank(gk.data_ptr(), 0, u.data_ptr(), x_new.data_ptr(), 12, 5, 3, 2, index.data_ptr(), beta.data_ptr(),
                                          x_new.data_ptr(), _stream()) == N.OK
    torch.cuda.synchronize()
    assert bool((index == -7).all()) and bool((beta == -7.0).all()) and bool((x_new == 0xEE).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# a fixed-node walk

_GREEN = {}


def _walk_setup(kind):
    """(case, Lambda, module, exact-walker function of a Structure)"""
    if kind == "rbm":
        c = E.GREEN_CASES[0]
        assert (c.kind, c.sorb, c.noA, c.noB, c.H, c.regime) == ("real", 12, 3, 2, 24, "fe2s2")
        ref, lam, _ = E.green_reference(c)
        return c, lam, E._module(c, ref), lambda st: X.walker(ref.rbm, st)
    import jgreen_exact as JG
    import jrbm_exact as J
    import test_gpu_jgreen as TG

    c = JG.STEP_CASE
    ref, lam, _ = JG.green_reference(c)
    return c, lam, TG._module(ref), lambda st: J.walker(ref.rbm, ref.M, st)


def _exact_row(kind, c, lam, make_walker, occ, comb_bits):
    """eloc_exact.Green of a determinant in the oracle's column order, cached by determinant"""
    key = (kind, occ.tobytes())
    if key not in _GREEN:
        h1, h2 = E.integrals(c.ints, c.sorb)
        w = make_walker(X.structure(occ, h1, h2))
        _GREEN[key] = X.green(w, lam, X.match_columns(w, comb_bits))
    return _GREEN[key]


@pytest.mark.parametrize("kind", ["rbm", "jrbm"])
def test_a_fixed_node_walk_never_crosses_the_node(kind):
    """64 walkers, 12 generations of the fused green_kernel -> sample_update -> branching (xi from the host).  Every generation the rows are
    read back; even walkers get random uniforms, odd ones a CDF boundary of their own row (next to a zero-weight column where it has one).
    Per walker: the move obeys the law on the GPU's own row; x_new is x or a column that the exact reference keeps for sure (a sign-
    preserving move); |beta - sum g_exact| <= sum of the entry bounds + (m - 1) 2^-53 sum g_exact."""
    from oracle import oracle
    from pynqs_amd import gfmc, public_function as pf

    c, lam, module, make_walker = _walk_setup(kind)
    sorb, noA, noB = c.sorb, c.noA, c.noB
    h1, h2 = E.integrals(c.ints, sorb)
    n, gens = 64, 12
    rng = np.random.default_rng(17)
    x = _dev(_bra(E.rand_occ(n, sorb, noA, noB, seed=99)))
    w = torch.ones(n, dtype=torch.float64, device="cuda")
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    worst_beta, moved, on_zero_total = 0.0, 0, 0
    try:
        ab = lambda xx, func: pf.ansatz_batch(func, xx, 100000, sorb, x.device, torch.float64)  # noqa: E731
        for gen in range(gens):
            eloc, gk, comb, _, neg = gfmc.green_kernel(x, lam, _dev(h1), _dev(h2), module, ab, sorb, noA + noB, noA, noB)
            assert isinstance(comb, gfmc.CombRows), "the row did not come from the fused kernel"
            gk_h, x_h = gk.cpu().numpy(), x.cpu().numpy()
            comb_h = oracle.comb(x_h, sorb, noA, noB)[0]
            bits = np.unpackbits(comb_h, axis=-1, bitorder="little")[..., :sorb]
            rows = [GX.Row(g) for g in gk_h]
            u = rng.random(n)
            on_zero = 0
            for i in range(1, n, 2):
                pos = np.flatnonzero(rows[i].g > 0)
                zf = pos[[GX.zero_follows(rows[i], int(j)) for j in pos]]
                pick = zf if zf.size else pos
                if pick.size:
                    bu = GX.boundary_uniforms(rows[i], GX.OFFSETS, [int(rng.choice(pick))])
                    if bu.size:
                        u[i] = float(rng.choice(bu))
                j = GX.nearest_boundary(rows[i], u[i])
                on_zero += int(j >= 0 and GX.zero_follows(rows[i], j))
            assert on_zero >= 1, (gen, "no boundary uniform next to a zero-weight column")
            on_zero_total += on_zero
            x_new, w_new, beta, acc = gfmc.sample_update(x, w, comb, gk, _dev(u.reshape(n, 1)))
            xn_h, beta_h = x_new.cpu().numpy(), beta.cpu().numpy().reshape(n)
            assert np.array_equal(w_new.cpu().numpy(), w.cpu().numpy() * beta_h)
            index = np.empty(n, dtype=np.int64)
            for i in range(n):
                hit = np.flatnonzero((comb_h[i] == xn_h[i]).all(1))
                assert hit.size == 1, (gen, i, "x_new is no column of the comb")
                index[i] = hit[0]
                assert GX.accepts(rows[i], u[i], index[i]), (gen, i, u[i], int(index[i]), GX.exact_index(rows[i], u[i]), gk_h[i, index[i]])
                g = _exact_row(kind, c, lam, make_walker, bits[i, 0], bits[i])
                assert bool(neg[i]) == g.clamp
                assert index[i] == 0 or (g.keep[index[i]] and g.sure[index[i]]), (gen, i, int(index[i]), "a move across the node")
                s = float(g.g.sum())
                bound = float(g.bound.sum()) + (g.g.size - 1) * GX.U * s
                worst_beta = max(worst_beta, abs(float(X.LD(beta_h[i]) - g.g.sum())) / bound)
                assert abs(float(X.LD(beta_h[i]) - g.g.sum())) <= bound, (gen, i, beta_h[i], s, bound)
            assert acc == int((index != 0).sum())
            moved += acc
            x = gfmc.branching(x_new, w_new, _dev(rng.random(n)))
            w = torch.ones(n, dtype=torch.float64, device="cuda")
    finally:
        torch.set_default_dtype(old)
    print(f"walk {kind}: {gens} generations of {n} walkers, {moved} moves, {on_zero_total} boundary uniforms next to a zero-weight column, "
          f"{len([k for k in _GREEN if k[0] == kind])} exact rows, worst |beta - sum g| / bound {worst_beta:.3g}")
    assert moved > 0
