"""The yardstick of tests/ss_exact.py itself, on the CPU, and the cases of tests/test_gpu_ss_exact.py:
  * at scale 2^0 against oracle.eloc_sample_space (real and complex) and against the sum over the rows of oracle.comb_hij_fused with the
    table looked up on the host: the float64 oracle and the yardstick agree within the bound; the partner sum against the same rows with
    the package's own spin_flip_onv / spin_flip_sign;
  * the yardstick's own E(x) is unchanged to 4 longdouble ulps when every amplitude is multiplied by 2^k, for every k the GPU tests use;
  * every case's preconditions, from the reference alone: bound <= 1e-9 sum_k a_k |psi'_k| / |psi(x)| for every walker, as many walkers
    with psi(x) = 0 as were constructed that way, no sum near 2^1023 at the largest k and no term subnormal at the smallest, eps of the
    REDUCE cases inside a gap of the |h_k| wider than any rounding of a float32 / float64 matrix element (so that every precision keeps
    the same columns) with <x|H|x> kept, the two-word walkers' excitations on both sides of bit 64, and |psi| ~ 1e250 for the RBM case."""
import time

import numpy as np
import pytest

import ss_exact as S
import test_gpu_ss_exact as T

_CLOCK = {}


@pytest.fixture(scope="module", autouse=True)
def _clock():
    _CLOCK["t0"] = time.time()
    yield


def _oracle_inputs(name, table, values):
    from oracle import oracle as O

    s = T.SHAPES[name]
    h1, h2 = T.integrals(s.ints, s.sorb)
    bra = T._onv(T.walkers(name), s.sorb)
    keys = T._onv(T.table_keys(name, table), s.sorb)
    order = O.sort_keys(keys, s.sorb)
    return O, s, h1, h2, bra, np.ascontiguousarray(keys[order]), np.ascontiguousarray(T.mantissas(name, table, values)[order])


@pytest.mark.parametrize("values", ["real", "complex"])
@pytest.mark.parametrize("name,table", [("s12", "half"), ("s12", "absent2"), ("s66", "half"), ("s130", "half"), ("fe2s2", "half"),
                                         ("s40e33", "half"), ("s72e65", "half")])
def test_yardstick_matches_the_oracle_at_scale_one(name, table, values):
    O, s, h1, h2, bra, keys, wf = _oracle_inputs(name, table, values)
    e, p0 = O.eloc_sample_space(bra, h1, h2, s.sorb, s.noA + s.noB, s.noA, s.noB, keys, wf)
    plain, part = T.yardstick(name, table, values, 0)
    np.testing.assert_array_equal(p0, T.psi_array(plain, wf.dtype))
    ratio, finite_zero = T.ratios(plain, e)
    print(T.report(f"oracle.eloc_sample_space {name} {table} {values}", ratio))
    assert finite_zero == 0 and bool((ratio <= 1.0).all())
    # the rows of oracle.comb_hij_fused, the table looked up on the host by the bytes of the packed determinant
    import torch

    from pynqs_amd import public_function as pf

    comb, hm = O.comb_hij_fused(bra, h1, h2, s.sorb, s.noA + s.noB, s.noA, s.noB)
    where = {k.tobytes(): i for i, k in enumerate(keys)}
    look = lambda rows: np.array([wf[where[r.tobytes()]] if r.tobytes() in where else 0 for r in rows], dtype=wf.dtype)  # noqa: E731
    e2, e3 = np.zeros(len(plain), dtype=wf.dtype), np.zeros(len(plain), dtype=wf.dtype)
    with np.errstate(all="ignore"):
        for i in range(len(plain)):
            psi = look(comb[i])
            e2[i] = (hm[i] * psi).sum() / psi[0]
            ct = torch.from_numpy(np.ascontiguousarray(comb[i]))
            e3[i] = (hm[i] * pf.spin_flip_sign(ct, s.sorb).numpy() * look(pf.spin_flip_onv(ct, s.sorb).numpy())).sum() / psi[0]
    r2, _ = T.ratios(plain, e2)
    r3, _ = T.ratios(part, e3)
    print(T.report("sum over oracle.comb_hij_fused rows", r2), T.report("partner sum over the same rows", r3))
    assert bool((r2 <= 1.0).all()) and bool((r3 <= 1.0).all())


def test_cases_are_scale_invariant_bounded_and_count_their_zero_walkers():
    ulp = 2 * S.X.R.U_LD
    for case in T.CASES:
        name, table = case
        nzero = T.zero_walkers(name, table)
        s = T.SHAPES[name]
        assert table != "one" or T.table_keys(name, table).shape[0] == 1
        if table == "absent2":
            assert nzero >= 2
        for values in T.VALUES:
            ks = T.scales_of(values)
            assert set(ks) >= {0, 300, -300, 520, -520, 600, -600} and (values.endswith("spread") or 900 in ks)
            base, base_part = T.yardstick(name, table, values, 0)
            worst = 0.0
            for k in ks:
                plain, part = T.yardstick(name, table, values, k)
                assert sum(r.zero for r in plain) == nzero == sum(r.zero for r in part), (case, values, k)
                for r0, r in list(zip(base, plain)) + list(zip(base_part, part)):
                    if r.zero:
                        continue
                    assert abs(complex(r.E - r0.E)) <= 4 * ulp * abs(complex(r0.E)), (case, values, k)
                    if r.m == 0:  # (an empty sum, e.g. a flip pass that finds no partner: exactly zero, nothing to round)
                        assert r.E == 0 and r.bound == 0
                        continue
                    assert np.isfinite(r.bound) and 0 < r.bound <= 1e-9 * r.A, (case, values, k, r.bound, r.A)
                    assert r.top < 1023 and r.low > -1000, (case, values, k, r.top, r.low)
                    worst = max(worst, r.bound / r.A)
            if table in ("all", "half"):  # the flip passes are not empty sums
                assert sum(r.m for r in base_part) >= 20 * (1 if s.n < 10 else 10), (case, [r.m for r in base_part])
            if values.endswith("spread"):  # the moduli do span 2^+-200 inside one neighbourhood
                _, cols, _ = T.neighbourhoods(name, table)
                m = np.abs(T.mantissas(name, table, values))
                spans = [np.log2(m[c.pos[c.pos >= 0]].max() / m[c.pos[c.pos >= 0]].min()) for c in cols if (c.pos >= 0).sum() > 30]
                assert not spans or max(spans) > 300, (case, max(spans))
            print(f"{T.case_id(case)} {values}: {s.n} walkers, {nzero} with psi(x) = 0, {T.table_keys(name, table).shape[0]} keys, max bound / A {worst:.3g}")


def test_two_word_walkers_cross_bit_64_and_large_tables_stream_in_chunks():
    occ = T.walkers("s66")
    assert occ[:, :64].any(1).all() and occ[:, 64:].any() and not occ[:, 64:].all()
    _, cols, colsf = T.neighbourhoods("s66", "half")
    for c in cols + colsf:   # holes / particles (and their spin-flip partners) on both sides of bit 64 among the keys that are found
        found = np.concatenate([c.st.occ[None, :], c.st.bits])[c.pos >= 0]
        moved = found ^ c.st.occ[None, :]
        assert moved[:, :64].any() and moved[:, 64:].any()
    for name, n in (("s130", 2), ("fe2s2", 4)):  # more than 2048 keys for a handful of walkers: the streamed kernel cuts the keys into chunks
        assert T.table_keys(name, "all").shape[0] > 2 * 2048 and T.SHAPES[name].n == n
    # chunks per walker of the column-major launch (plan_chunks; the REDUCE front end without draws cuts a row the same way): one
    # workgroup divides by psi(x) itself at sorb 12, several meet through atomics and the divide kernel follows for the others
    from pynqs_amd import reduce_front as RF

    chunks = {name: RF.geometry(s.n, s.sorb, s.noA + s.noB, s.noA, s.noB, 0)[0] // s.n for name, s in T.SHAPES.items()}
    assert chunks["s12"] == chunks["s12one"] == 1 and min(chunks["fe2s2"], chunks["s66"], chunks["s130"]) > 1, chunks
    far = T.table_keys("s66", "far")[3:]
    assert all((np.bitwise_xor(r[None, :], occ).sum(1) >= 6).all() for r in far)


def test_many_electron_shapes_reach_the_second_round_of_the_diagonals_lanes():
    """33 electrons on one word, 65 on two (fast_diag strides its 64 lanes over the electrons: 65 is the first count with a second round);
    two distinct walkers each, the tables "all" and "half", every amplitude set; the diagonal is a sum of nele (nele + 1) / 2 terms and
    each single one of nele, which is what the bound's t_k counts"""
    for name, sorb, nele in (("s40e33", 40, 33), ("s72e65", 72, 65)):
        s = T.SHAPES[name]
        assert (s.sorb, s.noA + s.noB, s.n, s.ints) == (sorb, nele, 2, "syn") and {t for n, t in T.CASES if n == name} == {"all", "half"}
        occ = T.walkers(name)
        assert len({r.tobytes() for r in occ}) == 2
        for st in T.structures(name):
            assert st.t0 == nele * (nele + 1) // 2 and set(np.unique(st.t).tolist()) == {1, nele}
        tab, cols, colsf = T.neighbourhoods(name, "half")
        for c in cols:   # about half of a walker's columns are found, singles and doubles among them
            found = c.pos[1:] >= 0
            assert c.pos[0] >= 0 and 0.4 < found.mean() < 0.6 and (c.st.t[found] == nele).any() and (c.st.t[found] == 1).any()
    assert max(s.noA + s.noB for n, s in T.SHAPES.items() if n not in ("s40e33", "s72e65")) == 30


def test_reduce_cases_have_eps_inside_a_gap():
    for c in T.REDUCE_CASES:
        sts = T.reduce_structures(c)
        eps, half = T.reduce_eps(c)
        if c.eps == "0":
            # eps = 0 keeps every column: the REDUCE form is the full sum
            tab = S.Table(T._unique_rows(np.concatenate([T.walkers(c.shape)[T.reduce_rows(c)]] + [st.bits for st in sts])))
            v = S.as_ld(np.random.default_rng(1).random(tab.bits.shape[0]) + 0.25)
            for st in sts:
                a, b = S.table_sum(S.reduce_columns(st, tab, 0.0), v), S.table_sum(S.columns(st, tab), v)
                assert a.E == b.E and a.bound == b.bound and a.m == b.m
            continue
        u_t = S.U32 if c.f32 else S.U
        margin = max(S.weight_margin(st, u_t) for st in sts) + u_t * eps   # (the kernel compares with eps rounded to the integrals' type)
        h = np.concatenate([np.abs(np.concatenate([[st.h0], st.h])).astype(np.float64) for st in sts])
        assert float(np.abs(h - eps).min()) >= half * (1 - 1e-12) and half > 4 * margin, (c.name, eps, half, margin)
        kept = int((h >= eps).sum())
        assert 0.2 * h.size <= kept <= 0.8 * h.size and all(abs(float(st.h0)) >= eps for st in sts), (c.name, kept, h.size)
        print(f"{c.name}: eps {eps:.6g} in a gap of half width {half:.3g} ({half / margin:.3g} roundings), {kept} of {h.size} columns kept")


def test_rbm_case_has_amplitudes_near_1e250():
    ref = T.rbm_reference()
    assert len(ref) == T.RBM_N
    for w, r in ref:
        lg = float(w.psi.re[0]) / np.log(10.0)
        assert 240 < lg < 260 and w.lnmax / np.log(10.0) < 270, lg     # |psi|^2 ~ 1e500 is beyond a double, psi itself is not
        assert np.isfinite(r.bound) and 0 < r.bound <= 1e-9 * r.A, (r.bound, r.A)
    print("log10 |psi(x)|:", [round(float(w.psi.re[0]) / np.log(10.0), 1) for w, _ in ref])


def test_zz_run_time():
    dt = time.time() - _CLOCK["t0"]
    print(f"tests/test_ss_exact.py: {dt:.1f} s")
    assert dt < 90.0
