"""The yardstick of tests/test_gpu_reduce_replay.py checked by itself, without a GPU (tests/reduce_replay.py: the documented draw law of the
short-row semi-stochastic REDUCE form replayed on the host from the CPU oracle's rows):
  * it reproduces both committed draw fixtures completely -- walker, column, hits, n_kept, row_sum;
  * every case of the GPU file has ZERO undecided draws (no target within tau of a CDF boundary: the kernel has no freedom left) and is
    non-vacuous: a drawn column outside the first segment (rows longer than a segment), a column drawn more than once (N > 1), and the
    property its `covers` line claims;
  * the replay's own law: Pearson's chi-square pooled over R seeds against w32 / S' stays under chi2.isf(1e-9, dof) at every shape and draw
    count that the GPU file gives the hierarchical forms, so that those inputs stay under the threshold by themselves;
  * the walker index and the seed enter the key."""
import numpy as np
import pytest

import reduce_replay as RR
from conftest import golden


@pytest.mark.parametrize("name", ["reduce_draws_fe2s2.npz", "reduce_draws_bdg_rnn_fe2s2.npz"])
def test_replay_reproduces_the_committed_draws(name, fe2s2):
    g = golden(name)
    hm, kets = RR.oracle_rows(g["x"], fe2s2["h1e"], fe2s2["h2e"], 40, 15, 15)
    r = RR.replay_rows(hm, kets, float(g["eps"]), int(g["eps_sample"]), int(g["kernel_seed"]))
    walker, col, hits = r.records()
    assert np.array_equal(walker, g["draw_walker"]) and np.array_equal(col, g["draw_col"]) and np.array_equal(hits, g["draw_hits"])
    assert int(r.keep.sum()) == int(g["n_kept"])
    ncomb = hm.shape[1]
    err = np.abs(g["row_sum"].astype(RR.LD) - r.S) / r.S
    print(f"{name}: {walker.size} records, closest target {float(r.margin.min()):.3g} tau, row_sum error / bound {float(err.max()) / (ncomb * 2.0 ** -52):.3g}")
    assert bool((err <= ncomb * RR.LD(2.0) ** -52).all())
    assert r.undecided == 0


def test_fixture_seed_is_what_the_energy_case_runs_with():
    c = RR.CASE_BY_NAME["through_energy"]
    g = golden("reduce_draws_fe2s2.npz")
    assert RR.kernel_seeds(c) == [int(g["kernel_seed"])] and c.seed == int(g["torch_seed"]) and np.array_equal(RR.inputs(c.name)[0], g["x"])
    assert (c.N, RR.inputs(c.name)[3]) == (int(g["eps_sample"]), float(g["eps"]))


def _segments_without_width(w32_row):
    pad = (-w32_row.size) % RR.SEG
    return ~(np.pad(w32_row, (0, pad)).reshape(-1, RR.SEG) > 0).any(1)


@pytest.mark.parametrize("case", RR.CASES, ids=lambda c: c.name)
def test_case_is_decided_and_not_vacuous(case):
    x, h1, h2, eps = RR.inputs(case.name)
    assert x.shape[0] == case.n and h1.dtype == (np.float32 if case.f32 else np.float64)
    for seed in RR.kernel_seeds(case):
        r = RR.reference(case.name, seed)
        n, ncomb = r.hm.shape
        walker, col, hits = r.records()
        print(f"{case.name} seed {seed}: ncomb {ncomb}, {walker.size} drawn records, closest target {float(r.margin.min()):.3g} tau")
        assert r.undecided == 0, "choose another seed and record it in reduce_replay.SEED"
        assert ncomb <= RR.MAX_COLS and case.N <= RR.MAX_DRAWS
        drawable = (r.w32 > 0).any(1)
        assert np.array_equal(r.hits.sum(1), np.where(drawable, case.N, 0))
        if case.name != "no_width":
            assert bool(drawable.any())
            if ncomb > RR.SEG and not str(case.eps).startswith("single"):
                assert bool((col >= RR.SEG).any())
            if case.N > 1:
                assert bool((hits > 1).any())
        # what the case is there for
        pos = (r.w32 > 0).sum(1)
        if case.name == "one_segment":
            assert ncomb <= 16 and case.noA != case.noB
        elif case.name == "sixteen_columns":
            assert ncomb == 16
        elif case.name == "multiple_of_16":
            assert ncomb % 16 == 0 and ncomb > 16 and case.N == 1000
        elif case.name in ("multiple_of_16_plus_1", "five_segments_plus_1"):
            assert ncomb % 16 == 1 and ncomb > 16 and case.N == (1024 if case.name == "multiple_of_16_plus_1" else 1025)
            assert r.w32[:, -1].any() and bool(r.hits[:, -1].any())      # the lone column of the last segment is drawn
        elif case.name.startswith("fe2s2"):
            assert ncomb == 7876 and case.N in (1, 16383)
        elif case.name == "near_8192":
            assert RR.MAX_COLS - 2 * RR.SEG < ncomb <= RR.MAX_COLS
            assert bool((col >= (ncomb // RR.SEG) * RR.SEG).any())       # a column of the last segment is drawn
        elif str(case.eps).startswith("single"):
            assert case.N == RR.MAX_DRAWS and bool((pos == 1).all()) and bool((x == x[0]).all())
            assert hits.tolist() == [RR.MAX_DRAWS] * n and int(r.keep.sum(1).min()) > 0
            assert (int(col[0]) == ncomb - 1) == (case.eps == "single_last")
        elif case.name == "eps_zero":
            assert eps == 0 and not r.keep.any() and bool(r.hits[:, 0].any())      # the diagonal is drawn
        elif case.name == "eps_above_all":
            assert eps > float(np.abs(r.hm).max()) and not r.keep.any() and bool(r.hits[:, 0].any())
        elif case.name == "no_width":
            assert not drawable.any() and walker.size == 0 and bool(r.keep.any(1).all()) and bool((r.S == 0).all())
            assert np.array_equal(r.keep, r.hm != 0)
        elif case.name == "sparse":
            empty = [_segments_without_width(w) for w in r.w32[drawable]]
            assert bool((r.hm == 0).any(1).all())
            assert any(e[0] and not e.all() for e in empty) and any(e[-1] and not e.all() for e in empty)
            assert any(bool((~e[:k]).any() and e[k] and (~e[k + 1:]).any()) for e in empty for k in range(1, e.size - 1))
            # draws behind an empty first segment, in front of an empty last one, and on both sides of an empty middle one
            assert any(e[0] and h.any() for e, h in zip(empty, r.hits[drawable])) and any(e[-1] and h.any() for e, h in zip(empty, r.hits[drawable]))
        elif case.f32:
            assert r.hm.dtype == np.float32 and np.array_equal(r.w32, np.where(r.keep, np.float32(0), np.abs(r.hm)))
            assert case.N in (1000, 1025, 2500)
        elif case.name in ("one_word", "two_words", "three_words", "many_walkers"):
            assert x.shape[1] == 8 * {"one_word": 1, "two_words": 2, "three_words": 3, "many_walkers": 1}[case.name]
            assert case.name in ("three_words", "many_walkers") or case.noA != case.noB
            assert case.name != "many_walkers" or n == 5000
        elif case.name == "no_dedup_table":
            assert not case.dedup
        elif case.name == "wavefunction_table":
            assert case.lut
        elif case.name == "through_energy":
            assert case.via == "energy"
        elif case.name == "graph_replay":
            assert case.via == "graph" and len(RR.kernel_seeds(case)) == 4
        else:
            raise AssertionError("a case without a stated property")


def test_every_draw_count_and_row_length_of_the_list_is_there():
    assert {1, 7, 64, 1000, 1024, 1025, 2500, 16383} <= {c.N for c in RR.CASES}
    assert {1, 2, 3} <= {(c.sorb - 1) // 64 + 1 for c in RR.CASES}


@pytest.mark.parametrize("shape", RR.HIER, ids=lambda h: h.name)
def test_the_replay_follows_its_law(shape):
    """The host replay under the chi-square that the GPU file gives the hierarchical forms, at their shapes, draw counts and R: the
    threshold is chi2.isf(1e-9, dof), derived, and a correct sampler stays under it."""
    hm = RR.hier_rows(shape.name)
    counts, p = RR.replay_counts(hm, shape.eps, shape.N, range(1, RR.R_SEEDS + 1))
    stat, dof, limit = RR.chi_square(counts, p, RR.R_SEEDS * shape.N)
    print(f"{shape.name}: host replay chi-square {stat:.1f}, dof {dof}, threshold {limit:.1f}")
    assert dof > 0 and stat < limit
    # against the exact law |H| / S too: float32 widths move a probability by 6e-8 relative, far below what these counts resolve
    stat2, dof2, limit2 = RR.chi_square(counts, RR.exact_law(hm, shape.eps), RR.R_SEEDS * shape.N)
    assert dof2 == dof and stat2 < limit2 and abs(stat2 - stat) < 1e-3 * stat


def test_the_chi_square_sees_a_wrong_law():
    """the statistic is no formality: a law proportional to |H|^1.2 exceeds the threshold at the same shape, N and R"""
    shape = RR.HIER_BY_NAME["flush_row_f32"]
    hm = RR.hier_rows(shape.name)
    w32 = RR.widths32(hm, RR.keep_mask(hm, shape.eps))
    bent = (w32.astype(np.float64) ** 1.2).astype(np.float32)
    counts = np.zeros(hm.shape, dtype=np.int64)
    for s in range(1, RR.R_SEEDS + 1):
        for i in range(hm.shape[0]):
            counts[i] += np.bincount(RR.draw(bent[i], s, i, shape.N)[0], minlength=hm.shape[1])
    stat, dof, limit = RR.chi_square(counts, RR.exact_law(hm, shape.eps), RR.R_SEEDS * shape.N)
    print(f"|H|^1.2: chi-square {stat:.1f}, dof {dof}, threshold {limit:.1f}")
    assert stat > limit


def test_walker_and_seed_enter_the_key():
    hm, kets = RR.rows("eps_zero")
    same = np.repeat(hm[:1], 2, axis=0)
    a = RR.replay_rows(same, np.repeat(kets[:1], 2, axis=0), 0.0, 64, 1)
    assert not np.array_equal(a.hits[0], a.hits[1])                       # identical rows, different walker indices
    b = RR.replay_rows(same, np.repeat(kets[:1], 2, axis=0), 0.0, 64, 2)
    assert not np.array_equal(a.hits[0], b.hits[0]) and not np.array_equal(a.hits[1], b.hits[1])   # seed and seed + 1
    assert not np.array_equal(RR.uniforms(1, 1, 8), RR.uniforms(2, 0, 8))     # (seed, walker) is not folded into seed + walker
