"""The yardstick of the spin-flip-projected local energy (tests/flip_exact.py) itself, on the CPU: the reference's own numbers for 32
Fe2S2 walkers (tests/golden/eloc_flip_multipsi_fe2s2.npz, simple_flip) within 1e-8 Ha; at sorb 8 (2a2b, all 36 determinants) the
reference formula evaluated densely with the oracle's matrix elements; the mirrored-table identity and the sign rule on every column of
every case of tests/test_gpu_eloc_flip_exact.py; that the decomposition E_proj = [E + eta eta_m R Ebar] / N^2 is the formula; and the
NON-VACUITY of those cases: wherever a case has an open-shell walker, the yardstick with sigma_k = +1 and the one with Ebar := E(flip x)
must each miss the true value by more than 10 bounds on at least 90 % of the open-shell walkers -- a kernel without the signs, or one
that took the spin-symmetric shortcut, fails the GPU tests.  (One exception, by construction and not by seed: with no beta electron,
1a0b, eta_m = +1 for every determinant, so sigma_k = +1 IS the truth there and only the second variant can differ.)"""
import time

import numpy as np
import pytest

import eloc_exact as X
import flip_exact as F
import jrbm_exact as J
import rbm_exact as R
import test_gpu_eloc_flip_exact as G
from conftest import golden, synth_integrals

_CLOCK = {}


@pytest.fixture(scope="module", autouse=True)
def _clock():
    _CLOCK["t0"] = time.time()
    yield


def test_reference_fixture_fe2s2():
    d, d0, s = golden("eloc_flip_multipsi_fe2s2.npz"), golden("eloc_e2e_fe2s2.npz"), golden("fe2s2_inputs.npz")
    h1, h2 = np.ascontiguousarray(s["h1e"], dtype=np.float64), np.ascontiguousarray(s["h2e"], dtype=np.float64)
    occ = np.unpackbits(np.ascontiguousarray(d["x"]), axis=1, bitorder="little")[:, :40]
    rbm = R.make("real", d0["W"], d0["hb"], d0["vb"])
    eta, norm = float(d["eta"]), float(d["extra_norm"])
    worst_e = worst_p = 0.0
    for i, row in enumerate(occ):
        w = F.walker(rbm, X.structure(row, h1, h2), eta, norm)
        worst_e = max(worst_e, abs(float(w.E_proj.real) - float(d["eloc_simple_flip"][i])))
        worst_p = max(worst_p, abs(float(np.exp(w.w.psi.re[0])) / float(d["psi_simple_flip"][i]) - 1))
        assert w.bound() < 1e-9
    print(f"Fe2S2 fixture, 32 walkers: max |E_proj - reference| {worst_e:.3e} Ha, psi {worst_p:.3e} relative")
    assert worst_e <= 1e-8 and worst_p <= 1e-12


@pytest.mark.parametrize("kind,jreg", [("real", None), ("tanh", None), ("pRBM", None), ("real", "j-asym")])
@pytest.mark.parametrize("eta", [1.0, -1.0])
def test_complete_space_sorb8_matches_the_dense_formula(kind, jreg, eta):
    from oracle import oracle

    d = golden("c1_sorb8_all36.npz")
    sorb, noA, noB = int(d["sorb"]), int(d["noA"]), int(d["noB"])
    onv, occ = np.ascontiguousarray(d["onv"]), d["occ"]
    assert (sorb, noA, noB) == (8, 2, 2) and occ.shape == (36, 8)
    h1, h2 = synth_integrals(sorb)  # (random per spin orbital: not spin-symmetric)
    rbm = R.regime_params("fe2s2", kind, sorb, 12, 0)
    M = J.jastrow_params(jreg, sorb) if jreg else None
    Hm = oracle.hij(onv, onv, h1, h2, sorb, noA + noB)
    dense = F.dense_reference(rbm, occ, Hm, eta, 1.3, M)
    for i, row in enumerate(occ):
        w = F.walker(rbm, X.structure(row, h1, h2), eta, 1.3, M)
        scale = float((np.abs(Hm[i]) * (1 + abs(w.R))).sum()) * max(1.0, float(w.w.rabs.max()), float((w.wbar.rabs * abs(w.R)).max()))
        assert abs(complex(w.E_proj - dense[i])) <= 64 * X.U * scale, (i, complex(w.E_proj), complex(dense[i]))


def _columns(w: F.FlipWalker):
    return w.w.st


def test_identities_and_non_vacuity_of_every_gpu_case():
    seen = set()
    for c in G.ALL_CASES + G.ROUTE_CASES:
        key = (c.kind, c.sorb, c.noA, c.noB, c.H, c.n, c.regime, c.eta, G.norm_value(c), c.jreg, c.closed, c.seed)
        if key in seen:
            continue
        seen.add(key)
        t0 = time.time()
        ref = G.reference(c, wrong=True)
        assert len(ref.walkers) == c.n
        nopen = miss_sigma = miss_eflip = 0
        for w in ref.walkers:
            st, b = w.w.st, w.bound()
            assert np.isfinite(b) and b > 0 and np.isfinite(complex(w.E_proj).real) and np.isfinite(complex(w.E_proj).imag)
            assert w.w.lnmax <= G.T.LN_FINITE and w.wbar.lnmax <= G.T.LN_FINITE, (G.case_id(c), w.w.lnmax, w.wbar.lnmax)
            if c.kind == "tanh":
                assert abs(w.w.vis0) >= 1e-3 and abs(w.wbar.vis0) >= 1e-3, (G.case_id(c), w.w.vis0, w.wbar.vis0)
            # the sign rule: on every column
            assert np.array_equal(F.sigma_rule(st.occ, st.flips), w.sigma), G.case_id(c)
            # the mirrored-table identity, on every column: psi(flip x'_k) / psi(flip x) of the original parameters (what Ebar was summed
            # from) is the mirrored parameters' ratio of the same excitation (wbar.r), and psi(flip x) their psi(x)
            Ebar_mirror = st.h0 + (st.h.astype(X.CLD) * w.sigma * w.wbar.r).sum()
            assert abs(complex(Ebar_mirror - w.Ebar)) <= 1e-15 * w.wbar.A, (G.case_id(c), complex(Ebar_mirror), complex(w.Ebar))
            fx = (J.exact_ld(ref.rbm, ref.M, (F.flip_bits(st.occ).astype(np.float64) * 2 - 1)[None]) if ref.M is not None
                  else R.exact_ld(ref.rbm, (F.flip_bits(st.occ).astype(np.float64) * 2 - 1)[None]))
            assert abs(float(fx.re[0] - w.wbar.psi.re[0])) <= 1e-15 * max(1.0, abs(float(fx.re[0])))
            # the decomposition is the formula
            dec = (w.E + c.eta * w.eta_m_x * w.R * w.Ebar) / X.LD(w.norm) ** 2
            assert abs(complex(dec - w.E_proj)) <= 1e-15 * (w.w.A + abs(w.R) * w.wbar.A) / w.norm ** 2
            assert w.open_shell == (not c.closed) or not w.open_shell
            if c.closed:
                assert not w.open_shell and abs(complex(w.R) - 1) == 0
            if w.open_shell:
                nopen += 1
                miss_sigma += abs(complex(w.wrong_sigma - w.E_proj)) > 10 * b
                miss_eflip += abs(complex(w.wrong_eflip - w.E_proj)) > 10 * b
        print(f"{G.case_id(c)}: open-shell {nopen} of {c.n}, sigma = +1 misses {miss_sigma}, E(flip x) misses {miss_eflip}, "
              f"max bound {max(w.bound() for w in ref.walkers):.2e}, {time.time() - t0:.2f} s")
        if nopen:
            if c.noB > 0:   # (no beta electron: sigma_k = +1 is the truth, module docstring)
                assert miss_sigma >= 0.9 * nopen, G.case_id(c)
            else:
                assert all(bool((w.sigma == 1).all()) for w in ref.walkers)
            assert miss_eflip >= 0.9 * nopen, G.case_id(c)


def test_abi_symbols_exist_and_every_case_takes_the_form_it_names():
    """host logic only (no GPU): the eight entry points are exported, the _flip_supported / _flip_form queries answer as the plain
    kernels' do, and every GPU case is launched in the form it names (resident / windowed, one workgroup per walker / chunked)"""
    from pynqs_amd import _native as N

    lib = N.lib()
    for name in ("pynqs_eloc_rbm_signed", "pynqs_eloc_rbm_flip", "pynqs_eloc_rbm_flip_supported", "pynqs_eloc_rbm_flip_form",
                 "pynqs_eloc_jrbm_signed", "pynqs_eloc_jrbm_flip", "pynqs_eloc_jrbm_flip_supported", "pynqs_eloc_jrbm_flip_form"):
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    forms = set()
    for c in G.ALL_CASES:
        sys_ = (c.sorb, c.noA + c.noB, c.noA, c.noB, c.H)
        assert G.form_of(c) == c.form, (G.case_id(c), G.form_of(c))
        assert lib.pynqs_eloc_rbm_flip_supported(*sys_) == lib.pynqs_eloc_rbm_supported(*sys_) == 1
        if c.entry == "jflip":
            assert lib.pynqs_eloc_jrbm_flip_supported(*sys_) == lib.pynqs_eloc_jrbm_supported(*sys_) == 1
            assert lib.pynqs_eloc_jrbm_flip_form(c.n, *sys_) == lib.pynqs_eloc_jrbm_form(c.n, *sys_)
        forms.add((c.entry, c.form, (c.sorb - 1) // 64 + 1))
    assert {f[:2] for f in forms} >= {("flip", G.R1), ("flip", G.RC), ("flip", G.W1), ("flip", G.WC), ("signed", G.R1), ("signed", G.RC),
                                      ("signed", G.W1), ("jflip", G.R1), ("jflip", G.RC)}
    assert {(f[0], f[2]) for f in forms} >= {("flip", 1), ("flip", 2), ("flip", 3), ("jflip", 1), ("jflip", 2), ("jflip", 3)}
    assert lib.pynqs_eloc_jrbm_flip_supported(40, 5, 3, 2, 1200) == 0 and lib.pynqs_eloc_jrbm_flip_form(2, 40, 5, 3, 2, 1200) == -1  # (no windowed Jastrow form)


def test_route_cases_are_well_conditioned_for_an_absolute_tolerance():
    """the comparison with the generic route is 1e-8 Ha absolute: the yardstick's own bound must be far below it, for E_loc and <S-S+>"""
    for c in G.ROUTE_CASES:
        for spin in (False, True):
            ref = G.reference(c, spin=spin)
            worst = max(w.bound() for w in ref.walkers)
            print(G.case_id(c), "spin integrals" if spin else "integrals", f"max bound {worst:.2e} Ha, max |E_proj| {max(abs(complex(w.E_proj)) for w in ref.walkers):.3e}")
            assert worst <= 1e-9, (G.case_id(c), spin, worst)


def test_closed_shell_fe2s2_is_spin_symmetric():
    """what tests/test_gpu_eloc_flip_exact.py's factor test rests on: with Fe2S2's own integrals and flip x = x, Ebar = E"""
    for eta in (1.0, -1.0):
        _, ref = G.closed_shell_fe2s2(eta)
        for w in ref.walkers:
            assert not w.open_shell and abs(complex(w.Ebar - w.E)) <= 1e-13 * w.w.A, complex(w.Ebar - w.E)
            assert abs(complex(w.E_proj - w.E * (1 + eta * w.eta_m_x) / X.LD(w.norm) ** 2)) <= 1e-13 * w.w.A


def test_zz_run_time():
    dt = time.time() - _CLOCK["t0"]
    print(f"tests/test_flip_exact.py: {dt:.1f} s")
    assert dt < 120.0
