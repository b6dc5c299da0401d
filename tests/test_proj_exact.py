"""The yardstick of tests/proj_exact.py itself, on the CPU, and the cases of tests/test_gpu_proj_exact.py:
  * on whole sectors of 6 and 8 spin orbitals against an independent brute force -- the dense rows of the CPU oracle's comb_hij_fused,
    determinants as Python integers, every sum and quotient in exact rational arithmetic (fractions) on the float64 inputs -- for every
    form and every method: the two agree within the bound (the oracle's float64 matrix elements carry the t_k u a_k the bound grants);
  * every case's preconditions, from the reference alone: psi(x), f(x) and every T finite and non-zero; eps in the middle of the largest
    gap of the |h_k| with column 0 kept; every applicable wrong variant of proj_exact.VARIANTS moves E or S by at least 100 x the bound on
    at least one walker; the sampled cases have drawn columns that are not kept and walkers whose hits sum to N_s."""
import time
from fractions import Fraction

import numpy as np
import pytest

import proj_exact as P

_CLOCK = {}
METHODS = ("simple", "reduce", "sampled", "ss")


@pytest.fixture(scope="module", autouse=True)
def _clock():
    _CLOCK["t0"] = time.time()
    yield


# ---- the brute force: shares no code with eloc_exact / ss_exact / proj_exact.local -----------------------------------------------------
class Q:
    """a complex number with rational parts"""

    def __init__(self, re, im=0):
        self.re, self.im = Fraction(re), Fraction(im)

    @staticmethod
    def of(z):
        z = complex(z)
        return Q(Fraction(z.real), Fraction(z.imag))

    def __add__(self, o):
        return Q(self.re + o.re, self.im + o.im)

    def __mul__(self, o):
        o = o if isinstance(o, Q) else Q(o)
        return Q(self.re * o.re - self.im * o.im, self.re * o.im + self.im * o.re)

    def conj(self):
        return Q(self.re, -self.im)

    def __truediv__(self, o):
        d = o.re * o.re + o.im * o.im
        n = self * o.conj()
        return Q(n.re / d, n.im / d)

    def value(self):
        return P.CLD(P.LD(self.re.numerator) / P.LD(self.re.denominator) + 1j * (P.LD(self.im.numerator) / P.LD(self.im.denominator)))


def _key(bits) -> int:
    return sum(int(b) << j for j, b in enumerate(bits))


def _flip(key: int) -> int:
    odd = 0x5555555555555555
    return ((key >> 1) & odd) | ((key & odd) << 1)


def _eta_m(key: int) -> int:
    return -1 if bin(key & (key >> 1) & 0x5555555555555555).count("1") & 1 else 1


def brute(cs, i, form, method, drawn=None, Ns=0):
    """(E, S) of walker i, exact rationals rounded once at the end"""
    from oracle import oracle as O

    s = cs.shape
    flip, multi, eta = P.FORMS[form]
    bra = O.pm01_to_onv(np.ascontiguousarray(cs.occ[i:i + 1]), s.sorb)
    comb, hm = O.comb_hij_fused(bra, *cs.h, s.sorb, s.noA + s.noB, s.noA, s.noB)
    comb2, sm = O.comb_hij_fused(bra, *cs.hs, s.sorb, s.noA + s.noB, s.noA, s.noB)
    assert np.array_equal(comb, comb2)
    keys = [int.from_bytes(row.tobytes(), "little") for row in comb[0]]
    psi = {_key(d): Q.of(v) for d, v in zip(cs.dets, cs.psi)}
    f = {_key(d): Q.of(v) for d, v in zip(cs.dets, cs.f)}
    inside = {_key(d) for d, m in zip(cs.dets, cs.half) if m}
    zero, one = Q(0), Q(1)

    def amp(y):
        if method == "ss" and y not in inside:
            return zero
        return psi[y] * (f[y] if multi else one)

    h = [Fraction(float(v)) for v in hm[0]]
    sp = [Fraction(float(v)) for v in sm[0]]
    eps = Fraction(cs.eps)
    K = range(len(keys))
    w = list(h)
    if method in ("reduce", "sampled"):
        K = [k for k in K if abs(h[k]) >= eps]
        if method == "sampled":
            rest = sum(abs(v) for v in h if abs(v) < eps)
            for y, hits in drawn.items():
                k = keys.index(y)
                assert abs(h[k]) < eps
                K.append(k)
                w[k] = Fraction(hits, Ns) * (1 if h[k] > 0 else -1) * rest
    E, Sv = zero, zero
    for k in K:
        y = keys[k]
        T = amp(y)
        if flip:
            T = T + amp(_flip(y)) * (eta * _eta_m(y))
        E, Sv = E + T * w[k], Sv + T * sp[k]
    x = keys[0]
    n2 = Fraction(P.NORM) ** 2 if (flip or multi) else Fraction(1)
    G = (f[x].conj() if multi else one) / (psi[x] * n2)
    return (E * G).value(), (Sv * G).value()


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", sorted(P.SMALL))
def test_yardstick_matches_an_exact_brute_force(name, method):
    cs = P.case(name)
    Ns = 40 if method == "sampled" else 0
    worst = 0.0
    for form in P.forms_of(cs.shape):
        drawn = [cs.host_draws(i, Ns) for i in range(cs.shape.n)] if Ns else None
        ref = P.reference(cs, form, "reduce" if method == "sampled" else method, drawn=drawn, Ns=Ns)
        for i, r in enumerate(ref):
            by_key = {_key(cs.cols[i].bits[k]): hits for k, hits in drawn[i].items()} if Ns else None
            E, Sv = brute(cs, i, form, method, by_key, Ns)
            assert abs(r.E - E) <= r.bE and abs(r.S - Sv) <= r.bS, (name, method, form, i, r.E, E, r.bE, r.S, Sv, r.bS)
            assert abs(r.E) > 1e6 * r.bE and abs(r.S) > 1e6 * r.bS     # (the agreement says something)
            worst = max(worst, float(abs(r.E - E)) / r.bE, float(abs(r.S - Sv)) / r.bS)
    print(f"proj_exact against the brute force, {name} {method}: worst difference / bound {worst:.3g}")


# ---- the cases' preconditions ---------------------------------------------------------------------------------------------------------
def case_methods(name):
    return [m for m in METHODS if m != "sampled" or name in P.SAMPLED]


@pytest.mark.parametrize("name", sorted(P.SHAPES))
def test_amplitudes_and_eps_of_every_case(name):
    cs = P.case(name)
    assert np.isfinite(cs.psi).all() and np.isfinite(cs.f).all() and (np.abs(cs.psi) > 0).all() and (np.abs(cs.f) > 0).all()
    assert (np.abs(cs.psi_r) > 0).all() and (np.abs(cs.f_r) > 0).all()
    mod = np.abs(cs.psi)
    assert mod.max() / mod.min() > 1e4 and np.abs(cs.f).max() / np.abs(cs.f).min() > 30      # decades of moduli
    assert cs.half[: cs.shape.n].all() and 0.3 < cs.half.mean() < 0.7
    import ss_exact as S

    eps, gap = S.eps_in_largest_gap([c.st for c in cs.cols])
    assert (eps, gap) == (cs.eps, cs.gap)
    for c in cs.cols:
        assert abs(c.h[0]) >= eps and float(np.abs(np.abs(c.h) - eps).min()) >= gap * (1 - 1e-9)
        assert gap > 1e3 * S.weight_margin(c.st, P.U)       # float64 and longdouble keep the same columns
        assert (np.abs(c.h) < eps).sum() >= 2 and (np.abs(c.h) >= eps).sum() >= 8
    for form in P.forms_of(cs.shape):
        for method in ("simple", "ss"):
            for ref_i, r in enumerate(P.reference(cs, form, method)):
                assert r.psi != 0 and np.isfinite(complex(r.E)) and np.isfinite(complex(r.S)) and r.bE > 0 and r.bS > 0
                live = np.abs(r.T) > 0
                assert np.isfinite(r.T.astype(np.complex128)).all()
                if method == "simple":
                    # T is non-zero, except where the projection annihilates a closed-shell determinant: flip y = y and eta eta_m(y) = -1
                    # make T(y) = psi(y) (1 - 1), an exact zero on the GPU as well
                    flip, _, eta = P.FORMS[form]
                    closed = (P.F.flip_bits(c_bits := cs.cols[ref_i].bits) == c_bits).all(1)
                    assert np.array_equal(~live, closed & (eta * cs.cols[ref_i].em < 0) if flip else np.zeros(live.size, dtype=bool))
                else:
                    assert live[0] and not live.all()
                assert r.bE < 1e-9 * r.AE and r.bS < 1e-9 * r.AS


@pytest.mark.parametrize("name", sorted(P.SHAPES))
def test_every_applicable_wrong_variant_is_visible(name):
    cs = P.case(name)
    weakest = (np.inf, None)
    for method in case_methods(name):
        Ns = P.SAMPLED.get(name, 0) if method == "sampled" else 0
        drawn = [cs.host_draws(i, Ns) for i in range(cs.shape.n)] if Ns else None
        m = "reduce" if method == "sampled" else method
        if Ns:
            for i, d in enumerate(drawn):
                kept = np.abs(cs.cols[i].h) >= cs.eps
                assert sum(d.values()) == Ns and len(d) >= 2 and not any(kept[k] for k in d)
        for form in P.forms_of(cs.shape):
            ref = P.reference(cs, form, m, drawn=drawn, Ns=Ns)
            for v in P.VARIANTS:
                if not P.applicable(v, form, m, bool(Ns)):
                    continue
                bad = P.reference(cs, form, m, drawn=drawn, Ns=Ns, variant=v)
                moved = max(max(float(abs(b.E - r.E)) / r.bE, float(abs(b.S - r.S)) / r.bS) for b, r in zip(bad, ref))
                assert moved >= 100.0, (name, method, form, v, moved)
                if moved < weakest[0]:
                    weakest = (moved, (method, form, v))
    print(f"{name}: the least visible wrong variant moves a walker by {weakest[0]:.3g} bounds: {weakest[1]}")


def test_zz_run_time():
    assert time.time() - _CLOCK["t0"] < 120.0
