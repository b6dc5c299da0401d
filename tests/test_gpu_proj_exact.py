"""The local energies energy.local_energy builds on top of its kernels -- spin-flip projected (eta = +1 and -1), multi-psi with a complex
f, both, each without and with <S-S+>, and the plain form with <S-S+> -- on every route, against the exact yardstick of
tests/proj_exact.py (numpy longdouble; the contract and the a-priori bound are that module's docstring):
    per walker  |E_got - E| <= bound_E,  |S_got - S| <= bound_S,  psi(x) bit-equal to the given value;  no walker is left out.
Every run goes through energy.local_energy (one through total_energy) with table-backed modules for psi and f (tests/table_ansatz.py),
integrals that are NOT spin-symmetric, amplitudes over six (psi) and two (f) decades, extra_norm = 1.3 as a device tensor; a spy on the
four path functions asserts which path answered.  Shapes (proj_exact.SHAPES): one ONV word with one segment per walker, unequal spins,
one word with two segments per walker, two words, three words; the numbers of segments are asserted.  The drawn columns of the
semi-stochastic runs are read from the records of the front end the call used (their law is pinned by tests/test_gpu_reduce_replay*.py).
tests/test_proj_exact.py checks the yardstick and every case's preconditions without a GPU."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import proj_exact as P
import ss_exact as S
from table_ansatz import Holder, TableAmplitude

pytestmark = pytest.mark.gpu

PATHS = ("_eloc_reduce_front", "_eloc_reduce_multipass", "_eloc_sample_space_fused", "_eloc_generic")
SEGMENTS = {"s12": (8, 1), "s12u": (8, 1), "s32": (8, 2), "s66": (12, 6), "s130": (20, 10)}   # (segments, per walker), deterministic
SEGMENTS_SAMPLED = {"s12": (8, 1), "s66": (2, 1)}
# route -> (module switches, local_energy arguments, the path that must answer, proj_exact's method, proj_exact's route)
ROUTES = {
    "simple-generic": ({}, {}, "_eloc_generic", "simple", "generic"),
    "reduce-front": ({}, dict(reduce_psi=True), "_eloc_reduce_front", "reduce", "front"),
    "reduce-multipass": (dict(FUSED_ONEPASS=False), dict(reduce_psi=True), "_eloc_reduce_multipass", "reduce", "multipass"),
    "reduce-generic": (dict(FUSED=False), dict(reduce_psi=True), "_eloc_generic", "reduce", "generic"),
    "sampled-front": (dict(FRONT_SAMPLED_MIN_WALKERS=1), dict(reduce_psi=True), "_eloc_reduce_front", "reduce", "front"),
    "ss-keys": (dict(SS_KEYS=True, SS_INDEX=False), dict(use_sample_space=True), "_eloc_sample_space_fused", "ss", "ss"),
    "ss-columns": (dict(SS_KEYS=False), dict(use_sample_space=True), "_eloc_sample_space_fused", "ss", "ss"),
    "ss-indexed": (dict(SS_KEYS=True, SS_INDEX=True), dict(use_sample_space=True), "_eloc_sample_space_fused", "ss", "ss"),
    "ss-generic": (dict(FUSED=False), dict(use_sample_space=True), "_eloc_generic", "ss", "generic"),
}
CASES = [(name, route) for name in P.SHAPES for route in ROUTES if route != "sampled-front" or name in P.SAMPLED]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _onv(bits: np.ndarray, sorb: int) -> np.ndarray:
    from oracle import oracle

    return oracle.pm01_to_onv(np.ascontiguousarray(bits, dtype=np.uint8), sorb)


def _bits(onv: np.ndarray, sorb: int) -> np.ndarray:
    return np.ascontiguousarray(np.unpackbits(np.ascontiguousarray(onv), axis=-1, bitorder="little")[..., :sorb])


class Device:
    """A case on the GPU: walkers, both integral sets, the table-backed modules (complex and real) and the SAMPLE_SPACE tables."""

    def __init__(self, name: str) -> None:
        from pynqs_amd import public_function as pf

        cs = P.case(name)
        s = cs.shape
        self.cs, self.s, dev = cs, s, torch.device("cuda")
        self.sys = (s.sorb, s.noA + s.noB, s.noA, s.noB)
        self.x = _dev(_onv(cs.occ, s.sorb))
        self.h, self.hs = tuple(_dev(a) for a in cs.h), tuple(_dev(a) for a in cs.hs)
        keys = _dev(_onv(cs.dets, s.sorb))
        half = torch.from_numpy(cs.half).cuda()
        self.norm = torch.tensor(P.NORM, dtype=torch.float64, device=dev)
        self.ansatz, self.lut = {}, {}
        for real, psi, f in ((False, cs.psi, cs.f), (True, cs.psi_r, cs.f_r)):
            pm, fm = TableAmplitude(keys, _dev(psi), s.sorb), TableAmplitude(keys, _dev(f), s.sorb)
            self.ansatz[real] = (pm, Holder(pm, fm))
            self.lut[real] = pf.WavefunctionLUT(keys[half].contiguous(), _dev(psi)[half].contiguous(), s.sorb, device=dev)
        self.where = [{row.tobytes(): k for k, row in enumerate(np.ascontiguousarray(c.bits))} for c in cs.cols]

    def run(self, energy, form: str, spin: bool, real: bool, kw: dict, fn=None):
        from pynqs_amd import public_function as pf

        flip, multi, eta = P.FORMS[form]
        dt = torch.float64 if real else torch.complex128
        ab = lambda xx, func: pf.ansatz_batch(func, xx, 100000, self.s.sorb, self.x.device, dt)  # noqa: E731
        old = pf.SpinProjection._eta
        pf.SpinProjection.init(4 if eta > 0 else 2, 0)
        try:
            assert pf.SpinProjection.eta == eta
            args = dict(dtype=dt, use_spin_raising=spin, h1e_spin=self.hs[0], h2e_spin=self.hs[1], use_multi_psi=multi, use_spin_flip=flip,
                        extra_norm=self.norm, **kw)
            if kw.get("use_sample_space"):
                args["WF_LUT"] = self.lut[real]
            ansatz = self.ansatz[real][1 if multi else 0]
            if fn is not None:
                return fn(ansatz, args)
            e, sl, p, _ = energy.local_energy(self.x, *self.h, ansatz, ab, *self.sys, **args)
            return e, sl, p
        finally:
            pf.SpinProjection._eta = old

    def drawn(self, fe, Ns: int):
        """[{column: hits} per walker] from the records of the front end a call used; the kept records must be the columns |h_k| >= eps, the
        drawn ones sub-eps, distinct, and their hits must sum to Ns"""
        cs, sorb = self.cs, self.s.sorb
        walker, _, w, _, onv, is_drawn = (t.cpu().numpy() for t in fe.records())
        bits = _bits(onv, sorb)
        out = []
        for i, c in enumerate(cs.cols):
            mine, where = walker == i, self.where[i]
            kept = sorted(where[b.tobytes()] for b in bits[mine & ~is_drawn])
            assert kept == np.flatnonzero(np.abs(c.h) >= S.LD(cs.eps)).tolist(), i
            hits = np.abs(w[mine & is_drawn].astype(np.float64)) * Ns / float(S.row_sum(c.st, cs.eps))
            assert hits.size and float(np.abs(hits - np.rint(hits)).max()) < 1e-6
            d = {}
            for b, v in zip(bits[mine & is_drawn], np.rint(hits)):
                k = where[b.tobytes()]
                assert k not in d and abs(c.h[k]) < cs.eps and v >= 1, (i, k)
                d[k] = int(v)
            assert sum(d.values()) == Ns, (i, sum(d.values()))
            out.append(d)
        return out


@functools.lru_cache(maxsize=None)
def device(name: str) -> Device:
    return Device(name)


@functools.lru_cache(maxsize=None)
def reference(name: str, form: str, method: str, real: bool, route: str):
    return P.reference(P.case(name), form, method, real=real, routes=(route,))


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:   # (a fault leaves the context unusable: every later test would only report it again)
        pytest.exit(f"GPU error, the session ends here: {err}", returncode=3)


@pytest.fixture
def spy(monkeypatch):
    """which path function answered a local_energy call, and the front ends reduce_front_finish handed out"""
    from pynqs_amd import energy

    seen = SimpleNamespace(paths=[], fronts=[], slots=[])
    for name in PATHS:
        def wrapped(c, _orig=getattr(energy, name), _name=name):
            out = _orig(c)
            if out is not None:
                seen.paths.append(_name)
            return out
        monkeypatch.setattr(energy, name, wrapped)

    def finish(t, _orig=energy.reduce_front_finish):
        out = _orig(t)
        seen.fronts.append(out[0])
        return out

    def launch(*a, _orig=energy.reduce_front_launch, **kw):
        seen.slots.append(kw.get("slot", 0))
        return _orig(*a, **kw)

    monkeypatch.setattr(energy, "reduce_front_finish", finish)
    monkeypatch.setattr(energy, "reduce_front_launch", launch)
    return seen


def ratios(ref, got, which: str) -> np.ndarray:
    """|got - exact| / bound per walker (inf where got is not finite)"""
    got = np.asarray(got)
    assert got.shape == (len(ref),)
    out = []
    for r, g in zip(ref, got):
        g = complex(g)
        want, bound = (r.E, r.bE) if which == "E" else (r.S, r.bS)
        out.append(float(abs(S.CLD(g) - want)) / bound if np.isfinite(g.real) and np.isfinite(g.imag) else np.inf)
    return np.array(out)


def psi_wanted(cs, real: bool) -> np.ndarray:
    return (cs.psi_r if real else cs.psi)[[c.pos[0] for c in cs.cols]]


def compare(tag, ref, cs, real, spin, e, sl, p, worst, msg) -> None:
    want = psi_wanted(cs, real)
    p = p.cpu().numpy()
    if p.dtype != want.dtype or not np.array_equal(p.view(np.float64), want.view(np.float64)):
        msg.append(f"{tag}: psi(x) is not the given value bit for bit")
    rE = ratios(ref, e.cpu().numpy(), "E")
    rS = ratios(ref, sl.cpu().numpy(), "S") if spin else np.zeros(1)
    if not spin and bool((sl != 0).any()):
        msg.append(f"{tag}: <S-S+> was not asked for and is not zero")
    for which, r in (("E", rE), ("S", rS)):
        top = float(np.where(np.isnan(r), np.inf, r).max())
        if top > worst[0]:
            worst[:] = [top, f"{tag} {which}"]
        if not bool((r <= 1.0).all()):
            msg.append(f"{tag} {which}: error / bound {top:.3g} at walker {int(np.argmax(r))}, {int((~(r <= 1)).sum())} of {r.size} outside")


def runs_of(name: str):
    """(form, <S-S+>, real amplitudes) of a shape: every form without and with <S-S+> in complex128 -- the plain form only with it --,
    and on the first shape every form once more in float64 with real amplitudes"""
    forms = P.forms_of(P.SHAPES[name])
    out = [(f, sp, False) for f in forms for sp in (False, True) if f != "plain" or sp]
    return out + ([(f, True, True) for f in forms] if name == "s12" else [])


@pytest.mark.parametrize("name,route", CASES, ids=lambda v: str(v))
def test_local_energy_meets_the_bound(name, route, spy, monkeypatch):
    from pynqs_amd import energy, reduce_front as RF

    switches, kw, path, method, proute = ROUTES[route]
    d = device(name)
    cs, s = d.cs, d.s
    sampled = route == "sampled-front"
    Ns = P.SAMPLED[name] if sampled else 0
    nseg = (SEGMENTS_SAMPLED if sampled else SEGMENTS)[name]
    assert s.ncomb == int(energy.get_Num_SinglesDoubles(s.sorb, s.noA, s.noB)) + 1
    assert RF.geometry(s.n, *d.sys, Ns)[0] == nseg[0]
    for k, v in switches.items():
        monkeypatch.setattr(energy, k, v)
    kw = dict(kw)
    if method == "reduce":
        kw.update(eps=cs.eps, eps_sample=Ns)
    energy.reset_caches()
    torch.manual_seed(20250 + s.sorb)
    worst, msg = [0.0, "-"], []
    for form, spin, real in runs_of(name):
        tag = f"{form}{' S-S+' if spin else ''}{' float64' if real else ''}"
        del spy.paths[:], spy.fronts[:]
        e, sl, p = d.run(energy, form, spin, real, kw)
        assert spy.paths == [path], (tag, spy.paths)
        if path == "_eloc_reduce_front":
            assert len(spy.fronts) == 1 and spy.fronts[0].nchunks == nseg[1] and spy.fronts[0].nseg == nseg[0]
        if sampled:
            ref = P.reference(cs, form, method, real=real, drawn=d.drawn(spy.fronts[0], Ns), Ns=Ns, routes=(proute,))
        else:
            ref = reference(name, form, method, real, proute)
        compare(tag, ref, cs, real, spin, e, sl, p, worst, msg)
    print(f"PROJ {name} {route}: worst error / bound {worst[0]:.3g} ({worst[1]}) over {len(runs_of(name))} runs")
    assert not msg, msg


def test_total_energy_in_uneven_chunks_meets_the_bound(spy):
    """8 walkers in chunks of 3, 3 and 2: the look-ahead launches the next chunk's front end on the second stream; flip + multi-psi, REDUCE
    deterministic; the per-walker energies against the same bounds"""
    from pynqs_amd import energy

    name, form = "s12", "flip-multi"
    d = device(name)
    cs = d.cs
    energy.reset_caches()

    def fn(ansatz, args):
        args = {k: v for k, v in args.items() if k not in ("use_spin_raising", "h1e_spin", "h2e_spin")}
        return energy.total_energy(d.x, 3, -1, *d.h, ansatz, *d.sys, **args)

    assert energy.OVERLAP
    e, sl, _ = d.run(energy, form, False, False, dict(reduce_psi=True, eps=cs.eps, eps_sample=0), fn)
    assert spy.paths == ["_eloc_reduce_front"] * 3 and spy.slots == [0, 1, 0] and [f.n for f in spy.fronts] == [3, 3, 2]
    ref = reference(name, form, "reduce", False, "front")
    r = ratios(ref, e.cpu().numpy(), "E")
    print(f"PROJ {name} total_energy chunks 3+3+2 {form}: worst error / bound {float(r.max()):.3g}")
    assert bool((r <= 1.0).all()) and not bool((sl != 0).any()), r
