"""The local-energy kernels that take their amplitudes from a table or a list -- pynqs_eloc_sample_space, _hash, _flip, _hash_flip,
_keys and _indexed (both flip settings), and pynqs_reduce_contract -- against the exact yardstick of tests/ss_exact.py (numpy longdouble
from the packed integrals, membership by determinant bits), at every amplitude scale 2^k, k in SCALES: the tolerance is the a-priori
rounding bound of that module's docstring,
    |E_got - E_exact| <= [sum_k dw_k |A_k| + m u sum_k wabs_k |A_k|] / |A(x)| + c_q u |E_exact|                      per walker,
psi(x) must be the table's value bit for bit, and a walker whose psi(x) is 0 must come out non-finite (counted, not skipped).  E_loc is
homogeneous of degree 0 in psi: the forms that add in a fixed order (the indexed kernel, the contraction) must return at every k the
very bits they return at k = 0.  The native entry points are called directly, so that every kernel form is reached by construction;
one run each goes through energy.local_energy.  tests/test_ss_exact.py checks the yardstick itself on the CPU and every case's
preconditions (bound <= 1e-9 of the sum of moduli, the number of psi(x) = 0 walkers, no sum near 2^1023, eps inside a gap of the |h_k|)."""
import functools
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

import eloc_exact as X
import rbm_exact as R
import ss_exact as S
from conftest import golden, rand_occ, synth_integrals

pytestmark = pytest.mark.gpu

# +-520 lies just past the point where |psi|^2 leaves the range of a double; +900 is the largest scale at which the sums stay finite
SCALES = (0, 300, -300, 520, -520, 600, -600, 900)
SPREAD = 200                                   # the second value set: moduli 2^e, e uniform in [-SPREAD, SPREAD], inside one neighbourhood
SCALES_SPREAD = tuple(k for k in SCALES if abs(k) + SPREAD < 1000)   # (2^(900 + 200) is not a double: that set stops at +-600)

Shape = namedtuple("Shape", "name sorb noA noB n ints")
SHAPES = {s.name: s for s in (
    Shape("s12", 12, 3, 2, 77, "syn"),         # one ONV word; 77 walkers: the last workgroup of every launch is partly filled
    Shape("s12one", 12, 3, 2, 1, "syn"),       # n = 1
    Shape("s66", 66, 3, 4, 3, "syn"),          # two words, flipped orbitals on both sides of bit 64
    Shape("s130", 130, 3, 2, 2, "syn"),        # three words
    Shape("fe2s2", 40, 15, 15, 4, "fe2s2"),    # plan_chunks gives several chunks per walker: atomics and the separate divide kernel
    # beyond the 30 electrons of Fe2S2 (the order-free sums fast_diag / fast_single and the key-major kernel's diagonal() under every
    # entry point): 33 electrons on one word, and 65 on two, where fast_diag's 64 lanes come round a second time
    Shape("s40e33", 40, 17, 16, 2, "syn"),
    Shape("s72e65", 72, 33, 32, 2, "syn"))}
# tables: "all": every walker, every connected determinant and their spin-flip partners (for unequal spins those lie in the other sector:
# the plain sums must pass them over, the flip passes find them); "half": the walkers and a random half of the others; "walkers":
# the walkers only; "far": the walkers and keys that connect to nothing; "one": one key, the first walker; "absent2": "all" without the
# first two (distinct) walkers.  "all" of s130 and fe2s2 has 1e5 / 3e4 keys for 2 / 4 walkers: the streamed key-major kernel runs with
# nchunks > 1 there.
CASES = [("s12", t) for t in ("all", "half", "walkers", "one", "absent2")] + [("s12one", "all"), ("s12one", "walkers")] + \
        [("s66", t) for t in ("all", "half", "far", "absent2")] + [("s130", "all"), ("s130", "half")] + \
        [("fe2s2", t) for t in ("all", "half", "absent2")] + [(name, t) for name in ("s40e33", "s72e65") for t in ("all", "half")]
VALUES = ("real", "complex", "real-spread", "complex-spread")
# entry point, flip pass, keys sorted (binary search / hash table) or shuffled (key-major), adds in a fixed order
Form = namedtuple("Form", "name entry flip shuffled fixed")
FORMS = [Form("sorted", "pynqs_eloc_sample_space", False, False, False), Form("hash", "pynqs_eloc_sample_space_hash", False, False, False),
         Form("sorted-flip", "pynqs_eloc_sample_space_flip", True, False, False), Form("hash-flip", "pynqs_eloc_sample_space_hash_flip", True, False, False),
         Form("keys", "pynqs_eloc_sample_space_keys", False, True, False), Form("keys-flip", "pynqs_eloc_sample_space_keys", True, True, False),
         Form("indexed", "pynqs_eloc_sample_space_indexed", False, True, True), Form("indexed-flip", "pynqs_eloc_sample_space_indexed", True, True, True)]


def scales_of(values: str):
    return SCALES_SPREAD if values.endswith("spread") else SCALES


@functools.lru_cache(maxsize=None)
def integrals(ints: str, sorb: int):
    if ints == "fe2s2":
        d = golden("fe2s2_inputs.npz")
        return np.ascontiguousarray(d["h1e"], dtype=np.float64), np.ascontiguousarray(d["h2e"], dtype=np.float64)
    return synth_integrals(sorb)


def bits_of(onv: np.ndarray, sorb: int) -> np.ndarray:
    return np.ascontiguousarray(np.unpackbits(np.ascontiguousarray(onv), axis=-1, bitorder="little")[..., :sorb])


@functools.lru_cache(maxsize=None)
def walkers(name: str) -> np.ndarray:
    """0/1 [n, sorb]"""
    s = SHAPES[name]
    if s.ints == "fe2s2":
        return bits_of(golden("fe2s2_inputs.npz")["ci_space"][: s.n], s.sorb)
    occ = rand_occ(s.n, s.sorb, s.noA, s.noB, seed=11 * s.sorb + s.n)
    if s.sorb == 66:  # orbitals 64 and 65 are the second word: occupied / empty in turn, so that holes and particles lie on both sides
        from test_gpu_eloc_exact import _force

        occ = np.concatenate([_force(occ[i:i + 1], w) for i, w in enumerate(({64: 1, 65: 0, 62: 0}, {64: 0, 65: 1, 63: 1}, {64: 1, 65: 1, 62: 1}))])
    assert occ[:, 0::2].sum(1).tolist() == [s.noA] * s.n and occ[:, 1::2].sum(1).tolist() == [s.noB] * s.n
    return occ


@functools.lru_cache(maxsize=None)
def structures(name: str, f32: bool = False):
    s = SHAPES[name]
    h1, h2 = integrals(s.ints, s.sorb)
    if f32:
        h1, h2 = h1.astype(np.float32).astype(np.float64), h2.astype(np.float32).astype(np.float64)
    cache = {}
    return [cache.setdefault(row.tobytes(), X.structure(row, h1, h2)) for row in walkers(name)]


def _unique_rows(bits: np.ndarray) -> np.ndarray:
    seen, keep = set(), []
    for i, row in enumerate(bits):
        b = row.tobytes()
        if b not in seen:
            seen.add(b)
            keep.append(i)
    return bits[keep]


@functools.lru_cache(maxsize=None)
def table_keys(name: str, table: str) -> np.ndarray:
    """the keys of a case, 0/1 [nk, sorb], distinct, in the order of their construction"""
    s, occ, sts = SHAPES[name], walkers(name), structures(name)
    g = np.random.default_rng(1000 + len(table) + s.sorb)
    own = _unique_rows(occ)
    conn = np.concatenate([st.bits for st in sts])
    conn = _unique_rows(np.concatenate([conn, S.flip_bits(np.concatenate([own, conn]))]))  # (their spin-flip partners: what the flip passes find)
    mine = {r.tobytes() for r in own}
    conn = conn[[r.tobytes() not in mine for r in conn]]
    if table == "all":
        return np.concatenate([own, conn])
    if table == "half":
        return np.concatenate([own, conn[g.random(conn.shape[0]) < 0.5]])
    if table == "walkers":
        return own
    if table == "one":
        return own[:1]
    if table == "absent2":
        assert own.shape[0] >= 3
        return np.concatenate([own[2:], conn])
    assert table == "far"
    far = _unique_rows(rand_occ(400, s.sorb, s.noA, s.noB, seed=5))
    far = far[[(np.bitwise_xor(r[None, :], occ).sum(1) >= 6).all() for r in far]][:40]
    assert far.shape[0] == 40
    return np.concatenate([own, far])


def zero_walkers(name: str, table: str) -> int:
    """walkers constructed without their own key: psi(x) = 0"""
    occ = walkers(name)
    if table == "one":
        return int((occ != occ[0]).any(1).sum())
    if table == "absent2":
        own = _unique_rows(occ)
        return int(sum(1 for r in occ if (r == own[0]).all() or (r == own[1]).all()))
    return 0


def mantissas(name: str, table: str, values: str) -> np.ndarray:
    """the table's amplitudes at scale 2^0: float64 / complex128 [nk]; moduli in [0.25, 1.25) (spread: times 2^e), free signs / phases"""
    nk = table_keys(name, table).shape[0]
    g = np.random.default_rng(zlib.crc32(f"{name} {table} {values}".encode()))
    mod = g.random(nk) + 0.25
    if values.endswith("spread"):
        mod = np.ldexp(mod, g.integers(-SPREAD, SPREAD + 1, nk).astype(np.int32))
    if values.startswith("real"):
        return mod * np.where(g.random(nk) < 0.5, -1.0, 1.0)
    return mod * np.exp(2j * np.pi * g.random(nk))


@functools.lru_cache(maxsize=None)
def neighbourhoods(name: str, table: str):
    """(ss_exact.Table, [ss_exact.Columns per walker], [the same for the flip passes])"""
    tab = S.Table(table_keys(name, table))
    cache = {}

    def cols(st, flip):
        key = (id(st), flip)
        if key not in cache:
            cache[key] = S.columns(st, tab, flip)
        return cache[key]

    sts = structures(name)
    return tab, [cols(st, False) for st in sts], [cols(st, True) for st in sts]


def yardstick(name: str, table: str, values: str, k: int):
    """([ss_exact.Result per walker] of the plain sum, the same of the partner sum over psi(x) of the plain one) at scale 2^k"""
    _, plain, part = neighbourhoods(name, table)
    v = S.scaled(S.as_ld(mantissas(name, table, values)), k)
    p = [S.table_sum(c, v) for c in plain]
    return p, [S.table_sum(c, v, psi_x=r.psi) for c, r in zip(part, p)]


def psi_array(results, dtype) -> np.ndarray:
    """psi(x) of the results as the kernels return it"""
    z = np.array([complex(r.psi) for r in results])
    return z if np.dtype(dtype).kind == "c" else np.ascontiguousarray(z.real)


def case_id(c):
    return "-".join(str(v) for v in c)


def report(what, ratio):
    ratio = np.atleast_1d(np.asarray(ratio, dtype=np.float64))
    worst = int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)))
    print(f"{what}: worst error / bound {ratio[worst]:.3g} at {worst} of {ratio.size}")
    return f"{what}: error / bound {ratio[worst]:.3g} at {worst}, {int((~(ratio <= 1)).sum())} of {ratio.size} outside"


def ratios(results, got: np.ndarray):
    """(|E_got - E_exact| / bound per walker with psi(x) != 0, inf where the kernel's value is not finite; the walkers with psi(x) = 0
    whose value IS finite)"""
    got = np.asarray(got)
    assert got.shape == (len(results),)
    out, finite_zero = [], 0
    for r, g in zip(results, got):
        g = complex(g)
        fin = np.isfinite(g.real) and np.isfinite(g.imag)
        if r.zero:
            finite_zero += int(fin)
        else:
            err = float(abs(S.CLD(g) - r.E)) if fin else np.inf
            out.append(err / r.bound if r.bound > 0 else (0.0 if err == 0 else np.inf))  # (no term at all: the sum is an exact zero)
    return np.array(out), finite_zero


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _onv(bits: np.ndarray, sorb: int) -> np.ndarray:
    from oracle import oracle

    return oracle.pm01_to_onv(np.ascontiguousarray(bits, dtype=np.uint8), sorb)


class Device:
    """A case on the GPU: walkers, plan, the keys sorted (with their hash table) and shuffled (with their block index)."""

    def __init__(self, name: str, table: str, key_bits=None) -> None:
        """key_bits: the keys (0/1 [nk, sorb]) of a table that table_keys does not construct (tests/test_gpu_key_tables.py)"""
        from pynqs_amd import C_extension as cx, public_function as pf

        s = SHAPES[name]
        self.s, dev = s, torch.device("cuda")
        h1, h2 = integrals(s.ints, s.sorb)
        self.h1, self.h2 = _dev(h1), _dev(h2)
        self.plan = cx.plan_for(self.h1, self.h2, s.sorb, dev)
        self.x = _dev(_onv(walkers(name), s.sorb))
        keys = _dev(_onv(table_keys(name, table) if key_bits is None else key_bits, s.sorb))
        self.nk = keys.size(0)
        self.lut = pf.WavefunctionLUT(keys, torch.zeros(self.nk, dtype=torch.float64, device=dev), s.sorb, device=dev)
        assert self.lut.hashtable is not None
        self.to_sorted = self.lut.idx_sorted.to(dev)  # position of the i-th constructed key in the sorted table
        self.perm = torch.randperm(self.nk, generator=torch.Generator().manual_seed(3)).to(dev)
        self.shuffled = keys[self.perm].contiguous()
        self.index = cx.keys_index_build(self.shuffled, s.sorb)

    def values(self, v: np.ndarray):
        """(in the sorted keys' order, in the shuffled keys' order)"""
        v = _dev(v)
        srt = torch.empty_like(v)
        srt[self.to_sorted] = v
        return srt, v[self.perm].contiguous()

    def run(self, f: Form, v_sorted, v_shuffled, psi0=None):
        """(E or the partner sum, psi(x)) of one entry point, host arrays; flip passes take psi0"""
        from pynqs_amd import _native as N

        s, lib = self.s, N.lib()
        cplx = v_sorted.is_complex()
        n = self.x.size(0)
        out = torch.full((n,), 7.0, dtype=v_sorted.dtype, device="cuda")
        p0 = torch.full((n,), 7.0, dtype=v_sorted.dtype, device="cuda") if psi0 is None else _dev(psi0)
        st = torch.cuda.current_stream().cuda_stream
        head = (self.x.data_ptr(), n, s.sorb, s.noA + s.noB, s.noA, s.noB, self.plan.data_ptr())
        fn = getattr(lib, f.entry)
        if f.shuffled:
            tab = (self.shuffled.data_ptr(), self.nk) + ((self.index.index.data_ptr(),) if f.fixed else ())
            rc = fn(*head, *tab, v_shuffled.data_ptr(), int(cplx), int(f.flip), out.data_ptr(), p0.data_ptr(), st)
        else:
            tab = (self.lut.hashtable.table.data_ptr(), self.nk) if "hash" in f.entry else (self.lut.bra_key.data_ptr(), self.nk)
            a, b = (p0, out) if f.flip else (out, p0)
            rc = fn(*head, *tab, v_sorted.data_ptr(), int(cplx), a.data_ptr(), b.data_ptr(), st)
        N.check(rc, f.entry)
        return out.cpu().numpy(), p0.cpu().numpy()


@functools.lru_cache(maxsize=None)
def device(name: str, table: str) -> Device:
    return Device(name, table)


@pytest.mark.parametrize("values", VALUES)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_entry_point_meets_the_bound_at_every_scale(case, values):
    name, table = case
    d = device(name, table)
    mant = mantissas(name, table, values)
    nzero = zero_walkers(name, table)
    msg, bad, first = [], 0, {}
    for k in scales_of(values):
        plain, part = yardstick(name, table, values, k)
        psi_want = psi_array(plain, mant.dtype)
        assert sum(r.zero for r in plain) == nzero
        vs, vh = d.values(S.scaled(mant, k))
        for f in FORMS:
            e, p0 = d.run(f, vs, vh, psi_want if f.flip else None)
            np.testing.assert_array_equal(p0, psi_want, err_msg=f"{f.name} 2^{k}: psi(x)")
            ratio, finite_zero = ratios(part if f.flip else plain, e)
            line = report(f"SS {case_id(case)} {values} {f.name} 2^{k}", ratio) if ratio.size else f"{f.name} 2^{k}: no walker in the table"
            if finite_zero or not bool((ratio <= 1.0).all()):
                bad += 1
                msg.append(line + f"; finite E_loc at psi(x) = 0: {finite_zero} of {nzero}")
            if f.fixed:  # a fixed order of additions: power-of-two scaling changes no bit
                ok = np.array([not r.zero for r in plain])
                if k == 0:
                    first[f.name] = e
                elif not np.array_equal(e[ok].view(np.float64), first[f.name][ok].view(np.float64)):
                    bad += 1
                    msg.append(f"{f.name} 2^{k}: {int((e[ok] != first[f.name][ok]).sum())} of {int(ok.sum())} walkers differ from 2^0 in some bit")
    assert bad == 0, msg


# ---- through the energy layer ------------------------------------------------------------------------------------------------------
ROUTE_CASE = ("s12", "half")


@pytest.mark.parametrize("key_major", [True, False], ids=["key-major", "column-major"])
def test_local_energy_sample_space_at_every_scale(key_major, monkeypatch):
    """energy.local_energy(use_sample_space=True) with SS_KEYS forced both ways, complex amplitudes"""
    from pynqs_amd import energy

    name, table = ROUTE_CASE
    d, s = device(name, table), SHAPES[name]
    monkeypatch.setattr(energy, "SS_KEYS", key_major)
    mant = mantissas(name, table, "complex")
    msg, bad = [], 0
    for k in SCALES:
        plain, _ = yardstick(name, table, "complex", k)
        d.lut._wf_value = d.values(S.scaled(mant, k))[0]
        e, _, p0, _ = energy.local_energy(d.x, d.h1, d.h2, None, None, s.sorb, s.noA + s.noB, s.noA, s.noB, dtype=torch.complex128, WF_LUT=d.lut,
                                          use_sample_space=True)
        np.testing.assert_array_equal(p0.cpu().numpy(), psi_array(plain, np.complex128))
        ratio, _ = ratios(plain, e.cpu().numpy())
        line = report(f"SS local_energy {'key-major' if key_major else 'column-major'} 2^{k}", ratio)
        if not bool((ratio <= 1.0).all()):
            bad += 1
            msg.append(line)
    assert bad == 0, msg


FLIP_SCALES = (0, 300, -300)   # extra_norm^2 = 2^(2k) must itself be a double


def flip_reference(k: int):
    """[(E, bound) per walker] of E = (plain + eta partner) / extra_norm^2 with the table and extra_norm both scaled by 2^k: the two sums'
    bounds, one rounding for their addition (the division by a power of two is exact)"""
    name, table = ROUTE_CASE
    s = SHAPES[name]
    eta = -1 if ((s.noA + s.noB) // 2) % 2 else 1
    plain, part = yardstick(name, table, "complex", k)
    n2 = S.scaled(np.array([1.0], dtype=S.LD), 2 * k)[0]
    return [((a.E + eta * b.E) / n2, float((S.LD(a.bound + b.bound) + S.U * (abs(a.E) + abs(b.E))) / n2)) for a, b in zip(plain, part)]


@pytest.mark.parametrize("key_major", [True, False], ids=["key-major", "column-major"])
def test_local_energy_spin_flip_sample_space(key_major, monkeypatch):
    from pynqs_amd import energy, public_function as pf

    name, table = ROUTE_CASE
    d, s = device(name, table), SHAPES[name]
    monkeypatch.setattr(energy, "SS_KEYS", key_major)
    mant = mantissas(name, table, "complex")
    pf.SpinProjection.init(s.noA + s.noB, 0)
    try:
        msg, bad = [], 0
        for k in FLIP_SCALES:
            ref = flip_reference(k)
            d.lut._wf_value = d.values(S.scaled(mant, k))[0]
            en = torch.tensor(2.0 ** k, dtype=torch.float64, device="cuda")
            e, _, _, _ = energy.local_energy(d.x, d.h1, d.h2, None, None, s.sorb, s.noA + s.noB, s.noA, s.noB, dtype=torch.complex128, WF_LUT=d.lut,
                                             use_sample_space=True, use_spin_flip=True, extra_norm=en)
            e = e.cpu().numpy()
            ratio = np.array([float(abs(S.CLD(complex(g)) - E)) / b if np.isfinite(complex(g).real + complex(g).imag) else np.inf for g, (E, b) in zip(e, ref)])
            line = report(f"SS local_energy spin-flip {'key-major' if key_major else 'column-major'} 2^{k}", ratio)
            if not bool((ratio <= 1.0).all()):
                bad += 1
                msg.append(line)
        assert bad == 0, msg
    finally:
        pf.SpinProjection.init(30, 0)


# ---- the contraction of the REDUCE front end ------------------------------------------------------------------------------------
RShape = namedtuple("RShape", "name shape n f32 N eps lut")
# eps: "0" (the full sum) or "gap" (ss_exact.eps_in_largest_gap of the case's walkers); N: drawn records per walker; lut: the first so many
# determinants of the CI space are a wave-function table asked inside the kernel (links <= -2)
REDUCE_CASES = [RShape("s12-eps0", "s12", 24, False, 0, "0", 0), RShape("s12-gap", "s12", 24, False, 0, "gap", 0),
                RShape("s12-gap-N300", "s12", 24, False, 300, "gap", 0), RShape("s12-f32-gap-N300", "s12", 24, True, 300, "gap", 0),
                RShape("fe2s2-gap-N300-table", "fe2s2", 4, False, 300, "gap", 3000)]


def reduce_rows(c: RShape) -> np.ndarray:
    """the case's walkers: the c.n of the shape's with the largest |<x|H|x>| (eps must leave column 0, which brings psi(x), among the kept)"""
    h0 = np.array([abs(float(st.h0)) for st in structures(c.shape, c.f32)])
    return np.sort(np.argsort(-h0, kind="stable")[: c.n])


def reduce_structures(c: RShape):
    sts = structures(c.shape, c.f32)
    return [sts[i] for i in reduce_rows(c)]


def reduce_eps(c: RShape):
    """(eps, half width of the gap)"""
    return (0.0, np.inf) if c.eps == "0" else S.eps_in_largest_gap(reduce_structures(c))


def reduce_reference(c: RShape, all_bits: np.ndarray, rec_walker, rec_bits, rec_w, rec_drawn):
    """(ss_exact.Table over all_bits, [ss_exact.Columns per walker]) from the records' discrete data: which columns were drawn, how often"""
    eps, _ = reduce_eps(c)
    sts = reduce_structures(c)
    tab = S.Table(all_bits)
    cols = []
    for i, st in enumerate(sts):
        where = {row.tobytes(): j for j, row in enumerate(np.concatenate([st.occ[None, :], st.bits]))}
        mine = rec_walker == i
        kept_got = sorted(where[b.tobytes()] for b in rec_bits[mine & ~rec_drawn])
        h = np.concatenate([[st.h0], st.h])
        assert kept_got == np.flatnonzero(np.abs(h) >= S.LD(eps)).tolist(), (c.name, i)
        drawn = None
        if c.N:
            Srow = S.row_sum(st, eps)
            hits = np.abs(rec_w[mine & rec_drawn].astype(np.float64)) * c.N / float(Srow)
            assert float(np.abs(hits - np.rint(hits)).max()) < (2e-2 if c.f32 else 1e-6)
            drawn = {where[b.tobytes()]: int(v) for b, v in zip(rec_bits[mine & rec_drawn], np.rint(hits))}
        cols.append(S.reduce_columns(st, tab, eps, drawn, c.N, S.U32 if c.f32 else S.U))
        assert bool((cols[-1].pos[cols[-1].wabs > 0] >= 0).all())  # every record's determinant has an amplitude
    return tab, cols


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("case", REDUCE_CASES, ids=lambda c: c.name)
def test_contraction_meets_the_bound_at_every_scale(case, cplx):
    from pynqs_amd import energy, public_function as pf

    c, s = case, SHAPES[case.shape]
    dev = torch.device("cuda")
    h1, h2 = integrals(s.ints, s.sorb)
    dt = torch.float32 if c.f32 else torch.float64
    h1e, h2e = _dev(h1).to(dt), _dev(h2).to(dt)
    x = _dev(_onv(walkers(c.shape)[reduce_rows(c)], s.sorb))
    eps, _ = reduce_eps(c)
    g = np.random.default_rng(5 + c.N)
    lut, lut_bits, lut_mant = None, np.zeros((0, s.sorb), dtype=np.uint8), np.zeros(0)
    if c.lut:
        lut_onv = np.ascontiguousarray(golden("fe2s2_inputs.npz")["ci_space"][: c.lut])
        lut = pf.WavefunctionLUT(_dev(lut_onv), torch.zeros(c.lut, dtype=torch.float64, device=dev), s.sorb, device=dev)
        lut_bits = bits_of(lut.bra_key.cpu().numpy(), s.sorb)  # (the sorted order: the links are positions in it)
        lut_mant = g.random(c.lut) + 0.25
    energy._FRONTS.clear()
    fe, nu = energy.reduce_front(x, h1e, h2e, s.sorb, s.noA + s.noB, s.noA, s.noB, eps, c.N, lut.hashtable if lut is not None else None, seed=17)
    walker, _, w, link, onv, drawn = fe.records()
    assert (lut is None) or bool((link <= -2).any()) and bool((link >= 0).any())  # the table serves part of the records
    uniq_bits = bits_of(fe.uniq_onv[:nu].cpu().numpy(), s.sorb)
    mant = np.concatenate([g.random(nu) + 0.25, lut_mant])
    mant = mant * np.exp(2j * np.pi * g.random(mant.size)) if cplx else mant * np.where(g.random(mant.size) < 0.5, -1.0, 1.0)
    _, cols = reduce_reference(c, np.concatenate([uniq_bits, lut_bits]), walker.cpu().numpy(), bits_of(onv.cpu().numpy(), s.sorb), w.cpu().numpy(),
                               drawn.cpu().numpy())
    msg, bad, first = [], 0, None
    for k in SCALES:
        v = S.scaled(mant, k)
        vl = S.as_ld(v)
        want = [S.contract(cc.w, cc.dw, cc.wabs, np.where(cc.pos >= 0, vl[np.maximum(cc.pos, 0)], 0), vl[cc.pos[0]], cplx) for cc in cols]
        e, px = fe.contract(_dev(v[:nu]), _dev(v[nu:]) if lut is not None else None)
        e, px = e.cpu().numpy(), px.cpu().numpy()
        np.testing.assert_array_equal(px, psi_array(want, v.dtype), err_msg=f"2^{k}: psi(x)")
        ratio, _ = ratios(want, e)
        line = report(f"SS contract {c.name} {'complex' if cplx else 'real'} 2^{k}", ratio)
        if not bool((ratio <= 1.0).all()):
            bad += 1
            msg.append(line)
        if k == 0:
            first = e
        elif not np.array_equal(e.view(np.float64), first.view(np.float64)):  # one wave per walker, fixed order: the same bits at every scale
            bad += 1
            msg.append(f"2^{k}: {int((e != first).sum())} of {e.size} walkers differ from 2^0 in some bit")
    assert bad == 0, msg


# ---- REDUCE end to end through an RBM whose amplitudes are near 1e250 ----------------------------------------------------------------
RBM_SHAPE, RBM_H, RBM_N = "s12", 400, 8


@functools.lru_cache(maxsize=None)
def big_rbm():
    """ComplexRBM with 400 hidden units, Re b_h such that ln 2cosh theta_h ~ 1.44 per unit: |psi(x)| ~ 1e250"""
    s = SHAPES[RBM_SHAPE]
    g = np.random.default_rng(42)
    W = 0.05 * (g.random((RBM_H, s.sorb)) - 0.5) + 0.05j * (g.random((RBM_H, s.sorb)) - 0.5)
    hb = 1.376 + 0.05 * (g.random(RBM_H) - 0.5) + 0.3j * (g.random(RBM_H) - 0.5)
    vb = 0.1 * (g.random(s.sorb) - 0.5) + 0.1j * (g.random(s.sorb) - 0.5)
    return R.make("complex", W, hb, vb)


@functools.lru_cache(maxsize=None)
def rbm_reference():
    """[(eloc_exact.Walker, ss_exact.Result) per walker]"""
    rbm = big_rbm()
    out = []
    for st in structures(RBM_SHAPE)[:RBM_N]:
        w = X.walker(rbm, st)
        rows = np.concatenate([st.occ[None, :], st.bits]).astype(np.float64) * 2 - 1
        out.append((w, S.rbm_reduce(w, R.exact_ld(rbm, rows).cond, RBM_H)))
    return out


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_reduce_through_an_rbm_of_amplitude_1e250(fused, monkeypatch):
    """local_energy(reduce_psi=True, eps=0) with energy.FUSED both ways against eloc_exact.walker, whose ratios live in the log domain"""
    from pynqs_amd import energy, public_function as pf
    from pynqs_amd.rbm import ComplexRBM

    s, rbm, ref = SHAPES[RBM_SHAPE], big_rbm(), rbm_reference()
    monkeypatch.setattr(energy, "FUSED", fused)
    h1, h2 = integrals(s.ints, s.sorb)
    x = _dev(_onv(walkers(RBM_SHAPE)[:RBM_N], s.sorb))
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        energy._FRONTS.clear()
        m = ComplexRBM(_dev(R.pairs(rbm.W)), _dev(R.pairs(rbm.hb)), _dev(R.pairs(rbm.vb))).cuda()
        ab = lambda xx, func: pf.ansatz_batch(func, xx, 100000, s.sorb, x.device, torch.complex128)  # noqa: E731
        e, _, p, _ = energy.local_energy(x, _dev(h1), _dev(h2), m, ab, s.sorb, s.noA + s.noB, s.noA, s.noB, dtype=torch.complex128, reduce_psi=True, eps=0.0)
    finally:
        torch.set_default_dtype(old)
    psi = R.Exact(rbm.kind, *(np.concatenate([getattr(w.psi, f) for w, _ in ref]) for f in ("re", "im", "vis", "cond", "y", "sech2")))
    rp = R.amp_ratio(rbm, p.cpu().numpy(), psi)
    ratio, _ = ratios([r for _, r in ref], e.cpu().numpy())
    msg = [report(f"SS reduce rbm-1e250 {'fused' if fused else 'unfused'} E_loc", ratio), report("psi(x)", rp)]
    assert bool((ratio <= 1.0).all()) and bool((rp <= 1.0).all()), msg
