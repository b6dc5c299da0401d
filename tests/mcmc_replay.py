"""Host side of the many-chain Metropolis tests: the documented random streams (include/pynqs_amd.h, "many-chain Metropolis sampling"),
exact ln|psi| of the RBM flavours from their float64 parameters, and a step-by-step replay of the accept rule against a run's records.

The replay takes every step from the kernel's own recorded state before it (teacher forcing), draws the proposal from the CPU oracle
(column r0 of oracle.comb, column 0 being the state itself) and decides with the exact amplitudes:
    accept  iff  |psi(x)| == 0  or  ln u <= 2 (ln|psi(x')| - ln|psi(x)|).
A step is a tie when |ln u - 2 delta| < tau, tau = 1e-10 (scale(x) + scale(x')), scale = 1 + sum_h |Re theta_h| + |Re a.x|: either
decision is allowed there.  ln|psi| is evaluated in numpy longdouble straight from theta = b + W x (no incremental state), or with
mpmath at 40 digits where the set of states is small; the longdouble values are spot-checked against mpmath."""
from __future__ import annotations

from dataclasses import dataclass

import mpmath
import numpy as np

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
ACCEPT_KEY = np.uint64(0x243F6A8885A308D3)  # PYNQS_MCMC_ACCEPT_KEY
TAU = 1e-10
LDS_BYTES = 64 * 1024  # the fused kernel keeps its table in LDS up to this size
MP_DPS = 40
MP_WORK = 3e5  # states x hidden units x orbitals up to which every state is evaluated with mpmath


def mix64(z):
    with np.errstate(over="ignore"):
        z = (z + np.uint64(0x9E3779B97F4A7C15)) & M64
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def umulhi32(h, m):
    """(h * m) >> 64 for m < 2^32."""
    m = np.uint64(m)
    with np.errstate(over="ignore"):
        hi, lo = h >> np.uint64(32), h & np.uint64(0xFFFFFFFF)
        return (hi * m + ((lo * m) >> np.uint64(32))) >> np.uint64(32)


def host_r0(seed, t, c, nsd):
    """The proposal's rank r0 of step t, chain c (0: stay, else column r0 of the state's singles and doubles)."""
    return umulhi32(mix64(mix64(np.uint64(seed)) ^ mix64((np.uint64(t) << np.uint64(32)) + c)), nsd + 1).astype(np.int64)


def host_u(seed, t, c):
    """The acceptance draw u in (0, 1] of step t, chain c."""
    h = mix64(mix64(np.uint64(seed) ^ ACCEPT_KEY) ^ mix64((np.uint64(t) << np.uint64(32)) + c))
    return ((h >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def mcmc_group(nhidden: int) -> int:
    """Lanes per chain of the fused kernel (kernels_mcmc.hip: 8 hidden units per lane, a power of two)."""
    G = 1
    while 8 * G < nhidden:
        G *= 2
    return G


def table_doubles(kind: str, sorb: int, H: int) -> int:
    """Size in doubles of the RBM table (include/pynqs_amd.h, pynqs_rbm_table_build / pynqs_crbm_table_build)."""
    if kind in ("complex", "cos"):
        Hs = ((H + 1) & ~1) + 1
        return 2 * (3 * sorb * Hs + Hs + sorb)
    Hq = ((H + 7) & ~7) + 1
    return (3 * sorb * Hq + Hq + sorb + 1) & ~1


def pm1(words: np.ndarray, sorb: int) -> np.ndarray:
    """uint64 [n, len] ONV words -> float64 [n, sorb] +-1 (orbital o = bit o)."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :sorb]
    return bits.astype(np.float64) * 2.0 - 1.0


@dataclass
class Rbm:
    """The amplitude of one flavour: W [H, sorb], hb [H], vb [sorb] float64 (complex128 for "complex"; "cos" and "pRBM" ignore vb in
    |psi|).  ln|psi| is the fused kernel's: real a.x + sum ln 2cosh theta, tanh ln|tanh a.x| + sum ln 2cosh theta, complex
    Re a.x + sum ln|2cosh theta|, cos sum ln|2cos theta| (2^H times the module's psi: the same ratios), pRBM 0."""
    kind: str
    W: np.ndarray
    hb: np.ndarray
    vb: np.ndarray

    @property
    def H(self) -> int:
        return self.W.shape[0]

    def lnabs_ld(self, x: np.ndarray):
        """(ln|psi| longdouble [n], scale float64 [n]) of the +-1 rows x, in numpy longdouble."""
        n = x.shape[0]
        if self.kind == "pRBM":
            return np.zeros(n, dtype=np.longdouble), np.ones(n)
        xl = x.astype(np.longdouble)
        with np.errstate(divide="ignore"):
            if self.kind == "complex":
                a = self.hb.real.astype(np.longdouble) + xl @ self.W.real.T.astype(np.longdouble)
                b = self.hb.imag.astype(np.longdouble) + xl @ self.W.imag.T.astype(np.longdouble)
                # |2cosh(a + ib)|^2 = 4 (cos^2 b + sinh^2 a): no cancellation, no overflow below |a| ~ 5000 in longdouble
                lnh = (0.5 * np.log(4 * (np.cos(b) ** 2 + np.sinh(a) ** 2))).sum(1)
                ax = xl @ self.vb.real.astype(np.longdouble)
                return lnh + ax, 1.0 + np.abs(a).sum(1).astype(np.float64) + np.abs(ax).astype(np.float64)
            th = self.hb.astype(np.longdouble) + xl @ self.W.T.astype(np.longdouble)
            if self.kind == "cos":
                return np.log(np.abs(2 * np.cos(th))).sum(1), np.ones(n)
            lnh = np.log(2 * np.cosh(th)).sum(1)
            ax = xl @ self.vb.astype(np.longdouble)
            vis = np.log(np.abs(np.tanh(ax))) if self.kind == "tanh" else ax
            return lnh + vis, 1.0 + np.abs(th).sum(1).astype(np.float64) + np.abs(ax).astype(np.float64)

    def lnabs_mp(self, row: np.ndarray) -> mpmath.mpf:
        """ln|psi| of one +-1 row with mpmath at MP_DPS digits (the parameters converted exactly)."""
        mp = mpmath.mp
        with mpmath.workdps(MP_DPS):
            if self.kind == "pRBM":
                return mp.mpf(0)
            xs = [int(v) for v in row]

            def dot(w, b):
                return mp.fsum([mp.mpf(b)] + [mp.mpf(float(wo)) if xo > 0 else -mp.mpf(float(wo)) for wo, xo in zip(w, xs)])

            if self.kind == "complex":
                tot = mp.mpf(0)
                for h in range(self.H):
                    th = mp.mpc(dot(self.W[h].real, self.hb[h].real), dot(self.W[h].imag, self.hb[h].imag))
                    tot += mp.log(abs(2 * mp.cosh(th)))
                return tot + dot(self.vb.real, 0.0)
            if self.kind == "cos":
                return mp.fsum([mp.log(abs(2 * mp.cos(dot(self.W[h], self.hb[h])))) for h in range(self.H)])
            tot = mp.fsum([mp.log(2 * mp.cosh(dot(self.W[h], self.hb[h]))) for h in range(self.H)])
            ax = dot(self.vb, 0.0)
            if self.kind == "tanh":
                t = mp.tanh(ax)
                return tot + (mp.log(abs(t)) if t != 0 else mp.mpf("-inf"))
            return tot + ax

    def lnabs(self, x: np.ndarray, rng: np.random.Generator, nspot: int = 8):
        """(ln|psi| float64-rounded longdouble [n] as longdouble, scale [n], source) of the rows x: mpmath for all rows when the work is
        small, else longdouble with `nspot` rows checked against mpmath (to 1e-4 tau)."""
        ld, scale = self.lnabs_ld(x)
        if x.shape[0] * self.H * x.shape[1] <= MP_WORK or self.kind == "pRBM":
            idx, source = np.arange(x.shape[0]), "mpmath"
        else:
            idx, source = rng.choice(x.shape[0], size=min(nspot, x.shape[0]), replace=False), "longdouble"
        for k in idx:
            m = self.lnabs_mp(x[k])
            if mpmath.isinf(m):
                assert np.isneginf(ld[k]), (k, ld[k])
                continue
            err = abs(float(m - mpmath.mpf(str(ld[k])))) if np.isfinite(ld[k]) else np.inf
            assert err <= 1e-4 * TAU * scale[k], (self.kind, k, float(m), ld[k], err)
            if source == "mpmath":
                ld[k] = np.longdouble(mpmath.nstr(m, 30))
        return ld, scale, source


@dataclass
class Replay:
    steps: int            # chain-steps replayed
    ties: int
    mismatches: int       # non-tie steps whose record differs from the rule
    accepted: np.ndarray  # int64 [nchains]: moves accepted (record == proposal; a move to the state itself included)
    lnpsi_err: float      # max |lnpsi - exact| / tau of the final states (nan without lnpsi)
    source: str
    exact: dict           # state key -> (ln|psi|, scale) of every state evaluated
    prev: np.ndarray      # uint64 [T, nchains, len]: the state before every step
    prop: np.ndarray      # uint64 [T, nchains, len]: its proposal
    first_bad: str


def _keys(rows: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(rows).view(np.dtype((np.void, rows.dtype.itemsize * rows.shape[1]))).ravel()


def proposals(oracle, prev: np.ndarray, r0: np.ndarray, sorb: int, noA: int, noB: int) -> np.ndarray:
    """Column r0 of oracle.comb(prev) for every row (prev uint64 [n, len], r0 int64 [n]), in chunks of bounded memory."""
    L = prev.shape[1]
    uniq, inv = np.unique(prev, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    nc = oracle.num_sd(sorb, noA, noB) + 1
    out = np.empty_like(prev)
    chunk = max(1, (64 << 20) // (nc * L * 8))
    order = np.argsort(inv, kind="stable")
    bounds = np.searchsorted(inv[order], np.arange(0, uniq.shape[0] + chunk, chunk))
    for k in range(len(bounds) - 1):
        lo = k * chunk
        sel = order[bounds[k]:bounds[k + 1]]
        if sel.size == 0:
            continue
        comb, _ = oracle.comb(uniq[lo:lo + chunk].view(np.uint8), sorb, noA, noB)
        comb = comb.view(np.uint64).reshape(-1, nc, L)
        out[sel] = comb[inv[sel] - lo, r0[sel]]
    return out


def replay(oracle, rbm: Rbm, sorb: int, noA: int, noB: int, seed: int, chain_base: int, t0: int, x0: np.ndarray, records: np.ndarray,
           lnpsi=None, rng_seed: int = 0) -> Replay:
    """Replay steps t0 .. t0 + T - 1 of nchains chains (x0 uint64 [nchains, len] the states before step t0, records uint64 [T, nchains,
    len] the states after every step) with the exact rule; lnpsi (float64 [nchains], optional): the kernel's ln|psi| of the final states."""
    T, nch, L = records.shape
    prev = np.concatenate([x0[None], records[:-1]], 0)
    c = np.uint64(chain_base) + np.arange(nch, dtype=np.uint64)
    nsd = oracle.num_sd(sorb, noA, noB)
    r0 = np.stack([host_r0(seed, t0 + k, c, nsd) for k in range(T)])
    u = np.stack([host_u(seed, t0 + k, c) for k in range(T)])
    prop = proposals(oracle, prev.reshape(-1, L), r0.reshape(-1), sorb, noA, noB).reshape(T, nch, L)
    allrows = np.concatenate([prev.reshape(-1, L), prop.reshape(-1, L), records[-1]], 0)
    uniq, inv = np.unique(allrows, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    lnu_ld, scale_u, source = rbm.lnabs(pm1(uniq, sorb), np.random.default_rng(rng_seed))
    n = T * nch
    ip, iq, ifin = inv[:n], inv[n:2 * n], inv[2 * n:]
    Lp, Lq = lnu_ld[ip], lnu_ld[iq]
    zero = np.isneginf(Lp)
    with np.errstate(invalid="ignore"):
        d2 = np.where(zero, np.longdouble(0), 2 * (Lq - Lp))
    lnu = np.log(u.reshape(-1).astype(np.longdouble))
    want = zero | (lnu <= d2)
    tau = TAU * (scale_u[ip] + scale_u[iq])
    same = ip == iq
    tie = ~zero & ~same & np.isfinite(d2) & (np.abs((lnu - d2).astype(np.float64)) < tau)
    rec = records.reshape(-1, L)
    is_q = (rec == prop.reshape(-1, L)).all(1)
    is_p = (rec == prev.reshape(-1, L)).all(1)
    bad = ~(is_q | is_p) | (~tie & np.where(want, ~is_q, ~is_p))
    first_bad = ""
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        first_bad = (f"step {t0 + k // nch} chain {chain_base + k % nch}: r0 {r0.reshape(-1)[k]}, ln|psi| {float(Lp[k])} -> "
                     f"{float(Lq[k])}, ln u {float(lnu[k])}, rule {'accept' if want[k] else 'reject'}, record = "
                     f"{'proposal' if is_q[k] else 'state' if is_p[k] else 'neither'}")
    err = float("nan")
    if lnpsi is not None:
        fin = lnu_ld[ifin]
        lp = np.asarray(lnpsi, dtype=np.float64)
        both_inf = np.isneginf(fin) & np.isneginf(lp)
        d = np.where(both_inf, 0.0, np.abs((lp.astype(np.longdouble) - fin).astype(np.float64)))
        err = float(np.nanmax(np.where(np.isnan(d), np.inf, d) / (TAU * scale_u[ifin])))
    exact = {bytes(k): (lnu_ld[j], scale_u[j]) for j, k in enumerate(_keys(uniq))}
    return Replay(n, int(tie.sum()), int(bad.sum()), is_q.reshape(T, nch).sum(0), err, source, exact, prev, prop, first_bad)
