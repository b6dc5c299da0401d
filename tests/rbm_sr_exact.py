"""Host-side exact reference of stochastic reconfiguration for the RBM amplitudes (pynqs_rbm_sr_prepare / _matvec / _cg_step and
pynqs_amd.sr.FusedRbmSR; include/pynqs_amd.h), on top of rbm_exact.exact_ld's tanh theta: the log-derivatives O, their mean Obar, the
matrix S, the product S v, the gradient F and the solution d of (S + shift) d = F, all in numpy longdouble from the float64 parameters,
the +-1 rows and the probabilities alone; nothing depends on a kernel's output.

Layout.  Holomorphic index k runs over weights [H][sorb], hidden_bias [H], visible_bias [sorb] (P = H sorb + H + sorb); the flat real
vector is that for real parameters and (re, im) interleaved for complex parameters (P_real = 2 P), the modules' own storage order.
    O_nk = (tanh theta_nh x_no, tanh theta_nh, x_no),  Obar = sum_n p_n O_n,  J = O - Obar,
    c = J z,   y = J^H diag(p) c = sum_n p_n conj(O_n) c_n   (sum_n p_n c_n = 0 when p sums to 1 and Obar is the same p's mean),
    S v = y (real) or (Re y, Im y) (pairs): the real form [[A, -B], [B, A]] of S_c = J^H diag(p) J = A + i B.
d: with R = the real form of diag(sqrt p) J (S = R^T R), (S + shift)^-1 = (1 - R^T (shift + R R^T)^-1 R) / shift needs a matrix of the
size of the walkers only; that float64 solve is refined with longdouble residuals F - (S + shift) d (formed matrix-free) until the
correction is below 1e-17 of |d| or no longer shrinks: a residual formed in longdouble carries its own rounding, about 2^-64 |S| |d| times
a modest growth factor, which the inverse turns into cond(S + shift) 2^-64 of |d| -- 1e-16 ... 1e-15 at the condition numbers of the
test cases (1e3 ... 1e5), so 1e-17 is reached only on the well-conditioned ones.  solve() returns the size of the last correction, the
tests require it below SOLVE_FLOOR = 1e-13 (a thousandth of what the tightest comparison with d allows) and add it to what they allow.

A-priori bound on the product (written before any kernel output was looked at; u = 2^-53).  The kernel forms c_n, then g_n = p_n c_n,
then y_k = sum_n conj(O_nk) g_n by the gradient kernel's outer products with tanh theta read from the table prepare wrote.  Per entry
    |y_k - y_exact_k| <= u [4 sum_n p_n |c_n| |O_nk| + sum_n p_n |c_n| (adds max(1, |t_nh|) + (sorb + 2) S_h sech2_nh)] + sum_n p_n ec_n |O_nk|,
    adds = 42 + n / 128 + world,   t = tanh theta,   S_h = |b_h| + sum_o |W_ho|,   sech2 = |1 - t^2|,
(visible-bias entries: u (4 + adds) sum_n p_n |c_n| + sum_n p_n ec_n), which is rbm_exact's gradient bound with f_n = p_n c_n -- the
roundings of the product p_n c_n and of conj(t) g act on p_n |c_n| |O_nk|; the 32 + n / 128 + 4 additions and the absolute error of tanh
formed as (1 - e) / (1 + e) give adds max(1, |t|), with world + 1 more for the all-reduce and its division; theta's error (sorb + 1) u S_h
goes through d tanh / d theta = sech2 -- plus the error ec_n of c_n itself carried through |O_nk|.  c_n = x.z_a + sum_h t_nh u_nh - Obar.z
with u_nh = z_b,h + sum_o z_W,ho x_no, a chain of sorb fused multiply-adds on terms of modulus <= Z_h = |z_b,h| + sum_o |z_W,ho|:
    ec_n = u [ sum_h |t_nh| (sorb + 1) Z_h                                  (the chains u_nh)
             + sum_h (8 max(1, |t_nh|) + (sorb + 2) S_h sech2_nh) Z_h       (the table's tanh: a few u absolute, and theta's error)
             + (H / 8 + 20) M_n                                             (the products and the H / 8 + 8 + 2 additions of the sum)
             + (sorb + 1) sum_o |z_a,o|                                     (the chain x.z_a)
             + (P / 256 + 12) sum_k |Obar_k| |z_k| ]                        (Obar.z: P / 256 terms per thread, a tree of 8 levels)
           + sum_k bobar_k |z_k|                                            (Obar's own error)
    M_n = sum_h |t_nh| Z_h + sum_o |z_a,o| + sum_k |Obar_k| |z_k|   (what the partial sums of c_n are bounded by),
    bobar_k = u [4 sum_n p_n |O_nk| + sum_n p_n (adds max(1, |t_nh|) + (sorb + 2) S_h sech2_nh)]   (the gradient bound with f_n = p_n),
    table:  |t - t_exact| <= u (8 max(1, |t|) + (sorb + 2) S_h sech2).
For (re, im) pairs the bound of k holds for both parts.  On every test case the bound must stay below 1e-9 max_k |y_k| (asserted by the
tests: a bound that loose would hide a wrong kernel)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import rbm_exact as R

LD, CLD, U = R.LD, R.CLD, R.U
SOLVE_FLOOR = 1e-13  # see the module docstring


@dataclass
class SrExact:
    rbm: object
    x: np.ndarray       # [n, sorb] +-1
    p: np.ndarray       # [n] longdouble
    ex: R.Exact
    O: np.ndarray       # [n, P] longdouble / clongdouble
    Obar: np.ndarray    # [P]
    world: int = 1

    @property
    def cplx(self) -> bool:
        return self.rbm.kind == "complex"

    @property
    def P(self) -> int:
        return self.O.shape[1]

    def to_z(self, v) -> np.ndarray:
        v = np.asarray(v).astype(LD).reshape(-1)
        return v[0::2] + 1j * v[1::2] if self.cplx else v

    def to_flat(self, y) -> np.ndarray:
        if not self.cplx:
            return np.asarray(y).real.astype(LD)
        out = np.empty(2 * y.shape[0], dtype=LD)
        out[0::2], out[1::2] = y.real, y.imag
        return out

    def spread(self, b) -> np.ndarray:
        """a per-k bound -> the flat layout"""
        return np.repeat(b, 2) if self.cplx else np.asarray(b)

    def c(self, v) -> np.ndarray:
        z = self.to_z(v)
        return self.O @ z - self.Obar @ z

    def matvec(self, v) -> np.ndarray:
        """S v, flat longdouble"""
        g = self.p * self.c(v)
        return self.to_flat(np.conj(self.O).T @ g if self.cplx else self.O.T @ g)

    def real_form(self) -> np.ndarray:
        """R (float64) with S = R^T R: diag(sqrt p) (O - Obar), complex entries a + i b as [[a, -b], [b, a]] on interleaved rows / columns"""
        M = (np.sqrt(self.p)[:, None] * (self.O - self.Obar[None, :]))
        if not self.cplx:
            return M.astype(np.float64)
        n, P = M.shape
        out = np.empty((2 * n, 2 * P))
        out[0::2, 0::2] = out[1::2, 1::2] = M.real
        out[1::2, 0::2] = M.imag
        out[0::2, 1::2] = -M.imag
        return out

    def S_dense(self) -> np.ndarray:
        """S as a dense longdouble matrix (small cases only)"""
        M = np.sqrt(self.p)[:, None] * (self.O - self.Obar[None, :])
        if not self.cplx:
            return M.T @ M
        Sc = np.conj(M).T @ M
        P = Sc.shape[0]
        out = np.empty((2 * P, 2 * P), dtype=LD)
        out[0::2, 0::2] = out[1::2, 1::2] = Sc.real
        out[1::2, 0::2] = Sc.imag
        out[0::2, 1::2] = -Sc.imag
        return out

    def solve(self, F, shift: float, sweeps: int = 60):
        """(d, relative size of the last correction): (S + shift) d = F"""
        F = np.asarray(F).astype(LD).reshape(-1)
        Rm = self.real_form()
        Kinv = np.linalg.inv(Rm @ Rm.T + shift * np.eye(Rm.shape[0]))
        d = np.zeros_like(F)
        last = np.inf
        for _ in range(sweeps):
            prev = last
            r = (F - (self.matvec(d) + LD(shift) * d)).astype(np.float64)
            dd = (r - Rm.T @ (Kinv @ (Rm @ r))) / shift
            d = d + dd.astype(LD)
            nd = float(np.sqrt((d * d).sum()))
            last = float(np.sqrt((dd * dd).sum())) / nd if nd > 0 else 0.0
            if last <= 1e-17 or (prev < 1e-12 and last >= 0.5 * prev):  # converged, or stagnating at the residual's own rounding
                break
        return d, last

    def residual(self, F, d, shift: float) -> np.ndarray:
        """F - (S + shift) d, flat longdouble"""
        d = np.asarray(d).astype(LD).reshape(-1)
        return np.asarray(F).astype(LD).reshape(-1) - (self.matvec(d) + LD(shift) * d)

    # ---- the a-priori bounds of the module docstring (float64, per holomorphic k unless said otherwise)
    def _pieces(self):
        n, sorb = self.x.shape
        H = self.rbm.H
        ay = np.abs(self.ex.y).astype(np.float64)
        S = R.hidden_scale(self.rbm).astype(np.float64)
        adds = 42 + n / 128 + self.world
        tanh_term = adds * np.maximum(1.0, ay) + (sorb + 2) * S[None, :] * self.ex.sech2
        return n, sorb, H, ay, S, adds, tanh_term

    def table_bound(self) -> np.ndarray:
        """[n, H]"""
        n, sorb, H, ay, S, adds, tanh_term = self._pieces()
        return U * (8 * np.maximum(1.0, ay) + (sorb + 2) * S[None, :] * self.ex.sech2)

    def _assemble(self, wgt, extra, ay, tanh_term, sorb, adds):
        """per-k bound for walker weights wgt_n (p_n |c_n| or p_n) and carried errors extra_n"""
        bh = U * (4 * (wgt[:, None] * ay).sum(0) + (wgt[:, None] * tanh_term).sum(0)) + (extra[:, None] * ay).sum(0)
        ba = np.full(sorb, U * (4 + adds) * wgt.sum() + extra.sum())
        return np.concatenate([np.repeat(bh, sorb), bh, ba])

    def obar_bound(self) -> np.ndarray:
        n, sorb, H, ay, S, adds, tanh_term = self._pieces()
        p = self.p.astype(np.float64)
        return self._assemble(p, np.zeros(n), ay, tanh_term, sorb, adds)

    def product_bound(self, v) -> np.ndarray:
        """flat [P_real]: the bound on |(S v)_k - (S v)_exact_k|"""
        n, sorb, H, ay, S, adds, tanh_term = self._pieces()
        p = self.p.astype(np.float64)
        z = self.to_z(v)
        az = np.abs(z).astype(np.float64)
        aW, ab, aa = az[:H * sorb].reshape(H, sorb), az[H * sorb:H * sorb + H], az[H * sorb + H:]
        Z = ab + aW.sum(1)
        dotabs = float((np.abs(self.Obar).astype(np.float64) * az).sum())
        M = ay @ Z + aa.sum() + dotabs
        ec = U * ((ay * ((sorb + 1) * Z)[None, :]).sum(1)
                  + ((8 * np.maximum(1.0, ay) + (sorb + 2) * S[None, :] * self.ex.sech2) * Z[None, :]).sum(1)
                  + (H / 8 + 20) * M + (sorb + 1) * aa.sum() + (self.P / 256 + 12) * dotabs) + float((self.obar_bound() * az).sum())
        pc = p * np.abs(self.c(v)).astype(np.float64)
        return self.spread(self._assemble(pc, p * ec, ay, tanh_term, sorb, adds))


def sr_exact(rbm, x: np.ndarray, prob: np.ndarray, world: int = 1) -> SrExact:
    assert rbm.kind in ("real", "complex")
    ex = R.exact_ld(rbm, x)
    n, sorb = x.shape
    xl = x.astype(LD)
    y = ex.y
    O = np.concatenate([(y[:, :, None] * xl[:, None, :]).reshape(n, -1), y, xl.astype(y.dtype)], 1)
    p = np.asarray(prob, dtype=np.float64).astype(LD)
    return SrExact(rbm, x, p, ex, O, p @ O, world)


def energy_gradient(se: SrExact, prob, eloc, e_total, powc=None) -> np.ndarray:
    """F, flat longdouble: what pynqs_rbm_grad returns (2 Re G, -2 Im G), from rbm_exact.grad_exact"""
    ge = R.grad_exact(se.rbm, se.x, prob, eloc, e_total, powc)
    G = np.concatenate([ge.GW.reshape(-1), ge.Ghb, ge.Gvb])
    if not se.cplx:
        return (2 * G).astype(LD)
    out = np.empty(2 * G.shape[0], dtype=LD)
    out[0::2], out[1::2] = 2 * G.real, -2 * G.imag
    return out


def module_rbm(module):
    """mcmc_replay.Rbm from a pynqs_amd.rbm.RealRBM / ComplexRBM (parameters moved to the host)"""
    ps = [p.detach().cpu().numpy() for p in module.parameters()]
    return R.make("complex" if ps[0].ndim == 3 else "real", *ps)


def flat_of(tensors) -> np.ndarray:
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in tensors])


# ---- seeded inputs shared by the host tests (tests/test_rbm_sr_exact.py) and the GPU tests (tests/test_gpu_rbm_sr.py) ---------------------
# (kind, sorb, electrons per spin, H, n): the case list of tests/test_gpu_rbm_grad.py, then n around the workgroup of 32
CASES = [("complex", 40, 15, 40, 1000), ("complex", 40, 15, 37, 777), ("complex", 12, 3, 5, 64), ("complex", 120, 30, 70, 300),
         ("complex", 184, 46, 33, 130), ("real", 40, 15, 80, 1000), ("real", 72, 6, 9, 65),
         ("real", 40, 15, 80, 1), ("complex", 40, 15, 37, 31), ("real", 66, 10, 7, 33)]
# (kind, sorb, electrons per spin, H, n) for the product tests alone (the longdouble dense solve of the solve tests would be too slow at these
# P): where the kernels' control flow depends on the sizes.  rbm_sr_reduce_kernel gives each of its 4 waves a slice of the ceil(n / 32)
# workgroups' partial sums and loads 16 of them per trip: n = 2049 is 65 workgroups, 17 per slice, a second trip of one; n = 4100 is 129
# workgroups, 33 per slice, three trips, and a last workgroup of 4 walkers.  The product kernel passes over 32 hidden units at a time:
# H = 32 and 64 are whole passes, H = 129 leaves one unit to a fifth (P = 5329 real, 2 x 5329 complex).
PRODUCT_SHAPES = [(kind, 12, 3, 5, n) for n in (2049, 4100) for kind in ("real", "complex")] + \
                 [(kind, 40, 15, H, 64) for H in (32, 64, 129) for kind in ("real", "complex")]
# (kind, sorb, H, n, regime of rbm_exact.regime_params): hidden units at theta = -50 ... -362
SATURATED = [("real", 40, 80, 257, "chunk-50"), ("complex", 40, 40, 255, "two-200"), ("real", 40, 40, 100, "one-338-w"),
             ("complex", 130, 9, 65, "one-338")]


def module_params(kind: str, sorb: int, H: int, seed: int = 3):
    """(W, hb, vb) as float64 host arrays, the recipe of tests/test_gpu_rbm_grad.py::_modules (complex: trailing [2])"""
    import torch

    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5)  # noqa: E731
    if kind == "complex":
        return tuple(t.numpy() for t in (0.3 * r(H, sorb, 2), 0.4 * r(H, 2), 0.2 * r(sorb, 2)))
    return tuple(t.numpy() for t in (0.3 * r(H, sorb), 0.4 * r(H), 0.2 * r(sorb)))


def case_inputs(kind: str, sorb: int, no: int, H: int, n: int, eloc_cplx=None):
    """(rbm, words uint64 [n, len], prob, eloc, e_total) of a case: walkers from bench.synth_walkers, probabilities and local energies
    as tests/test_gpu_rbm_grad.py draws them; e_total is the float64 sum the caller would pass (one walker: offset, or F = 0)."""
    import torch

    import bench as B

    W, hb, vb = module_params(kind, sorb, H)
    rbm = R.make(kind, W, hb, vb)
    words = np.ascontiguousarray(B.synth_walkers(n, sorb, no, no, 17).numpy()).view(np.uint64).reshape(n, -1)
    return (rbm, words) + weights_and_energies(n, kind == "complex" if eloc_cplx is None else eloc_cplx)


def weights_and_energies(n: int, eloc_cplx: bool):
    import torch

    g = torch.Generator().manual_seed(5)
    prob = torch.rand(n, generator=g, dtype=torch.float64)
    prob = (prob / prob.sum()).numpy()
    eloc = (torch.randn(n, generator=g, dtype=torch.float64) - 100.0).numpy()
    if eloc_cplx:
        eloc = eloc + 0.1j * torch.randn(n, generator=g, dtype=torch.float64).numpy()
    e_total = (prob * eloc).sum() if n > 1 else eloc[0] + (0.37 - 0.05j if eloc_cplx else 0.37)
    return prob, eloc, e_total


def saturated_inputs(kind: str, sorb: int, H: int, n: int, regime: str):
    rbm = R.regime_params(regime, kind, sorb, H, 0)
    words = R.rand_words(n, sorb, 17)
    if regime == "one-338-w":  # most walkers occupy the orbitals coupled to the saturated unit, the others empty some of them
        bits = R.pm1(words, sorb) > 0
        bits[: n // 2, R.forced_orbitals(sorb)] = True
        words = R.pack_bits(bits)
    return (rbm, words) + weights_and_energies(n, kind == "complex")


def probe_vectors(se: SrExact, seed: int = 9):
    """[(name, v flat float64)]: a random vector, a unit vector in each parameter block (both parts for pairs), zero"""
    g = np.random.default_rng([seed, se.P])
    C = 2 if se.cplx else 1
    H, sorb = se.rbm.H, se.x.shape[1]
    out = [("random", g.standard_normal(C * se.P))]
    for name, k in (("unit W", (H // 2) * sorb + sorb // 3), ("unit hb", H * sorb + H - 1), ("unit vb", H * sorb + H + sorb // 2)):
        for c in range(C):
            v = np.zeros(C * se.P)
            v[C * k + c] = 1.0
            out.append((f"{name}[{c}]", v))
    out.append(("zero", np.zeros(C * se.P)))
    return out
