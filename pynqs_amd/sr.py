"""Stochastic reconfiguration (the natural gradient; vmc/grad/sr.py, switched on by `sr=True` in the reference's optimiser) for the
reference's RBM amplitudes, matrix-free: (S + diag_shift I) d = F is solved by conjugate gradients on the product S v, which
pynqs_rbm_sr_matvec forms from the packed bits and a table of tanh theta (include/pynqs_amd.h, "stochastic reconfiguration"): nothing
of size n x P or P x P exists, where the reference materialises O[n, P], builds the dense S and calls torch.linalg.inv on one rank.

    S = Re(<O* O> - <O*><O>) on the real parameter vector (weights, hidden_bias, visible_bias as the module stores them; (re, im) pairs
    of a ComplexRBM: the real form [[A, -B], [B, A]] of the Hermitian matrix of the holomorphic parameters),
    F = the energy gradient exactly as FusedRbmGrad returns it,        theta <- theta - lr d   with torch.optim.SGD(lr).

Under torch.distributed every rank holds its shard of the walkers (probabilities pre-scaled by the world size, as everywhere in this
package): one all-reduce of Obar per solve and one of the product per iteration; the decision to stop is rank 0's, broadcast.

FusedRbmSR serves RealRBM / ComplexRBM, FusedJastrowRbmSR the JastrowRBM (the parameter vector gains the block jastrow [sorb, sorb] and
the product the term x^T Z x; pynqs_jrbm_sr_*).  Both are the private _FusedSR (buffers, conjugate gradients, all-reduces, status
broadcast) with their own gradient object and their own two native calls."""
from __future__ import annotations

import warnings

import torch
from torch import Tensor, nn

from .distributed import get_world_size
from .grad import FusedJastrowRbmGrad, FusedRbmGrad

# slots of the solver's device scalars (include/pynqs_amd.h: PYNQS_SR_*)
_RHO, _RHS2, _DONE, _ITER, _TRUE2, _PAP, _CONVERGED, _BREAKDOWN, _NSC = range(9)
_INIT, _STEP, _RESIDUAL = 0, 1, 2


class _FusedSR:
    """What FusedRbmSR and FusedJastrowRbmSR share: the flat buffers, the conjugate-gradient driver on pynqs_rbm_sr_cg_step, the
    all-reduces and the status broadcast.  A subclass sets `_who`, builds its
    gradient object, calls _setup() and provides _workspace_bytes(n), _native_prepare(n) and _native_matvec(v, y)."""

    _who = "_FusedSR"

    def _setup(self, grad, sorb: int, diag_shift: float, tol: float, max_iter: int, check_every: int) -> None:
        if not (diag_shift >= 0.0) or not (tol > 0.0) or max_iter < 1 or check_every < 1:
            raise ValueError(f"{self._who}: diag_shift >= 0, tol > 0, max_iter >= 1, check_every >= 1")
        g = self.grad = grad
        self.N, self.module, self.sorb, self.H = g.N, g.module, sorb, g.H
        self.diag_shift, self.tol, self.max_iter, self.check_every = float(diag_shift), float(tol), int(max_iter), int(check_every)
        dev = g.flat.device
        self.np = g.flat.numel() - 1  # P_real
        new = lambda: torch.zeros(self.np, dtype=torch.float64, device=dev)  # noqa: E731
        self.obar, self.d, self._r, self._p, self._y, self._rhs = new(), new(), new(), new(), new(), new()
        self._sc = torch.zeros(_NSC, dtype=torch.float64, device=dev)
        self.views, self._fviews, o = [], [], 0
        for shape in g.shapes:
            k = int(torch.Size(shape).numel())
            self.views.append(self.d[o:o + k].view(shape))
            self._fviews.append(self._rhs[o:o + k].view(shape))
            o += k
        self.work = None
        self._onv = self._prob = None
        self.iterations, self.converged, self.residual = 0, False, float("nan")
        self.energy_grad = None
        self.events = None  # set to a list to collect (before, after) events of every all-reduce of a product

    @property
    def params(self):
        return self.grad.params

    def _stream(self):
        return torch.cuda.current_stream(self.d.device).cuda_stream

    def prepare(self, onv: Tensor, state_prob: Tensor) -> None:
        """tanh theta of the walkers -> the table, Obar (all-reduced) -> self.obar; the walkers and probabilities are kept for matvec."""
        dev = self.d.device
        n = onv.size(0)
        if onv.dtype != torch.uint8 or onv.dim() != 2 or onv.size(1) != 8 * ((self.sorb - 1) // 64 + 1) or onv.device != dev:
            raise ValueError(f"{self._who}: walkers as packed onv uint8[n, 8 len] on the parameters' device")
        prob = (state_prob.real if state_prob.is_complex() else state_prob).to(device=dev, dtype=torch.float64).contiguous()
        if prob.numel() != n:
            raise ValueError(f"{self._who}: one probability per walker")
        need = self._workspace_bytes(n)
        if need < 0:
            raise ValueError(f"{self._who}: bad sizes")
        if self.work is None or self.work.numel() * 8 < need:
            self.work = torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev)
        self._onv, self._prob = onv.contiguous(), prob
        self._native_prepare(n)
        self._all_reduce(self.obar, divide=True)

    def _all_reduce(self, t: Tensor, divide: bool) -> None:
        ws = get_world_size()
        ev = None
        if self.events is not None:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
        if ws > 1:
            import torch.distributed as dist

            dist.all_reduce(t, dist.ReduceOp.SUM)
            if divide:
                t.div_(ws)
        if ev is not None:
            ev[1].record()
            self.events.append(ev)

    def _product(self, v: Tensor, y: Tensor, divide: bool) -> None:
        """y <- the all-reduced SUM of the ranks' products (divided by the world size if `divide`)"""
        if self._onv is None:
            raise RuntimeError(f"{self._who}: prepare(onv, state_prob) first")
        self._native_matvec(v, y)
        self._all_reduce(y, divide)

    def _flat_arg(self, v: Tensor) -> Tensor:
        if v.numel() != self.np or v.device != self.d.device:
            raise ValueError(f"{self._who}: a flat vector of {self.np} doubles on the parameters' device")
        return v.detach().to(torch.float64).reshape(-1).contiguous()

    def matvec(self, v_flat: Tensor) -> Tensor:
        """S v (no shift), all-reduced over the ranks, for the walkers of the last prepare()"""
        y = torch.empty(self.np, dtype=torch.float64, device=self.d.device)
        self._product(self._flat_arg(v_flat), y, True)
        return y

    def _cg(self, mode: int) -> None:
        N = self.N
        N.check(N.lib().pynqs_rbm_sr_cg_step(mode, self.np, self._y.data_ptr(), self._rhs.data_ptr(), self.d.data_ptr(), self._r.data_ptr(),
                                             self._p.data_ptr(), self._sc.data_ptr(), 1.0 / get_world_size(), self.diag_shift, self.tol,
                                             self._stream()), "pynqs_rbm_sr_cg_step")

    def _status(self):
        """the solver's scalars as rank 0 sees them: every rank takes the same decisions from them"""
        sc = self._sc
        if get_world_size() > 1:
            import torch.distributed as dist

            sc = sc.clone()
            dist.broadcast(sc, 0)
        return sc.cpu().tolist()

    def solve(self, rhs_flat: Tensor) -> Tensor:
        """d with (S + diag_shift) d = rhs by conjugate gradients from zero; returns self.d (overwritten by the next solve)"""
        rhs = self._flat_arg(rhs_flat)
        if rhs.data_ptr() != self._rhs.data_ptr():
            self._rhs.copy_(rhs)
        self._cg(_INIT)
        st = self._status()
        used = 0
        while not st[_CONVERGED]:
            left = self.max_iter - used
            if st[_DONE]:
                # the recurrence says done (or max_iter is spent): the true residual decides; CG restarts from it when it disagrees
                self._product(self.d, self._y, False)
                self._cg(_RESIDUAL)
                st = self._status()
                if st[_CONVERGED] or left <= 0 or st[_BREAKDOWN]:
                    break
                continue
            if left <= 0:
                self._sc[_DONE] = 1.0
                st[_DONE] = 1.0
                continue
            for _ in range(min(self.check_every, left)):
                self._product(self._p, self._y, False)
                self._cg(_STEP)
            st = self._status()
            used = int(st[_ITER])
        self.iterations = int(st[_ITER])
        self.converged = bool(st[_CONVERGED])
        self.residual = 0.0 if st[_RHS2] == 0 else (st[_TRUE2] / st[_RHS2]) ** 0.5  # (not a number when rhs holds one: not 0)
        if not self.converged:
            warnings.warn(f"{self._who}: conjugate gradients stopped after {self.iterations} iterations at a relative residual of "
                          f"{self.residual:.3e} (tol {self.tol:.1e}, max_iter {self.max_iter}); the last iterate is used", RuntimeWarning, stacklevel=2)
        return self.d

    def __call__(self, onv: Tensor, state_prob: Tensor, eloc: Tensor, e_total, extra_psi_pow=1.0) -> Tensor:
        loss = self.grad(onv, state_prob, eloc, e_total, extra_psi_pow)  # F (all-reduced) in grad.flat, p.grad = its views
        self._rhs.copy_(self.grad.flat[:self.np])
        self.energy_grad = [v.clone() for v in self._fviews]
        self.prepare(onv, state_prob)
        self.solve(self._rhs)
        for p, v in zip(self.params, self.views):
            p.grad = v
        return loss


class FusedRbmSR(_FusedSR):
    """SR direction for pynqs_amd.rbm.RealRBM (rbm_type "real") and ComplexRBM with float64 parameters on the GPU (what FusedRbmGrad
    accepts; anything else: ValueError).  Calling convention of FusedRbmGrad:

        loss = sr(onv, state_prob, eloc, e_total, extra_psi_pow=1.0)

    After the call every p.grad is a view of the direction d (so torch.optim.SGD(lr) performs theta <- theta - lr d), `energy_grad` holds
    F per parameter, `iterations` the CG iterations, `converged` whether the TRUE residual met `tol`, `residual` the true relative
    residual |F - (S + diag_shift) d| / |F| from one product after the loop (0 when F = 0).  CG starts from zero; when the recurrence's
    residual meets the tolerance the true residual is formed, and if that does not meet it the iteration goes on from the current
    iterate with the true residual, inside the same max_iter.  When max_iter is reached the last iterate is installed, `converged` is
    False and a warning is issued.  Every sum runs in a fixed order: two calls give the same bits.
    prepare(onv, state_prob), matvec(v_flat) -> S v (all-reduced) and solve(rhs_flat) -> d_flat serve users with their own right-hand
    side; flat vectors have the layout weights, hidden_bias, visible_bias (each as stored, (re, im) interleaved)."""

    _who = "FusedRbmSR"

    def __init__(self, nqs: nn.Module, sorb: int, diag_shift: float = 0.02, tol: float = 1e-6, max_iter: int = 1000, check_every: int = 8) -> None:
        g = FusedRbmGrad(nqs, sorb)  # (refuses other modules)
        self.flavour = g.flavour
        self._setup(g, sorb, diag_shift, tol, max_iter, check_every)

    def _workspace_bytes(self, n: int) -> int:
        return self.N.lib().pynqs_rbm_sr_workspace(n, self.sorb, self.H, self.flavour)

    def _native_prepare(self, n: int) -> None:
        N = self.N
        W, hb, _ = (p.detach().contiguous() for p in self.params)
        N.check(N.lib().pynqs_rbm_sr_prepare(self._onv.data_ptr(), n, self.sorb, W.data_ptr(), hb.data_ptr(), self.H, self.flavour,
                                             self._prob.data_ptr(), self.work.data_ptr(), self.obar.data_ptr(), self._stream()), "pynqs_rbm_sr_prepare")

    def _native_matvec(self, v: Tensor, y: Tensor) -> None:
        N = self.N
        N.check(N.lib().pynqs_rbm_sr_matvec(self._onv.data_ptr(), self._onv.size(0), self.sorb, self.H, self.flavour, self._prob.data_ptr(),
                                            self.work.data_ptr(), self.obar.data_ptr(), v.data_ptr(), y.data_ptr(), self._stream()),
                "pynqs_rbm_sr_matvec")

    def tanh_table(self) -> Tensor:
        """tanh theta of the prepared walkers, [n, H] (complex128 for a ComplexRBM): a copy of the kernels' table, for tests"""
        n, H = self._onv.size(0), self.H
        if self.flavour == self.N.RBM_COMPLEX:
            return torch.view_as_complex(self.work[:2 * n * H].view(H, n, 2)).t().contiguous()
        return self.work[:n * H].view(H, n).t().contiguous()


class FusedJastrowRbmSR(_FusedSR):
    """SR direction for pynqs_amd.rbm.JastrowRBM, psi(x) = exp(a.x + x^T M x) prod_h 2cosh(theta_h), with float64 parameters on the GPU
    (what FusedJastrowRbmGrad accepts; anything else, and a complex local energy: ValueError).  Calling convention, attributes and
    methods of FusedRbmSR; the flat layout is weights, hidden_bias, visible_bias, jastrow [sorb, sorb], P = H sorb + H + sorb + sorb^2:

        O_n = (tanh theta_nh x_no, tanh theta_nh, x_no, x_ni x_nj),
        c_n = x_n.z_a + sum_h tanh theta_nh (z_b,h + sum_o z_W,ho x_no) + x_n^T Z x_n - Obar.z,      (S v)_k = sum_n p_n O_nk c_n,

    Z the jastrow block of v (pynqs_jrbm_sr_matvec).  S does not depend on M; F is what FusedJastrowRbmGrad returns.  Three facts:
      - S is singular on the jastrow block by construction.  O_ii = 1, so row and column ii of S vanish and d_ii = F_ii / diag_shift
        (F_ii = 2 sum_n f_n: rounding-level when e_total is the weighted mean of eloc); O_ij = O_ji; and with fixed particle numbers
        sum_j x_i x_j is proportional to x_i.  diag_shift regularises all of this and conjugate gradients from zero stay in the range
        of S; diag_shift = 0 is accepted, as by FusedRbmSR, and then relies on that alone.
      - The jastrow block is bit-symmetric: the product forms one sum for i <= j and writes it to (i, j) and (j, i), F_M from
        pynqs_jastrow_grad has the property too, and the vector updates of conjugate gradients act entry by entry: after a call
        jastrow.grad[i, j] == jastrow.grad[j, i] bit for bit.
      - Only the symmetric part of Z reaches c_n (x^T Z x = tr Z + sum_{i<j} (Z_ij + Z_ji) x_i x_j, the form the kernel evaluates): an
        antisymmetric Z with zero RBM blocks is in the null space of S."""

    _who = "FusedJastrowRbmSR"

    def __init__(self, nqs: nn.Module, sorb: int, diag_shift: float = 0.02, tol: float = 1e-6, max_iter: int = 1000, check_every: int = 8) -> None:
        self._setup(FusedJastrowRbmGrad(nqs, sorb), sorb, diag_shift, tol, max_iter, check_every)  # (refuses other modules)

    def _workspace_bytes(self, n: int) -> int:
        return self.N.lib().pynqs_jrbm_sr_workspace(n, self.sorb, self.H)

    def _native_prepare(self, n: int) -> None:
        N = self.N
        W, hb, _, _ = (p.detach().contiguous() for p in self.params)
        N.check(N.lib().pynqs_jrbm_sr_prepare(self._onv.data_ptr(), n, self.sorb, W.data_ptr(), hb.data_ptr(), self.H, self._prob.data_ptr(),
                                              self.work.data_ptr(), self.obar.data_ptr(), self._stream()), "pynqs_jrbm_sr_prepare")

    def _native_matvec(self, v: Tensor, y: Tensor) -> None:
        N = self.N
        N.check(N.lib().pynqs_jrbm_sr_matvec(self._onv.data_ptr(), self._onv.size(0), self.sorb, self.H, self._prob.data_ptr(),
                                             self.work.data_ptr(), self.obar.data_ptr(), v.data_ptr(), y.data_ptr(), self._stream()),
                "pynqs_jrbm_sr_matvec")

    def tanh_table(self) -> Tensor:
        """tanh theta of the prepared walkers, [n, H]: a copy of the kernels' table, for tests"""
        n, H = self._onv.size(0), self.H
        return self.work[:n * H].view(H, n).t().contiguous()
