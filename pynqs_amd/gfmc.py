"""Fixed-node Green's-function Monte-Carlo step (mirror of PyNQS' gfmc/walker.py:167-279).

green_kernel(): for every walker x the row G(x' <- x) = psi(x') <x'|Lambda - H_eff|x> / psi(x) over its S+D
list, the fixed-node effective Hamiltonian with the sign-flip potential on the diagonal, and the local energy;
sample_update(): one multinomial move per walker by inverse-CDF (row cumsum + searchsorted).  The law of the move (never a column
without weight, a row of sum zero stays where it is; include/pynqs_amd.h) is held in exact arithmetic by tests/gfmc_exact.py.
Enumeration and matrix elements come from the fused HIP kernel; psi from pynqs_amd.energy.Func.
"""
from __future__ import annotations

from functools import partial
from typing import Callable, Optional, Tuple

import torch
from torch import Tensor

from . import C_extension as CX
from . import _native as N
from .C_extension import get_comb_hij_fused
from .distributed import all_gather_varlen, get_rank, get_world_size
from .energy import Func, _jastrow_rbm_params, _rbm_lds_ok, _real_rbm_params
from .public_function import WavefunctionLUT, get_Num_SinglesDoubles

# trial function = RBM with real parameters ("real" / "tanh"), or a JastrowRBM: the whole row in one kernel (pynqs_green_rbm / pynqs_green_jrbm)
FUSED_GREEN = True


class CombRows:
    """What green_kernel returns in place of comb_x when the row came from the fused kernel: the S+D list of every walker is
    NOT materialised; sample_update turns the chosen column into x' by its rank (pynqs_gfmc_sample_rank).  materialize() gives
    the [n, ncomb, 8 * len] tensor of the reference for callers that want it."""

    def __init__(self, x: Tensor, sorb: int, nele: int, noa: int, nob: int) -> None:
        self.x, self.sorb, self.nele, self.noa, self.nob = x, sorb, nele, noa, nob
        self.shape = (x.size(0), get_Num_SinglesDoubles(sorb, noa, nob) + 1, x.size(1))

    def materialize(self) -> Tensor:
        return CX.get_comb_tensor(self.x, self.sorb, self.nele, self.noa, self.nob, False)[0]


def green_kernel(x: Tensor, Lambda: float, h1e: Tensor, h2e: Tensor, ansatz, ansatz_batch: Callable[..., Tensor], sorb: int,
                 nele: int, noa: int, nob: int, dtype: torch.dtype = torch.double, WF_LUT: Optional[WavefunctionLUT] = None,
                 use_unique: bool = True) -> Tuple[Tensor, Tensor, Tensor, bool, Tensor]:
    """gfmc/walker.py:167-235.  Returns (eloc[n], green_kernel[n, ncomb], comb_x[n, ncomb, 8*len], stop_flag,
    mask of walkers whose diagonal kernel was negative and has been clamped to 0)."""
    with torch.no_grad():
        assert x.dim() == 2
        batch = x.shape[0]
        device = h1e.device
        fused = (FUSED_GREEN and WF_LUT is None and dtype == torch.double and x.is_cuda and sorb % 2 == 0
                 and h1e.dtype in (torch.float64, torch.float32))
        prm = _real_rbm_params(ansatz) if fused else None
        jprm = _jastrow_rbm_params(ansatz) if fused and prm is None else None
        if prm is not None and prm[3] in ("real", "tanh") and _rbm_lds_ok(sorb, nele, noa, nob, prm[0].size(0)):
            # enumeration, matrix elements, amplitude ratios, fixed-node construction and E_loc in one kernel
            plan = CX.plan_for(*CX.integrals_f64(h1e, h2e), sorb, x.device)
            table = CX.RBMTable(*prm[:3])
            xc = x.contiguous()
            rows = CombRows(xc, sorb, nele, noa, nob)
            eloc = torch.empty(batch, dtype=torch.float64, device=x.device)
            gk = torch.empty((batch, rows.shape[1]), dtype=torch.float64, device=x.device)
            neg = torch.empty(batch, dtype=torch.uint8, device=x.device)
            if batch:
                N.check(N.lib().pynqs_green_rbm(xc.data_ptr(), batch, sorb, nele, noa, nob, plan.data_ptr(), table.data_ptr(), table.nhidden,
                                                CX.RBM_FLAVOURS[prm[3]], float(Lambda), eloc.data_ptr(), None, gk.data_ptr(), neg.data_ptr(),
                                                torch.cuda.current_stream(x.device).cuda_stream), "pynqs_green_rbm")
            return eloc, gk, rows, False, neg.bool()
        if jprm is not None and CX.eloc_jrbm_supported(sorb, nele, noa, nob, jprm[0].size(0)):
            # the same with the two-body Jastrow factor on the real RBM (pynqs_green_jrbm)
            xc = x.contiguous()
            eloc, gk, neg, _ = CX.green_jrbm(xc, *CX.integrals_f64(h1e, h2e), CX.RBMTable(*jprm[:3]), CX.JastrowTable(jprm[3]), sorb, nele, noa, nob,
                                             float(Lambda))
            return eloc, gk, CombRows(xc, sorb, nele, noa, nob), False, neg.bool()
        f = partial(ansatz_batch, func=ansatz)
        comb_x, comb_hij = get_comb_hij_fused(x, h1e, h2e, sorb, nele, noa, nob)
        bra_len = comb_x.shape[2]
        gamma = torch.where(comb_hij >= 0, 0, torch.pi)  # H = |H| exp(i gamma)
        psi_x1 = Func(f, comb_x.reshape(-1, bra_len), WF_LUT, use_unique).reshape(batch, -1).real
        phase = torch.angle(psi_x1)
        alpha = phase - phase[..., 0].unsqueeze(-1)
        mask = torch.cos(alpha + gamma) < 0.0  # sign-preserving moves
        mask[..., 0] = True
        ratio = psi_x1 / psi_x1[..., 0].unsqueeze(-1)
        hij_eff = torch.where(mask, comb_hij, 0.0).to(psi_x1.dtype)
        v_sf = torch.sum(torch.where(~mask, comb_hij, 0.0) * ratio, -1)  # sign-flip potential
        hij_eff[..., 0] += v_sf
        eloc = (ratio * hij_eff).sum(-1)
        K = -hij_eff
        K[..., 0] += Lambda
        gk = psi_x1.conj() * K.conj() / psi_x1[..., 0].unsqueeze(-1).conj()
        neg = gk[..., 0] < 0
        gk[..., 0][neg] = 0.0
        assert torch.all(gk[..., 1:] >= 0)
        return eloc, gk, comb_x, False, neg


FUSED_SAMPLE = True  # one kernel for sum + cumsum + searchsorted + gather (pynqs_gfmc_sample) when the row is float64 on the GPU


def sample_update(x: Tensor, weight: Tensor, comb_x: Tensor, green_kernel: Tensor, rand_num: Optional[Tensor] = None):
    """gfmc/walker.py:260-279: x_new ~ G(. <- x) / beta, weight *= beta."""
    if isinstance(comb_x, CombRows):
        if not (green_kernel.is_cuda and green_kernel.dtype == torch.float64 and green_kernel.size(0) > 0):
            comb_x = comb_x.materialize()
        else:
            n = green_kernel.size(0)
            dev = green_kernel.device
            if rand_num is None:
                rand_num = torch.rand((n, 1), dtype=torch.float64, device=dev)
            gk, rn = green_kernel.contiguous(), rand_num.to(torch.float64).contiguous()
            index = torch.empty(n, dtype=torch.int64, device=dev)
            beta = torch.empty((n, 1), dtype=torch.float64, device=dev)
            x_new = torch.empty_like(comb_x.x)
            N.check(N.lib().pynqs_gfmc_sample_rank(gk.data_ptr(), n, rn.data_ptr(), comb_x.x.data_ptr(), comb_x.sorb, comb_x.nele, comb_x.noa,
                                                   comb_x.nob, index.data_ptr(), beta.data_ptr(), x_new.data_ptr(),
                                                   torch.cuda.current_stream(dev).cuda_stream), "pynqs_gfmc_sample_rank")
            return x_new, weight * beta.squeeze(), beta, int((index != 0).sum().item())
    if (FUSED_SAMPLE and green_kernel.is_cuda and green_kernel.dtype == torch.float64 and green_kernel.dim() == 2
            and comb_x.is_cuda and comb_x.dtype == torch.uint8 and green_kernel.size(0) > 0):
        n, m = green_kernel.shape
        L = comb_x.size(-1) // 8
        dev = green_kernel.device
        if rand_num is None:
            rand_num = torch.rand((n, 1), dtype=torch.float64, device=dev)
        gk, cx, rn = green_kernel.contiguous(), comb_x.contiguous(), rand_num.to(torch.float64).contiguous()
        index = torch.empty(n, dtype=torch.int64, device=dev)
        beta = torch.empty((n, 1), dtype=torch.float64, device=dev)
        x_new = torch.empty((n, 8 * L), dtype=torch.uint8, device=dev)
        N.check(N.lib().pynqs_gfmc_sample(gk.data_ptr(), n, m, rn.data_ptr(), cx.data_ptr(), 64 * L, index.data_ptr(), beta.data_ptr(),
                                          x_new.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "pynqs_gfmc_sample")
        return x_new, weight * beta.squeeze(), beta, int((index != 0).sum().item())
    beta = green_kernel.sum(-1, keepdim=True)
    cum_prob = green_kernel.cumsum(-1) / beta
    if rand_num is None:
        rand_num = torch.rand_like(beta)
    index = torch.searchsorted(cum_prob, rand_num, right=False).reshape(-1)
    # cumsum's last entry and sum's total round differently: a uniform next to 1 can lie beyond the last quotient, and a row of sum zero is
    # 0 / 0.  As the kernel does: the last column with weight, and index 0 for the empty row (searchsorted's own answer is out of range)
    m = green_kernel.size(-1)
    empty = ~(beta.reshape(-1) > 0)
    over = (index >= m) & ~empty
    if bool(over.any()):
        last = m - 1 - (green_kernel.flip(-1) > 0).to(torch.uint8).argmax(-1).reshape(-1)
        index = torch.where(over, last, index)
    index = torch.where(empty, torch.zeros_like(index), index)
    x_new = comb_x[torch.arange(beta.size(0), device=comb_x.device), index]
    weight_new = weight * beta.squeeze()
    accept_nums = index.nonzero().size(0)
    return x_new, weight_new, beta, accept_nums


def branching(x: Tensor, weight: Tensor, xi: Optional[Tensor] = None) -> Tensor:
    """gfmc/walker.py:340-408: stochastic reconfiguration (comb resampling) of the walkers of ALL ranks by weight.
    Output slot k (global numbering, this rank owns `x.size(0)` consecutive ones) takes the walker whose interval of
    the global cumulative weight contains (k + xi_k) / N_total.  Same arithmetic as the reference (per-rank cumsum +
    offset of the previous ranks, clamped at 1); instead of gathering everything on rank 0 and scattering the
    result, every rank all-gathers the cumulative weights and the walkers (N_total * (8 + 8 * len) bytes) and picks
    its own slots -- one exchange step, no rank-0 serialisation.  xi: uniforms for this rank's slots (default torch.rand)."""
    ws, rank = get_world_size(), get_rank()
    dev = x.device
    batch = x.size(0)
    w_sums = all_gather_varlen(weight.sum(0, keepdim=True)).cumsum(0)  # cumulative weight of ranks 0..r
    sizes = all_gather_varlen(torch.tensor([batch], dtype=torch.int64, device=dev)).cumsum(0)
    # walkers on the ranks in front.  (The reference writes x_size_all[rank] - x_size_all[0], walker.py:369, which is the
    # same number only when all shards have the same size; with shards that differ by one it repeats / drops a slot.)
    offset = sizes[rank] - batch
    if xi is None:
        xi = torch.rand(batch, device=dev)
    rand_prob = (torch.arange(batch, device=dev) + offset + xi) / sizes[-1]
    pre = 0 if rank == 0 else w_sums[rank - 1]
    cum_prob = (weight / w_sums[-1]).cumsum(0) + pre / w_sums[-1]
    cum_prob.clamp_(max=1.0)
    x_all = all_gather_varlen(x)
    cum_all = all_gather_varlen(cum_prob)
    index = torch.searchsorted(cum_all, rand_prob.to(cum_all.dtype), right=False).reshape(-1).clamp_(max=x_all.size(0) - 1)
    return x_all[index]
