"""One- and two-body reduced density matrices of a sampled state, in the integrals' own packed layouts (include/pynqs_amd.h, "reduced
density matrices"):

    rdm1[q sorb + p] = dE / dh1e[q sorb + p],     rdm2[t] = dE / dh2e[t],     E = sum_x w_x Re E_loc(x),

so that dot(h1e, rdm1) + dot(h2e, rdm2) is the SIMPLE energy estimate for ANY integrals.  Two routes, chosen as energy.py chooses
FUSED_RBM: a RealRBM (rbm_type "real", float64 parameters on the GPU) within pynqs_rdm_rbm_supported takes the fused kernel
(pynqs_rdm_rbm: nothing of size n x ncomb exists, bit-reproducible), a JastrowRBM (float64 parameters on the GPU, jastrow [sorb, sorb])
within pynqs_rdm_jrbm_supported the same kernel in its Jastrow flavour (pynqs_rdm_jrbm); everything else takes the generic route: chunks of walkers,
get_comb_tensor, the module's own forward on every x', psi(x') / psi(x), pynqs_rdm_scatter (f64 atomics: not bit-reproducible).
Under torch.distributed every rank passes its shard of the walkers with probabilities pre-scaled by the world size, as everywhere in
this package; both packed arrays are all-reduced in one flat buffer and divided by the world size."""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch
from torch import Tensor

from . import C_extension as CX
from . import _native as N
from .distributed import get_world_size

FUSED_RBM = True  # False: always the generic route (the tests cross-check the two)


def _sizes(sorb: int):
    pair = sorb * (sorb - 1) // 2
    return sorb * sorb, pair * (pair + 1) // 2


class RDM:
    """rdm1 (float64 [sorb^2]) and rdm2 (float64 [pair (pair + 1) / 2]), packed as h1e / h2e are, on the device they were computed on."""

    def __init__(self, rdm1: Tensor, rdm2: Tensor, sorb: int, nele: int, noa: int, nob: int, fused: bool = False) -> None:
        n1, n2 = _sizes(sorb)
        if rdm1.numel() != n1 or rdm2.numel() != n2 or rdm1.dtype != torch.float64 or rdm2.dtype != torch.float64:
            raise ValueError(f"RDM: rdm1 / rdm2 must be float64 of {n1} / {n2} elements for sorb = {sorb}")
        self.rdm1, self.rdm2 = rdm1.reshape(-1), rdm2.reshape(-1)
        self.sorb, self.nele, self.noa, self.nob, self.fused = sorb, nele, noa, nob, fused

    def energy(self, h1e: Tensor, h2e: Tensor) -> Tensor:
        """dot(h1e, rdm1) + dot(h2e, rdm2): the energy estimate of the walkers the matrices were formed from, for these integrals"""
        if h1e.numel() != self.rdm1.numel() or h2e.numel() != self.rdm2.numel():
            raise ValueError("RDM.energy: packed integrals of another sorb")
        d = self.rdm1.device
        return torch.dot(h1e.reshape(-1).to(d, torch.float64), self.rdm1) + torch.dot(h2e.reshape(-1).to(d, torch.float64), self.rdm2)

    def dense(self):
        """(gamma [s, s], Gamma [s, s, s, s]) as numpy arrays: gamma[p, q] = <a+_p a_q> (symmetrised) and the antisymmetric
        Gamma[p, q, r, s] = <a+_p a+_q a_s a_r> in the layout decompress_h1e_h2e defines for the integrals, so that
        E = sum h[p, q] gamma[p, q] + 1/4 sum <pq||rs> Gamma[p, q, r, s].  (A packed off-diagonal slot holds the Hermitian sum of
        (pq, rs) and (rs, pq): each of the two gets half of it.)"""
        s = self.sorb
        r1 = self.rdm1.detach().cpu().numpy()
        r2 = self.rdm2.detach().cpu().numpy().copy()
        pair = s * (s - 1) // 2
        diag = np.arange(pair) * (np.arange(pair) + 1) // 2 + np.arange(pair)
        keep = r2[diag].copy()
        r2 *= 0.5
        r2[diag] = keep
        g1, g2 = CX.decompress_h1e_h2e(r1, r2, s)
        return 0.5 * (g1 + g1.T), g2

    def spin_free(self):
        """(D [K, K], d [K, K, K, K]) over the K = sorb / 2 spatial orbitals: D_pq = sum_sigma <p+_sigma q_sigma>,
        d_pqrs = sum_{sigma tau} <p+_sigma r+_tau s_tau q_sigma>, so that E = sum h_pq D_pq + 1/2 sum (pq|rs) d_pqrs."""
        g1, g2 = self.dense()
        K = self.sorb // 2
        D = g1[0::2, 0::2] + g1[1::2, 1::2]
        d = np.zeros((K,) * 4)
        for a in (0, 1):
            for b in (0, 1):
                # <p+_a r+_b s_b q_a> = Gamma[p a, r b, q a, s b]
                d += g2[a::2, b::2, a::2, b::2].transpose(0, 2, 1, 3)
        return D, d

    def natural_occupations(self) -> np.ndarray:
        """eigenvalues of the symmetrised spin-free D, descending"""
        D, _ = self._spatial_one_body()
        return np.linalg.eigvalsh(D)[::-1].copy()

    def _spatial_one_body(self):
        g1 = self.rdm1.detach().cpu().numpy().reshape(self.sorb, self.sorb)
        g1 = 0.5 * (g1 + g1.T)
        return g1[0::2, 0::2] + g1[1::2, 1::2], g1[0::2, 0::2] - g1[1::2, 1::2]

    def spin_density(self) -> np.ndarray:
        """<n_p alpha> - <n_p beta> per spatial orbital"""
        return np.diag(self._spatial_one_body()[1]).copy()


def _check(x: Tensor, state_prob: Tensor, sorb: int, nele: int, noa: int, nob: int) -> Tensor:
    L = (sorb - 1) // 64 + 1
    if sorb < 2 or sorb % 2 or sorb > CX.MAX_SORB or noa < 0 or nob < 0 or nele != noa + nob or max(noa, nob) > sorb // 2:
        raise ValueError("reduced_density_matrices: an even sorb, nele = noa + nob, noa, nob <= sorb / 2")
    if x.dtype != torch.uint8 or x.dim() != 2 or x.size(1) != 8 * L or not x.is_cuda:
        raise ValueError("reduced_density_matrices: walkers as packed onv uint8[n, 8 len] on the GPU")
    if state_prob.numel() != x.size(0):
        raise ValueError("reduced_density_matrices: one probability per walker")
    prob = (state_prob.real if state_prob.is_complex() else state_prob).to(device=x.device, dtype=torch.float64).reshape(-1).contiguous()
    if x.size(0):
        occ = CX.onv_to_tensor(x.contiguous(), sorb) > 0
        tail = x.contiguous().view(torch.int64).view(-1, L)[:, -1] >> (sorb - 64 * (L - 1)) if sorb % 64 else None
        if bool((occ[:, 0::2].sum(1) != noa).any()) or bool((occ[:, 1::2].sum(1) != nob).any()) or (tail is not None and bool((tail != 0).any())):
            raise ValueError("reduced_density_matrices: every walker must have noa alpha and nob beta electrons and no bit at or above sorb")
    return prob


def _fused_params(ansatz, sorb: int, nele: int, noa: int, nob: int):
    """(W, hb, vb, M or None) if the fused kernel serves this ansatz (M: the Jastrow matrix of a JastrowRBM), else None"""
    from .rbm import JastrowRBM, RealRBM

    m = getattr(ansatz, "module", ansatz)
    jastrow = isinstance(m, JastrowRBM)
    if not jastrow and (not isinstance(m, RealRBM) or m.rbm_type != "real"):
        return None
    W, hb, vb = m.weights, m.hidden_bias, m.visible_bias
    if W.dtype != torch.float64 or hb.dtype != torch.float64 or vb.dtype != torch.float64 or not W.is_cuda or W.dim() != 2 or W.size(1) != sorb:
        return None
    if jastrow:
        M = m.jastrow
        if M.dtype != torch.float64 or M.device != W.device or tuple(M.shape) != (sorb, sorb):
            return None
        if not N.lib().pynqs_rdm_jrbm_supported(sorb, nele, noa, nob, int(W.size(0))):
            return None
        return W.detach(), hb.detach().reshape(-1), vb.detach().reshape(-1), M.detach()
    if not N.lib().pynqs_rdm_rbm_supported(sorb, nele, noa, nob, int(W.size(0))):
        return None
    return W.detach(), hb.detach().reshape(-1), vb.detach().reshape(-1), None


def _rdm_fused(x: Tensor, prob: Tensor, params, sorb: int, nele: int, noa: int, nob: int, out: Tensor) -> None:
    W, hb, vb, M = params
    dev = x.device
    if W.device != dev:
        raise ValueError("reduced_density_matrices: walkers and parameters on different devices")
    table = CX.RBMTable(W, hb, vb)
    jtable = CX.JastrowTable(M) if M is not None else None
    n, H = x.size(0), int(W.size(0))
    need = (N.lib().pynqs_rdm_rbm_workspace if M is None else N.lib().pynqs_rdm_jrbm_workspace)(n, sorb, H)
    if need < 0:
        raise ValueError("reduced_density_matrices: bad sizes")
    work = torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev)
    n1, _ = _sizes(sorb)
    tail = (H, work.data_ptr(), out.data_ptr(), out[n1:].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if M is None:
        N.check(N.lib().pynqs_rdm_rbm(x.data_ptr(), n, sorb, nele, noa, nob, prob.data_ptr(), table.data_ptr(), *tail), "pynqs_rdm_rbm")
    else:
        N.check(N.lib().pynqs_rdm_jrbm(x.data_ptr(), n, sorb, nele, noa, nob, prob.data_ptr(), table.data_ptr(), jtable.data_ptr(), *tail),
                "pynqs_rdm_jrbm")


def scatter(x: Tensor, prob: Tensor, ratio: Tensor, sorb: int, nele: int, noa: int, nob: int, out: Tensor) -> None:
    """pynqs_rdm_scatter: ADD the contributions of the walkers x (weights prob) with the ratio rows psi(x'_k) / psi(x), float64 or
    complex128 [n, ncomb] in get_comb_tensor's column order, into out = (rdm1 | rdm2) flat"""
    n = x.size(0)
    ncomb = CX.get_Num_SinglesDoubles(sorb, noa, nob) + 1
    n1, n2 = _sizes(sorb)
    if ratio.shape != (n, ncomb) or ratio.dtype not in (torch.float64, torch.complex128) or out.numel() != n1 + n2 or out.dtype != torch.float64:
        raise ValueError(f"rdm.scatter: ratio float64 / complex128 [{n}, {ncomb}], out float64 [{n1 + n2}]")
    if not (x.is_cuda and x.device == prob.device == ratio.device == out.device):
        raise ValueError("rdm.scatter: all tensors on one GPU")
    cplx = ratio.is_complex()
    r = (torch.view_as_real(ratio) if cplx else ratio).contiguous()
    N.check(N.lib().pynqs_rdm_scatter(x.contiguous().data_ptr(), n, sorb, nele, noa, nob, prob.contiguous().data_ptr(), r.data_ptr(), int(cplx),
                                      out.data_ptr(), out[n1:].data_ptr(), torch.cuda.current_stream(x.device).cuda_stream), "pynqs_rdm_scatter")


def _rdm_generic(x: Tensor, prob: Tensor, ansatz: Callable[[Tensor], Tensor], sorb: int, nele: int, noa: int, nob: int, nbatch: int, out: Tensor) -> None:
    n = x.size(0)
    ncomb = CX.get_Num_SinglesDoubles(sorb, noa, nob) + 1
    if nbatch <= 0:
        nbatch = max(1, (1 << 26) // (ncomb * sorb))  # +-1 rows of a chunk: at most 512 MiB
    for b in range(0, n, nbatch):
        xs = x[b:b + nbatch].contiguous()
        comb, _ = CX.get_comb_tensor(xs, sorb, nele, noa, nob)
        m = xs.size(0)
        with torch.no_grad():
            psi = ansatz(CX.onv_to_tensor(comb.view(m * ncomb, -1), sorb)).reshape(m, ncomb)
        psi = psi.to(torch.complex128 if psi.is_complex() else torch.float64)
        scatter(xs, prob[b:b + nbatch], psi / psi[:, :1], sorb, nele, noa, nob, out)


def reduced_density_matrices(x: Tensor, state_prob: Tensor, ansatz, sorb: int, nele: int, noa: int, nob: int, fused: Optional[bool] = None,
                             nbatch: int = 0) -> RDM:
    """RDM of the walkers x (packed onv uint8[n, 8 len] on the GPU) with the probabilities state_prob (pre-scaled by the world size under
    torch.distributed) for the amplitude `ansatz` (an nn.Module: +-1 rows -> psi).  fused: None = the fused kernel where it serves
    (module flag FUSED_RBM), True = insist on it (ValueError where it does not serve), False = the generic route; nbatch: walkers per chunk
    of the generic route (0: sized from ncomb).  Bad inputs raise ValueError."""
    prob = _check(x, state_prob, sorb, nele, noa, nob)
    x = x.contiguous()
    params = _fused_params(ansatz, sorb, nele, noa, nob) if fused is not False and (FUSED_RBM or fused) else None
    if fused and params is None:
        raise ValueError("reduced_density_matrices: fused=True needs a RealRBM (rbm_type 'real') within pynqs_rdm_rbm_supported or a "
                         "JastrowRBM within pynqs_rdm_jrbm_supported, float64 parameters on the GPU")
    n1, n2 = _sizes(sorb)
    out = torch.zeros(n1 + n2, dtype=torch.float64, device=x.device)
    if params is not None:
        _rdm_fused(x, prob, params, sorb, nele, noa, nob, out)
    elif x.size(0):
        _rdm_generic(x, prob, ansatz, sorb, nele, noa, nob, int(nbatch), out)
    ws = get_world_size()
    if ws > 1:
        import torch.distributed as dist

        dist.all_reduce(out, dist.ReduceOp.SUM)
        out.div_(ws)
    return RDM(out[:n1], out[n1:], sorb, nele, noa, nob, fused=params is not None)
