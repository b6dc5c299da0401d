"""Many-chain Metropolis sampler on the GPU (PyNQS' Sampler.MCMC, vmc/sample.py:480-569).

The reference runs one chain in a Python loop on the CPU: per step one `spin_flip_rand` proposal (a uniform single or double
excitation, or no move), one full `nqs` forward on one determinant and `random() <= min(1, |psi'|^2 / |psi|^2)`; it raises for
world_size > 1.  Here `nchains` chains advance together, with the rule and the random streams written out in include/pynqs_amd.h:

- an RBM (pynqs_amd.rbm.RealRBM "real" / "tanh" / "pRBM" / "cos", ComplexRBM, or PyNQS' RBMWavefunction: whatever
  energy._real_rbm_params / _complex_rbm_params recognise) runs in the fused kernel pynqs_mcmc_rbm: every chain keeps its hidden-unit
  state on chip and a step costs a few multiplications per hidden unit, many steps per launch;
- a Jastrow-RBM (pynqs_amd.rbm.JastrowRBM, float64 parameters on the GPU: energy._jastrow_rbm_params) runs in the same kernel with the
  Jastrow factor's ln-ratio added to the hidden units' (pynqs_mcmc_jrbm);
- any other ansatz takes the generic path, one step at a time: pynqs_spin_flip_rand -> the module's forward on the proposals (as
  +-1 rows, onv_to_tensor) -> pynqs_mcmc_accept.

Both paths make the same decisions for the same seed (the fused kernel is tested against the generic one).  Under torch.distributed
every rank runs its own chains (chain_base = rank * nchains by default) and the ranks' samples are merged with
sample_comm.gather_scatter_sample, which the reference's MCMC does not support.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import C_extension as CX
from . import _native as N
from . import public_function as pf
from .distributed import get_rank, get_world_size, shard_bounds

__all__ = ["MCMCSampler", "mcmc_rbm_supported", "mcmc_jrbm_supported"]

# chain-steps x hidden units of one fused launch at most: ~1 ms of kernel time at the Fe2S2 size, a few ms at sorb 192
_LAUNCH_WORK = 1 << 28
_MAX_STEPS_PER_LAUNCH = 256


def mcmc_rbm_supported(sorb: int, num_hidden: int, rbm_type: str = "real") -> bool:
    flav = CX.RBM_TYPE_FLAVOUR.get(rbm_type)
    return flav is not None and bool(N.lib().pynqs_mcmc_rbm_supported(sorb, num_hidden, flav))


def mcmc_jrbm_supported(sorb: int, num_hidden: int) -> bool:
    """Whether a JastrowRBM of this size has the fused chain kernel (pynqs_mcmc_jrbm)."""
    return bool(N.lib().pynqs_mcmc_jrbm_supported(sorb, num_hidden))


def _jastrow_params(ansatz):
    """energy._jastrow_rbm_params where every parameter is float64 (float32 parameters take the generic path, whose forward runs in
    float32: the float64 kernel would decide otherwise), else None."""
    from .energy import _jastrow_rbm_params

    prm = _jastrow_rbm_params(ansatz)
    if prm is None:
        return None
    m = getattr(ansatz, "module", ansatz)
    if any(t.dtype != torch.float64 or not t.is_cuda for t in (m.weights, m.hidden_bias, m.visible_bias, m.jastrow)):
        return None
    return prm


def _electrons(onv_words: Tensor) -> Tuple[Tensor, Tensor]:
    """(alpha count, beta count) per row of uint64 words (viewed as int64)."""
    bits = onv_words.view(torch.uint8).view(onv_words.size(0), -1)
    occ = torch.stack([(bits >> k) & 1 for k in range(8)], -1).reshape(bits.size(0), -1).long()  # orbital j = bit j
    return occ[:, 0::2].sum(1), occ[:, 1::2].sum(1)


class _Fused:
    """The parameters of an RBM laid out for pynqs_mcmc_rbm, or of a Jastrow-RBM for pynqs_mcmc_jrbm (rebuilt on every run: the
    parameters change between runs)."""

    def __init__(self, ansatz, sorb: int) -> None:
        from .energy import _complex_rbm_params, _real_rbm_params

        self.log_scale, self.real_valued, self.jastrow_table = 0.0, True, None
        real = _real_rbm_params(ansatz)
        jas = _jastrow_params(ansatz) if real is None else None
        if jas is not None:
            W, hb, vb, M = jas
            self.kind, self.params = "real", (W, hb, vb, M)
            if W.size(1) != sorb:
                raise RuntimeError(f"RBM weights have {W.size(1)} visible units, the sampler sorb = {sorb}")
            self.table, self.jastrow_table = CX.RBMTable(W, hb, vb), CX.JastrowTable(M)
        elif real is not None:
            W, hb, vb, kind = real
            self.kind, self.params = kind, (W, hb, vb)
            if W.size(1) != sorb:
                raise RuntimeError(f"RBM weights have {W.size(1)} visible units, the sampler sorb = {sorb}")
            self.table = CX.RBMTable(W, hb, vb)
        else:
            W, hb, vb, self.log_scale, self.real_valued = _complex_rbm_params(ansatz)
            self.kind, self.params = "complex", (W, hb, vb)
            if W.size(1) != sorb:
                raise RuntimeError(f"RBM weights have {W.size(1)} visible units, the sampler sorb = {sorb}")
            self.table = CX.CRBMTable(W, hb, vb)
        self.flavour = CX.RBM_TYPE_FLAVOUR[self.kind]
        self.nhidden = int(W.size(0))

    @staticmethod
    def applies(ansatz, sorb: int) -> bool:
        from .energy import _complex_rbm_params, _real_rbm_params

        real = _real_rbm_params(ansatz)
        if real is not None:
            return mcmc_rbm_supported(sorb, real[0].size(0), real[3]) and real[0].size(1) == sorb
        jas = _jastrow_params(ansatz)
        if jas is not None:
            return mcmc_jrbm_supported(sorb, jas[0].size(0)) and jas[0].size(1) == sorb
        cplx = _complex_rbm_params(ansatz)
        return cplx is not None and mcmc_rbm_supported(sorb, cplx[0].size(0), "complex") and cplx[0].size(1) == sorb

    def psi(self, onv: Tensor, sorb: int) -> Tensor:
        """psi of the rows (the module's values: cos -> the complex kernel's value times 2^-H, real-valued)."""
        if self.jastrow_table is not None:
            return CX.jrbm_forward(onv, *self.params, sorb)
        W, hb, vb = self.params
        if self.kind == "complex":
            psi = CX.rbm_forward(onv, W, hb, vb, sorb, "complex")
            if self.log_scale:
                psi = psi * torch.exp(torch.tensor(-self.log_scale, dtype=torch.float64, device=psi.device))
            return psi.real.contiguous() if self.real_valued else psi
        return CX.rbm_forward(onv, W, hb, vb, sorb, self.kind)


class MCMCSampler:
    """nchains Metropolis chains over the determinants with noA alpha and noB beta electrons in sorb spin orbitals.

    initial_state: uint8 [1 | nchains, 8 len] packed ONVs (one row is copied to every chain).  chain_base: the global index of
    chain 0 (default rank * nchains).  The chain states, the step counter and the accept counts persist between calls of run(), so a
    VMC loop keeps its chains warm across parameter updates."""

    def __init__(self, sorb: int, nele: int, noA: int, noB: int, nchains: int, seed: int, initial_state: Tensor,
                 chain_base: Optional[int] = None) -> None:
        if noA + noB != nele:
            raise RuntimeError(f"nele = {nele} != noA + noB = {noA + noB}")
        if not 1 <= sorb <= 192:
            raise RuntimeError(f"sorb = {sorb} outside [1, 192]")
        if nchains < 1:
            raise RuntimeError("nchains must be positive")
        L = (sorb - 1) // 64 + 1
        if initial_state.dtype != torch.uint8 or initial_state.dim() != 2 or initial_state.size(1) != 8 * L or \
                initial_state.size(0) not in (1, nchains):
            raise RuntimeError(f"initial_state must be uint8 [1 or {nchains}, {8 * L}]")
        dev = initial_state.device if initial_state.is_cuda else torch.device("cuda", torch.cuda.current_device())
        x = initial_state.to(dev).contiguous().view(torch.int64)
        x = x.expand(nchains, L).contiguous() if x.size(0) == 1 else x.clone()
        na, nb = _electrons(x)
        if bool((na != noA).any()) or bool((nb != noB).any()):
            raise RuntimeError(f"initial_state: every chain needs {noA} alpha and {noB} beta electrons")
        if sorb % 64 and bool((x[:, -1] >> (sorb % 64)).any()):
            raise RuntimeError(f"initial_state has occupied orbitals beyond sorb = {sorb}")
        self.sorb, self.nele, self.noA, self.noB, self.nchains = sorb, nele, noA, noB, nchains
        self.seed = int(seed) & (2**64 - 1)
        self.chain_base = get_rank() * nchains if chain_base is None else int(chain_base)
        if self.chain_base < 0 or self.chain_base + nchains > 2**32:
            raise RuntimeError("chain indices must stay in [0, 2^32)")
        self.device, self.len = dev, L
        self._x = x                      # int64 [nchains, len]: the chains' states
        self.step = 0                    # index t of the next step
        self.n_accept = torch.zeros(nchains, dtype=torch.int64, device=dev)  # over the recorded windows
        self.n_counted = 0               # steps per chain in the recorded windows
        self.lnpsi: Optional[Tensor] = None  # ln|psi| of the states after a fused run
        self.last_records: Optional[Tensor] = None

    @property
    def states(self) -> Tensor:
        """uint8 [nchains, 8 len]: the chains' current states."""
        return self._x.view(torch.uint8).view(self.nchains, -1)

    @property
    def acceptance(self) -> float:
        return float(self.n_accept.sum()) / max(1, self.n_counted * self.nchains)

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---- one launch of the fused kernel
    def _fused_launch(self, f: _Fused, nsteps: int, every: int, record: bool) -> Optional[Tensor]:
        rec = torch.empty((nsteps // every, self.nchains, self.len), dtype=torch.int64, device=self.device) if record else None
        self.lnpsi = torch.empty(self.nchains, dtype=torch.float64, device=self.device)
        if f.jastrow_table is not None:
            N.check(N.lib().pynqs_mcmc_jrbm(self._x.data_ptr(), self.nchains, self.sorb, self.noA, self.noB, f.table.data_ptr(),
                                            f.jastrow_table.data_ptr(), f.nhidden, self.seed, self.chain_base, self.step, nsteps, every,
                                            rec.data_ptr() if record else None, self.n_accept.data_ptr() if record else None,
                                            self.lnpsi.data_ptr(), self._stream()), "pynqs_mcmc_jrbm")
        else:
            N.check(N.lib().pynqs_mcmc_rbm(self._x.data_ptr(), self.nchains, self.sorb, self.noA, self.noB, f.table.data_ptr(), f.nhidden,
                                           f.flavour, self.seed, self.chain_base, self.step, nsteps, every,
                                           rec.data_ptr() if record else None, self.n_accept.data_ptr() if record else None,
                                           self.lnpsi.data_ptr(), self._stream()), "pynqs_mcmc_rbm")
        self.step += nsteps
        return rec

    # ---- one step of the generic path
    def _generic_step(self, ansatz, psi: Tensor, record: bool) -> Optional[Tensor]:
        prop = torch.empty_like(self._x)
        N.check(N.lib().pynqs_spin_flip_rand(self._x.data_ptr(), self.nchains, self.sorb, self.noA, self.noB, self.seed,
                                             (self.step << 32) + self.chain_base, prop.data_ptr(), self._stream()), "spin_flip_rand")
        psi_p = self._forward(ansatz, prop).to(psi.dtype).contiguous()
        row = torch.empty_like(self._x) if record else None
        cplx = psi.is_complex()
        N.check(N.lib().pynqs_mcmc_accept(self._x.data_ptr(), psi.data_ptr(), prop.data_ptr(), psi_p.data_ptr(), self.nchains, self.sorb,
                                          int(cplx), self.seed, self.chain_base, self.step, row.data_ptr() if record else None,
                                          self.n_accept.data_ptr() if record else None, self._stream()), "pynqs_mcmc_accept")
        self.step += 1
        return row

    def _forward(self, ansatz, words: Tensor) -> Tensor:
        onv = words.view(torch.uint8).view(words.size(0), -1)
        with torch.no_grad():
            out = ansatz(CX.onv_to_tensor(onv, self.sorb))
        if out.dtype not in (torch.float64, torch.complex128):
            out = out.to(torch.complex128 if out.is_complex() else torch.float64)
        return out.reshape(-1)

    def run(self, ansatz, n_therm: int, n_sample: int, every: int = 1, keep_records: bool = False):
        """n_therm discarded steps, then n_sample steps recording the states after every `every`-th one.  Returns Sampler.MCMC's tuple
        (sample_unique uint8 [m, 8 len] in torch.unique(dim=0) order, sample_counts int64 [m], sample_prob float64 [m], WF_LUT) -- under
        torch.distributed the rank's shard of the merged samples, its probabilities pre-scaled by world_size, and the LUT of all of them.
        keep_records: also keep the records (int64 [n_sample // every, nchains, len] words) in self.last_records."""
        if n_therm < 0 or n_sample < 0 or every < 1:
            raise RuntimeError("n_therm, n_sample >= 0 and every >= 1")
        fused = _Fused(ansatz, self.sorb) if _Fused.applies(ansatz, self.sorb) else None
        uniq = torch.empty((0, self.len), dtype=torch.int64, device=self.device)
        counts = torch.empty(0, dtype=torch.int64, device=self.device)
        kept = []

        def merge(rows: Tensor):  # (distinct rows, counts) of everything recorded so far: memory bounded by one launch + the distinct set
            nonlocal uniq, counts
            if rows.numel() == 0:
                return
            if keep_records:
                kept.append(rows.view(-1, self.nchains, self.len))
            allr = torch.cat([uniq, rows.reshape(-1, self.len)])
            allc = torch.cat([counts, torch.ones(allr.size(0) - uniq.size(0), dtype=torch.int64, device=self.device)])
            u, inv = pf.unique_onv(allr.view(torch.uint8).view(allr.size(0), -1))
            counts = torch.zeros(u.size(0), dtype=torch.int64, device=self.device).index_add_(0, inv, allc)
            uniq = u.contiguous().view(torch.int64).view(-1, self.len)

        if fused is not None:
            per = max(1, min(_MAX_STEPS_PER_LAUNCH, _LAUNCH_WORK // (self.nchains * max(fused.nhidden, 1))))
            left = n_therm
            while left > 0:
                k = min(per, left)
                self._fused_launch(fused, k, 1, False)
                left -= k
            per_s = max(every, per // every * every)
            left = n_sample
            while left > 0:
                k = min(per_s, left)
                merge(self._fused_launch(fused, k, every, True))
                left -= k
        else:
            psi = self._forward(ansatz, self._x).clone()
            for _ in range(n_therm):
                self._generic_step(ansatz, psi, False)
            for k in range(n_sample):
                row = self._generic_step(ansatz, psi, (k + 1) % every == 0)
                if row is not None:
                    merge(row)
        self.n_counted += n_sample
        self.last_records = torch.cat(kept) if kept else (torch.empty((0, self.nchains, self.len), dtype=torch.int64, device=self.device)
                                                          if keep_records else None)
        u8 = uniq.view(torch.uint8).reshape(uniq.size(0), 8 * self.len)
        u8, inv = torch.unique(u8, dim=0, sorted=True, return_inverse=True)
        counts = torch.zeros(u8.size(0), dtype=torch.int64, device=self.device).index_add_(0, inv, counts)
        psi_u = fused.psi(u8, self.sorb) if fused is not None else self._forward(ansatz, u8.contiguous().view(torch.int64))
        if get_world_size() > 1:
            from .sample_comm import gather_scatter_sample

            ws = get_world_size()
            u_r, _, prob_r, lut, merged = gather_scatter_sample(u8, counts, psi_u, self.sorb, use_LUT=True, use_same_tree=False, is_onv=True)
            b, e = shard_bounds(merged.size(0), ws, get_rank())
            return u_r, merged[b:e], prob_r, lut
        prob = counts.double() / max(1, int(counts.sum()))
        return u8, counts, prob, pf.WavefunctionLUT(u8, psi_u, self.sorb, self.device)
