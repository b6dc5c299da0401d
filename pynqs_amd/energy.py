"""Local energy E_loc(x) = sum_x' <x|H|x'> psi(x') / psi(x)  -- mirror of PyNQS' vmc/energy/{eloc,flip,etot}.py.

Same entry points and argument meaning as the reference:
    local_energy(x, h1e, h2e, ansatz, ansatz_batch, sorb, nele, noa, nob, ...) -> (eloc, sloc, psi, times)
    total_energy(x, nbatch, fp_batch, h1e, h2e, ansatz, sorb, nele, noa, nob, ...) -> (eloc, sloc, placeholder)
    Func(func, x, WF_LUT, use_unique)
with the three methods of the reference (SIMPLE / REDUCE / SAMPLE_SPACE, vmc/energy/eloc.py:75-114) and their
spin-flip-projected and multi-psi variants (vmc/energy/flip.py).

What differs is where the work happens (all on the MI355X, through pynqs_amd.C_extension / the C ABI):
  * enumeration and <x|H|x'> always come from the fused kernel (the reference's SIMPLE/REDUCE call the
    unfused pair get_comb_tensor + get_hij_torch, whose outputs are bit-identical to the fused call);
  * SAMPLE_SPACE (also its spin-flip projected, multi-psi and <S-S+> forms) runs as ONE kernel per sum, nothing materialised, in one
    of two forms chosen per call (choose_sample_space_kernel): over the walker's excitation lists with a filter in front
    (pynqs_eloc_sample_space[_hash]), or over the TABLE (pynqs_eloc_sample_space_keys: work ~ walkers x keys instead of walkers x ncomb,
    the form for large orbital spaces);
  * SIMPLE with an RBM ansatz (real parameters: rbm_type real / tanh / pRBM; complex parameters; cos) evaluates the amplitude ratios
    inside the kernel (pynqs_eloc_rbm[_flavour], pynqs_eloc_crbm); its spin-flip-projected form, for the real-parameter flavours and the
    Jastrow-RBM, as two passes of the same kernels and a combine kernel (pynqs_eloc_rbm_flip, pynqs_eloc_jrbm_flip);
  * REDUCE compacts the kept columns on chip (pynqs_reduce_count / _emit, and pynqs_reduce_sample for eps_sample > 0) instead of
    writing the whole (batch, ncomb) comb / Hmat and filtering afterwards; the projected / multi-psi / <S-S+> factors are evaluated on
    the kept records.  With an RBM of the reference's family, or a Jastrow-RBM, the amplitudes of the distinct x' come from their parent
    walkers (pynqs_rbm_forward_children; for the Jastrow-RBM followed by pynqs_jastrow_children_apply), not from the module.
`FUSED = False` (and FUSED_RBM / FUSED_SAMPLED) force the generic tensor path (used by the tests to cross-check the fast paths).

local_energy is a dispatcher over one function per path, asked in this order (each returns (eloc, sloc, psi, times); None: it declines):
  1. _eloc_sample_space_fused        SAMPLE_SPACE in one kernel per sum
  2. _eloc_simple_rbm                SIMPLE with an RBM evaluated in the kernel (declines: not such an RBM, or it does not fit the LDS)
  3. _eloc_reduce_front              REDUCE through the one-launch front end (declines: a long row outgrew its LDS list)
  4. _eloc_reduce_multipass          REDUCE, eps_sample = 0, compaction in several passes
  5. _eloc_reduce_multipass_sampled  REDUCE, eps_sample > 0, plain form, selection and draws in several passes
  6. _eloc_generic                   the reference's tensor algebra on the (batch, ncomb) matrices
"""
from __future__ import annotations

import logging
import math
import os
import threading
import time
import weakref
from dataclasses import dataclass
from functools import partial
from types import SimpleNamespace
from typing import Callable, Optional, Tuple

import torch
from torch import Tensor

from . import C_extension as CX
from . import _native as N
from . import reduce_front as RF
from .C_extension import get_comb_hij_fused, get_hij_torch
from .distributed import get_rank, get_world_size
from .public_function import (SpinProjection, WavefunctionLUT, ansatz_batch, check_para, get_nbatch, get_Num_SinglesDoubles,
                              spin_flip_onv, spin_flip_sign, split_batch_idx, unique_onv)
from .rbm import ComplexRBM, JastrowRBM, RealRBM

_LOG = logging.getLogger("pynqs_amd")


def _env_flag(name: str, default: Optional[bool]) -> Optional[bool]:
    """The "1" / "0" switches of the environment: True / False, and `default` for anything else (or nothing) there."""
    return {"1": True, "0": False}.get(os.environ.get(name, ""), default)


FUSED = True  # use the fused sample-space / reduce kernels when the configuration allows it
FUSED_SAMPLED = True  # REDUCE with eps_sample > 0: select and draw on chip (reduce_compact_sampled) instead of torch.multinomial on the matrix
FUSED_RBM = True  # SIMPLE method: evaluate a real RBM ansatz inside the kernel (pynqs_eloc_rbm) instead of calling the module
OVERLAP = _env_flag("PYNQS_OVERLAP", True)  # total_energy: front end of the next walker chunk on a second stream
_SIDE_STREAMS: dict = {}
# The caches below (front-end workspaces, routing decisions, timed kernel choices) are process-wide and guarded by ONE lock: a workspace is
# popped by the call that uses it and put back when that call has its counters, so two threads never share one; decisions are written once
# per key.  reset_caches() drops everything (e.g. between two systems in one process).  The C ABI underneath has no global state at all.
_LOCK = threading.RLock()
# .value: the total_energy call in progress in THIS thread (an object per call, restored when the call ends or raises): what per-parameter-state
# caches of local_energy are valid for
_CALL_TOKEN = threading.local()


def _call_token():
    return getattr(_CALL_TOKEN, "value", None)


def _side_stream(device):
    key = str(device)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device)
    return _SIDE_STREAMS[key]


# REDUCE on rows of more than FRONT_LONG_ROW columns: the one-launch front end only while a segment's kept records fit its LDS list, else
# the multi-pass path (reduce_compact / reduce_compact_sampled).  Measured (tools/reduce_big_paths.py, one MI355X, local_energy with a real
# RBM, ms one-launch / multi-pass): rows of 7.9e3 and 3.1e4 columns (sorb 40, 56) the one-launch form wins in either of its forms (4.2 / 13.2,
# 0.56 / 1.14, 8.4 / 43.6, 5.7 / 6.4, sampled 0.9 / 2.6 and 6.2 / 9.0); rows of 2.3e5 and 1.2e6 columns (sorb 80, 120): LIST form 5.3 / 6.4,
# 10.6 / 10.4, sampled 13.0 / 14.6, 2.7 / 3.0 -- its other (look-back) form 22 / 6.1, 94 / 30, 96 / 38, sampled 68 / 14 and 54 / 16.
FRONT_ROUTE = True
FRONT_SAMPLED_MIN_WALKERS = 512   # long rows with draws: the whole row is one workgroup's, fewer walkers than this leave CUs idle


def __getattr__(name):
    # FRONT_LONG_ROW is the library's own constant (the plan's long_row flag compares with it), read when first asked for.  It is not a module
    # global: `import *` does not export it, and setting it changes nothing that _long_row_cap decides (that is the plan's flag)
    if name == "FRONT_LONG_ROW":
        return int(N.lib().pynqs_reduce_onepass_long_row())
    raise AttributeError(name)


_FRONT_DENSE: "set[tuple]" = set()   # long-row systems whose kept records outgrew the LDS list (this process)
# De-duplication of the x' costs random probes into a table of 2-4 slots per distinct determinant: 64 MB for Fe2S2 (8192 walkers, 1.5 M distinct
# of 10 M records: it stays in the 256 MB cache and saves 85 % of the amplitude evaluations), 1.6 GB at sorb 80 with 4096 walkers, where
# 21.5 M of 21.5 M records are distinct and the probes cost 16x the enumeration (46.6 against 2.8 ms per launch, tools/onepass_flush_stamps.py).
# local_energy therefore looks at the first call of a (system, batch size): when more than FRONT_NODEDUP_RATIO of the records were distinct
# the following calls run without the table (every record its own row; E_loc is the same, the ansatz sees <= 1 / ratio as many rows).
FRONT_NODEDUP = _env_flag("PYNQS_FRONT_NODEDUP", True)
FRONT_NODEDUP_RATIO = 0.9
_FRONT_NODEDUP: "dict[tuple, Optional[tuple]]" = {}   # key -> (cap_doubles, cap_unique) of the table-less front end, or None: keep the table
FRONT_NODEDUP_RECHECK = 64   # routed calls after which the decision (table or no table) for a (system, batch size, eps) is measured again:
_FRONT_NODEDUP_CALLS: dict = {}  # the first VMC iterations see the most diverse walkers; a run must not stay table-less once they concentrate
FUSED_ONEPASS = True  # REDUCE: the one-launch front end (reduce_front.ReduceFrontEnd); False: the multi-pass compaction of round 2
SPECULATE_RBM = _env_flag("PYNQS_SPECULATE_RBM", True)  # REDUCE with an RBM: amplitudes and contraction enqueued before the counters are read (_rbm_ahead)


def Func(func: Callable[..., Tensor], x: Tensor, WF_LUT: Optional[WavefunctionLUT] = None, use_unique: bool = False) -> Tensor:
    """vmc/energy/flip.py:29-63: psi(x) through the lookup table for known determinants, the ansatz (on the
    unique rows if use_unique) for the others."""
    use_lut = WF_LUT is not None
    batch = x.size(0)
    if use_lut:
        lut_idx, lut_not_idx, lut_value = WF_LUT.lookup(x)
    _x = x[lut_not_idx] if use_lut else x
    if use_unique:
        unique_x, inverse = unique_onv(_x) if _x.dtype == torch.uint8 and _x.dim() == 2 and _x.size(1) % 8 == 0 \
            else torch.unique(_x, dim=0, return_inverse=True)
        psi0 = torch.index_select(func(unique_x), 0, inverse)
    else:
        psi0 = func(_x)
    if not use_lut:
        return psi0
    psi = torch.empty(batch, dtype=psi0.dtype, device=psi0.device)
    psi[lut_idx] = lut_value.to(psi0.dtype)
    psi[lut_not_idx] = psi0
    return psi


def _real_dtype(dtype: torch.dtype) -> torch.dtype:
    return dtype.to_real() if dtype.is_complex else dtype


def _contract(f_psi: Tensor, psi_x1: Tensor, hij: Tensor) -> Tensor:
    """eloc.py:185-186: ((f_psi.T / psi_0).T * H).sum(-1)."""
    return ((f_psi.T / psi_x1[..., 0]).T * hij).sum(-1)


def _f_psi(psi_x1: Tensor, f: Optional[Tensor], eta_m: Optional[Tensor], psi_flip: Optional[Tensor], f_flip: Optional[Tensor], extra_norm):
    """The numerator of the projected / multi-psi forms on (batch, n_comb) matrices, column 0 = the walker itself (flip.py:254-303):
    (f psi + eta eta_m f(flip) psi(flip)) conj(f(x)) / N^2;  f None: no multi-psi (f = 1), eta_m None: no projection (no second term)."""
    if eta_m is None:
        return psi_x1 if f is None else psi_x1 * f * f[..., 0].reshape(-1, 1).conj() / extra_norm**2
    eta = SpinProjection.eta
    if f is None:
        return (psi_x1 + eta * eta_m * psi_flip) / extra_norm**2
    return (f * psi_x1 + eta * eta_m * f_flip * psi_flip) * f[..., 0].reshape(-1, 1).conj() / extra_norm**2


def _amplitudes(comb_flat: Tensor, sel: Optional[Tensor], batch: int, n_comb: int, ansatz, ansatz_extra, WF_LUT, use_unique,
                use_multi_psi, use_spin_flip, extra_norm, dtype, sorb, device):
    """psi (and, for the projected / multi-psi forms, f*psi) on the selected columns, scattered into
    (batch, n_comb) arrays that are zero elsewhere (eloc.py:300-311, flip.py:254-303)."""
    x = comb_flat if sel is None else comb_flat[sel]

    def scatter(v: Tensor, dt=None) -> Tensor:
        if sel is None:
            return v.reshape(batch, n_comb)
        out = torch.zeros(batch * n_comb, dtype=dt or v.dtype, device=device)
        out[sel] = v.to(out.dtype)
        return out.reshape(batch, n_comb)

    def on(fn, xx, lut) -> Tensor:
        return scatter(Func(fn, xx, lut, use_unique).to(dtype), dtype)

    psi_x1 = on(ansatz, x, WF_LUT)
    eta_m = psi_flip = f = f_flip = None
    if use_spin_flip:
        x_flip = spin_flip_onv(x, sorb)
        eta_m = scatter(spin_flip_sign(x, sorb))
        psi_flip = on(ansatz, x_flip, WF_LUT)
    if use_multi_psi:
        f = on(ansatz_extra, x, None)
        f_flip = on(ansatz_extra, x_flip, None) if use_spin_flip else None
    return psi_x1, _f_psi(psi_x1, f, eta_m, psi_flip, f_flip, extra_norm)


def _amplitudes_sample_space(flat: Tensor, batch: int, n_comb: int, ansatz_extra, WF_LUT, use_multi_psi, use_spin_flip, extra_norm, sorb):
    """_amplitudes for SAMPLE_SPACE: psi only from the table (eloc.py:381-385, flip.py:375-383), f only on its hits; misses stay 0."""
    def in_table(xx: Tensor):
        out = torch.zeros(xx.size(0), device=xx.device, dtype=WF_LUT.dtype)
        idx, _, value = WF_LUT.lookup(xx)
        out[idx] = value
        return out.reshape(batch, n_comb), idx

    def f_on(xx: Tensor, hit: Tensor) -> Tensor:
        out = torch.zeros(xx.size(0), device=xx.device, dtype=WF_LUT.dtype)
        out[hit] = Func(ansatz_extra, xx[hit], None, True).to(out.dtype)
        return out.reshape(batch, n_comb)

    psi_x1, hit = in_table(flat)
    eta_m = psi_flip = f = f_flip = None
    if use_spin_flip:
        flip = spin_flip_onv(flat, sorb)
        eta_m = spin_flip_sign(flat, sorb).reshape(batch, n_comb)
        psi_flip, hit_f = in_table(flip)
    if use_multi_psi:
        f = f_on(flat, hit)
        f_flip = f_on(flip, hit_f) if use_spin_flip else None
    return psi_x1, _f_psi(psi_x1, f, eta_m, psi_flip, f_flip, extra_norm)


def _reduce_select(comb_hij: Tensor, eps: float, eps_sample: int) -> Tensor:
    """Column selection of the REDUCE method (eloc.py:257-298).  With eps_sample > 0 the small elements are
    importance-sampled (torch.multinomial, RNG dependent) and comb_hij is re-weighted in place."""
    batch, n_comb = comb_hij.shape
    device = comb_hij.device
    if eps_sample <= 0:
        return torch.where(comb_hij.reshape(-1).abs() >= eps)[0]
    if eps > 0.0:
        hij_abs = comb_hij.abs()
        mask = hij_abs >= eps
        index = torch.where(mask.flatten())[0]
        hij = torch.where(mask, 0, hij_abs)
    else:
        index = None
        hij = comb_hij.abs()
    prob = hij / hij.sum(1, keepdim=True)
    counts = torch.multinomial(prob, eps_sample, replacement=True)
    counts += torch.arange(batch, device=device).reshape(-1, 1) * n_comb
    index1, count = counts.unique(sorted=True, return_counts=True)
    prob = prob.flatten()
    comb_hij.view(-1)[index1] = (count / eps_sample) * comb_hij.flatten()[index1] / prob[index1]
    return index1 if index is None else torch.cat([index, index1])


def _real_rbm_params(ansatz):
    """(weights [H, sorb], hidden_bias [H], visible_bias [sorb], rbm_type) if `ansatz` (possibly DDP-wrapped) is an RBM with real
    parameters and one of the fused formulas (pynqs_amd.rbm.RealRBM, or PyNQS' RBMWavefunction, rbm_type "real" / "tanh" / "pRBM",
    rbm.py:199-211), else None."""
    m = getattr(ansatz, "module", ansatz)
    kind = getattr(m, "rbm_type", None)
    if kind not in CX.RBM_FLAVOURS or not (isinstance(m, RealRBM) or hasattr(m, "effective_theta")):
        return None
    W, hb, vb = getattr(m, "weights", None), getattr(m, "hidden_bias", None), getattr(m, "visible_bias", None)
    if W is None or hb is None or vb is None or W.dtype not in (torch.float64, torch.float32) or not W.is_cuda or W.dim() != 2:
        return None
    # (float32 parameters are handed to the float64 kernel as they are: an exact conversion)
    return W.detach().double(), hb.detach().reshape(-1).double(), vb.detach().reshape(-1).double(), kind


def _complex_rbm_params(ansatz):
    """((re, im) weights [H, sorb, 2], hidden_bias [H, 2], visible_bias [sorb, 2] or None, log_scale, real_valued) for the fused kernel
    with complex running products (pynqs_eloc_crbm): an RBM with complex parameters (pynqs_amd.rbm.ComplexRBM, or PyNQS'
    RBMWavefunction(rbm_type="complex") -- the reference's params_* layout), or rbm_type "cos" with real parameters, which is the same
    function of i W, i b up to 2^H (cos t = cosh(i t)); else None."""
    m = getattr(ansatz, "module", ansatz)
    kind = getattr(m, "rbm_type", None)
    if isinstance(m, ComplexRBM) or (kind == "complex" and hasattr(m, "params_weights")):
        W, hb, vb = m.params_weights, m.params_hidden_bias, getattr(m, "params_visible_bias", None)
        if W is None or hb is None or not W.is_cuda or W.dtype != torch.float64 or W.size(-1) != 2:
            return None
        H = hb.numel() // 2
        return W.detach().reshape(H, -1, 2), hb.detach().reshape(H, 2), (vb.detach().reshape(-1, 2) if vb is not None else None), 0.0, False
    if kind == "cos" and (isinstance(m, RealRBM) or hasattr(m, "effective_theta")):
        W, hb = getattr(m, "weights", None), getattr(m, "hidden_bias", None)
        if W is None or hb is None or not W.is_cuda or W.dtype not in (torch.float64, torch.float32) or W.dim() != 2:
            return None
        W, hb = W.detach().double(), hb.detach().reshape(-1).double()
        return torch.stack([torch.zeros_like(W), W], -1), torch.stack([torch.zeros_like(hb), hb], -1), None, W.size(0) * math.log(2.0), True
    return None


def _jastrow_rbm_params(ansatz):
    """(weights [H, sorb], hidden_bias [H], visible_bias [sorb], jastrow [sorb, sorb]) if `ansatz` (possibly DDP-wrapped) is a
    pynqs_amd.rbm.JastrowRBM with its parameters on the GPU, else None."""
    m = getattr(ansatz, "module", ansatz)
    if not isinstance(m, JastrowRBM):
        return None
    W, hb, vb, M = m.weights, m.hidden_bias, m.visible_bias, m.jastrow
    if W.dtype not in (torch.float64, torch.float32) or not W.is_cuda or W.dim() != 2 or M.shape != (W.size(1), W.size(1)):
        return None
    return W.detach().double(), hb.detach().reshape(-1).double(), vb.detach().reshape(-1).double(), M.detach().double()


def _rbm_lds_ok(sorb: int, nele: int, noa: int, nob: int, nhidden: int) -> bool:
    """pynqs_eloc_rbm keeps exp(+-4W) of all (orbital, hidden unit) pairs in LDS (160 KiB per workgroup)."""
    return bool(N.lib().pynqs_eloc_rbm_supported(sorb, nele, noa, nob, nhidden))


def _fast_sample_space_ok(x, h1e, sorb, WF_LUT) -> bool:
    return (FUSED and WF_LUT is not None and WF_LUT.sort
            and sorb % 2 == 0 and h1e.dtype in (torch.float64, torch.float32)
            and WF_LUT.dtype in (torch.float64, torch.complex128, torch.float32, torch.complex64)
            and x.is_cuda and WF_LUT.bra_key.is_cuda)


# SAMPLE_SPACE: walk the table (key-major, pynqs_eloc_sample_space_keys: work ~ walkers x keys) or the excitation lists (column-major,
# pynqs_eloc_sample_space[_hash]: work ~ walkers x ncomb)?  By measurement the key-major kernel wins while the table has
# fewer than SS_KEYS_RATIO[words] x ncomb keys (Fe2S2, ncomb 7876: crossover at ~1.3e4 keys; sorb 120 with 6.5e4 keys: 50x faster).  SS_KEYS = True / False (or PYNQS_SS_KEYS=1 / 0) forces one of them.
SS_KEYS: Optional[bool] = None
# (words of a determinant) -> (key-major below this many x ncomb keys, column-major above this many, ratio used when probing is off):
# between the two the cost depends on how many keys lie within a double excitation of a walker (a CAS-like table is dense in them, a
# table of samples is not), so the first call at a new (system, table size) times both kernels on up to 1024 walkers and remembers the
# winner (profiles/r02_*_sample_space_vs_table_size.txt: sorb 56, sparse table: key-major wins up to 30 x ncomb; Fe2S2's CAS table: up to
# 1.7 x ncomb; sorb 120 / 184: at every size tried).
SS_KEYS_ZONE = {1: (0.75, 64.0, 1.5), 2: (16.0, 256.0, 16.0), 3: (16.0, 256.0, 16.0)}
# Timing both kernels costs a host synchronisation inside a VMC step and makes the choice (key-major accumulates with float atomics) depend
# on the machine's state: OFF by default -- the fixed ratios above decide, the same on every rank and in every run.  PYNQS_SS_AUTOTUNE=1
# (or SS_AUTOTUNE = True) turns the probe on; with several ranks rank 0 probes and everybody takes its answer.
SS_AUTOTUNE = _env_flag("PYNQS_SS_AUTOTUNE", False)
_SS_CHOICE: dict = {}


def _key_major(nkeys: int, sorb: int, noa: int, nob: int, probe: Optional[Callable[[], bool]] = None, tag=()) -> bool:
    if nkeys >= 1 << 27:
        return False
    force = SS_KEYS if SS_KEYS is not None else _env_flag("PYNQS_SS_KEYS", None)   # (read at call time)
    if force is not None:
        return force
    ncomb = get_Num_SinglesDoubles(sorb, noa, nob) + 1
    lo, hi, ratio = SS_KEYS_ZONE[(sorb - 1) // 64 + 1]
    if nkeys <= lo * ncomb:
        return True
    if nkeys >= hi * ncomb:
        return False
    if probe is None or not SS_AUTOTUNE or get_world_size() > 1 or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
        # (a probe synchronises: never inside a graph capture; and never with several ranks -- the ranks do not reach this point in the same
        # calls (an empty shard never calls local_energy, the per-process cache answers some ranks and not others): the fixed ratio decides,
        # the same on every rank)
        return nkeys <= ratio * ncomb
    key = (sorb, noa, nob, (4 * nkeys).bit_length(), tag)  # table sizes in steps of sqrt(2)... of 2 with two guard bits: [2^k/4 steps]
    if key not in _SS_CHOICE:
        choice = bool(probe())
        _SS_CHOICE[key] = choice
        _LOG.info("SAMPLE_SPACE kernel for sorb %d, %d keys: %s (timed)", sorb, nkeys, "key-major" if choice else "column-major")
    return _SS_CHOICE[key]


# Key-major, streamed or INDEXED (round 3)?  The index (C_extension.keys_index_build: the keys sorted by each of five blocks of the
# orbitals) turns "compare with every key" into "compare with the keys that agree with the walker in a whole block": 13 instead of 65 536
# per walker for a table of samples at sorb 120 / 184 (0.043 / 0.059 ms per 8192 walkers instead of 0.20 / 0.29), but 21.5e3 of 18.5e3 for
# Fe2S2's CAS-like table, whose members share every block with thousands of others.  Building it costs ~0.06 ms + 1 us per 1000 keys and one
# host synchronisation, per table: it is bought when the (walker, key) pairs streamed against this table so far would have paid for it
# (the ski-rental rule: never worse than twice the better choice), and used when it is sparse enough.
RBM_FROM_PARENTS = True  # REDUCE with an RBM ansatz: psi(x') of the distinct x' from theta(parent walker) (pynqs_rbm_forward_children)
SS_INDEX: Optional[bool] = None  # True / False (or PYNQS_SS_INDEX=1 / 0): always / never; None: the rule above
SS_INDEX_PAIR_COST = {1: 2.4e-13, 2: 3.7e-13, 3: 5.3e-13}  # seconds per streamed (walker, key) pair, by words per determinant (measured)
SS_INDEX_CANDIDATE_COST = 6.0e-12  # seconds per (walker, key met through the index)


def _keys_index_for(WF_LUT, n: int, sorb: int):
    """The table's KeysIndex if the INDEXED form should run this call, else None (the streamed form runs and the call is counted)."""
    force = SS_INDEX if SS_INDEX is not None else _env_flag("PYNQS_SS_INDEX", None)   # (read at call time)
    if force is False or sorb % 2:
        return None
    keys = WF_LUT.bra_key
    nk, words = keys.size(0), (sorb - 1) // 64 + 1
    cached = getattr(WF_LUT, "_keys_index", None)
    of = getattr(WF_LUT, "_keys_index_of", None)   # (weakref(keys), version counter of keys) the index was built for
    ver = CX._ver(keys)
    if cached is not None and (cached.nkeys != nk or cached.index.device != keys.device or not isinstance(of, tuple) or of[0]() is not keys
                               or of[1] != ver or ver < 0):
        cached = None  # (the table was moved, rebuilt or written in place; untracked keys -- inference mode -- are indexed on every call)
    if cached is None:
        if torch.cuda.is_current_stream_capturing():
            return None  # (the build synchronises)
        pairs = getattr(WF_LUT, "_keys_streamed_pairs", 0) + n * nk
        if force is None and pairs * SS_INDEX_PAIR_COST[words] < 5.5e-5 + 1.1e-9 * nk:
            try:
                WF_LUT._keys_streamed_pairs = pairs
            except AttributeError:  # (a table object that takes no attributes: stay with the streamed form)
                pass
            return None
        cached = CX.keys_index_build(keys, sorb)
        try:
            WF_LUT._keys_index, WF_LUT._keys_index_of = cached, (weakref.ref(keys), ver)
        except AttributeError:
            pass
    if force is None and cached.per_walker * SS_INDEX_CANDIDATE_COST > nk * SS_INDEX_PAIR_COST[words]:
        return None  # dense: a walker would meet more keys through the index than it is worth
    return cached


def _launch_sample_space(key_major: bool, x, n, sorb, nele, noa, nob, plan, WF_LUT, wf, cplx, flip, eloc, psi0, part, st) -> None:
    lib = N.lib()
    keys, ht = WF_LUT.bra_key, getattr(WF_LUT, "hashtable", None)
    head = (x.data_ptr(), n, sorb, nele, noa, nob, plan.data_ptr())
    if key_major:   # one entry point for both sums: its flag says which
        ki = _keys_index_for(WF_LUT, n, sorb)
        if ki is not None:
            fn, name, table = lib.pynqs_eloc_sample_space_indexed, "pynqs_eloc_sample_space_indexed", (keys.data_ptr(), keys.size(0), ki.index.data_ptr())
        else:
            fn, name, table = lib.pynqs_eloc_sample_space_keys, "pynqs_eloc_sample_space_keys", (keys.data_ptr(), keys.size(0))
        rc = fn(*head, *table, wf.data_ptr(), int(cplx), 0, eloc.data_ptr(), psi0.data_ptr(), st)
        if rc == 0 and flip:
            rc = fn(*head, *table, wf.data_ptr(), int(cplx), 1, part.data_ptr(), psi0.data_ptr(), st)
        N.check(rc, name)
        return
    if ht is not None:  # 1-2 probes per x' instead of log2(nkeys) dependent ones
        fn, fn_flip, table = lib.pynqs_eloc_sample_space_hash, lib.pynqs_eloc_sample_space_hash_flip, (ht.table.data_ptr(), ht.nkeys)
    else:
        fn, fn_flip, table = lib.pynqs_eloc_sample_space, lib.pynqs_eloc_sample_space_flip, (keys.data_ptr(), keys.size(0))
    rc = fn(*head, *table, wf.data_ptr(), int(cplx), eloc.data_ptr(), psi0.data_ptr(), st)
    if rc == 0 and flip:
        rc = fn_flip(*head, *table, wf.data_ptr(), int(cplx), psi0.data_ptr(), part.data_ptr(), st)
    N.check(rc, "pynqs_eloc_sample_space")


def choose_sample_space_kernel(x, sorb, nele, noa, nob, plan, WF_LUT, wf, cplx) -> bool:
    """True: key-major (walk the table), False: column-major (walk the excitation lists).  Clear cases by the table size against ncomb;
    in between the two kernels are timed once on up to 1024 of the walkers and the result is remembered per (system, table-size bucket)."""
    dev = x.device

    def probe() -> bool:
        m = min(x.size(0), 1024)
        xs = x[:m].contiguous()
        e = torch.empty(m, dtype=wf.dtype, device=dev)
        p0 = torch.empty(m, dtype=wf.dtype, device=dev)
        stream = torch.cuda.current_stream(dev)
        t = {}
        for mode in (True, False):
            _launch_sample_space(mode, xs, m, sorb, nele, noa, nob, plan, WF_LUT, wf, cplx, False, e, p0, None, stream.cuda_stream)  # warm
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(3):
                _launch_sample_space(mode, xs, m, sorb, nele, noa, nob, plan, WF_LUT, wf, cplx, False, e, p0, None, stream.cuda_stream)
            b.record(stream)
            b.synchronize()
            t[mode] = a.elapsed_time(b)
        return t[True] <= t[False]

    # (the cache key must be the same on every rank: shard sizes are not)
    return _key_major(WF_LUT.bra_key.size(0), sorb, noa, nob, probe, (bool(cplx), x.size(0) >= 1024 if get_world_size() == 1 else None))


def _sample_space_fused(x, h1e, h2e, sorb, nele, noa, nob, WF_LUT, wf: Optional[Tensor] = None, flip: bool = False) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """(sum_k H_k t(x'_k) / t(x), t(x), second sum) with t = the table values `wf` (default: WF_LUT's psi), all in ONE kernel pass
    per sum.  flip: also  sum_k H_k eta_m(x'_k) t(flip(x'_k)) / t(x)  (the projected form's partner term, one more pass)."""
    h1e, h2e = CX.integrals_f64(h1e, h2e)  # float32 integrals: exact up-conversion, the kernels are float64
    plan = CX.plan_for(h1e, h2e, sorb, x.device)
    dev = x.device
    wf = WF_LUT.wf_value if wf is None else wf
    wf = wf.to(torch.complex128 if wf.dtype.is_complex else torch.float64).contiguous()
    cplx = wf.dtype.is_complex
    n = x.size(0)
    eloc = torch.empty(n, dtype=wf.dtype, device=dev)
    psi0 = torch.empty(n, dtype=wf.dtype, device=dev)
    part = torch.empty(n, dtype=wf.dtype, device=dev) if flip else None
    st = torch.cuda.current_stream(dev).cuda_stream
    key_major = choose_sample_space_kernel(x, sorb, nele, noa, nob, plan, WF_LUT, wf, cplx)
    _launch_sample_space(key_major, x, n, sorb, nele, noa, nob, plan, WF_LUT, wf, cplx, flip, eloc, psi0, part, st)
    return eloc, psi0, part


def _emit_kept(x, sorb, nele, noa, nob, plan, code, eps, tile_counts, h_dtype, st):
    """(row, col, onv, h, counts) of the kept records from their counts per (walker, tile) -- by pynqs_reduce_count or _count_sums: prefix
    sums, ONE read-back (the total), the emit."""
    dev, n = x.device, x.size(0)
    ends = torch.cumsum(tile_counts.view(-1), 0, dtype=torch.int64)
    tile_off = (ends - tile_counts.view(-1)).contiguous()
    counts = tile_counts.sum(1, dtype=torch.int64)
    m = int(ends[-1].item()) if n else 0
    col = torch.empty(m, dtype=torch.int32, device=dev)
    onv = torch.empty((m, 8 * ((sorb - 1) // 64 + 1)), dtype=torch.uint8, device=dev)
    h = torch.empty(m, dtype=h_dtype, device=dev)
    row = torch.repeat_interleave(torch.arange(n, device=dev), counts)
    if m:
        N.check(N.lib().pynqs_reduce_emit(x.data_ptr(), n, sorb, nele, noa, nob, plan.data_ptr(), code, eps, tile_off.data_ptr(),
                                          col.data_ptr(), onv.data_ptr(), h.data_ptr(), st), "pynqs_reduce_emit")
    return row, col, onv, h, counts


def _compact_setup(x, h1e, h2e, sorb, nele, noa, nob):
    """What both multi-pass compactions start from: (plan, code of the integrals' type, stream, counts per (walker, tile) to be filled)."""
    plan = CX.plan_for(h1e, h2e, sorb, x.device)
    T = N.lib().pynqs_reduce_tiles(x.size(0), sorb, nele, noa, nob)
    if T < 0:
        raise RuntimeError("pynqs_reduce_tiles: bad arguments")
    code = N.PYNQS_F64 if h1e.dtype == torch.float64 else N.PYNQS_F32
    return plan, code, torch.cuda.current_stream(x.device).cuda_stream, torch.empty((x.size(0), T), dtype=torch.int32, device=x.device)


def reduce_compact(x: Tensor, h1e: Tensor, h2e: Tensor, sorb: int, nele: int, noa: int, nob: int, eps: float, sort: bool = False):
    """Kept columns of the REDUCE method, compacted on the GPU: (row int64[m], col int32[m], onv uint8[m, 8*len],
    h[m], counts int64[n]) with |h| >= eps.  Rows ascend; inside a row the records come in the kernels' reproducible
    tile order (sort=True: ascending columns like the reference's boolean mask, at the price of a sort)."""
    plan, code, st, tile_counts = _compact_setup(x, h1e, h2e, sorb, nele, noa, nob)
    N.check(N.lib().pynqs_reduce_count(x.data_ptr(), x.size(0), sorb, nele, noa, nob, plan.data_ptr(), code, float(eps), tile_counts.data_ptr(), st),
            "pynqs_reduce_count")
    row, col, onv, h, counts = _emit_kept(x, sorb, nele, noa, nob, plan, code, float(eps), tile_counts, h1e.dtype, st)
    if sort and col.numel():
        order = torch.argsort((row << 32) | col.long())
        col, onv, h = col[order], onv[order], h[order]
    return row, col, onv, h, counts


def reduce_compact_sampled(x: Tensor, h1e: Tensor, h2e: Tensor, sorb: int, nele: int, noa: int, nob: int, eps: float, eps_sample: int,
                           seed: Optional[int] = None):
    """The semi-stochastic selection of vmc/energy/eloc.py:257-296 without the [n, ncomb] matrices.
    Returns (kept, sampled): kept = (row, col, onv, h, counts) of the columns with |h| >= eps (empty when eps <= 0:
    the reference then draws from all columns), sampled = (row, col, onv, w, counts) with one record per distinct
    drawn column and w = (hits / eps_sample) * sign(h) * S_row, S_row = sum of the sub-eps |h| of the row.
    The draws over the tiles of a row come from torch.multinomial, the ones inside a tile from a counter-based
    generator in the kernel seeded with `seed` (default: drawn from torch's generator)."""
    plan, code, st, tile_counts = _compact_setup(x, h1e, h2e, sorb, nele, noa, nob)
    dev, lib, (n, T), L = x.device, N.lib(), tile_counts.shape, (sorb - 1) // 64 + 1
    eps_eff = float(eps) if eps > 0.0 else float("inf")
    tile_sums = torch.empty((n, T), dtype=torch.float64, device=dev)
    N.check(lib.pynqs_reduce_count_sums(x.data_ptr(), n, sorb, nele, noa, nob, plan.data_ptr(), code, eps_eff, tile_counts.data_ptr(),
                                        tile_sums.data_ptr(), st), "pynqs_reduce_count_sums")
    kept = _emit_kept(x, sorb, nele, noa, nob, plan, code, eps_eff, tile_counts, h1e.dtype, st)   # (same records as reduce_compact)
    # draws over the tiles, then inside the tiles
    S = tile_sums.sum(1)
    live = S > 0
    probs = torch.where(live.unsqueeze(1), tile_sums, torch.ones_like(tile_sums))
    ids = torch.multinomial(probs, eps_sample, replacement=True)
    flat_ids = (ids + torch.arange(n, device=dev).unsqueeze(1) * T).view(-1)
    tile_draws = torch.bincount(flat_ids, minlength=n * T).view(n, T).to(torch.int32)  # (scatter_add_ here: 0.6 ms of atomics)
    tile_draws = (tile_draws * live.unsqueeze(1).to(torch.int32)).contiguous()
    d_ends = torch.cumsum(tile_draws.view(-1), 0, dtype=torch.int64)
    sample_off = (d_ends - tile_draws.view(-1)).contiguous()
    total = n * eps_sample  # upper bound; rows with S == 0 leave their slots unused
    s_col = torch.full((total,), -1, dtype=torch.int32, device=dev)
    s_onv = torch.empty((total, 8 * L), dtype=torch.uint8, device=dev)
    s_h = torch.empty(total, dtype=h1e.dtype, device=dev)
    scale = (S / eps_sample).contiguous()
    if seed is None:
        seed = _draw_seed()
    N.check(lib.pynqs_reduce_sample(x.data_ptr(), n, sorb, nele, noa, nob, plan.data_ptr(), code, eps_eff, tile_draws.data_ptr(),
                                    sample_off.data_ptr(), scale.data_ptr(), seed, s_col.data_ptr(), s_onv.data_ptr(), s_h.data_ptr(), st),
            "pynqs_reduce_sample")
    # slot k belongs to the walker whose draws cover it
    draws_per_row = tile_draws.sum(1, dtype=torch.int64)
    slot_row = torch.repeat_interleave(torch.arange(n, device=dev), draws_per_row)
    used = int(d_ends[-1].item()) if n else 0
    valid = s_col[:used] >= 0
    keep = torch.nonzero(valid).squeeze(1)  # one compaction for the four arrays
    s_row = slot_row[keep]
    # records per walker: a segmented sum over its slot range (scatter_add_ here: 0.6 ms of atomics on 5 M rows)
    s_counts = _segment_sum(valid.to(torch.float64), draws_per_row).to(torch.int64) if used else \
        torch.zeros(n, dtype=torch.int64, device=dev)
    return kept, (s_row, s_col[keep], s_onv[keep], s_h[keep], s_counts)

# ---- REDUCE through the one-launch front end ---------------------------------------------------------------------------------
_FRONTS: "dict[tuple, RF.ReduceFrontEnd]" = {}
_MAX_FRONTS = 6


def _draw_seed() -> int:
    """from torch's host generator (reproducible after torch.manual_seed), decorrelated between the ranks: after the usual
    manual_seed(seed) every rank's generator is in the same state, and the kernels' streams are keyed by (seed, walker, tile, k)"""
    s = int(torch.randint(0, 2**62, (1,)).item())
    r = get_rank()
    return (s ^ ((r + 1) * 0x9E3779B97F4A7C15)) & (2**63 - 1) if r else s


class _FrontDense(RuntimeError):
    """a long row kept more records than the one-launch front end's LDS list holds: the caller takes the multi-pass path"""

    def __init__(self) -> None:
        super().__init__("rows of this system keep more records per segment than the one-launch REDUCE front end's LDS list holds: "
                         "reduce_compact / reduce_compact_sampled serve them faster (energy.FRONT_ROUTE = False forces the one-launch form)")


def _dense_key(device, sorb, nele, noa, nob, eps_sample) -> tuple:
    return (str(device), sorb, nele, noa, nob, int(eps_sample) > 0)


def _long_row_cap(n, h1e, sorb, nele, noa, nob, eps_sample) -> Optional[int]:
    """None on rows the one-launch front end serves in either form; else the cap_doubles up to which it is used (-1: never)"""
    if not FRONT_ROUTE or not RF.plan(n, sorb, nele, noa, nob, int(eps_sample), h1e.dtype).long_row:
        return None
    return RF.list_capacity(n, sorb, nele, noa, nob, int(eps_sample), h1e.dtype)


def _nodedup_key(device, n, sorb, nele, noa, nob, eps_sample, eps=None) -> tuple:
    return (str(device), int(n), sorb, nele, noa, nob, int(eps_sample), None if eps is None else float(eps))


def _new_front(n, x, h1e, sorb, nele, noa, nob, eps_sample, pm1_dtype, want_pm1, cap_d=None, cap_u=None, dedup=True):
    if not dedup and cap_d is not None and cap_d > RF.list_capacity(n, sorb, nele, noa, nob, int(eps_sample), h1e.dtype, without_table=True):
        dedup = True   # (only the LIST forms of the kernel run without the table)
    if cap_d is None:
        nseg, fixed, _, _ = RF.geometry(n, sorb, nele, noa, nob, eps_sample)
        ncomb = get_Num_SinglesDoubles(sorb, noa, nob) + 1
        per_seg = (ncomb * max(n, 1) + max(nseg, 1) - 1) // max(nseg, 1)
        cap_d, cap_u = min(per_seg, max(64, per_seg // 32)), max(4096, 32 * n)
        limit = _long_row_cap(n, h1e, sorb, nele, noa, nob, eps_sample)
        if limit is not None and limit >= 0:
            cap_d = min(cap_d, limit)   # (long rows: start in the LIST form; reduce_front_finish leaves the path if that overflows)
    return RF.ReduceFrontEnd(n, sorb, nele, noa, nob, eps_sample, h1e.dtype, x.device, cap_d, cap_u, pm1_dtype, want_pm1=want_pm1, dedup=dedup)


@dataclass(slots=True)
class _FrontTicket:
    """one enqueued front-end launch (reduce_front_launch), for reduce_front_finish: the workspace and its cache key, the counters' pinned
    host copy and the event behind it, and the call's arguments (an overflow repeats the call)"""
    fe: RF.ReduceFrontEnd
    key: tuple
    host: Tensor
    ev: torch.cuda.Event
    x: Tensor
    plan: object
    h1e: Tensor
    system: tuple   # (sorb, nele, noa, nob)
    eps: float
    eps_sample: int
    seed: int
    lut: object
    pm1_dtype: torch.dtype
    want_pm1: bool
    route: bool


def reduce_front_launch(x: Tensor, h1e: Tensor, h2e: Tensor, sorb: int, nele: int, noa: int, nob: int, eps: float, eps_sample: int = 0,
                        lut=None, seed: Optional[int] = None, pm1_dtype: Optional[torch.dtype] = None, want_pm1: bool = True, slot: int = 0,
                        route: bool = False, consumer=None):
    """Enqueue the fused REDUCE front end for the walkers x on the CURRENT stream (buffers cached per (device, batch size, system,
    eps_sample, slot)) together with an asynchronous copy of its counters to pinned host memory; returns a ticket for reduce_front_finish.
    Nothing is waited for: a caller can enqueue the front end of the NEXT chunk of walkers on a second stream while the ansatz works on
    the current one (total_energy does: SURVEY 7.6).
    route (local_energy's calls): on rows of more than FRONT_LONG_ROW columns reduce_front_finish raises _FrontDense instead of growing the
    buffers past the front end's LDS list (the multi-pass path is the faster one there); a direct caller gets the front end regardless."""
    plan = CX.plan_for(h1e, h2e, sorb, x.device)
    n = x.size(0)
    pm1_dtype = pm1_dtype or (torch.float32 if torch.get_default_dtype() == torch.float32 else torch.float64)
    key = (str(x.device), n, sorb, nele, noa, nob, int(eps_sample), h1e.dtype, pm1_dtype, bool(want_pm1), int(slot), bool(route))
    with _LOCK:
        fe = _FRONTS.pop(key, None)
    caps = None
    if route and FRONT_NODEDUP:
        nk = _nodedup_key(x.device, n, sorb, nele, noa, nob, eps_sample, eps)
        if _FRONT_NODEDUP.get(nk) is not None and slot == 0:
            # (only the table-less state is revisited: being stuck WITH a table costs probes, being stuck without one costs an ansatz
            # evaluation per duplicate; counting the records of a call is a read-back of its own)
            _FRONT_NODEDUP_CALLS[nk] = _FRONT_NODEDUP_CALLS.get(nk, 0) + 1
            if _FRONT_NODEDUP_CALLS[nk] >= FRONT_NODEDUP_RECHECK:   # measure again: this call runs with the table and counts
                _FRONT_NODEDUP.pop(nk)
                _FRONT_NODEDUP_CALLS[nk] = 0
        caps = _FRONT_NODEDUP.get(nk)
    if fe is not None and fe.dedup == (caps is not None):
        # (a workspace from before the decision to drop the table, e.g. the second slot of total_energy's look-ahead; or a table-less one
        # when the decision is measured again: that call must run WITH the table, else reduce_front_finish has nothing to count)
        fe = None
    if fe is None:
        fe = _new_front(n, x, h1e, sorb, nele, noa, nob, eps_sample, pm1_dtype, want_pm1, *(caps or (None, None)), dedup=caps is None)
    if seed is None:
        seed = _draw_seed() if eps_sample > 0 else 0
    if consumer is not None:
        fe.record_stream(consumer)  # (the caller launches on one stream and reads the workspace on another)
    fe.run(x, plan.buf, eps, seed, lut)
    host = torch.empty(4, dtype=torch.int32, pin_memory=True)
    host.copy_(fe.counters, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(x.device))
    return _FrontTicket(fe=fe, key=key, host=host, ev=ev, x=x, plan=plan, h1e=h1e, system=(sorb, nele, noa, nob), eps=eps, eps_sample=eps_sample,
                        seed=seed, lut=lut, pm1_dtype=pm1_dtype, want_pm1=want_pm1, route=route)


def reduce_front_finish(t: _FrontTicket):
    """(front end, number of distinct x') of a ticket: waits for THAT launch only (its event), grows the buffers and repeats the call on
    the current stream if it reported an overflow."""
    t.ev.synchronize()
    fe, x, n, system = t.fe, t.x, t.x.size(0), t.system
    cnt = tuple(int(v) for v in t.host.tolist()[:3])
    while fe.overflowed(cnt):
        nu, flags, mx = cnt
        cap_d = max(fe.cap_doubles, int(mx * 1.25) + 16) if mx > fe.cap_doubles else fe.cap_doubles
        cap_u = fe.cap_unique
        limit = _long_row_cap(n, t.h1e, *system, t.eps_sample) if t.route else None
        if limit is not None and cap_d > limit:
            _FRONT_DENSE.add(_dense_key(x.device, *system, t.eps_sample))
            raise _FrontDense()
        if flags & RF.OVERFLOW_TABLE:
            cap_u = max(4 * cap_u, int(nu * 1.5))   # (the kernel stops inserting once the table is full: nu is a lower bound then)
        elif nu > cap_u:
            cap_u = int(nu * 1.25) + 1024
        fe = _new_front(n, x, t.h1e, *system, t.eps_sample, t.pm1_dtype, t.want_pm1, cap_d, cap_u, dedup=fe.dedup)
        fe.run(x, t.plan.buf, t.eps, t.seed, t.lut)
        cnt = fe.counters_host()
    nk = _nodedup_key(x.device, n, *system, t.eps_sample, t.eps)
    if t.route and FRONT_NODEDUP and fe.dedup and nk not in _FRONT_NODEDUP:
        # the first call for this system and batch size: how many of the records were distinct?  (one more read-back, once)
        records = fe.count_records()
        list_ok = fe.cap_doubles <= RF.list_capacity(n, *system, int(t.eps_sample), t.h1e.dtype, without_table=True)
        drop = bool(list_ok and t.lut is None and cnt[0] > FRONT_NODEDUP_RATIO * records)
        _LOG.info("REDUCE front end, sorb %d, %d walkers, eps %g: %d of %d records distinct -> %s", system[0], n, t.eps, cnt[0], records,
                  "no de-duplication table from now on" if drop else "de-duplication table kept")
        if drop:
            _FRONT_NODEDUP[nk] = (fe.cap_doubles, int(records * 1.05) + 4096)
            return fe, cnt[0]   # (not kept: the next call builds the table-less front end)
        _FRONT_NODEDUP[nk] = None
    with _LOCK:
        _FRONTS[t.key] = fe  # (most recently used last)
        while len(_FRONTS) > _MAX_FRONTS:
            _FRONTS.pop(next(iter(_FRONTS)))
    return fe, cnt[0]


def reset_caches() -> None:
    """Drop every process-wide cache of this module: front-end workspaces, the table / no-table and front-end / multi-pass decisions,
    timed kernel choices.  (Results never depend on them; which FORM of a kernel a call takes does.)"""
    with _LOCK:
        _FRONTS.clear(); _FRONT_NODEDUP.clear(); _FRONT_NODEDUP_CALLS.clear(); _FRONT_DENSE.clear(); _SS_CHOICE.clear(); _AUTO_NBATCH.clear()


def reduce_front(x: Tensor, h1e: Tensor, h2e: Tensor, sorb: int, nele: int, noa: int, nob: int, eps: float, eps_sample: int = 0,
                 lut=None, seed: Optional[int] = None, pm1_dtype: Optional[torch.dtype] = None, want_pm1: bool = True, route: bool = False):
    """Run the fused REDUCE front end on the walkers x (vmc/energy/eloc.py:243-298 + flip.py:29-63 in one launch) and return
    (front end, number of distinct x').  Buffers are cached per (device, batch size, system, eps_sample) and grown when a call
    reports that it needed more (the call is then repeated); ONE device-to-host read per call, after the kernel has been enqueued."""
    return reduce_front_finish(reduce_front_launch(x, h1e, h2e, sorb, nele, noa, nob, eps, eps_sample, lut, seed, pm1_dtype, want_pm1, route=route))


def _rbm_forward_params(ansatz, dtype):
    """(weights, hidden bias, visible bias, kind) if the forward kernels (pynqs_rbm_forward[_children]) give this ansatz' amplitudes in
    `dtype`: a real RBM whose flavour matches dtype (pRBM is complex-valued, the others real), else an RBM with complex parameters -- not
    "cos" -- with a complex dtype, else a Jastrow-RBM with a real dtype: kind "jastrow" and two more entries, M and its JastrowTable
    (pynqs_jrbm_forward, pynqs_rbm_forward_children + pynqs_jastrow_children_apply); else None.  THE place that decides it: once per
    local_energy call / per look-ahead of total_energy."""
    rp = _real_rbm_params(ansatz)
    if rp is not None and dtype.is_complex == (rp[3] == "pRBM"):
        return rp
    cp = _complex_rbm_params(ansatz) if rp is None and dtype.is_complex else None
    if cp is not None:
        return None if cp[4] else (cp[0], cp[1], cp[2], "complex")
    jp = _jastrow_rbm_params(ansatz) if rp is None and not dtype.is_complex else None
    if jp is None or N.lib().pynqs_jastrow_table_bytes(jp[3].size(0)) < 0:
        return None
    return jp[0], jp[1], jp[2], "jastrow", jp[3], _jastrow_table_for(getattr(ansatz, "module", ansatz).jastrow, jp[3])


_JTABLE = threading.local()  # .value: (total_energy call token, M's storage, M's version, JastrowTable): one table per total_energy call


def _jastrow_table_for(param: Tensor, M: Tensor):
    """The JastrowTable of M (float64, detached; param: the module's own tensor, whose version counter tells an update).  Inside a
    total_energy call the table of the first chunk serves every chunk and the look-ahead; a direct local_energy call builds its own."""
    token = _call_token()
    key = (token, param.data_ptr(), CX._ver(param), str(param.device))
    hit = getattr(_JTABLE, "value", None)
    if token is not None and key[2] >= 0 and hit is not None and hit[0] == key:
        return hit[1]
    table = CX.JastrowTable(M)
    _JTABLE.value = (key, table) if token is not None else None
    return table


def _reduce_front_options(ansatz, WF_LUT, dtype, use_multi_psi, use_spin_flip):
    """(wave-function hash table asked inside the kernel or None, _rbm_forward_params if the amplitudes of the distinct x' come from
    pynqs_rbm_forward, else None) for local_energy's REDUCE path -- one definition for local_energy and for total_energy's look-ahead."""
    plain = not (use_multi_psi or use_spin_flip)
    # the table is asked inside the kernel when it has a GPU hash table and psi is all that is needed on x' (f of the multi-psi
    # form has no table; the projected forms look flip(x') up as well): otherwise on the distinct rows
    ht = getattr(WF_LUT, "hashtable", None) if (WF_LUT is not None and plain) else None
    # an RBM of the reference's family gets its amplitudes on the distinct x' from the packed bits (pynqs_rbm_forward): no +-1 rows
    if not FUSED_RBM or use_multi_psi or (WF_LUT is not None and ht is None):
        return ht, None
    return ht, _rbm_forward_params(ansatz, dtype)


def _rbm_ahead(ticket, x, rbm, lut, dtype, sorb, other_stream: bool):
    """(front end, eloc, psi(x)) with the RBM amplitudes of the distinct x' (from their parent walkers, device-side row count) and the
    contraction enqueued behind the front end of `ticket` without waiting for its counters; None when the sizes do not allow it.
    rbm: _rbm_forward_params of the ansatz."""
    fe = ticket.fe
    W, hb, vb, kind = rbm[:4]
    jastrow = kind == "jastrow"
    if not (RBM_FROM_PARENTS and (CX.jrbm_forward_children_supported(sorb, W.size(0)) if jastrow
                                  else CX.rbm_forward_children_supported(sorb, W.size(0), kind))):
        return None
    if other_stream:   # (total_energy's look-ahead enqueued the front end on its second stream)
        torch.cuda.current_stream(x.device).wait_event(ticket.ev)
    if jastrow:
        psi_u = CX.jrbm_forward_children(fe.uniq_onv, fe.uniq_parent, x, W, hb, vb, rbm[4], sorb, count=fe.counters, jastrow_table=rbm[5]).to(dtype)
    else:
        psi_u = CX.rbm_forward_children(fe.uniq_onv, fe.uniq_parent, x, W, hb, vb, sorb, kind, count=fe.counters).to(dtype)
    eloc, psi_x = fe.contract(psi_u, lut.wf_value if lut is not None else None)
    return fe, eloc, psi_x


def _front_ok(x, h1e, sorb, nele, noa, nob, eps_sample) -> bool:
    if not (FUSED and FUSED_ONEPASS and x.is_cuda and sorb % 2 == 0 and h1e.dtype in (torch.float64, torch.float32)
            and (eps_sample == 0 or FUSED_SAMPLED) and RF.supported(x.size(0), sorb, nele, noa, nob, int(eps_sample))):
        return False
    limit = _long_row_cap(x.size(0), h1e, sorb, nele, noa, nob, eps_sample)
    if limit is None:
        return True
    if int(eps_sample) > 0 and x.size(0) < FRONT_SAMPLED_MIN_WALKERS:
        return False   # (one workgroup per walker: 256 walkers at sorb 184 19.5 ms against 15.4 multi-pass; 1024 walkers 56 against 63)
    return limit >= 0 and _dense_key(x.device, sorb, nele, noa, nob, eps_sample) not in _FRONT_DENSE


def _segment_sum(values: Tensor, lengths: Tensor) -> Tensor:
    """sums over consecutive segments of `values` (a walker's records are contiguous): a segmented sum instead of index_add_ (atomics: 2.7 of
    5.0 ms on Fe2S2); complex values through their (re, im) view"""
    if values.is_complex():
        return torch.view_as_complex(torch.segment_reduce(torch.view_as_real(values).contiguous(), "sum", lengths=lengths, unsafe=True))
    return torch.segment_reduce(values, "sum", lengths=lengths, unsafe=True)


def _projected_t(c, onv: Tensor, psi: Tensor, f: Optional[Tensor]) -> Tensor:
    """The projected / multi-psi factor on records or distinct rows `onv` (flip.py:153-319):
        T = f psi + eta eta_m(x') f(flip x') psi(flip x')        (f = 1 without multi-psi, no second term without the projection)
    from psi (and f, multi-psi) on them.  The callers apply conj(f(x)) / N^2: per walker after the front end's contraction, per record on
    the multi-pass path -- two orders of the same product, which this function leaves to them."""
    t = f * psi if c.use_multi_psi else psi
    if c.use_spin_flip:
        onv_flip = spin_flip_onv(onv, c.sorb)
        psi_flip = Func(c.ansatz_f, onv_flip, c.WF_LUT, c.use_unique).to(c.dtype)
        if c.use_multi_psi:
            psi_flip = Func(c.ansatz_extra, onv_flip, None, c.use_unique).to(c.dtype) * psi_flip
        t = t + SpinProjection.eta * spin_flip_sign(onv, c.sorb) * psi_flip
    return t


def _f_on_keys(c) -> Tensor:
    """f on the sample-space keys (the reference stores f in the table's dtype, flip.py:392): once per parameter state, not once
    per chunk of walkers -- total_energy calls local_energy for every chunk, and the table has up to 1e5-1e6 keys"""
    WF_LUT, extra = c.WF_LUT, c.ansatz.module.extra
    # valid within ONE total_energy call (its token): parameters updated through `p.data.add_` -- the reference's own GD step,
    # vmc/optim/_base.py:619 -- keep their version counters, so nothing across calls proves that f is still current
    stamp = (id(extra), WF_LUT.bra_key.data_ptr(), WF_LUT.bra_key.size(0), str(WF_LUT.dtype), _call_token())
    cached = getattr(WF_LUT, "_pynqs_f_keys", None)
    if cached is not None and cached[0] == stamp and stamp[4] is not None:
        return cached[1]
    f_keys = Func(partial(c.ansatz_batch, func=extra), WF_LUT.bra_key, None, True).to(WF_LUT.dtype)
    try:
        WF_LUT._pynqs_f_keys = (stamp, f_keys)
    except AttributeError:  # (a table object that takes no attributes)
        pass
    return f_keys


def _in_sample_space(c, h1, h2, f_keys):
    """(sum over the sample space with the integrals (h1, h2), psi(x)): the energy, and with the S-S+ integrals <S-S+> (eloc.py:377-400)"""
    x, WF_LUT = c.x, c.WF_LUT
    if not (c.use_multi_psi or c.use_spin_flip):
        e1, p0, _ = _sample_space_fused(x, h1, h2, *c.system, WF_LUT)
        return e1, p0
    # projected / multi-psi forms (flip.py:322-418, eloc.py:381-392) on the same kernel:
    #   E_loc = conj(f(x)) [ sum_k H_k (f psi)(x'_k) + eta sum_k H_k eta_m(x'_k) (f psi)(flip x'_k) ] / (N^2 psi(x))
    # (f psi) is a table over the sample space
    wf = WF_LUT.wf_value * f_keys if c.use_multi_psi else WF_LUT.wf_value
    e1, p0, part = _sample_space_fused(x, h1, h2, *c.system, WF_LUT, wf, c.use_spin_flip)
    if c.use_spin_flip:
        e1 = e1 + SpinProjection.eta * part
    if c.use_multi_psi:
        # t(x) = f(x) psi(x): back to sum / psi(x) and the reference's factor conj(f(x)); psi(x), f(x) from the table
        # (pynqs_amd's table answers through its hash table; the reference's own WavefunctionLUT class has no `find`)
        pos, found = WF_LUT.find(x) if hasattr(WF_LUT, "find") else CX.wavefunction_lut(WF_LUT.bra_key, x, c.sorb)
        pos = pos.clamp_min(0)
        p0 = torch.where(found, WF_LUT.wf_value[pos], torch.zeros((), dtype=WF_LUT.dtype, device=x.device))
        f_x = torch.where(found, f_keys[pos], torch.zeros((), dtype=f_keys.dtype, device=x.device))
        e1 = e1 * f_x * f_x.conj()
    return e1 / c.extra_norm**2, p0


def _eloc_sample_space_fused(c):
    """SAMPLE_SPACE in one kernel per sum (every form)."""
    f_keys = _f_on_keys(c) if c.use_multi_psi else None
    eloc, psi0 = _in_sample_space(c, c.h1e, c.h2e, f_keys)
    sloc = _in_sample_space(c, c.h1e_spin, c.h2e_spin, f_keys)[0] if c.use_spin_raising else torch.zeros_like(eloc)
    t1 = time.time_ns()
    return eloc.to(c.dtype), sloc.to(c.dtype), psi0.to(c.dtype), ((t1 - c.t0) / 1e6, 0.0, 0.0)


def _eloc_simple_rbm(c):
    """SIMPLE with an RBM: amplitude ratios on chip.  None: not such an RBM / `dtype` is not its own / its parameters do not fit the LDS.
    use_spin_flip (flip.py, _simple_flip): the real-parameter flavours and the Jastrow-RBM run the plain pass, the signed pass on the
    spin-mirrored tables and the combine kernel (pynqs_eloc_rbm_flip / pynqs_eloc_jrbm_flip); complex parameters and "cos" decline."""
    x, dtype, system = c.x, c.dtype, c.system
    flip = c.use_spin_flip
    prm = _real_rbm_params(c.ansatz)
    cprm = _complex_rbm_params(c.ansatz) if prm is None and not flip else None
    jprm = _jastrow_rbm_params(c.ansatz) if prm is None and cprm is None else None
    # the phase flavour (pRBM) is complex-valued; the others need a real `dtype` like the module itself
    if (prm is not None and dtype in ((torch.complex128, torch.complex64) if prm[3] == "pRBM" else (torch.double, torch.float32))
            and _rbm_lds_ok(*system, prm[0].size(0))):
        table, run, psi_kw = CX.RBMTable(*prm[:3]), partial(CX.eloc_rbm, rbm_type=prm[3]), {}
        if flip:   # (the mirrored table belongs to the same parameter state: built wherever the plain one is)
            mirror = CX.mirrored_rbm_table(*prm[:3])
            run = lambda x, h1, h2, tab, *sys, **kw: CX.eloc_rbm_flip(x, h1, h2, tab, mirror, *sys, SpinProjection.eta, c.extra_norm,  # noqa: E731
                                                                      rbm_type=prm[3], **kw)
    # complex parameters (complex running products in the kernel); "cos" is real-valued and rides on the same kernel
    elif (cprm is not None and dtype in ((torch.double, torch.float32) if cprm[4] else (torch.complex128, torch.complex64))
            and N.lib().pynqs_eloc_crbm_supported(*system, cprm[0].size(0))):
        table, run, psi_kw = CX.CRBMTable(*cprm[:3]), CX.eloc_crbm, dict(log_scale=cprm[3])
    # a real RBM times a two-body Jastrow factor: the real kernel with the pair factors (pynqs_eloc_jrbm), real-valued
    elif jprm is not None and dtype in (torch.double, torch.float32) and CX.eloc_jrbm_supported(*system, jprm[0].size(0)):
        jtable = CX.JastrowTable(jprm[3])
        table, psi_kw = CX.RBMTable(*jprm[:3]), {}
        run = lambda x, h1, h2, tab, *sys, **kw: CX.eloc_jrbm(x, h1, h2, tab, jtable, *sys, **kw)  # noqa: E731
        if flip:
            mirror, jmirror = CX.mirrored_rbm_table(*jprm[:3]), CX.mirrored_jastrow_table(jprm[3])
            run = lambda x, h1, h2, tab, *sys, **kw: CX.eloc_jrbm_flip(x, h1, h2, tab, jtable, mirror, jmirror, *sys, SpinProjection.eta,  # noqa: E731
                                                                       c.extra_norm, **kw)
    else:
        return None
    eloc, psi0 = run(x, *CX.integrals_f64(c.h1e, c.h2e), table, *system, **psi_kw)
    # <S-S+> (eloc.py:173-188): the same kernel with the S-S+ integrals
    sloc = run(x, *CX.integrals_f64(c.h1e_spin, c.h2e_spin), table, *system, want_psi=False)[0] if c.use_spin_raising else torch.zeros_like(eloc)
    if cprm is not None and cprm[4]:
        eloc, sloc, psi0 = eloc.real, sloc.real, psi0.real
    t1 = time.time_ns()
    return eloc.to(dtype), sloc.to(dtype), psi0.to(dtype), ((t1 - c.t0) / 1e6, 0.0, 0.0)


def _on_distinct(c, fe, nu, fn, lut) -> Tensor:
    """a function of the determinant on the distinct x' (the +-1 rows the kernel wrote are the module's input already)"""
    if lut is not None:
        return Func(fn, fe.uniq_onv[:nu], lut, False).to(c.dtype)
    takes_rows = fe.uniq_pm1 is not None and getattr(c.ansatz_batch, "accepts_pm1_rows", False) and fe.pm1_dtype == torch.get_default_dtype()
    return fn(fe.uniq_pm1[:nu] if takes_rows else fe.uniq_onv[:nu]).to(c.dtype)


def _rbm_on_distinct(c, fe, nu, rbm) -> Tensor:
    """psi on the distinct x' by one kernel (rbm: _rbm_forward_params).  Every distinct x' is its parent walker with <= 4 orbitals flipped
    (the front end notes the parent): theta(x') from theta(x) by 4 updates per hidden unit when the parameters fit the LDS, else from scratch"""
    W, hb, vb, kind = rbm[:4]
    if kind == "jastrow":  # the RBM's children kernel, then the Jastrow factor from the parents; else both from scratch in one kernel
        if RBM_FROM_PARENTS and CX.jrbm_forward_children_supported(c.sorb, W.size(0)):
            return CX.jrbm_forward_children(fe.uniq_onv[:nu], fe.uniq_parent, c.x, W, hb, vb, rbm[4], c.sorb, jastrow_table=rbm[5]).to(c.dtype)
        return CX.jrbm_forward(fe.uniq_onv[:nu], W, hb, vb, rbm[4], c.sorb).to(c.dtype)
    if RBM_FROM_PARENTS and CX.rbm_forward_children_supported(c.sorb, W.size(0), kind):
        return CX.rbm_forward_children(fe.uniq_onv[:nu], fe.uniq_parent, c.x, W, hb, vb, c.sorb, kind).to(c.dtype)
    return CX.rbm_forward(fe.uniq_onv[:nu], W, hb, vb, c.sorb, kind).to(c.dtype)


def _front_spin_raising(c, fe, amp_u, tab, num_over_psi) -> Tensor:
    """<S-S+> over the front end's records (eloc.py:250-310: the raw S-S+ matrix elements, also on the drawn columns); amp_u: psi (plain
    form, num_over_psi None) or T on the distinct x'"""
    x = c.x
    xs = x if fe.nchunks == 1 else x.repeat_interleave(fe.nchunks, 0)
    hs = get_hij_torch(xs, fe.rec_onv.view(fe.nseg, fe.stride, -1), c.h1e_spin, c.h2e_spin, c.sorb, c.nele).reshape(-1).to(fe.h_dtype)
    hs_s = get_hij_torch(x, fe.srec_onv.view(x.size(0), fe.eps_sample, -1), c.h1e_spin, c.h2e_spin, c.sorb, c.nele).reshape(-1).to(fe.h_dtype) \
        if fe.eps_sample else None
    if num_over_psi is None:
        return fe.contract(amp_u, tab, rec_w=hs, srec_w=hs_s)[0]
    return fe.contract(amp_u, None, divide=False, rec_w=hs, srec_w=hs_s)[0] * num_over_psi


def _eloc_reduce_front(c):
    """REDUCE through the one-launch front end (deterministic and semi-stochastic, every form).  None: a long row kept more records than
    the front end's LDS list holds (_FrontDense) -- the multi-pass paths serve the system, from now on."""
    dtype = c.dtype
    ht, rbm = _reduce_front_options(c.ansatz, c.WF_LUT, dtype, c.use_multi_psi, c.use_spin_flip)
    plain = not (c.use_multi_psi or c.use_spin_flip)
    ahead = None
    try:
        ticket = c.front_ticket
        if ticket is None:
            ticket = reduce_front_launch(c.x, c.h1e, c.h2e, *c.system, c.eps, int(c.eps_sample), ht, want_pm1=rbm is None, route=True)
        if rbm is not None and SPECULATE_RBM and plain and not c.use_spin_raising:
            # An RBM of the reference's family needs nothing from the host between the front end and the contraction: the amplitude
            # kernel takes the number of distinct x' from the device, so both are enqueued BEFORE the counters are waited for (the wait
            # + two launches used to leave the GPU idle for ~0.2 ms of a 1 ms call).  Used if the counters then report no overflow.
            ahead = _rbm_ahead(ticket, c.x, rbm, c.WF_LUT if ht is not None else None, dtype, c.sorb, c.front_ticket is not None)
        fe, nu = reduce_front_finish(ticket)
    except _FrontDense:
        return None
    t2 = time.time_ns()
    if ahead is not None and ahead[0] is fe:
        eloc, psi_x = ahead[1], ahead[2]
        return eloc.to(dtype), torch.zeros_like(eloc).to(dtype), psi_x.to(dtype), ((t2 - c.t0) / 1e6, 0.0, 0.0)
    psi_u = _rbm_on_distinct(c, fe, nu, rbm) if rbm is not None else _on_distinct(c, fe, nu, c.ansatz_f, c.WF_LUT if ht is None else None)
    tab = c.WF_LUT.wf_value if ht is not None else None
    if plain:
        amp_u, num_over_psi = psi_u, None
        eloc, psi_x = fe.contract(psi_u, tab)
    else:
        # projected / multi-psi forms: E_loc = conj(f(x)) sum_k w_k T(x'_k) / (N^2 psi(x)), T per distinct x'
        f_u = _on_distinct(c, fe, nu, c.ansatz_extra, None) if c.use_multi_psi else None
        amp_u = _projected_t(c, fe.uniq_onv[:nu], psi_u, f_u)
        num, _ = fe.contract(amp_u, None, divide=False)
        _, psi_x = fe.contract(psi_u, None, divide=False)
        scale = 1.0 / c.extra_norm**2
        if c.use_multi_psi:
            scale = scale * fe.contract(f_u, None, divide=False)[1].conj()
        num_over_psi = scale / psi_x
        eloc = num * num_over_psi
    sloc = _front_spin_raising(c, fe, amp_u, tab, num_over_psi) if c.use_spin_raising else torch.zeros_like(eloc)
    t3 = time.time_ns()
    return eloc.to(dtype), sloc.to(dtype), psi_x.to(dtype), ((t2 - c.t0) / 1e6, 0.0, (t3 - t2) / 1e6)


def _eloc_reduce_multipass(c):
    """REDUCE (deterministic) with on-chip compaction in several passes: rows too long for the one-launch front end.  Also the spin-flip
    projected and multi-psi forms (flip.py:200-319): their extra factors are evaluated on the kept records only."""
    x, dtype = c.x, c.dtype
    row, col, onv, h, counts = reduce_compact(x, c.h1e, c.h2e, *c.system, c.eps)
    t2 = time.time_ns()
    first = col == 0

    def at_x(v: Tensor) -> Tensor:
        """value on the kept column 0 of each row; 0 if it was filtered out (as in the reference)"""
        out = torch.zeros(x.size(0), dtype=dtype, device=x.device)
        out[row[first]] = v[first]
        return out

    psi = Func(c.ansatz_f, onv, c.WF_LUT, c.use_unique).to(dtype)
    psi_x = at_x(psi)
    f = Func(c.ansatz_extra, onv, None, c.use_unique).to(dtype) if c.use_multi_psi else None
    t = _projected_t(c, onv, psi, f)
    if c.use_multi_psi:
        t = t * at_x(f).conj()[row]
    if c.use_multi_psi or c.use_spin_flip:
        t = t / c.extra_norm**2
    ratio = t / psi_x[row]
    eloc = _segment_sum(ratio * h.to(_real_dtype(dtype)), counts)
    if c.use_spin_raising:
        # <S-S+> over the same kept columns (eloc.py:250-310): its matrix elements for the (x, x') pairs of the records
        h_spin = get_hij_torch(x[row].contiguous(), onv.unsqueeze(1), c.h1e_spin, c.h2e_spin, c.sorb, c.nele).reshape(-1)
        sloc = _segment_sum(ratio * h_spin.to(_real_dtype(dtype)), counts)
    else:
        sloc = torch.zeros_like(eloc)
    t3 = time.time_ns()
    return eloc.to(dtype), sloc.to(dtype), psi_x, ((t2 - c.t0) / 1e6, 0.0, (t3 - t2) / 1e6)


def _eloc_reduce_multipass_sampled(c):
    """Semi-stochastic REDUCE (eps_sample > 0) with the selection done on chip, in several passes (plain form only)."""
    x, dtype = c.x, c.dtype
    (row, col, onv, h, counts), (s_row, s_col, s_onv, s_w, s_counts) = reduce_compact_sampled(x, c.h1e, c.h2e, *c.system, c.eps, int(c.eps_sample))
    t2 = time.time_ns()
    psi_all = Func(c.ansatz_f, torch.cat([onv, s_onv]), c.WF_LUT, c.use_unique).to(dtype)
    psi, psi_s = psi_all[: onv.size(0)], psi_all[onv.size(0):]
    # psi(x): column 0 among the kept records (every row keeps it unless |H_00| < eps, where the reference divides by 0 too),
    # else among the drawn ones
    psi_x = torch.zeros(x.size(0), dtype=dtype, device=x.device)
    first_s = s_col == 0
    psi_x[s_row[first_s]] = psi_s[first_s]
    first = col == 0
    psi_x[row[first]] = psi[first]
    rdt = _real_dtype(dtype)
    eloc = _segment_sum((psi / psi_x[row]) * h.to(rdt), counts) + _segment_sum((psi_s / psi_x[s_row]) * s_w.to(rdt), s_counts)
    t3 = time.time_ns()
    return eloc.to(dtype), torch.zeros_like(eloc).to(dtype), psi_x, ((t2 - c.t0) / 1e6, 0.0, (t3 - t2) / 1e6)


def _eloc_generic(c):
    """The generic path: the same tensor algebra as the reference, on the materialised (batch, ncomb) matrices."""
    x, dtype = c.x, c.dtype
    comb_x, comb_hij = get_comb_hij_fused(x, c.h1e, c.h2e, *c.system)
    t1 = time.time_ns()
    hij_spin = get_hij_torch(x, comb_x, c.h1e_spin, c.h2e_spin, c.sorb, c.nele) if c.use_spin_raising else None
    t2 = time.time_ns()
    batch, n_comb, bra_len = comb_x.shape
    flat = comb_x.reshape(-1, bra_len)
    if c.use_sample_space:
        psi_x1, f_psi = _amplitudes_sample_space(flat, batch, n_comb, c.ansatz_extra, c.WF_LUT, c.use_multi_psi, c.use_spin_flip,
                                                 c.extra_norm, c.sorb)
    else:
        sel = _reduce_select(comb_hij, c.eps, c.eps_sample) if c.reduce_psi else None
        psi_x1, f_psi = _amplitudes(flat, sel, batch, n_comb, c.ansatz_f, c.ansatz_extra, c.WF_LUT, c.use_unique, c.use_multi_psi,
                                    c.use_spin_flip, c.extra_norm, dtype, c.sorb, x.device)
    rdt = _real_dtype(dtype)
    eloc = _contract(f_psi, psi_x1, comb_hij.to(rdt))
    sloc = _contract(f_psi, psi_x1, hij_spin.to(rdt)) if c.use_spin_raising else torch.zeros_like(eloc)
    t3 = time.time_ns()
    return eloc.to(dtype), sloc.to(dtype), psi_x1[..., 0].to(dtype), ((t1 - c.t0) / 1e6, (t2 - t1) / 1e6, (t3 - t2) / 1e6)


def local_energy(
    x: Tensor, h1e: Tensor, h2e: Tensor, ansatz, ansatz_batch: Callable[..., Tensor], sorb: int, nele: int, noa: int, nob: int,
    dtype=torch.double, use_spin_raising: bool = False, h1e_spin: Optional[Tensor] = None, h2e_spin: Optional[Tensor] = None,
    WF_LUT: Optional[WavefunctionLUT] = None, use_unique: bool = True, reduce_psi: bool = False, eps: float = 1e-12,
    eps_sample: int = 0, use_sample_space: bool = False, index: Optional[Tuple[int, int]] = None, alpha: float = 2,
    use_multi_psi: bool = False, use_spin_flip: bool = False, extra_norm: Optional[Tensor] = None, _front_ticket=None,
) -> Tuple[Tensor, Tensor, Tensor, Tuple[float, float, float]]:
    """vmc/energy/eloc.py:23-132.  Returns (eloc[n], sloc[n], psi(x)[n], (t_enumerate, t_hij, t_psi) in ms).
    _front_ticket (not in the reference): a reduce_front_launch ticket for exactly these walkers and arguments, enqueued earlier
    (total_energy's look-ahead on a second stream).
    A dispatcher: the paths of the module docstring in their order; a path that returns None has declined and the next one is asked."""
    with torch.no_grad():
        check_para(x)
        assert x.dim() == 2
        if use_sample_space:
            assert WF_LUT is not None, "WF_ULT must be used if use_sample"
        if reduce_psi and not use_sample_space:
            assert eps >= 0.0 and eps_sample >= 0
        if extra_norm is None:
            extra_norm = 1.0
        c = SimpleNamespace(
            x=x, h1e=h1e, h2e=h2e, ansatz=ansatz, ansatz_batch=ansatz_batch, system=(sorb, nele, noa, nob), sorb=sorb, nele=nele, dtype=dtype,
            use_spin_raising=use_spin_raising, h1e_spin=h1e_spin, h2e_spin=h2e_spin, WF_LUT=WF_LUT, use_unique=use_unique, reduce_psi=reduce_psi,
            eps=eps, eps_sample=eps_sample, use_sample_space=use_sample_space, use_multi_psi=use_multi_psi, use_spin_flip=use_spin_flip,
            extra_norm=extra_norm, front_ticket=_front_ticket, ansatz_f=None, ansatz_extra=None, t0=time.time_ns())
        plain = not (use_multi_psi or use_spin_flip)
        gpu_ok = FUSED and x.is_cuda and sorb % 2 == 0   # (every fused kernel packs an even number of spin orbitals)
        if use_sample_space and _fast_sample_space_ok(x, h1e, sorb, WF_LUT):
            return _eloc_sample_space_fused(c)
        # (the spin-flip-projected form too, for the real-parameter RBMs and the Jastrow-RBM: _eloc_simple_rbm declines the others)
        simple_rbm = (gpu_ok and FUSED_RBM and not reduce_psi and not use_sample_space and WF_LUT is None and not use_multi_psi
                      and h1e.dtype in (torch.float64, torch.float32))
        out = _eloc_simple_rbm(c) if simple_rbm else None
        if out is not None:
            return out
        # (ansatz_f: psi; ansatz_extra: f of the multi-psi form -- functions of a batch of determinants)
        c.ansatz_extra = partial(ansatz_batch, func=ansatz.module.extra) if use_multi_psi else None
        c.ansatz_f = partial(ansatz_batch, func=ansatz.module.sample if use_multi_psi else ansatz)
        front = reduce_psi and not use_sample_space and x.size(0) > 0 and _front_ok(x, h1e, sorb, nele, noa, nob, eps_sample)
        out = _eloc_reduce_front(c) if front else None
        if out is not None:
            return out
        if gpu_ok and reduce_psi and not use_sample_space and eps_sample == 0:
            return _eloc_reduce_multipass(c)
        if gpu_ok and FUSED_SAMPLED and reduce_psi and not use_sample_space and eps_sample > 0 and plain and not use_spin_raising:
            return _eloc_reduce_multipass_sampled(c)
        return _eloc_generic(c)


AUTO_NBATCH_KEEP = 64   # calls of one shape served from the last answer before the device memory is looked at again
_AUTO_NBATCH: dict = {}


def auto_nbatch(x, h1e, sorb, nele, noa, nob, ansatz, WF_LUT, dtype, reduce_psi, eps_sample, use_sample_space, use_multi_psi, use_spin_flip,
                use_spin_raising, max_memory: float = 64.0, alpha: float = 0.25) -> int:
    """Walkers per local_energy call for the path local_energy will take on these arguments (same conditions as there)."""
    n = x.size(0)
    n_sd = get_Num_SinglesDoubles(sorb, noa, nob)
    fused = None
    if n and x.is_cuda and FUSED and sorb % 2 == 0:
        if use_sample_space and _fast_sample_space_ok(x, h1e, sorb, WF_LUT):
            fused = "sample_space"
        elif reduce_psi and not use_sample_space and _front_ok(x[: min(n, 4096)], h1e, sorb, nele, noa, nob, eps_sample):
            fused = "reduce"
        elif (not reduce_psi and not use_sample_space and FUSED_RBM and WF_LUT is None and not (use_multi_psi or use_spin_flip)
              and (_real_rbm_params(ansatz) is not None or _complex_rbm_params(ansatz) is not None)):
            fused = "simple_rbm"
        elif (not reduce_psi and not use_sample_space and FUSED_RBM and WF_LUT is None and use_spin_flip and not use_multi_psi
              and h1e.dtype in (torch.float64, torch.float32)
              and ((_real_rbm_params(ansatz) is not None and _rbm_lds_ok(sorb, nele, noa, nob, _real_rbm_params(ansatz)[0].size(0)))
                   or (_jastrow_rbm_params(ansatz) is not None
                       and CX.eloc_jrbm_supported(sorb, nele, noa, nob, _jastrow_rbm_params(ansatz)[0].size(0))))):
            fused = "simple_rbm"   # (the spin-flip-projected form of the same kernels: nothing of size nbatch x ncomb either)
    dt = dtype if dtype in (torch.double, torch.complex128) else torch.double
    if fused is None:
        return max(1, get_nbatch(sorb, max(n, 1), n_sd, max_memory, alpha, x.device, use_sample_space, dt, fused=None, eps_sample=int(eps_sample)))
    # the fused paths ask once per total_energy call, i.e. once per VMC step: the answer (a function of the free device memory) is kept for
    # AUTO_NBATCH_KEEP calls of the same shape -- the allocator statistics behind it cost 0.2 ms, 15 % of a configs[1]-sized step
    key = (str(x.device), sorb, n, n_sd, fused, int(eps_sample), dt, float(max_memory), float(alpha))
    with _LOCK:
        hit = _AUTO_NBATCH.get(key)
        if hit is not None and hit[1] < AUTO_NBATCH_KEEP:
            hit[1] += 1
            return hit[0]
    nb = max(1, get_nbatch(sorb, max(n, 1), n_sd, max_memory, alpha, x.device, use_sample_space, dt, fused=fused, eps_sample=int(eps_sample)))
    with _LOCK:
        _AUTO_NBATCH[key] = [nb, 0]
        while len(_AUTO_NBATCH) > 64:
            _AUTO_NBATCH.pop(next(iter(_AUTO_NBATCH)))
    return nb


def total_energy(
    x: Tensor, nbatch: int, fp_batch: int, h1e: Tensor, h2e: Tensor, ansatz: Callable[..., Tensor], sorb: int, nele: int, noa: int,
    nob: int, WF_LUT: Optional[WavefunctionLUT] = None, use_unique: bool = True, dtype=torch.double, use_spin_raising: bool = False,
    h1e_spin: Optional[Tensor] = None, h2e_spin: Optional[Tensor] = None, reduce_psi: bool = False, eps: float = 1.0e-12,
    eps_sample: int = 0, use_sample_space: bool = False, alpha: float = 2.0, use_multi_psi: bool = False,
    use_spin_flip: bool = False, extra_norm: Optional[Tensor] = None,
) -> Tuple[Tensor, Tensor, Tensor]:
    """vmc/energy/etot.py:24-169: local energies of this rank's walkers in chunks of `nbatch` walkers, ansatz
    forwards in chunks of `fp_batch` rows; NaN guard; returns (eloc, sloc, placeholder).
    nbatch = 0 (not in the reference): sized for the path that will actually run (public_function.get_nbatch(fused=...)): the fused
    kernels need none of the memory the reference's formula budgets for, and few large launches run faster than many small ones."""
    dim = x.shape[0]
    device = x.device
    eloc = torch.zeros(dim, device=device).to(dtype)
    sloc = torch.zeros_like(eloc)
    prev_token = _call_token()
    _CALL_TOKEN.value = object()
    try:
        assert fp_batch > 0 or fp_batch == -1
        assert nbatch > 0 or nbatch in (-1, 0)
        if nbatch == 0:
            nbatch = auto_nbatch(x, h1e, sorb, nele, noa, nob, ansatz, WF_LUT, dtype, reduce_psi, eps_sample, use_sample_space, use_multi_psi,
                                 use_spin_flip, use_spin_raising)
        if nbatch == -1:
            nbatch = dim
        ends = split_batch_idx(dim, min_batch=nbatch) if dim else []

        def _ansatz_batch(x: Tensor, func: Callable[[Tensor], Tensor]) -> Tensor:
            return ansatz_batch(func, x, fp_batch, sorb, device, dtype)

        _ansatz_batch.accepts_pm1_rows = True  # (public_function.ansatz_batch takes uint8 determinants or ready +-1 rows)

        # REDUCE with several chunks of walkers: the front end of chunk k + 1 runs on a second stream while the ansatz works on the distinct x'
        # of chunk k ("overlap kernel(i+1) with forward(i) on two HIP streams"); two workspaces take turns.  OVERLAP = False or
        # PYNQS_OVERLAP=0: everything on the current stream.
        starts = [0] + list(ends[:-1])
        look_ahead = (OVERLAP and reduce_psi and not use_sample_space and len(ends) >= 2 and x.is_cuda
                      and all(_front_ok(x[b:e], h1e, sorb, nele, noa, nob, eps_sample) for b, e in ((starts[0], ends[0]), (starts[-1], ends[-1]))))
        tickets, done = {}, {}
        if look_ahead:
            main = torch.cuda.current_stream(device)
            side = _side_stream(device)
            ht_, rbm_ = _reduce_front_options(ansatz, WF_LUT, dtype, use_multi_psi, use_spin_flip)

            xc = x.contiguous()  # (once, on the main stream: the chunks are views of it, no copy kernel runs between the streams)

            def launch(k: int) -> None:
                xs = xc[starts[k]:ends[k]]
                if k == 0:
                    side.wait_stream(main)  # (xc and whatever else the caller wrote on the main stream; later launches read nothing newer than that --
                    #                          waiting every time would hold chunk k + 1's front end back until chunk k - 1 has been contracted)
                if k >= 2:
                    side.wait_event(done[k - 2])  # the workspace of slot k % 2 is free once chunk k - 2 has been contracted
                with torch.cuda.stream(side):
                    # (consumer: the workspace is allocated in the side stream's pool and read on the main stream -- the allocator must not hand
                    # its memory out again while main-stream work on it is pending)
                    tickets[k] = reduce_front_launch(xs, h1e, h2e, sorb, nele, noa, nob, eps, int(eps_sample), ht_, want_pm1=rbm_ is None, slot=k % 2, route=True,
                                                     consumer=main)

            launch(0)
        begin = 0
        for k, end in enumerate(ends):
            ticket = None
            if look_ahead:
                ticket = tickets.pop(k, None)
                if ticket is not None:
                    ticket.ev.synchronize()       # (host: the counters of chunk k are there)
                    main.wait_event(ticket.ev)     # (device: chunk k's records are there before the ansatz / contraction read them)
                # (a chunk whose rows outgrew the front end's LDS list sends the rest of the call to the multi-pass path: no more tickets)
                if k + 1 < len(ends) and _front_ok(x[starts[k + 1]:ends[k + 1]], h1e, sorb, nele, noa, nob, eps_sample):
                    launch(k + 1)                     # runs while the ansatz works on chunk k
            _eloc, _sloc, _psi, _ = local_energy(
                ticket.x if ticket is not None else x[begin:end], h1e, h2e, ansatz, _ansatz_batch, sorb, nele, noa, nob, dtype=dtype, WF_LUT=WF_LUT,
                use_spin_raising=False if reduce_psi else use_spin_raising, h1e_spin=h1e_spin, h2e_spin=h2e_spin, use_unique=use_unique,
                reduce_psi=reduce_psi, eps=eps, eps_sample=eps_sample, use_sample_space=use_sample_space, index=(begin, end), alpha=alpha,
                use_multi_psi=use_multi_psi, extra_norm=extra_norm, use_spin_flip=use_spin_flip, _front_ticket=ticket)
            if look_ahead:
                done[k] = torch.cuda.Event()
                done[k].record(main)
            if reduce_psi and use_spin_raising:
                # <S-S+> is recomputed in the sample space (etot.py:119-142)
                _sloc, _, _, _ = local_energy(x[begin:end], h1e_spin, h2e_spin, ansatz, _ansatz_batch, sorb, nele, noa, nob, dtype=dtype,
                                              WF_LUT=WF_LUT, use_spin_raising=False, use_sample_space=True, index=(begin, end), alpha=alpha)
            eloc[begin:end] = _eloc
            sloc[begin:end] = _sloc
            begin = end
    finally:
        _CALL_TOKEN.value = prev_token   # (also when a chunk raises: a later direct local_energy call must not match this call's token)
    if torch.any(torch.isnan(eloc)):
        raise ValueError("The Local energy exists nan")
    return eloc, sloc, torch.zeros(1, device=device, dtype=dtype)
