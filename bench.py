#!/usr/bin/env python3
"""bench.py -- local-energy throughput of the MI355X determinant engine (one process per GPU).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload NAME] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one pass of the hot path over one batch of walkers (every rank works on its own shard of
`--walkers` walkers: weak scaling).  W untimed warm-up steps, then exactly K steps bracketed by
barrier + torch.cuda.synchronize(); the maximum over ranks is the step time.  Rank 0 prints ONE JSON
line with `ms_per_step` and `roofline` (dominant kernel, live HIP-event timing of the same steps).
--dump-outputs DIR: after the timed steps rank 0 writes what its last step computed (the arrays a caller of the
timed path receives) as DIR/<name>.npy, float64 or float32, complex as [..., 2] (real, imaginary); past 64 MB in
all, a fixed seeded sample of the walkers (DIR/sample_walkers.npy).  The inputs of the timed steps are the same
from run to run (the semi-stochastic draws are re-seeded after the untimed pre-heat).
A plain run does nothing else.  --full adds the checks and the secondary measurements: `parity` (the last step
against the CPU oracle), `cpu_baseline` (reference/oracle timed on the host cores, rank 0, N = 1 only; not with
--no-cpu-baseline) and, for the default workload, `extra` (not with --no-extra).

Workloads (config.workload):
  fe2s2_reduce_vmc_step (default)   one COMPLETE local-energy step of a VMC iteration with the method the Fe2S2 example runs: semi-stochastic
                 REDUCE (eps = 1e-2, eps_sample = 1000): the one-launch REDUCE front end (enumerate, keep |H| >= eps, draw, de-duplicate,
                 +-1 rows of the distinct x') -> amplitudes on the distinct rows (PyTorch module) -> contraction kernel -> moments +
                 packed RCCL all-reduce -> gradient estimator.  See ReduceVmcStep.
  fe2s2_vmc_step   the same step with the SAMPLE_SPACE method: one COMPLETE local-energy step of a VMC iteration on this rank's shard of the walkers
                 (BASELINE configs C3/C4 on the shipped Fe2S2 problem): fused SAMPLE_SPACE local energies (enumerate, <x|H|x'>,
                 psi(x') from the sample table, contraction: one kernel) -> weighted moments kernel + ONE packed RCCL all-reduce
                 of (sum p E, sum p |E|^2, sum p) -> gradient estimator: micro-batched backward of a complex128 module under
                 DistributedDataParallel (bucketed RCCL all-reduce in the last micro-batch), vmc/grad/energy_grad.py:118-184.
  fe2s2_dropin   get_comb_hij_fused on the shipped Fe2S2 problem (sorb 40, 15a15b, ncomb 7876):
                 comb + Hmat materialised exactly like the reference API (HBM-write bound).
  syn<sorb>_dropin  same on synthetic dense integrals, sorb in {56, 120, 184}.
  fe2s2_eloc_sample_space   complete SAMPLE_SPACE local energies in one kernel (hash-table psi) + statistics
                 kernel + packed all-reduce.
  fe2s2_eloc_rbm / syn<sorb>_eloc_rbm   complete SIMPLE local energies with a real RBM (alpha = 2) evaluated inside the
                 kernel; the RBM table is rebuilt every step (parameters change every optimisation step).
With --full, the default workload and N = 1 the line also carries `extra`: the drop-in rows/s, the other fused workloads, the larger systems,
the REDUCE compaction throughput and the generic PyTorch-module paths, each measured in the same run.
Inputs are resident in HBM before the timed region.  Nothing here reads /root/reference.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.29 TB/s measured copy)
# vector-ALU issue peak in wave64 instructions per second: 256 CUs x 4 SIMDs x 2.4 GHz / VALU_CYCLES cycles per instruction.
# VALU_CYCLES: tools/micro/valu_peak.hip on one MI355X (profiles/r02_valu_peak.txt)
VALU_CYCLES = 2.0
VALU_PEAK_GINST = 256 * 4 * 2.4 / VALU_CYCLES


# ---------------------------------------------------------------------------------------------------
def synth_integrals(sorb: int, seed: int = 1234):
    g = torch.Generator().manual_seed(seed)
    h1 = torch.rand(sorb, sorb, generator=g, dtype=torch.float64) - 0.5
    h1 = (h1 + h1.T).reshape(-1).contiguous()
    pair = sorb * (sorb - 1) // 2
    h2 = torch.rand(pair * (pair + 1) // 2, generator=g, dtype=torch.float64) - 0.5
    return h1, h2


def synth_walkers(n: int, sorb: int, noA: int, noB: int, seed: int) -> torch.Tensor:
    """noA distinct even + noB distinct odd orbitals per walker, packed on the host."""
    g = np.random.default_rng(seed)
    k = sorb // 2
    ra = np.argsort(g.random((n, k)), axis=1)[:, :noA]
    rb = np.argsort(g.random((n, k)), axis=1)[:, :noB]
    L = (sorb - 1) // 64 + 1
    words = np.zeros((n, L), dtype=np.uint64)
    for orb in (2 * ra, 2 * rb + 1):
        for c in range(orb.shape[1]):
            o = orb[:, c]
            np.bitwise_or.at(words, (np.arange(n), o // 64), np.uint64(1) << (o % 64).astype(np.uint64))
    return torch.from_numpy(words.view(np.uint8).reshape(n, 8 * L))


def synth_connected(x: torch.Tensor, sorb: int, count: int, seed: int) -> torch.Tensor:
    """`count` determinants, each an alpha-beta double excitation of one of the walkers `x` (seeded)."""
    g = np.random.default_rng(seed)
    n, L = x.size(0), x.size(1) // 8
    src = x.numpy().view(np.uint64).reshape(n, L)[np.arange(count) % n].copy()
    orb = np.arange(sorb)
    occ = ((src[:, orb // 64] >> (orb % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)  # [count, sorb]
    rows = np.arange(count)
    for spin in (0, 1):
        same = (orb % 2 == spin)[None, :]
        score = g.random((count, sorb))
        hole = np.argmax(np.where(occ & same, score, -1.0), axis=1)
        part = np.argmax(np.where(~occ & same, score, -1.0), axis=1)
        for o in (hole, part):
            src[rows, o // 64] ^= np.uint64(1) << (o % 64).astype(np.uint64)
    return torch.from_numpy(src.view(np.uint8).reshape(count, 8 * L))


def load_fe2s2():
    d = np.load(os.path.join(ROOT, "tests", "golden", "fe2s2_inputs.npz"))
    return d


def algorithmic_bytes_dropin(sorb, nele, noA, noB, esize=8):
    """SURVEY.md 8(d) / BASELINE.md 3: bytes per walker of the drop-in fused call."""
    k = sorb // 2
    nvA, nvB = k - noA, k - noB
    nS = noA * nvA + noB * nvB
    nD = noA * (noA - 1) // 2 * (nvA * (nvA - 1) // 2) + noB * (noB - 1) // 2 * (nvB * (nvB - 1) // 2) + noA * noB * nvA * nvB
    ncomb = 1 + nS + nD
    L = (sorb - 1) // 64 + 1
    gathers = esize * (nD + nS * (1 + nele) + nele + nele * (nele - 1) // 2)
    out = ncomb * (esize + 8 * L)
    return gathers + out + 8 * L, ncomb


def dropin_byte_parts(sorb, nele, noA, noB, esize=8):
    """(integral gathers, outputs, inputs) in bytes per walker: the three terms of algorithmic_bytes_dropin."""
    total, ncomb = algorithmic_bytes_dropin(sorb, nele, noA, noB, esize)
    L = (sorb - 1) // 64 + 1
    out = ncomb * (esize + 8 * L)
    return total - out - 8 * L, out, 8 * L


# ---------------------------------------------------------------------------------------------------
class Workload:
    name = ""
    unit_per_walker = 1

    def step(self):  # enqueue one pass; returns (start_event, end_event) around the dominant kernel
        raise NotImplementedError

    def outputs(self):  # what a caller of the timed path receives from the last step: name -> tensor (--dump-outputs)
        raise NotImplementedError


def stats_output(stats):
    """(mean, var, sd, standard error) of dist_stats_moments as float64 [mean.real, mean.imag, var, sd, se]"""
    mean = stats[0]
    im = mean.imag if mean.is_complex() else torch.zeros_like(mean)
    return torch.stack([mean.real, im, stats[1], stats[2], stats[3]]).double()


def grad_outputs(module):
    return {f"grad_{k}": p.grad for k, p in module.named_parameters() if p.grad is not None}


DUMP_LIMIT_BYTES = 64 * 1000 * 1000  # --dump-outputs: all files together, .npy headers included


def dump_outputs(w, path):
    """--dump-outputs: the last step's outputs as path/<name>.npy -- float32 and integers of up to 16 bits as float32, the rest as float64,
    complex as [..., 2] real/imaginary pairs.  Past 64 MB in all, every array whose first axis is the walker axis keeps the same fixed,
    seeded sample of walkers, whose indices go to path/sample_walkers.npy."""
    arrs = {k: torch.as_tensor(t).detach() for k, t in w.outputs().items()}
    arrs = {k: torch.view_as_real(t.resolve_conj()) if t.is_complex() else t for k, t in arrs.items()}
    f32 = lambda t: t.dtype == torch.float32 or (not t.is_floating_point() and t.element_size() <= 2)  # noqa: E731
    nbytes = lambda t: t.numel() * (4 if f32(t) else 8)  # noqa: E731  (as written)
    total = sum(nbytes(t) for t in arrs.values())
    budget = DUMP_LIMIT_BYTES - 1024 * (len(arrs) + 1)  # (a header of at most 1 KiB per file, sample_walkers.npy's among them)
    if total > budget:
        per_walker = [k for k, t in arrs.items() if t.dim() > 0 and t.size(0) == w.n]
        row_bytes = sum(nbytes(arrs[k][0]) for k in per_walker) + 8  # (+ the walker's index)
        keep = int((budget - (total - (row_bytes - 8) * w.n)) // row_bytes)
        if keep < 1:
            raise SystemExit(f"--dump-outputs: one walker's outputs do not fit {DUMP_LIMIT_BYTES} bytes")
        idx = np.sort(np.random.default_rng(2024).choice(w.n, size=keep, replace=False))
        sel = torch.from_numpy(idx)
        for k in per_walker:
            arrs[k] = arrs[k].index_select(0, sel.to(arrs[k].device))
        arrs["sample_walkers"] = torch.from_numpy(idx.astype(np.float64))
    os.makedirs(path, exist_ok=True)
    for k, t in arrs.items():
        np.save(os.path.join(path, k + ".npy"), t.to(torch.float32 if f32(t) else torch.float64).cpu().numpy())
    return sorted(arrs)


class DropinFused(Workload):
    """get_comb_hij_fused: enumerate + <x|H|x'>, comb and Hmat written to HBM (reference API shape)."""

    def __init__(self, tag, sorb, nele, noA, noB, h1, h2, walkers, dev, path="plan"):
        from pynqs_amd import _native as N

        self.N = N
        self.lib = N.lib()
        self.name = f"{tag}_dropin"
        self.sorb, self.nele, self.noA, self.noB = sorb, nele, noA, noB
        self.h1, self.h2, self.x = h1.to(dev), h2.to(dev), walkers.to(dev).contiguous()
        self.n = self.x.size(0)
        self.bytes_per_walker, self.ncomb = algorithmic_bytes_dropin(sorb, nele, noA, noB)
        self.gather_bytes_per_walker, self.out_bytes_per_walker, self.in_bytes_per_walker = dropin_byte_parts(sorb, nele, noA, noB)
        L = (sorb - 1) // 64 + 1
        self.comb = torch.empty((self.n, self.ncomb, 8 * L), dtype=torch.uint8, device=dev)
        self.hmat = torch.empty((self.n, self.ncomb), dtype=torch.float64, device=dev)
        self.dev = dev
        self.comb_ptr = self.comb.data_ptr()
        self.path = path if sorb % 2 == 0 else "direct"
        self.kernel = "comb_hij_plan_kernel" if self.path == "plan" else "comb_hij_kernel"
        self.plan, self.plan_build_ms = None, None
        if self.path == "plan":
            # one-time re-layout of the integrals (include/pynqs_amd.h 'integral plan'); built once per
            # (h1e, h2e), outside the timed region like the integrals themselves
            nb = self.lib.pynqs_plan_bytes(sorb, N.PYNQS_F64)
            self.plan = torch.empty(nb // 8, dtype=torch.float64, device=dev)
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            st = torch.cuda.current_stream(dev)
            e0.record(st)
            N.check(self.lib.pynqs_plan_build(self.h1.data_ptr(), self.h2.data_ptr(), sorb, N.PYNQS_F64, self.plan.data_ptr(),
                                              st.cuda_stream), "plan_build")
            e1.record(st); e1.synchronize()
            self.plan_build_ms = e0.elapsed_time(e1)

    def step(self):
        st = torch.cuda.current_stream(self.dev)
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(st)
        if self.plan is not None:
            rc = self.lib.pynqs_comb_hij_fused_plan(self.x.data_ptr(), self.n, self.sorb, self.nele, self.noA, self.noB,
                                                    self.plan.data_ptr(), self.N.PYNQS_F64, self.comb_ptr,
                                                    self.hmat.data_ptr(), st.cuda_stream)
        else:
            rc = self.lib.pynqs_comb_hij_fused(self.x.data_ptr(), self.n, self.sorb, self.nele, self.noA, self.noB,
                                               self.h1.data_ptr(), self.h2.data_ptr(), self.N.PYNQS_F64,
                                               self.comb_ptr, self.hmat.data_ptr(), st.cuda_stream)
        e1.record(st)
        self.N.check(rc, "pynqs_comb_hij_fused")
        return e0, e1

    def outputs(self):  # (comb: the packed determinants' bytes, written as float32)
        return {"hmat": self.hmat, "comb": self.comb} if self.comb_ptr is not None else {"hmat": self.hmat}

    def parity_gate(self):
        """max |dH| against the CPU oracle on the first walkers (SURVEY.md 8d 'parity gate')."""
        from oracle import oracle as O

        m = min(self.n, 8)
        co, ho = O.comb_hij_fused(self.x[:m].cpu().numpy(), self.h1.cpu().numpy(), self.h2.cpu().numpy(), self.sorb,
                                  self.nele, self.noA, self.noB)
        ok_c = np.array_equal(self.comb[:m].cpu().numpy(), co)
        dh = float(np.abs(self.hmat[:m].cpu().numpy() - ho).max())
        return ok_c, dh

    def cpu_baseline(self, budget_s=15.0):
        """The reference's own CPU extension (oracle/_ref, compiled from its sources) when present, else the
        oracle port; all host cores; bounded sample of the same workload."""
        x = self.x.cpu(); h1 = self.h1.cpu(); h2 = self.h2.cpu()
        ref_dir = os.path.join(ROOT, "oracle", "_ref")
        kind, fn = "port", None
        # the GPU box gives one GPU's share of the host: 16 cores (build prompt); use min(affinity, 16)
        cores = min(len(os.sched_getaffinity(0)), 16)
        if self.sorb <= 64 and self.nele <= 40 and os.path.exists(os.path.join(ref_dir, "C_extension.so")):
            try:
                sys.path.insert(0, ref_dir)
                import C_extension as ref  # noqa: the reference module, MAX_SORB_LEN = 1

                torch.set_num_threads(cores)
                fn = lambda xs: ref.get_comb_hij_fused(xs, h1, h2, self.sorb, self.nele, self.noA, self.noB)
                kind = "reference"
            except Exception as e:  # pragma: no cover
                print(f"[bench] oracle/_ref not usable ({e}); falling back to the oracle port", file=sys.stderr)
        if fn is None:
            from oracle import oracle as O

            h1n, h2n = h1.numpy(), h2.numpy()
            fn = lambda xs: O.comb_hij_fused(xs.numpy(), h1n, h2n, self.sorb, self.nele, self.noA, self.noB, nthreads=cores)
        # calibrate the sample so that the timed part is ~budget_s
        m = max(1, min(self.n, 256))
        t0 = time.perf_counter(); fn(x[:m].contiguous()); dt = time.perf_counter() - t0
        rate = m / max(dt, 1e-6)
        sample = int(max(m, min(self.n, rate * budget_s / 4)))
        reps, done, t0 = 0, 0, time.perf_counter()
        while True:
            fn(x[:sample].contiguous()); reps += 1; done += sample
            if time.perf_counter() - t0 > budget_s * 0.8 or reps >= 50:
                break
        el = time.perf_counter() - t0
        out = {"value": done / el, "unit": "S+D rows/s", "cores": cores, "kind": kind,
               "sample": f"{reps} x get_comb_hij_fused on the first {sample} walkers of the same batch ({el:.1f} s)"}
        # the reference's production setting is OMP_NUM_THREADS=1 per GPU process (run.sh:3): the same call on one thread
        try:
            if kind == "reference":
                torch.set_num_threads(1)
                one = fn
            else:
                one = lambda xs: O.comb_hij_fused(xs.numpy(), h1n, h2n, self.sorb, self.nele, self.noA, self.noB, nthreads=1)
            m1 = max(1, min(self.n, 512))
            t0 = time.perf_counter(); r1 = 0
            while time.perf_counter() - t0 < 2.0:
                one(x[:m1].contiguous()); r1 += 1
            out["one_thread"] = {"value": m1 * r1 / (time.perf_counter() - t0), "unit": "S+D rows/s", "cores": 1,
                                 "sample": f"{r1} x the same call on the first {m1} walkers"}
        finally:
            if kind == "reference":
                torch.set_num_threads(cores)
        return out


class SampleSpaceFused(Workload):
    """Complete local energies, SAMPLE_SPACE method (vmc/energy/eloc.py:326-401), in ONE kernel: enumerate,
    <x|H|x'>, psi(x') from the sorted sample table, contraction.  Nothing is materialised.  psi is complex128
    like the Fe2S2 example's BDG-RNN amplitudes (synthetic, seeded)."""

    def __init__(self, tag, sorb, nele, noA, noB, h1, h2, walkers, keys, dev):
        from pynqs_amd import _native as N
        from pynqs_amd import public_function as pf

        self.N, self.lib = N, N.lib()
        self.name = f"{tag}_eloc_sample_space"
        self.sorb, self.nele, self.noA, self.noB = sorb, nele, noA, noB
        self.h1, self.h2, self.x = h1.to(dev), h2.to(dev), walkers.to(dev).contiguous()
        self.n = self.x.size(0)
        dropin, self.ncomb = algorithmic_bytes_dropin(sorb, nele, noA, noB)
        L = (sorb - 1) // 64 + 1
        # SURVEY.md 8(d) B_fused: integral gathers + walker in + E_loc out (complex128)
        self.bytes_per_walker = dropin - self.ncomb * (8 + 8 * L) + 16
        g = torch.Generator().manual_seed(7)
        nk = keys.size(0)
        amp = torch.exp(-3.0 * torch.rand(nk, generator=g, dtype=torch.float64))
        ph = 2 * np.pi * torch.rand(nk, generator=g, dtype=torch.float64)
        wf = torch.polar(amp, ph)
        self.lut = pf.WavefunctionLUT(keys.to(dev), wf.to(dev), sorb, device=dev)
        nb = self.lib.pynqs_plan_bytes(sorb, N.PYNQS_F64)
        self.plan = torch.empty(nb // 8, dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream(dev)
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(st)
        N.check(self.lib.pynqs_plan_build(self.h1.data_ptr(), self.h2.data_ptr(), sorb, N.PYNQS_F64, self.plan.data_ptr(), st.cuda_stream),
                "plan_build")
        e1.record(st); e1.synchronize()
        self.plan_build_ms = e0.elapsed_time(e1)
        self.eloc = torch.empty(self.n, dtype=torch.complex128, device=dev)
        self.psi0 = torch.empty(self.n, dtype=torch.complex128, device=dev)
        self.prob = torch.full((self.n,), 1.0 / self.n, dtype=torch.float64, device=dev)
        self.dev, self.path, self.kernel = dev, "plan", "eloc_sample_space_filtered_kernel"
        self.bound, self.pmc_name = "valu", f"{tag}_eloc_sample_space"
        # the same choice pynqs_amd.energy.local_energy makes: walk the table (work ~ walkers x keys) or the excitation lists (~ walkers x ncomb)
        from pynqs_amd import energy as E_

        self.key_major = E_.choose_sample_space_kernel(self.x, sorb, nele, noA, noB, self.plan, self.lut, self.lut.wf_value, True)
        if self.key_major:
            self.kernel, self.pmc_name = "eloc_sample_space_keys_kernel", f"{tag}_eloc_sample_space_keys"
            self.roofline_note = ("key-major kernel: the table is walked instead of the excitation lists (work ~ walkers x keys, not walkers x ncomb); "
                                  "popcount(x ^ key) <= 4 decides per pair, the few keys within a double excitation are evaluated from the bit patterns; "
                                  "bound by vector-ALU instruction issue, HBM traffic negligible")
        self.index = E_._keys_index_for(self.lut, self.n, sorb) if self.key_major else None  # (the energy layer's own rule, energy.py)
        if self.index is not None:
            import time as _t

            torch.cuda.synchronize(dev); t0 = _t.perf_counter()
            from pynqs_amd import C_extension as CX_

            CX_.keys_index_build(self.lut.bra_key, sorb)
            self.index_build_ms = (_t.perf_counter() - t0) * 1e3  # once per table, like the hash table of the column-major form; not in the step
            self.pmc_name = f"{tag}_eloc_sample_space_indexed"
            self.roofline_note = (f"INDEXED key-major kernel: the keys are indexed by five blocks of the orbitals (built once per table, {self.index_build_ms:.2f} ms incl. "
                                  f"the host read-back of its density); a walker meets {self.index.per_walker:.1f} of the {self.lut.bra_key.size(0)} keys instead of all of them. "
                                  "What is left is a chain of dependent memory round trips per walker (17-step binary searches, key -> integral / psi gathers, the "
                                  "nele (nele + 1) / 2 gathers of <x|H|x>): latency-bound, neither HBM nor vector-ALU issue is near its roof")
        if not self.key_major:
            self.roofline_note = ("filter-first kernel: a column whose Zobrist hash the filter rejects never has its integral gathered; HBM traffic is "
                                  "negligible and the kernel is bound by vector-ALU instruction issue (see valu_instructions_per_launch: ~1.5 wave64 instructions per column incl. the per-walker set-up and the evaluation of the candidates)")
        self.stats = None

    def launch_eloc(self, st):
        """the fused SAMPLE_SPACE local energy: key-major or column-major, the choice pynqs_amd.energy.local_energy makes"""
        if self.index is not None:
            keys = self.lut.bra_key
            return self.lib.pynqs_eloc_sample_space_indexed(self.x.data_ptr(), self.n, self.sorb, self.nele, self.noA, self.noB, self.plan.data_ptr(),
                                                            keys.data_ptr(), keys.size(0), self.index.index.data_ptr(), self.lut.wf_value.data_ptr(), 1, 0,
                                                            self.eloc.data_ptr(), self.psi0.data_ptr(), st.cuda_stream)
        if self.key_major:
            keys = self.lut.bra_key
            return self.lib.pynqs_eloc_sample_space_keys(self.x.data_ptr(), self.n, self.sorb, self.nele, self.noA, self.noB, self.plan.data_ptr(),
                                                         keys.data_ptr(), keys.size(0), self.lut.wf_value.data_ptr(), 1, 0, self.eloc.data_ptr(),
                                                         self.psi0.data_ptr(), st.cuda_stream)
        ht = self.lut.hashtable
        return self.lib.pynqs_eloc_sample_space_hash(self.x.data_ptr(), self.n, self.sorb, self.nele, self.noA, self.noB,
                                                     self.plan.data_ptr(), ht.table.data_ptr(), ht.nkeys, self.lut.wf_value.data_ptr(), 1,
                                                     self.eloc.data_ptr(), self.psi0.data_ptr(), st.cuda_stream)

    def step(self):
        st = torch.cuda.current_stream(self.dev)
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(st)
        rc = self.launch_eloc(st)
        e1.record(st)
        self.N.check(rc, "pynqs_eloc_sample_space")
        # <E_loc>, variance: one packed all-reduce over the ranks (RCCL), no barrier
        from pynqs_amd.stats import dist_stats_moments
        from pynqs_amd.distributed import get_world_size

        self.stats = dist_stats_moments(self.eloc, self.prob, None, get_world_size())
        return e0, e1

    def outputs(self):
        return {"eloc": self.eloc, "psi0": self.psi0, "stats": stats_output(self.stats)}

    def parity_gate(self):
        from oracle import oracle as O

        m = min(self.n, 8)
        e, p0 = O.eloc_sample_space(self.x[:m].cpu().numpy(), self.h1.cpu().numpy(), self.h2.cpu().numpy(), self.sorb, self.nele,
                                    self.noA, self.noB, self.lut.bra_key.cpu().numpy(), self.lut.wf_value.cpu().numpy())
        de = float(np.abs(self.eloc[:m].cpu().numpy() - e).max())
        return bool(np.array_equal(self.psi0[:m].cpu().numpy(), p0)), de

    def cpu_baseline(self, budget_s=15.0):
        from oracle import oracle as O

        cores = min(len(os.sched_getaffinity(0)), 16)
        x = self.x.cpu().numpy(); h1 = self.h1.cpu().numpy(); h2 = self.h2.cpu().numpy()
        keys = self.lut.bra_key.cpu().numpy(); wf = self.lut.wf_value.cpu().numpy()
        fn = lambda m: O.eloc_sample_space(x[:m], h1, h2, self.sorb, self.nele, self.noA, self.noB, keys, wf, nthreads=cores)
        t0 = time.perf_counter()
        fn(min(self.n, 64))  # warm the thread pool; also sizes the sample: one repetition of at most a quarter of the budget
        per_walker = (time.perf_counter() - t0) / min(self.n, 64)
        sample = int(max(cores, min(self.n, 4096, budget_s * 0.2 / max(per_walker, 1e-9))))
        reps, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < budget_s * 0.8 and reps < 200:
            fn(sample); reps += 1
        el = time.perf_counter() - t0
        return {"value": sample * reps / el, "unit": "local energies/s", "cores": cores, "kind": "port",
                "sample": f"{reps} x oracle eloc_sample_space (C restatement, OpenMP) on the first {sample} walkers of the same batch ({el:.1f} s)"}


class RbmFused(Workload):
    """Complete local energies, SIMPLE method (vmc/energy/eloc.py:121-203) with the reference's real RBM amplitude
    (vmc/ansatz/rbm/rbm.py:186-211, alpha = num_hidden / sorb), in ONE kernel: enumerate, <x|H|x'>, psi(x')/psi(x)
    from the flipped orbitals, contraction.  SURVEY.md 8(d) 'fused E_loc (RBM configs)'.  Bound by the f64 vector
    rate, not by HBM: `flops_per_walker` = 3 ncomb num_hidden (one fma + one multiplication per excitation and
    hidden unit), peak 78.6 TFLOP/s."""

    F64_VECTOR_PEAK_TFLOPS = 78.6

    def __init__(self, tag, sorb, nele, noA, noB, h1, h2, walkers, dev, alpha=2):
        from pynqs_amd import C_extension as cx

        self.cx = cx
        self.name = f"{tag}_eloc_rbm"
        self.sorb, self.nele, self.noA, self.noB = sorb, nele, noA, noB
        self.h1, self.h2, self.x = h1.to(dev), h2.to(dev), walkers.to(dev).contiguous()
        self.n = self.x.size(0)
        dropin, self.ncomb = algorithmic_bytes_dropin(sorb, nele, noA, noB)
        L = (sorb - 1) // 64 + 1
        self.bytes_per_walker = dropin - self.ncomb * (8 + 8 * L) + 8
        self.H = int(alpha * sorb)
        self.flops_per_walker = 3.0 * self.ncomb * self.H
        g = torch.Generator().manual_seed(7)  # weights 0.01 (rand - 0.5), seed 7
        self.W = (0.01 * (torch.rand(self.H, sorb, generator=g, dtype=torch.float64) - 0.5)).to(dev)
        self.hb = (0.01 * (torch.rand(self.H, generator=g, dtype=torch.float64) - 0.5)).to(dev)
        self.vb = (1.0 * (torch.rand(sorb, generator=g, dtype=torch.float64) - 0.5)).to(dev)
        st = torch.cuda.current_stream(dev)
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(st)
        self.plan = cx.plan_for(self.h1, self.h2, sorb)
        e1.record(st); e1.synchronize()
        self.plan_build_ms = e0.elapsed_time(e1)
        self.prob = torch.full((self.n,), 1.0 / self.n, dtype=torch.float64, device=dev)
        self.dev, self.path, self.kernel = dev, "plan", "eloc_rbm_kernel"
        self.stats = None
        self.eloc = self.psi = None

    def step(self):
        st = torch.cuda.current_stream(self.dev)
        # the parameters change every optimisation step: the table build is part of the step
        tab = self.cx.RBMTable(self.W, self.hb, self.vb)
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(st)
        self.eloc, self.psi = self.cx.eloc_rbm(self.x, self.h1, self.h2, tab, self.sorb, self.nele, self.noA, self.noB)
        e1.record(st)
        from pynqs_amd.stats import dist_stats_moments
        from pynqs_amd.distributed import get_world_size

        self.stats = dist_stats_moments(self.eloc, self.prob, None, get_world_size())
        return e0, e1

    def outputs(self):
        return {"eloc": self.eloc, "psi": self.psi, "stats": stats_output(self.stats)}

    def _oracle(self, m, nthreads=0):
        from oracle import oracle as O

        return O.eloc_simple_rbm(self.x[:m].cpu().numpy(), self.h1.cpu().numpy(), self.h2.cpu().numpy(), self.sorb, self.nele,
                                 self.noA, self.noB, self.W.cpu().numpy(), self.hb.cpu().numpy(), self.vb.cpu().numpy(), nthreads=nthreads)

    def parity_gate(self):
        # the oracle evaluates the RBM on every x': sorb * num_hidden multiply-adds per column, one thread per walker
        cost = float(self.ncomb) * self.H * self.sorb
        m = int(min(self.n, 8, 1e10 // cost))
        if m < 1:  # minutes of CPU time per walker: covered by tests/test_gpu_rbm.py at sizes the oracle finishes
            return None, None
        e, p0 = self._oracle(m)
        de = float(np.abs(self.eloc[:m].cpu().numpy() - e).max())
        return bool(np.allclose(self.psi[:m].cpu().numpy(), p0, rtol=1e-12, atol=0)), de

    def cpu_baseline(self, budget_s=15.0):
        cores = min(len(os.sched_getaffinity(0)), 16)
        if float(self.ncomb) * self.H * self.sorb > 1e10:  # sorb 120, alpha 2: 1.0 local energies/s on 16 threads (measured once)
            return None
        self._oracle(min(self.n, 16), cores)
        sample = min(self.n, 256)
        reps, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < budget_s * 0.8 and reps < 200:
            self._oracle(sample, cores); reps += 1
        el = time.perf_counter() - t0
        return {"value": sample * reps / el, "unit": "local energies/s", "cores": cores, "kind": "port",
                "sample": f"{reps} x oracle eloc_simple_rbm (C restatement: materialise + RBM forward on every x', OpenMP) on the first {sample} walkers ({el:.1f} s)"}


class VmcStep(SampleSpaceFused):
    """One complete local-energy step of a VMC iteration for this rank's walker shard (north star):
      1. E_loc(x) for every walker: fused SAMPLE_SPACE kernel (psi(x') from the hash table of the sampled determinants, complex128);
      2. <E>, var: weighted-moments kernel + ONE packed all-reduce of 4 doubles over the ranks (RCCL; dist_stats.py:18-56 issues two
         all-reduce + barrier pairs);
      3. gradient estimator (energy_grad.py:118-184): +-1 states (onv_to_tensor), loss = 2 Re sum p conj(ln psi)(E_loc - <E>) in
         micro-batches under DistributedDataParallel.no_sync(), the last backward runs DDP's bucketed all-reduce (RCCL over xGMI).
         By default the forward + backward is replayed from a HIP graph and followed by ONE all-reduce of the flat gradient buffer
         (GraphedGrad: same estimator, same mean-over-ranks reduction as DDP); --eager-grad runs grad() under DDP instead.
    The amplitude module is a complex128 RBM (alpha = 1, seeded; ansatz families are outside this package) standing in for the example's
    BDG-RNN: its forward/backward on 8192 x 40 inputs is ~60 small PyTorch kernels, reported separately as `grad_ms`."""

    def __init__(self, tag, sorb, nele, noA, noB, h1, h2, walkers, keys, dev, micro_batch=50000, graphed=True):
        super().__init__(tag, sorb, nele, noA, noB, h1, h2, walkers, keys, dev)
        import torch.distributed as dist

        from pynqs_amd import C_extension as cx, grad as G
        from pynqs_amd.rbm import ComplexRBM

        self.name = f"{tag}_vmc_step"
        self.cx, self.G = cx, G
        g = torch.Generator().manual_seed(7)
        H = sorb
        m = ComplexRBM(0.02 * (torch.rand(H, sorb, 2, generator=g, dtype=torch.float64) - 0.5),
                       0.02 * (torch.rand(H, 2, generator=g, dtype=torch.float64) - 0.5),
                       0.05 * (torch.rand(sorb, 2, generator=g, dtype=torch.float64) - 0.5)).to(dev)
        self.module = m
        # (the DDP wrapper only for the eager estimator: its reducer hooks must not sit on a module whose backward is graph-captured)
        self.nqs = torch.nn.parallel.DistributedDataParallel(m, device_ids=[dev.index]) if dist.is_initialized() and not graphed else m
        self.micro_batch = micro_batch
        self.phase_events = []
        # gradient estimator: forward + backward replayed from a HIP graph, then ONE RCCL all-reduce of the flat gradient buffer
        # (pynqs_amd.grad.GraphedGrad; mean over the ranks = DistributedDataParallel's convention); --eager-grad: grad() under DDP
        # the estimator's gradient: for an RBM analytically from the packed walkers (pynqs_rbm_grad; --autograd-grad: the module's forward +
        # backward replayed from a HIP graph, what any other ansatz gets); either way one all-reduce of the flat gradient buffer
        self.graphed = (G.FusedRbmGrad(m, sorb) if os.environ.get("PYNQS_BENCH_AUTOGRAD_GRAD") != "1" else
                        G.GraphedGrad(m, self.n, sorb, torch.complex128, dev)) if graphed else None
        self.fused_grad = isinstance(self.graphed, G.FusedRbmGrad)
        if self.graphed is not None:
            self.graphed.events = []

    def step(self):
        st = torch.cuda.current_stream(self.dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record(st)
        rc = self.launch_eloc(st)
        ev[1].record(st)
        self.N.check(rc, "pynqs_eloc_sample_space")
        from pynqs_amd.distributed import get_world_size
        from pynqs_amd.stats import dist_stats_moments

        self.stats = dist_stats_moments(self.eloc, self.prob, None, get_world_size())
        ev[2].record(st)
        states = None if self.fused_grad else self.cx.onv_to_tensor(self.x, self.sorb)
        for p in self.module.parameters():
            p.grad = None
        if self.graphed is not None:
            self.loss = self.graphed(self.x if self.fused_grad else states, self.prob, self.eloc, self.stats[0])
        else:
            self.loss = self.G.grad(self.nqs, states, self.prob, self.eloc, self.stats[0], 1.0, torch.complex128, self.micro_batch)
        ev[3].record(st)
        self.phase_events.append(ev)
        return ev[0], ev[1]

    def outputs(self):
        return {**super().outputs(), "loss": self.loss, **grad_outputs(self.module)}

    def phases_ms(self):
        """Mean GPU-timeline duration of (E_loc kernel, moments + all-reduce, states + gradient estimator) over the recorded steps."""
        evs, self.phase_events = self.phase_events, []
        if not evs:
            return None
        k = len(evs)
        out = {"eloc_kernel_ms": sum(e[0].elapsed_time(e[1]) for e in evs) / k,
               "stats_allreduce_ms": sum(e[1].elapsed_time(e[2]) for e in evs) / k,  # moments kernel + packed all-reduce + closing kernel
               "grad_ms": sum(e[2].elapsed_time(e[3]) for e in evs) / k}
        if self.graphed is not None and self.graphed.events:
            ge = self.graphed.events[-k:]
            out["grad_allreduce_ms"] = sum(a.elapsed_time(b) for a, b in ge) / len(ge)  # part of grad_ms (0 work at N = 1)
            self.graphed.events = []
        return out

    def cpu_baseline(self, budget_s=15.0):
        """The reference's own CPU extension (oracle/_ref, compiled from its sources where they lie) running the reference's
        SAMPLE_SPACE algorithm (vmc/energy/eloc.py:326-401): get_comb_hij_fused -> wavefunction_lut on all x' -> scatter of the hits
        -> contraction, on 16 host threads and on 1 (run.sh:3).  Falls back to the oracle port when oracle/_ref is absent."""
        ref_dir = os.path.join(ROOT, "oracle", "_ref")
        if not (self.sorb <= 64 and os.path.exists(os.path.join(ref_dir, "C_extension.so"))):
            return super().cpu_baseline(budget_s)
        sys.path.insert(0, ref_dir)
        import C_extension as ref  # noqa: the reference module, MAX_SORB_LEN = 1

        cores = min(len(os.sched_getaffinity(0)), 16)
        x = self.x.cpu(); h1 = self.h1.cpu(); h2 = self.h2.cpu()
        keys = self.lut.bra_key.cpu().contiguous(); wf = self.lut.wf_value.cpu()

        def fn(m):
            xs = x[:m].contiguous()
            comb, hij = ref.get_comb_hij_fused(xs, h1, h2, self.sorb, self.nele, self.noA, self.noB)
            flat = comb.reshape(-1, comb.size(2))
            idx, mask = ref.wavefunction_lut(keys, flat, self.sorb)
            psi = torch.zeros(flat.size(0), dtype=wf.dtype)
            psi[mask] = wf[idx[mask]]
            psi = psi.reshape(m, -1)
            return ((psi.T / psi[:, 0]).T * hij).sum(-1)

        def run(threads, budget):
            torch.set_num_threads(threads)
            m = 64
            t0 = time.perf_counter(); e = fn(m); per = (time.perf_counter() - t0) / m
            sample = int(max(64, min(self.n, 2048, budget * 0.25 / max(per, 1e-9))))
            reps, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < budget * 0.8 and reps < 100:
                e = fn(sample); reps += 1
            el = time.perf_counter() - t0
            return sample * reps / el, sample, reps, el, e

        v16, s16, r16, el16, e = run(cores, budget_s)
        dev_e = self.eloc[: e.numel()].cpu()
        agree = float((dev_e - e).abs().max())
        v1, s1, r1, el1, _ = run(1, 3.0)
        torch.set_num_threads(cores)
        return {"value": v16, "unit": "local energies/s", "cores": cores, "kind": "reference",
                "sample": f"{r16} x (reference get_comb_hij_fused + wavefunction_lut + contraction, eloc.py:326-401) on the first {s16} walkers of the same batch ({el16:.1f} s)",
                "max_abs_diff_gpu_vs_reference": agree,
                "one_thread": {"value": v1, "unit": "local energies/s", "cores": 1, "sample": f"{r1} x the same on the first {s1} walkers ({el1:.1f} s)"}}


class ReduceVmcStep(Workload):
    """One complete local-energy step with the method the Fe2S2 example itself runs (example/Fe2S2/Fe2S2-OO-dcut-20.py:103-113:
    ElocMethod.REDUCE, eps = 1e-2, eps_sample = 1000; vmc/energy/eloc.py:205-324), for this rank's walker shard:
      1. the REDUCE front end in ONE kernel (pynqs_reduce_onepass): every column of every walker's row enumerated, |<x|H|x'>| >= eps kept,
         the N = 1000 draws of the reference's torch.multinomial drawn inside the kernel from the sub-eps part, every selected x'
         de-duplicated through a hash table and the +-1 rows of the DISTINCT x' written as the amplitude module's input;
      2. psi on the distinct x' by the amplitude module (PyTorch-ROCm; ~1.5 M rows per 8192 walkers);
      3. E_loc(x) = sum_records w psi(x') / psi(x): one kernel (pynqs_reduce_contract);
      4. <E>, var: weighted-moments kernel + ONE packed all-reduce over the ranks (RCCL);
      5. the gradient estimator of vmc/grad/energy_grad.py:118-184 on the walkers (HIP-graph replay + one all-reduce of the flat
         gradient buffer, or grad() under DistributedDataParallel with --eager-grad).
    Nothing of size walkers x ncomb exists at any point, and nothing is read back between 1 and 5: buffers have fixed capacities
    (sized by one calibration call outside the timed region) and the overflow word is checked after the timed region.
    The amplitude module is a complex128 RBM (alpha = 1, seeded; ansatz families are outside this package) standing in for the
    example's BDG-RNN.  For an RBM ansatz pynqs_amd.energy evaluates psi on the distinct x' with one kernel from the packed bits
    (pynqs_rbm_forward) -- the default here; --torch-amplitudes runs the PyTorch module on the +-1 rows instead (what any other ansatz gets)."""

    bound = "valu"

    def __init__(self, tag, sorb, nele, noA, noB, h1, h2, walkers, dev, eps=1e-2, eps_sample=1000, micro_batch=50000, graphed=True,
                 fused_amplitudes=True, module=None, module_dtype=torch.complex128, fp_batch=0, autograd_grad=None):
        import torch.distributed as dist

        from pynqs_amd import _native as N, C_extension as cx, energy as E, grad as G, reduce_front as RF

        self.fused_amplitudes = fused_amplitudes
        from pynqs_amd.rbm import ComplexRBM

        self.N, self.cx, self.G, self.RF = N, cx, G, RF
        self.name = f"{tag}_reduce_vmc_step"
        self.kernel, self.pmc_name, self.path = "reduce_onepass_list_rowout_kernel", f"{tag}_reduce_vmc_step", "plan"
        self.sorb, self.nele, self.noA, self.noB, self.dev = sorb, nele, noA, noB, dev
        self.eps, self.eps_sample = eps, eps_sample
        self.h1, self.h2, self.x = h1.to(dev), h2.to(dev), walkers.to(dev).contiguous()
        self.n = self.x.size(0)
        _, self.ncomb = algorithmic_bytes_dropin(sorb, nele, noA, noB)
        # B_fused(walker) = integral gathers + the walker's words + the result (16 bytes: complex E_loc)
        self.fused_bytes_per_walker = dropin_byte_parts(sorb, nele, noA, noB)[0] + 8 * ((sorb - 1) // 64 + 1) + 16
        st = torch.cuda.current_stream(dev)
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(st)
        self.plan = cx.plan_for(self.h1, self.h2, sorb, dev)
        e1.record(st); e1.synchronize()
        self.plan_build_ms = e0.elapsed_time(e1)
        g = torch.Generator().manual_seed(7)
        m = ComplexRBM(0.02 * (torch.rand(sorb, sorb, 2, generator=g, dtype=torch.float64) - 0.5),
                       0.02 * (torch.rand(sorb, 2, generator=g, dtype=torch.float64) - 0.5),
                       0.05 * (torch.rand(sorb, 2, generator=g, dtype=torch.float64) - 0.5)).to(dev)
        # module given (extra.fe2s2_reduce_vmc_step_module_*): ANY nn.Module on the +-1 rows of the distinct x', in chunks of fp_batch rows; then the
        # amplitudes and the gradient are PyTorch's (no RBM kernels): what an ansatz outside this package gets
        if module is not None:
            m, fused_amplitudes = module.to(dev), False
        self.module_dtype, self.fp_batch = module_dtype, int(fp_batch)
        if autograd_grad is None:
            autograd_grad = os.environ.get("PYNQS_BENCH_AUTOGRAD_GRAD") == "1" or module is not None
        self.fused_amplitudes = fused_amplitudes
        self.module = m
        self.nqs = torch.nn.parallel.DistributedDataParallel(m, device_ids=[dev.index]) if dist.is_initialized() and not graphed else m
        self.micro_batch = micro_batch
        # calibration (untimed): one self-sizing call tells how many kept columns a walker has and how many distinct x' there are
        fe0, nu = E.reduce_front(self.x, self.h1, self.h2, sorb, nele, noA, noB, eps, eps_sample, None, seed=1, pm1_dtype=torch.float64)
        kept_max = int(fe0.seg_count[: fe0.nseg].max())
        E._FRONTS.clear()
        del fe0
        torch.cuda.empty_cache()
        self.front = RF.ReduceFrontEnd(self.n, sorb, nele, noA, noB, eps_sample, torch.float64, dev, int(kept_max * 1.25) + 16, int(nu * 1.1) + 1024,
                                       torch.float64, keep_onv=False, want_pm1=not fused_amplitudes)
        self.distinct_calibrated = nu
        self.from_parents = os.environ.get("PYNQS_BENCH_RBM_FROM_SCRATCH") != "1" and cx.rbm_forward_children_supported(sorb, sorb, "complex")
        self.psi_u = torch.zeros(self.front.cap_unique, dtype=torch.complex128, device=dev)
        self.seed = self.seed0 = 12345  # (every step draws with the next seed; timed() restarts the count after the pre-heat)
        self.prob = torch.full((self.n,), 1.0 / self.n, dtype=torch.float64, device=dev)
        # the estimator's gradient: for an RBM analytically from the packed walkers (pynqs_rbm_grad; --autograd-grad: the module's forward +
        # backward replayed from a HIP graph, what any other ansatz gets); either way one all-reduce of the flat gradient buffer
        self.graphed = (G.FusedRbmGrad(m, sorb) if not autograd_grad else G.GraphedGrad(m, self.n, sorb, module_dtype, dev)) if graphed else None
        self.fused_grad = isinstance(self.graphed, G.FusedRbmGrad)
        if self.graphed is not None:
            self.graphed.events = []
        self.phase_events = []
        self.stats = self.eloc = self.psi_x = None
        self.roofline_note = ("one launch: enumeration of all columns (exact matrix elements; the sub-eps ones also as float32 through global memory), kept columns "
                              "placed by the rank of their bit in an LDS bitmap, the N draws located one lane per draw in segments of 16 columns (binary search + 64 bytes read back), hit counts by the rank of "
                              "a column's bit in an LDS bitmap, hash-table de-duplication (four 16-byte coherent probes per thread side by side), records with direct row "
                              "links, the distinct x' with their parent walkers.  `achieved` / `frac`: SURVEY 8(d)'s form -- B_fused (integral gathers counted once each + walker "
                              "+ result) x walkers / the kernel's live time against 8 TB/s; the 2 MiB integral plan lives in the L2, so it says how far the kernel is from "
                              "being memory-bound, not how good it is.  What limits the kernel is VECTOR INSTRUCTION ISSUE (`limited_by`, `valu`: SQ_INSTS_VALU per launch / "
                              "live kernel time against the 2-cycle issue peak; `frac_of_4cycle_issue`: against the rate one wave sustains); "
                              "`traffic` = (2 FETCH_SIZE + WRITE_SIZE) x 1024 of the same profile")

    def step(self):
        st = torch.cuda.current_stream(self.dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        fe = self.front
        ev[0].record(st)
        self.seed += 1
        fe.run(self.x, self.plan.buf, self.eps, self.seed, None)
        ev[1].record(st)
        if self.fused_amplitudes:
            # the RBM amplitudes of the distinct x' by one kernel from the packed bits (pynqs_rbm_forward: what energy.local_energy does for an
            # RBM ansatz); all rows: static shape, nothing read back (rows beyond the distinct count are valid and unused)
            m_ = self.module
            if self.from_parents:  # theta(x') from theta(parent walker): 4 updates per hidden unit instead of sorb; only the rows the front end filled
                psi_u = self.cx.rbm_forward_children(fe.uniq_onv, fe.uniq_parent, self.x, m_.params_weights, m_.params_hidden_bias, m_.params_visible_bias,
                                                     self.sorb, "complex", count=fe.counters, out=self.psi_u)
            else:
                psi_u = self.cx.rbm_forward(fe.uniq_onv, m_.params_weights, m_.params_hidden_bias, m_.params_visible_bias, self.sorb, "complex")
        else:
            with torch.no_grad():
                rows, fp = fe.uniq_pm1, self.fp_batch
                psi_u = self.module(rows) if not fp else torch.cat([self.module(rows[i:i + fp]) for i in range(0, rows.size(0), fp)])
        ev[2].record(st)
        self.eloc, self.psi_x = fe.contract(psi_u)
        ev[3].record(st)
        from pynqs_amd.distributed import get_world_size
        from pynqs_amd.stats import dist_stats_moments

        self.stats = dist_stats_moments(self.eloc, self.prob, None, get_world_size())
        ev[4].record(st)
        states = None if self.fused_grad else self.cx.onv_to_tensor(self.x, self.sorb)
        for p in self.module.parameters():
            p.grad = None
        if self.graphed is not None:
            self.loss = self.graphed(self.x if self.fused_grad else states, self.prob, self.eloc, self.stats[0])
        else:
            self.loss = self.G.grad(self.nqs, states, self.prob, self.eloc, self.stats[0], 1.0, self.module_dtype, self.micro_batch)
        ev[5].record(st)
        self.phase_events.append(ev)
        return ev[0], ev[1]

    def outputs(self):
        return {"eloc": self.eloc, "psi_x": self.psi_x, "stats": stats_output(self.stats), "loss": self.loss, **grad_outputs(self.module)}

    def phases_ms(self):
        evs, self.phase_events = self.phase_events, []
        if not evs:
            return None
        k = len(evs)
        names = ("reduce_front_end_kernel_ms", "amplitudes_on_distinct_rows_ms", "contraction_kernel_ms", "stats_allreduce_ms", "grad_ms")
        out = {nm: sum(e[i].elapsed_time(e[i + 1]) for e in evs) / k for i, nm in enumerate(names)}
        if self.graphed is not None and self.graphed.events:
            ge = self.graphed.events[-k:]
            out["grad_allreduce_ms"] = sum(a.elapsed_time(b) for a, b in ge) / len(ge)
            self.graphed.events = []
        cnt = self.front.counters_host()  # the one read-back, after the timed region
        if self.front.overflowed(cnt):
            raise SystemExit(f"REDUCE front end overflowed during the run: {cnt}")
        out["distinct_rows_last_step"] = cnt[0]
        out["distinct_rows_capacity"] = self.front.cap_unique
        return out

    def parity_gate(self):
        """First walkers against the CPU oracle: the kept records are exactly |<x|H|x'>| >= eps of the oracle's row (bit for bit), the
        drawn records are sub-eps columns whose weights are whole multiples of S / N adding up to N draws, and E_loc equals the sum
        over these records evaluated on the host (amplitudes by the same module on the CPU)."""
        from oracle import oracle as O

        m = min(self.n, 8)
        fe = self.front
        walker, col, w, link, _, drawn = fe.records()
        sel = walker < m
        rows = fe.rows_of(link[sel]).cpu()
        walker, col, w, drawn = walker[sel].cpu(), col[sel].cpu().long(), w[sel].cpu(), drawn[sel].cpu()
        co, ho = O.comb_hij_fused(self.x[:m].cpu().numpy(), self.h1.cpu().numpy(), self.h2.cpu().numpy(), self.sorb, self.nele, self.noA, self.noB)
        ho = torch.from_numpy(ho)
        keep = ho.abs() >= self.eps
        got = torch.zeros_like(keep)
        got[walker[~drawn], col[~drawn]] = True
        exact = bool(torch.equal(got, keep)) and bool(torch.equal(w[~drawn], ho[walker[~drawn], col[~drawn]]))
        S = torch.where(keep, torch.zeros_like(ho), ho.abs()).sum(1)
        hits = w[drawn].abs() * self.eps_sample / S[walker[drawn]]
        exact = exact and bool(torch.allclose(hits, hits.round(), atol=1e-6)) and not bool(keep[walker[drawn], col[drawn]].any())
        tot = torch.zeros(m, dtype=torch.float64).index_add_(0, walker[drawn], hits.round())
        exact = exact and bool((tot == self.eps_sample).all())
        kets = torch.from_numpy(co).reshape(m, self.ncomb, -1)[walker, col]
        assert bool(torch.equal(fe.uniq_onv.cpu()[rows], kets)), "a record's link does not lead to its determinant"
        mod = type(self.module)(*(p.detach().cpu() for p in (self.module.params_weights, self.module.params_hidden_bias, self.module.params_visible_bias)))
        bits = np.unpackbits(kets.numpy(), axis=1, bitorder="little")[:, : self.sorb].astype(np.float64) * 2 - 1
        with torch.no_grad():
            psi = mod(torch.from_numpy(bits))
        num = torch.zeros(m, dtype=torch.complex128).index_add_(0, walker, w.to(torch.complex128) * psi)
        p0 = torch.zeros(m, dtype=torch.complex128)
        p0[walker[col == 0]] = psi[col == 0]
        de = float((self.eloc[:m].cpu() - num / p0).abs().max())
        return exact, de

    def cpu_baseline(self, budget_s=20.0):
        """The reference's own CPU extension (oracle/_ref, compiled from its sources where they lie) running the reference's _reduce_psi
        algorithm (vmc/energy/eloc.py:243-318) with the same module evaluated by PyTorch on the host: get_comb_tensor -> get_hij_torch ->
        |H| >= eps mask -> torch.multinomial on the sub-eps part -> unique -> Func (torch.unique(dim=0) + onv_to_tensor + module) ->
        scatter -> contraction.  16 host threads, and 1 (run.sh:3)."""
        ref_dir = os.path.join(ROOT, "oracle", "_ref")
        if not (self.sorb <= 64 and os.path.exists(os.path.join(ref_dir, "C_extension.so"))):
            return None
        sys.path.insert(0, ref_dir)
        import C_extension as ref  # noqa: the reference module, MAX_SORB_LEN = 1

        cores = min(len(os.sched_getaffinity(0)), 16)
        x = self.x.cpu(); h1 = self.h1.cpu(); h2 = self.h2.cpu()
        mod = type(self.module)(*(p.detach().cpu() for p in (self.module.params_weights, self.module.params_hidden_bias, self.module.params_visible_bias)))
        eps, N, sorb, nele, noA, noB = self.eps, self.eps_sample, self.sorb, self.nele, self.noA, self.noB
        old = torch.get_default_dtype()

        def fn(m):
            xs = x[:m].contiguous()
            comb = ref.get_comb_tensor(xs, sorb, nele, noA, noB, False)[0]
            ncomb, L8 = comb.size(1), comb.size(2)
            hij = ref.get_hij_torch(xs, comb, h1, h2, sorb, nele)
            habs = hij.abs()
            mask = habs >= eps
            idx = torch.where(mask.flatten())[0]
            hsub = torch.where(mask, 0, habs)
            prob = hsub / hsub.sum(1, keepdim=True)
            counts = torch.multinomial(prob, N, replacement=True)
            counts += torch.arange(m).reshape(-1, 1) * ncomb
            idx1, cnt = counts.unique(sorted=True, return_counts=True)
            pf_ = prob.flatten()
            hij.view(-1)[idx1] = (cnt / N) * hij.flatten()[idx1] / pf_[idx1]
            sel = torch.cat([idx, idx1])
            xk = comb.reshape(-1, L8)[sel]
            uniq, inv = torch.unique(xk, dim=0, return_inverse=True)
            with torch.no_grad():
                psi = mod(ref.onv_to_tensor(uniq, sorb))[inv]
            full = torch.zeros(m * ncomb, dtype=psi.dtype)
            full[sel] = psi
            full = full.reshape(m, ncomb)
            return ((full.T / full[:, 0]).T * hij).sum(-1)

        def run(threads, budget):
            torch.set_num_threads(threads)
            t0 = time.perf_counter(); fn(32); per = (time.perf_counter() - t0) / 32
            sample = int(max(32, min(self.n, 1024, budget * 0.25 / max(per, 1e-9))))
            reps, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < budget * 0.8 and reps < 100:
                e = fn(sample); reps += 1
            el = time.perf_counter() - t0
            return sample * reps / el, sample, reps, el, e

        try:
            torch.set_default_dtype(torch.float64)
            v16, s16, r16, el16, e = run(cores, budget_s)
            v1, s1, r1, el1, _ = run(1, 4.0)
        finally:
            torch.set_default_dtype(old)
            torch.set_num_threads(cores)
        # the estimator is stochastic on both sides: compare the batch means of the same walkers
        dmean = abs(complex(e.mean()) - complex(self.eloc[: e.numel()].mean().cpu()))
        return {"value": v16, "unit": "local energies/s", "cores": cores, "kind": "reference",
                "sample": f"{r16} x (reference get_comb_tensor + get_hij_torch + multinomial selection + unique + module on the host + contraction, "
                          f"eloc.py:243-318) on the first {s16} walkers of the same batch ({el16:.1f} s)",
                "abs_diff_of_mean_eloc_gpu_vs_reference_same_walkers": dmean,
                "one_thread": {"value": v1, "unit": "local energies/s", "cores": 1, "sample": f"{r1} x the same on the first {s1} walkers ({el1:.1f} s)"}}


class ReduceTotalEnergy(Workload):
    """BASELINE configs[1] / configs[2] / configs[4] at their STATED sizes (N2-sized sorb 56 with 4096 walkers and an RBM -- the
    config's own ansatz family --, sorb 120 with 8192 walkers, sorb 184 with 4096 = the shard of 32768 walkers over 8 GPUs; synthetic
    integrals -- no such system ships with the reference): deterministic REDUCE local energies
    through energy.total_energy exactly as a caller gets them -- fused-aware chunks of walkers (public_function.get_nbatch(fused=...)), the
    front end of chunk k + 1 on a second stream while the amplitudes of chunk k are formed (etot.py:24-169), the one-launch front end in its
    flushing LIST form, table-less once the x' prove distinct, RBM amplitudes of the distinct x' from their parent walkers, contraction.
    A step = one total_energy call over all walkers.  The amplitude is a real RBM (alpha = 1, seeded): a stand-in for the config's
    Transformer, which is outside this package (the determinant side is what is measured; `step_phases_gpu_ms` separates the two).
    Roofline: SURVEY 8(d)'s B_fused (integral gathers counted once each + walker + result) per walker x walkers / the step's GPU time against
    8 TB/s -- these rows ARE gather-bound: the 153 / 838 MiB plan does not fit the L2 and every column's integral is a 128-byte line fill."""

    bound = "hbm"
    roofline_algorithmic = True

    def __init__(self, tag, sorb, no, walkers, dev, eps):
        from pynqs_amd import C_extension as cx, energy as E, public_function as pf
        from pynqs_amd.rbm import RealRBM

        self.E, self.pf = E, pf
        self.name, self.kernel, self.path = f"{tag}_reduce_vmc_step", "reduce_onepass_list_flush_kernel", "plan"
        self.sorb, self.nele, self.noA, self.noB, self.dev, self.eps = sorb, 2 * no, no, no, dev, eps
        h1, h2 = synth_integrals(sorb)
        self.h1, self.h2 = h1.to(dev), h2.to(dev)
        total, self.ncomb = algorithmic_bytes_dropin(sorb, 2 * no, no, no)
        g_, o_, i_ = dropin_byte_parts(sorb, 2 * no, no, no)
        self.gather_bytes_per_walker, self.out_bytes_per_walker, self.in_bytes_per_walker = g_, 8, i_
        self.bytes_per_walker = g_ + i_ + 8          # B_fused: gathers + walker words + one float64 result
        st = torch.cuda.current_stream(dev)
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(st)
        self.plan_obj = cx.plan_for(self.h1, self.h2, sorb, dev)
        self.plan = self.plan_obj.buf
        e1.record(st); e1.synchronize()
        self.plan_build_ms = e0.elapsed_time(e1)
        g = torch.Generator().manual_seed(1)
        r = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64) - 0.5  # noqa: E731
        self.module = RealRBM(0.02 * r(sorb, sorb), 0.02 * r(sorb), 0.05 * r(sorb)).to(dev)
        self.ab = lambda xx, func: pf.ansatz_batch(func, xx, 1 << 22, sorb, dev, torch.float64)  # noqa: E731
        x = synth_walkers(walkers, sorb, no, no, 4321).to(dev)
        # (the synthetic diagonal falls below eps for a few walkers: NaN there as in the reference, which total_energy refuses -- keep the others)
        old = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)
        try:
            fin = [torch.isfinite(E.local_energy(x[b:b + 1024].contiguous(), self.h1, self.h2, self.module, self.ab, sorb, 2 * no, no, no, reduce_psi=True, eps=eps)[0])
                   for b in range(0, walkers, 1024)]
            self.x = x[torch.cat(fin)].contiguous()
            self.n = self.x.size(0)
            self.walkers_per_call = E.auto_nbatch(self.x, self.h1, sorb, 2 * no, no, no, self.module, None, torch.double, True, 0, False, False, False, False)
            for _ in range(2):  # sizing calls (buffers, the decision to drop the de-duplication table)
                self._call()
        finally:
            torch.set_default_dtype(old)
        self.prob = torch.full((self.n,), 1.0 / self.n, dtype=torch.float64, device=dev)
        self.stats = self.eloc = None
        self.roofline_note = (f"whole total_energy call ({self.n} walkers in chunks of {self.walkers_per_call}: front end + amplitudes + contraction), not the "
                              "kernel alone; `kernel_only` = the flushing LIST kernel on one chunk, HIP events around the launch")

    def _call(self):
        return self.E.total_energy(self.x, 0, -1, self.h1, self.h2, self.module, self.sorb, self.nele, self.noA, self.noB, reduce_psi=True, eps=self.eps)[0]

    def step(self):
        st = torch.cuda.current_stream(self.dev)
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        old = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)
        try:
            e0.record(st)
            self.eloc = self._call()
            e1.record(st)
        finally:
            torch.set_default_dtype(old)
        from pynqs_amd.distributed import get_world_size
        from pynqs_amd.stats import dist_stats_moments

        self.stats = dist_stats_moments(self.eloc, self.prob, None, get_world_size())
        return e0, e1

    def outputs(self):
        return {"eloc": self.eloc, "stats": stats_output(self.stats)}

    def kernel_only(self, reps=5):
        """the front-end kernel alone on the first chunk (what local_energy launches for it), HIP events around the launch"""
        E = self.E
        m = min(self.n, self.walkers_per_call)
        xs = self.x[:m].contiguous()
        fe = None
        for f in E._FRONTS.values():
            if f.n == m and f.sorb == self.sorb and f.eps_sample == 0:
                fe = f
        if fe is None:
            return None
        st = torch.cuda.current_stream(self.dev)
        fe.run(xs, self.plan, self.eps, 0, None)
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            fe.run(xs, self.plan, self.eps, 0, None)
        e1.record(st); e1.synchronize()
        ms = e0.elapsed_time(e1) / reps
        alg = self.bytes_per_walker * m
        return {"kernel": self.kernel, "walkers": m, "kernel_ms": ms, "table_less": not fe.dedup, "algorithmic_bytes_per_launch": alg,
                "achieved": alg / (ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "columns_per_s": self.ncomb * m / (ms * 1e-3)}

    def _oracle_eloc(self, m, nthreads=0, batch=2):
        """the reference's _reduce_psi by the CPU oracle: materialise comb + Hmat (OpenMP over walkers), |H| >= eps, the RBM on the kept x' (numpy), contract"""
        from oracle import oracle as O

        W, hb, vb = (t.detach().cpu().numpy() for t in (self.module.weights, self.module.hidden_bias, self.module.visible_bias))
        out = np.empty(m)
        for b in range(0, m, batch):  # (a few walkers at a time: 28.6 / 212 MB of drop-in output per walker; one OpenMP thread per walker)
            xs = self.x[b:min(b + batch, m)].cpu().numpy()
            co, ho = O.comb_hij_fused(xs, self.h1.cpu().numpy(), self.h2.cpu().numpy(), self.sorb, self.nele, self.noA, self.noB, nthreads=nthreads)
            for i in range(xs.shape[0]):
                keep = np.abs(ho[i]) >= self.eps
                psi = O.rbm_real_psi(np.ascontiguousarray(co[i][keep]), self.sorb, W, hb, vb)
                p0 = O.rbm_real_psi(np.ascontiguousarray(xs[i:i + 1]), self.sorb, W, hb, vb)[0]
                out[b + i] = (ho[i][keep] * psi).sum() / p0
        return out

    def parity_gate(self):
        m = min(self.n, 4 if self.sorb < 150 else 2)
        want = self._oracle_eloc(m)
        de = float(np.abs(self.eloc[:m].cpu().numpy() - want).max())
        return bool(de <= 1e-8), de

    def _reference_baseline(self, budget_s):
        """sorb <= 64: the reference's own CPU extension (oracle/_ref, MAX_SORB_LEN 1) running the reference's deterministic _reduce_psi
        (get_comb_tensor -> get_hij_torch -> |H| >= eps -> unique -> onv_to_tensor + the module on the host -> scatter -> contraction, eloc.py:243-318)"""
        ref_dir = os.path.join(ROOT, "oracle", "_ref")
        if not (self.sorb <= 64 and os.path.exists(os.path.join(ref_dir, "C_extension.so"))):
            return None
        sys.path.insert(0, ref_dir)
        import C_extension as ref  # noqa: the reference module

        cores = min(len(os.sched_getaffinity(0)), 16)
        x, h1, h2 = self.x.cpu(), self.h1.cpu(), self.h2.cpu()
        mod = type(self.module)(*(p.detach().cpu() for p in (self.module.weights, self.module.hidden_bias, self.module.visible_bias)))
        sorb, nele, noA, noB, eps = self.sorb, self.nele, self.noA, self.noB, self.eps
        old = torch.get_default_dtype()

        def fn(m):
            xs = x[:m].contiguous()
            comb = ref.get_comb_tensor(xs, sorb, nele, noA, noB, False)[0]
            ncomb, L8 = comb.size(1), comb.size(2)
            hij = ref.get_hij_torch(xs, comb, h1, h2, sorb, nele)
            sel = torch.where(hij.abs().flatten() >= eps)[0]
            uniq, inv = torch.unique(comb.reshape(-1, L8)[sel], dim=0, return_inverse=True)
            with torch.no_grad():
                psi = mod(ref.onv_to_tensor(uniq, sorb))[inv]
            full = torch.zeros(m * ncomb, dtype=psi.dtype)
            full[sel] = psi
            full = full.reshape(m, ncomb)
            return ((full.T / full[:, 0]).T * hij).sum(-1)

        try:
            torch.set_default_dtype(torch.float64)
            torch.set_num_threads(cores)
            t0 = time.perf_counter(); fn(16); per = (time.perf_counter() - t0) / 16
            sample = int(max(16, min(self.n, 512, budget_s * 0.4 / max(per, 1e-9))))
            reps, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < budget_s * 0.8 and reps < 50:
                e = fn(sample); reps += 1
            el = time.perf_counter() - t0
        finally:
            torch.set_default_dtype(old)
        de = float((e - self.eloc[:sample].cpu()).abs().max())
        return {"value": sample * reps / el, "unit": "local energies/s", "cores": cores, "kind": "reference",
                "sample": f"{reps} x (reference get_comb_tensor + get_hij_torch + |H| >= eps + unique + module on the host + contraction, eloc.py:243-318) on the "
                          f"first {sample} walkers ({el:.1f} s)", "max_abs_diff_eloc_gpu_vs_reference_same_walkers": de}

    def cpu_baseline(self, budget_s=20.0):
        r = self._reference_baseline(budget_s)
        if r is not None:
            return r
        cores = min(len(os.sched_getaffinity(0)), 16 if self.sorb < 150 else 8)  # (one thread per walker of a batch; 212 MB of output per walker at sorb 184)
        t0 = time.perf_counter(); self._oracle_eloc(cores, cores, cores); per = time.perf_counter() - t0
        sample = cores * int(max(1, min(self.n // cores, 8, budget_s * 0.8 / max(per, 1e-6))))
        t0 = time.perf_counter(); self._oracle_eloc(sample, cores, cores); el = time.perf_counter() - t0
        return {"value": sample / el, "unit": "local energies/s", "cores": cores, "kind": "port",
                "sample": f"oracle (C restatement, one OpenMP thread per walker: comb + Hmat materialised, |H| >= eps, the RBM on the kept x', contraction; "
                          f"eloc.py:243-318) on the first {sample} walkers, {cores} at a time ({el:.1f} s)"}


class DecoderAmplitude(torch.nn.Module):
    """Stand-in for BASELINE.json's 'Transformer ansatz' (DecoderWaveFunction defaults d_model 32, 6 layers,
    8 heads, vmc/ansatz/transformer/decoder.py:43-69): an autoregressive decoder over the sorb/2 spatial orbitals (4 occupation
    states each), psi(x) = exp(1/2 sum_i log p(t_i | t_<i)) cos(phase).  Random weights (seed 7); ansatz families themselves are
    outside this package -- this only gives the psi(x') calls of the local-energy path a realistic cost."""

    def __init__(self, sorb: int, d_model: int = 32, n_layers: int = 6, n_heads: int = 8):
        super().__init__()
        self.k = sorb // 2
        self.embed = torch.nn.Embedding(5, d_model)  # 4 occupations + start token
        self.pos = torch.nn.Parameter(0.02 * torch.randn(self.k, d_model))
        layer = torch.nn.TransformerEncoderLayer(d_model, n_heads, dim_feedforward=4 * d_model, dropout=0.0, batch_first=True)
        self.layers = torch.nn.TransformerEncoder(layer, n_layers, enable_nested_tensor=False)
        self.head = torch.nn.Linear(d_model, 4)
        self.phase = torch.nn.Linear(d_model, 1)
        self.register_buffer("mask", torch.triu(torch.ones(self.k, self.k, dtype=torch.bool), diagonal=1))

    def forward(self, x):  # x: +-1 [n, sorb]
        occ = (x > 0).long()
        tok = occ[:, 0::2] + 2 * occ[:, 1::2]  # [n, k]
        inp = torch.cat([torch.full_like(tok[:, :1], 4), tok[:, :-1]], 1)
        hid = self.layers(self.embed(inp) + self.pos, mask=self.mask)
        logp = torch.log_softmax(self.head(hid), -1).gather(-1, tok.unsqueeze(-1)).squeeze(-1).sum(-1)
        return torch.exp(0.5 * logp) * torch.cos(self.phase(hid[:, -1]).squeeze(-1))


WALKER_OFFSET = None  # --scaling strong: first walker of this rank's shard (weak scaling: rank * walkers)


def make_workload(name: str, walkers: int, rank: int, dev, path: str = "plan", keys: int = 65536, graphed: bool = True) -> Workload:
    first = rank * walkers if WALKER_OFFSET is None else WALKER_OFFSET
    if name == "fe2s2_reduce_vmc_step":
        d = load_fe2s2()
        ci = d["ci_space"]
        idx = (np.arange(walkers) + first) % ci.shape[0]
        return ReduceVmcStep("fe2s2", int(d["sorb"]), int(d["nele"]), int(d["noA"]), int(d["noB"]), torch.from_numpy(d["h1e"]),
                             torch.from_numpy(d["h2e"]), torch.from_numpy(np.ascontiguousarray(ci[idx])), dev, graphed=graphed,
                             fused_amplitudes=os.environ.get("PYNQS_BENCH_TORCH_AMPLITUDES") != "1")
    if name == "fe2s2_vmc_step":
        d = load_fe2s2()
        ci = d["ci_space"]
        idx = (np.arange(walkers) + first) % ci.shape[0]
        return VmcStep("fe2s2", int(d["sorb"]), int(d["nele"]), int(d["noA"]), int(d["noB"]), torch.from_numpy(d["h1e"]),
                       torch.from_numpy(d["h2e"]), torch.from_numpy(np.ascontiguousarray(ci[idx])), torch.from_numpy(ci.copy()), dev, graphed=graphed)
    if name == "fe2s2_eloc_sample_space":
        d = load_fe2s2()
        ci = d["ci_space"]
        idx = (np.arange(walkers) + first) % ci.shape[0]
        return SampleSpaceFused("fe2s2", int(d["sorb"]), int(d["nele"]), int(d["noA"]), int(d["noB"]), torch.from_numpy(d["h1e"]),
                                torch.from_numpy(d["h2e"]), torch.from_numpy(np.ascontiguousarray(ci[idx])), torch.from_numpy(ci.copy()), dev)
    if name == "fe2s2_eloc_rbm":
        d = load_fe2s2()
        ci = d["ci_space"]
        idx = (np.arange(walkers) + first) % ci.shape[0]
        return RbmFused("fe2s2", int(d["sorb"]), int(d["nele"]), int(d["noA"]), int(d["noB"]), torch.from_numpy(d["h1e"]),
                        torch.from_numpy(d["h2e"]), torch.from_numpy(np.ascontiguousarray(ci[idx])), dev)
    if name == "fe2s2_dropin":
        d = load_fe2s2()
        ci = d["ci_space"]
        idx = (np.arange(walkers) + first) % ci.shape[0]
        return DropinFused("fe2s2", int(d["sorb"]), int(d["nele"]), int(d["noA"]), int(d["noB"]), torch.from_numpy(d["h1e"]),
                           torch.from_numpy(d["h2e"]), torch.from_numpy(np.ascontiguousarray(ci[idx])), dev, path)
    if name.startswith("syn") and name.endswith("_reduce_vmc_step"):
        sorb = int(name[3:-16])
        no = {56: 7, 120: 30, 184: 46}.get(sorb, sorb // 4)
        eps = {56: 0.47, 120: 0.49995, 184: 0.49999}.get(sorb, 0.49)
        return ReduceTotalEnergy(f"syn{sorb}", sorb, no, walkers, dev, eps)
    if name.startswith("syn") and name.endswith("_eloc_rbm"):
        sorb = int(name[3:-9])
        no = {56: 7, 120: 30, 184: 46}.get(sorb, sorb // 4)
        h1, h2 = synth_integrals(sorb)
        return RbmFused(f"syn{sorb}", sorb, 2 * no, no, no, h1, h2, synth_walkers(walkers, sorb, no, no, 4321 + rank), dev)
    if name.startswith("syn") and name.endswith("_eloc_sample_space"):
        # sample space = this rank's walkers plus seeded double excitations of them (`keys` of them, 64 Ki by default): as in a VMC step, a tiny part of
        # the connected space is in the table
        sorb = int(name[3:-18])
        no = {56: 7, 120: 30, 184: 46}.get(sorb, sorb // 4)
        h1, h2 = synth_integrals(sorb)
        x = synth_walkers(walkers, sorb, no, no, 4321 + rank)
        more = synth_connected(x, sorb, max(keys - walkers, 0), 99)
        keys = torch.unique(torch.cat([x, more]), dim=0)
        return SampleSpaceFused(f"syn{sorb}", sorb, 2 * no, no, no, h1, h2, x, keys, dev)
    if name.startswith("syn") and name.endswith("_dropin"):
        sorb = int(name[3:-7])
        no = {56: 7, 120: 30, 184: 46}.get(sorb, sorb // 4)
        h1, h2 = synth_integrals(sorb)
        return DropinFused(f"syn{sorb}", sorb, 2 * no, no, no, h1, h2, synth_walkers(walkers, sorb, no, no, 4321 + rank), dev, path)
    raise SystemExit(f"unknown workload {name}")


# ---------------------------------------------------------------------------------------------------
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # a step of the headline workload takes about a millisecond; an untimed pre-heat (below) brings the clocks up before the
    # W warm-up steps, so that short runs (--steps 20) measure sustained clocks too
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--workload", default="fe2s2_reduce_vmc_step")
    ap.add_argument("--walkers", type=int, default=8192, help="walkers per GPU")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: --walkers per GPU; strong: --total-walkers split over the GPUs as the reference splits its unique samples (SURVEY 8(e))")
    ap.add_argument("--total-walkers", type=int, default=65536, help="--scaling strong: walkers of the whole job (BASELINE configs[3]: 65536)")
    ap.add_argument("--keys", type=int, default=65536, help="sample-space size of the syn<sorb>_eloc_sample_space workloads")
    ap.add_argument("--path", default="plan", choices=["plan", "direct"], help="integral-plan kernels or direct packed-triangle kernels")
    ap.add_argument("--no-comb", action="store_true", help="diagnostic: skip the comb output (Hmat only)")
    ap.add_argument("--eager-grad", action="store_true", help="fe2s2_vmc_step: gradient estimator by grad() under DistributedDataParallel instead of the HIP-graph replay")
    ap.add_argument("--autograd-grad", action="store_true", help="fe2s2_[reduce_]vmc_step: gradient estimator by the module's forward + backward replayed from a HIP graph instead of the analytic RBM gradient kernel")
    ap.add_argument("--torch-amplitudes", action="store_true", help="fe2s2_reduce_vmc_step: psi on the distinct x' by the PyTorch module instead of the fused RBM forward kernel")
    ap.add_argument("--full", action="store_true", help="also the oracle parity of the last step, the CPU baseline and the secondary workloads under 'extra'")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="--full: skip the secondary workloads reported under 'extra'")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs (rank 0's shard) as DIR/<name>.npy")
    args = ap.parse_args()

    # The contract is ONE JSON line on stdout.  Libraries write there too (RCCL 2.26 prints a five-line version banner on its
    # first communicator): everything but the final line goes to stderr.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus N > 1 must be launched with python -m torch.distributed.run --nproc-per-node N")
    assert torch.cuda.is_available(), "bench.py needs a GPU (there is no CPU fallback)"
    # rehearsal of the N > 1 code path on a one-GPU box: PYNQS_BENCH_REHEARSAL=1 puts every rank on cuda:0 and uses gloo
    # (RCCL refuses two ranks on one device); never a measurement
    rehearsal = os.environ.get("PYNQS_BENCH_REHEARSAL") == "1"
    if rehearsal:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1 or args.workload.endswith("_vmc_step"):
        import torch.distributed as dist

        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if rehearsal:
                dist.init_process_group("gloo")
            else:
                dist.init_process_group("nccl", device_id=dev)  # RCCL over xGMI
        else:
            # N = 1 runs the same code path as N > 1 (DDP wrapper, RCCL calls on a one-rank communicator)
            import socket

            s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
            dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)

    if args.torch_amplitudes:
        os.environ["PYNQS_BENCH_TORCH_AMPLITUDES"] = "1"
    if args.autograd_grad:
        os.environ["PYNQS_BENCH_AUTOGRAD_GRAD"] = "1"
    walkers_here = args.walkers
    if args.scaling == "strong":
        # contiguous shards, the first total % world ranks one walker longer (utils/distributed/comm.py:108-111, public_function.py:720-746),
        # probabilities pre-scaled by the world size (vmc/sample.py:772)
        global WALKER_OFFSET
        from pynqs_amd.distributed import shard_bounds

        b_, e_ = shard_bounds(args.total_walkers, world, rank)
        walkers_here, WALKER_OFFSET = e_ - b_, b_
    wl = make_workload(args.workload, walkers_here, rank, dev, args.path, args.keys, not args.eager_grad)
    if args.scaling == "strong" and hasattr(wl, "prob"):
        wl.prob.fill_(world / args.total_walkers)
    if args.no_comb:
        wl.comb_ptr = None

    def barrier():
        if dist is not None:
            if rehearsal:
                dist.barrier()
            else:
                dist.barrier(device_ids=[local_rank])
        torch.cuda.synchronize(dev)

    def preheat(w, seconds=0.4):
        """Untimed: run the step until the GPU has been busy for about `seconds` (clock ramp-up), then drop the recorded events.
        The number of steps is agreed between the ranks (a step contains collectives)."""
        t0 = time.perf_counter()
        for _ in range(8):
            w.step()
        torch.cuda.synchronize(dev)
        per = max((time.perf_counter() - t0) / 8, 1e-6)
        n = torch.tensor([min(int(seconds / per), 20000)], dtype=torch.int64, device=dev)
        if dist is not None and world > 1:
            dist.all_reduce(n, op=dist.ReduceOp.MAX)
        for _ in range(int(n.item())):
            w.step()
        torch.cuda.synchronize(dev)
        if hasattr(w, "phase_events"):
            w.phase_events = []
        if getattr(w, "graphed", None) is not None:
            w.graphed.events = []

    def timed(w, warmup, steps):
        preheat(w)
        if hasattr(w, "seed0"):  # (the pre-heat's length depends on the clock: the steps after it draw the same from run to run)
            w.seed = w.seed0
        for _ in range(warmup):
            w.step()
        if hasattr(w, "phase_events"):
            w.phase_events = []
        if getattr(w, "graphed", None) is not None:
            w.graphed.events = []
        barrier()
        t0 = time.perf_counter()
        events = [w.step() for _ in range(steps)]
        barrier()
        el = time.perf_counter() - t0
        kern_ms = sum(a.elapsed_time(b) for a, b in events) / max(1, len(events))
        tmax = torch.tensor([el], dtype=torch.float64, device=dev)
        if dist is not None:
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        return float(tmax.item()), kern_ms

    def roofline(w, kern_ms):
        """Roofline of the workload's dominant kernel from its live HIP-event duration.
        HBM-bound kernels (drop-in rows): achieved = HBM-MANDATORY bytes per launch / time, against 8 TB/s.  Mandatory = what has to cross
        the HBM interface with perfect caches: outputs + walkers + each integral-plan byte at most once (min(gathers, plan)); SURVEY 8(d)'s
        algorithmic bytes, which count every gather as HBM traffic although the Fe2S2 plan (2 MiB) lives in the L2, are kept beside it.
        Vector-ALU-bound kernels: achieved = VALU wave64-instructions per launch (rocprofv3 SQ_INSTS_VALU from profiles/pmc_<workload>.json,
        scaled to this launch's walkers) / time, against the chip's issue rate CUs x SIMDs x clock / cycles-per-instruction."""
        t = kern_ms * 1e-3
        pmc_path = os.path.join(ROOT, "profiles", f"pmc_{getattr(w, 'pmc_name', w.name)}.json")
        pmc = json.load(open(pmc_path)) if os.path.exists(pmc_path) else {}
        # a stored profile counts only if it was measured on THESE native sources (tools/pmc_roofline.py stores their sha256): a stale one
        # is named, and nothing derived from its counters is quoted
        from pynqs_amd.build import source_hash

        stale = bool(pmc) and pmc.get("csrc_sha256") != source_hash()
        stale_note = None
        if stale:
            stale_note = {"stale": True, "profile": os.path.basename(pmc_path), "profile_sha256": pmc.get("csrc_sha256"), "tree_sha256": source_hash(),
                          "note": "the stored counters were measured on other native sources: re-run tools/pmc_roofline.py; counter-derived fields are omitted"}
            pmc = {}
        traffic = pmc.get("hbm_bytes_per_launch")
        if traffic is not None and hasattr(w, "walkers_per_call"):
            traffic = traffic * w.n / w.walkers_per_call   # (a step = several launches of the kernel, one per chunk of walkers: the counters are per launch)
        elif traffic is not None and pmc.get("walkers"):
            traffic = traffic * w.n / pmc["walkers"]
        if hasattr(w, "flops_per_walker"):  # f64 vector-ALU bound kernel
            ach = w.flops_per_walker * w.n / t / 1e12
            out = {"bound": "valu_f64", "kernel": w.kernel, "achieved": ach, "peak": w.F64_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s",
                   "frac": ach / w.F64_VECTOR_PEAK_TFLOPS, "traffic": traffic, "kernel_ms": kern_ms,
                   "algorithmic_flops_per_launch": w.flops_per_walker * w.n}
            if pmc.get("valu_insts_per_launch") and pmc.get("walkers"):
                # instruction-issue view: all vector instructions of the launch against the measured issue rate of f64 instructions
                # (one per 4.4 cycles per SIMD, profiles/r02_valu_peak.txt); the kernel's integer part issues faster, so this is an upper bound
                gi = pmc["valu_insts_per_launch"] * w.n / pmc["walkers"] / t / 1e9
                out["valu_issue"] = {"achieved": gi, "peak_f64": 256 * 4 * 2.4 / 4.4, "unit": "G wave64-instr/s", "frac": gi / (256 * 4 * 2.4 / 4.4),
                                     "source": pmc.get("source")}
        elif getattr(w, "bound", "hbm") == "valu":
            insts = pmc.get("valu_insts_per_launch")
            if insts is not None:
                insts = insts * w.n / pmc["walkers"]
            peak = VALU_PEAK_GINST
            ach = insts / t / 1e9 if insts else None
            out = {"bound": "valu", "kernel": w.kernel, "achieved": ach, "peak": peak, "unit": "G wave64-instr/s",
                   "frac": ach / peak if ach else None, "frac_of_4cycle_issue": ach / (peak / 2) if ach else None,
                   "traffic": traffic, "kernel_ms": kern_ms, "valu_instructions_per_launch": insts,
                   "columns_per_s": w.ncomb * w.n / t,
                   "source": pmc.get("source", f"no {os.path.basename(pmc_path)}: instruction count unknown")}
            # SURVEY 8(d)'s form beside it: algorithmic bytes of the fused path (integral gathers counted once each + the walker + the result),
            # the counters' HBM-side bytes, the L2 hit rate of the launch
            alg = getattr(w, "fused_bytes_per_walker", getattr(w, "bytes_per_walker", None))
            if alg is not None:
                out["algorithmic_bytes_per_launch"] = alg * w.n
                if alg * w.n / t / 1e9 <= HBM_PEAK_GBS:
                    out["algorithmic_frac"] = alg * w.n / t / 1e9 / HBM_PEAK_GBS
                else:  # (the key-major sample-space kernels: the column-major byte count is not what they move)
                    out["algorithmic_bytes_note"] = "SURVEY 8(d)'s column-major byte count; this kernel walks the sample-space table instead and never visits most columns: no HBM fraction is derived from it"
            if traffic:
                out["hbm_traffic_frac"] = traffic / t / 1e9 / HBM_PEAK_GBS
            if pmc.get("l2_hit_rate") is not None:
                out["l2_hit_rate"] = pmc["l2_hit_rate"]
            if pmc.get("rocprof_kernel_avg_ns"):
                out["rocprof_kernel_ms"] = pmc["rocprof_kernel_avg_ns"] * 1e-6
            if alg is not None and alg * w.n / t / 1e9 <= HBM_PEAK_GBS:
                # The contract's shape at the top level -- SURVEY 8(d): algorithmic bytes per launch / the kernel's live time against 8 TB/s --
                # with the roof that actually limits the kernel (vector instruction issue) in `valu`.  (Not where the column-major byte count
                # does not describe the kernel: the key-major sample-space kernels never visit most columns and would show 200x the peak.)
                valu = {k: out[k] for k in ("achieved", "peak", "unit", "frac", "frac_of_4cycle_issue", "valu_instructions_per_launch", "source")}
                ach_b = alg * w.n / t / 1e9
                out.update({"bound": "hbm", "limited_by": "valu", "achieved": ach_b, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach_b / HBM_PEAK_GBS, "valu": valu})
                for k in ("frac_of_4cycle_issue", "valu_instructions_per_launch", "source"):
                    out.pop(k, None)
        else:
            plan_bytes = w.plan.numel() * w.plan.element_size() if getattr(w, "plan", None) is not None else w.gather_bytes_per_walker * w.n
            mandatory = (w.out_bytes_per_walker + w.in_bytes_per_walker) * w.n + min(w.gather_bytes_per_walker * w.n, plan_bytes)
            alg = w.bytes_per_walker * w.n
            # (rows whose integral plan does not fit the L2 -- the total_energy workloads: every column's integral is a line fill of its own,
            # SURVEY 8(d)'s algorithmic bytes ARE the traffic model; `mandatory` would count the 153 / 838 MiB plan once)
            ach = (alg if getattr(w, "roofline_algorithmic", False) else mandatory) / t / 1e9
            out = {"bound": "hbm", "kernel": w.kernel, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                   "traffic": traffic, "kernel_ms": kern_ms, "hbm_mandatory_bytes_per_launch": mandatory,
                   "algorithmic_bytes_per_launch": alg, "algorithmic_frac": alg / t / 1e9 / HBM_PEAK_GBS}
            if traffic:
                out["hbm_traffic_frac"] = traffic / t / 1e9 / HBM_PEAK_GBS
        if getattr(w, "roofline_note", None):
            out["note"] = w.roofline_note
        if stale_note:
            out["stale_profile"] = stale_note
        return out

    el, kern_ms = timed(wl, args.warmup, args.steps)
    phases = wl.phases_ms() if hasattr(wl, "phases_ms") else None   # (the REDUCE steps: also the overflow check of the run)
    if args.dump_outputs and rank == 0:
        dump_outputs(wl, args.dump_outputs)

    if rank == 0:
        total_walkers = (args.total_walkers if args.scaling == "strong" else wl.n * world) * args.steps
        out = {
            "metric": "local energies/sec (whole node)" if not isinstance(wl, DropinFused) else "S+D rows/sec: enumerate + <x|H|x'> materialised, no psi (whole node)",
            "value": total_walkers / el,
            "unit": "local energies/s" if not isinstance(wl, DropinFused) else "S+D rows/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": el / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f64",
            "data": ("REHEARSAL (all ranks on one GPU, gloo): not a measurement; " if rehearsal else "") +
                    "shipped Fe2S2 integrals + ci_space walkers (tests/golden fixture)" if args.workload.startswith("fe2s2")
                    else "synthetic (seeded dense integrals, random walkers)",
            "config": {"workload": wl.name, "sorb": wl.sorb, "nele": wl.nele, "ncomb": wl.ncomb,
                       "walkers_per_gpu": wl.n, "integral_layout": wl.path, "plan_build_ms": wl.plan_build_ms,
                       **({"keys_index_build_ms": wl.index_build_ms, "keys_met_per_walker": wl.index.per_walker, "keys": wl.index.nkeys}
                          if getattr(wl, "index", None) is not None else {}),
                       "parallelism": f"walker-sharded x{world} (one process per GPU)" + (
                           ("; packed RCCL all-reduce of (sum p E_loc, sum p |E_loc|^2, sum p); gradient estimator: " +
                            ("analytic RBM gradient kernel (pynqs_rbm_grad) + one RCCL all-reduce of the flat gradient buffer (mean over ranks, as DDP)" if getattr(wl, "fused_grad", False)
                             else "HIP-graph replay + one RCCL all-reduce of the flat gradient buffer (mean over ranks, as DDP)" if wl.graphed is not None
                             else "DDP bucketed RCCL all-reduce in the last micro-batch's backward"))
                           if isinstance(wl, (VmcStep, ReduceVmcStep)) else "; packed RCCL all-reduce of (sum p E_loc, sum p |E_loc|^2, sum p)" if hasattr(wl, "stats")
                           else "; no data-path collective")},
            "roofline": roofline(wl, kern_ms),
        }
        if args.full:
            ok_c, dh = wl.parity_gate()
            out["parity"] = ({"exact_part_bit_exact": bool(ok_c), "max_abs_diff_vs_oracle": dh} if ok_c is not None
                             else "oracle too slow at this size (tests/ cover the kernel at sizes it finishes)")
        if isinstance(wl, (VmcStep, ReduceVmcStep)):
            if phases is not None:
                # what crosses xGMI per step: one packed all-reduce of the moments, one of the flat gradient buffer (+ the loss)
                phases["stats_allreduce_bytes"] = 4 * 8
                phases["grad_allreduce_bytes"] = int(sum(p.numel() for p in wl.module.parameters()) + 1) * 8
            out["step_phases_gpu_ms"] = phases
            out["config"]["amplitude_module"] = "complex128 RBM, alpha = 1 (stand-in for the example's BDG-RNN), AD_MAX_DIM = %d as in example/Fe2S2 (one micro-batch for 8192 walkers)" % wl.micro_batch
        if isinstance(wl, (VmcStep, ReduceVmcStep)):
            # what the ranks agreed on in the last step: the all-reduced moments and the all-reduced gradient (for the N > 1 rehearsal test:
            # N ranks x W walkers must give what one rank gives on the N W walkers)
            mean = wl.stats[0]
            flat = torch.cat([p.grad.reshape(-1) for p in wl.module.parameters()])
            out["check"] = {"mean_eloc": [float(mean.real), float(mean.imag) if mean.is_complex() else 0.0], "var_eloc": float(wl.stats[1]),
                            "grad_l2": float(flat.double().norm()), "grad_first": [float(v) for v in flat[:4].double().cpu()]}
        if isinstance(wl, ReduceVmcStep):
            out["config"].update({"method": "REDUCE (vmc/energy/eloc.py:205-324), the Fe2S2 example's setting", "eps": wl.eps, "eps_sample": wl.eps_sample,
                                  "amplitudes_on_distinct_rows": ("pynqs_rbm_forward_children (from the parent walkers' hidden-unit factors by table multiplications)" if getattr(wl, "from_parents", False) else "pynqs_rbm_forward (one kernel, from the packed determinants)") if wl.fused_amplitudes
                                  else "the PyTorch module on the +-1 rows"})
        if isinstance(wl, ReduceTotalEnergy):
            if args.full:
                out["roofline"]["kernel_only"] = wl.kernel_only()
            out["config"].update({"method": "REDUCE (vmc/energy/eloc.py:205-324) through total_energy (etot.py:24-169)", "eps": wl.eps, "walkers_per_local_energy_call": wl.walkers_per_call,
                                  "amplitude_module": "real RBM, alpha = 1 (stand-in for the config's Transformer), amplitudes of the distinct x' by pynqs_rbm_forward_children"})
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = wl.cpu_baseline()
    # secondary measurements (--full, same run, N = 1 only): drop-in rows, the other fused local energies and the larger word counts
    if args.full and world == 1 and not args.no_extra and args.workload in ("fe2s2_dropin", "fe2s2_vmc_step", "fe2s2_reduce_vmc_step"):
        extra = {}
        for name, nw, steps in (("fe2s2_vmc_step", args.walkers, 300), ("fe2s2_dropin", args.walkers, 2000), ("fe2s2_eloc_sample_space", args.walkers, 1000), ("fe2s2_eloc_rbm", args.walkers, 500),
                                ("syn56_eloc_rbm", 4096, 200), ("syn120_dropin", 64, 500), ("syn184_dropin", 16, 200),
                                ("syn120_eloc_sample_space", args.walkers, 10), ("syn120_eloc_rbm", 512, 10),
                                ("syn184_eloc_sample_space", args.walkers, 10), ("syn184_eloc_rbm", 128, 3),
                                # BASELINE configs[2] / configs[4] at their stated sizes: deterministic REDUCE through total_energy
                                ("syn56_reduce_vmc_step", 4096, 20), ("syn120_reduce_vmc_step", 8192, 5), ("syn184_reduce_vmc_step", 4096, 3)):
            try:
                w2 = make_workload(name, nw, rank, dev, args.path)
                el2, k2 = timed(w2, max(2, steps // 10), steps)
                ok2, d2 = w2.parity_gate()
                extra[w2.name] = {"value": w2.n * steps / el2, "unit": "S+D rows (enumerate + <x|H|x'>, no psi)/s" if name.endswith("_dropin") else "local energies/s",
                                  "walkers": w2.n, "ncomb": w2.ncomb,
                                  "ms_per_step": el2 / steps * 1e3, "roofline": roofline(w2, k2),
                                  "parity": {"exact_part_bit_exact": bool(ok2), "max_abs_diff_vs_oracle": d2} if ok2 is not None
                                            else "oracle too slow at this size (tests/ cover the kernel at sizes it finishes)"}
                if hasattr(w2, "phases_ms"):
                    extra[w2.name]["step_phases_gpu_ms"] = w2.phases_ms()
                if isinstance(w2, ReduceTotalEnergy):
                    extra[w2.name]["roofline"]["kernel_only"] = w2.kernel_only()
                    extra[w2.name]["walkers_per_local_energy_call"] = w2.walkers_per_call
                if name in ("fe2s2_dropin", "fe2s2_eloc_rbm", "fe2s2_vmc_step", "syn56_reduce_vmc_step", "syn120_reduce_vmc_step", "syn184_reduce_vmc_step") and not args.no_cpu_baseline:
                    extra[w2.name]["cpu_baseline"] = w2.cpu_baseline(budget_s=8.0)
                del w2
                torch.cuda.empty_cache()
            except Exception as e:  # pragma: no cover  (keeps the primary line intact)
                extra[name] = {"error": repr(e)}
        # the default (semi-stochastic) step with a GENERIC ansatz: the amplitudes of the distinct x' by a PyTorch module on their +-1 rows and the
        # gradient estimator by autograd -- what any ansatz outside this package gets (SURVEY 8(d)(ii'): determinant-side ms and forward ms apart)
        try:
            d5 = load_fe2s2()
            ci5 = d5["ci_space"]
            args5 = ("fe2s2", int(d5["sorb"]), int(d5["nele"]), int(d5["noA"]), int(d5["noB"]), torch.from_numpy(d5["h1e"]), torch.from_numpy(d5["h2e"]),
                     torch.from_numpy(np.ascontiguousarray(ci5[np.arange(args.walkers) % ci5.shape[0]])), dev)
            torch.manual_seed(7)
            for tag5, steps5, kw5 in (("fe2s2_reduce_vmc_step_module_rbm_torch", 20, dict(fused_amplitudes=False, autograd_grad=True)),
                                      ("fe2s2_reduce_vmc_step_module_decoder_torch", 2,
                                       dict(module=DecoderAmplitude(int(d5["sorb"])).double().eval(), module_dtype=torch.float64, fp_batch=100_000, graphed=False))):
                old5 = torch.get_default_dtype()
                torch.set_default_dtype(torch.float64)
                try:
                    w5 = ReduceVmcStep(*args5, **kw5)
                    el5, k5 = timed(w5, 2, steps5)
                    ph5 = w5.phases_ms()
                finally:
                    torch.set_default_dtype(old5)
                det5 = ph5["reduce_front_end_kernel_ms"] + ph5["contraction_kernel_ms"] + ph5["stats_allreduce_ms"]
                extra[tag5] = {"value": w5.n * steps5 / el5, "unit": "local energies/s", "walkers": w5.n, "ms_per_step": el5 / steps5 * 1e3, "step_phases_gpu_ms": ph5,
                               "determinant_side_ms": det5, "ansatz_forward_ms": ph5["amplitudes_on_distinct_rows_ms"], "gradient_ms": ph5["grad_ms"],
                               "ansatz": "pynqs_amd.rbm.ComplexRBM (complex128, alpha = 1) as a PyTorch module on all rows of the distinct list; gradient: autograd replayed from a HIP graph"
                                         if "rbm" in tag5 else "autoregressive Transformer decoder stand-in (d_model 32, 6 layers, 8 heads, f64, random weights) in chunks of 100 000 rows; gradient: eager autograd",
                               "parity": "tests/test_gpu_reduce_golden_r3.py (the same front end + contraction with modules, 1e-8 Ha against the reference)"}
                del w5
                torch.cuda.empty_cache()
        except Exception as e:  # pragma: no cover
            extra["fe2s2_reduce_vmc_step_module"] = {"error": repr(e)}
        # (ii') of SURVEY.md 8(d): enumeration + |<x|H|x'>| >= eps compaction (count and emit passes, nothing materialised),
        # what an external PyTorch ansatz is fed with; eps keeps about 1 % of the columns
        try:
            from pynqs_amd import energy as E2

            for tag, sorb2, no2, nw2, eps2 in (("fe2s2_reduce_compact_eps1e-2", 40, 15, args.walkers, 1e-2), ("syn120_reduce_compact", 120, 30, 256, 0.495),
                                               ("syn184_reduce_compact", 184, 46, 64, 0.495)):
                if sorb2 == 40:
                    d0 = load_fe2s2()
                    h1c, h2c = torch.from_numpy(d0["h1e"]).to(dev), torch.from_numpy(d0["h2e"]).to(dev)
                    xc = torch.from_numpy(np.ascontiguousarray(d0["ci_space"][np.arange(nw2) % d0["ci_space"].shape[0]])).to(dev)
                else:
                    h1c, h2c = (t.to(dev) for t in synth_integrals(sorb2))
                    xc = synth_walkers(nw2, sorb2, no2, no2, 4321).to(dev)
                fn = lambda: E2.reduce_compact(xc, h1c, h2c, sorb2, 2 * no2, no2, no2, eps2)
                fn(); torch.cuda.synchronize(dev)
                t0 = time.perf_counter(); reps = 5
                for _ in range(reps):
                    r_ = fn()
                torch.cuda.synchronize(dev)
                el4 = (time.perf_counter() - t0) / reps
                ncomb2 = algorithmic_bytes_dropin(sorb2, 2 * no2, no2, no2)[1]
                extra[tag] = {"value": nw2 / el4, "unit": "walkers/s", "walkers": nw2, "ncomb": int(ncomb2), "ms_per_step": el4 * 1e3,
                              "columns_per_s": nw2 * ncomb2 / el4, "kept_per_walker": r_[1].numel() / nw2, "eps": eps2}
                del h1c, h2c, xc, r_
                torch.cuda.empty_cache()
        except Exception as e:  # pragma: no cover
            extra["reduce_compact"] = {"error": repr(e)}
        # deterministic REDUCE local energies beyond Fe2S2 (N2-, C3- and C5-sized rows, synthetic integrals) through energy.local_energy with
        # the RBM forward kernel on the x': the one-launch front end as local_energy routes it (flushing LIST form, table-less once the
        # x' prove distinct) beside round 2's multi-pass path
        try:
            from pynqs_amd import energy as E6, public_function as pf6
            from pynqs_amd.rbm import RealRBM as RealRBM6

            old_default6 = torch.get_default_dtype()
            torch.set_default_dtype(torch.float64)
            for tag, sorb6, no6, nw6, eps6, ns6 in (("syn56_reduce_local_energy", 56, 7, 4096, 0.47, 0), ("syn120_reduce_local_energy", 120, 30, 4096, 0.49995, 0),
                                                    ("syn184_reduce_local_energy", 184, 46, 1024, 0.49999, 0),
                                                    ("syn56_reduce_sample1000_local_energy", 56, 7, 4096, 0.47, 1000),
                                                    ("syn120_reduce_sample1000_local_energy", 120, 30, 1024, 0.4995, 1000)):
                h1c, h2c = (t.to(dev) for t in synth_integrals(sorb6))
                xc = synth_walkers(nw6, sorb6, no6, no6, 4321).to(dev)
                g6 = torch.Generator().manual_seed(1)
                m6 = RealRBM6(0.02 * (torch.rand(sorb6, sorb6, generator=g6) - 0.5), 0.02 * (torch.rand(sorb6, generator=g6) - 0.5),
                              0.05 * (torch.rand(sorb6, generator=g6) - 0.5)).to(dev)
                ab6 = lambda xx, func: pf6.ansatz_batch(func, xx, 1 << 22, sorb6, dev, torch.float64)  # noqa: E731
                res6 = {}
                for mode, onepass in (("one_launch_front_end", True), ("multi_pass_round2", False)):
                    old_op, E6.FUSED_ONEPASS = E6.FUSED_ONEPASS, onepass
                    try:
                        fn = lambda: E6.local_energy(xc, h1c, h2c, m6, ab6, sorb6, 2 * no6, no6, no6, reduce_psi=True, eps=eps6, eps_sample=ns6)[0]
                        fn(); fn(); fn(); torch.cuda.synchronize(dev)   # (sizing call, the call that may drop the table, one more)
                        t0 = time.perf_counter(); reps = 3
                        for _ in range(reps):
                            e6 = fn()
                        torch.cuda.synchronize(dev)
                        res6[mode] = ((time.perf_counter() - t0) / reps, e6)
                    finally:
                        E6.FUSED_ONEPASS = old_op
                el6, e6 = res6["one_launch_front_end"]
                fin6 = torch.isfinite(e6) & torch.isfinite(res6["multi_pass_round2"][1])
                ncomb6 = algorithmic_bytes_dropin(sorb6, 2 * no6, no6, no6)[1]
                extra[tag] = {"value": nw6 / el6, "unit": "local energies/s", "walkers": nw6, "ncomb": int(ncomb6), "eps": eps6, "eps_sample": ns6,
                              "ms_per_step": el6 * 1e3, "columns_per_s": nw6 * ncomb6 / el6, "multi_pass_round2_ms": res6["multi_pass_round2"][0] * 1e3,
                              "table_less": any(v is not None for k, v in E6._FRONT_NODEDUP.items() if k[2] == sorb6 and (k[6] > 0) == (ns6 > 0))}
                if ns6 == 0:
                    extra[tag]["max_abs_diff_between_the_paths"] = float((e6 - res6["multi_pass_round2"][1])[fin6].abs().max())
                else:  # (different draws on the two paths, and dense synthetic integrals make single estimates noisy: parity of this form is
                    # tests/test_gpu_reduce_route.py::test_semi_stochastic_flushing_form -- kept records bit-identical, draws checked one by one)
                    extra[tag]["parity"] = "tests/test_gpu_reduce_route.py::test_semi_stochastic_flushing_form"
                del h1c, h2c, xc, res6, e6
                E6._FRONTS.clear()
                torch.cuda.empty_cache()
            # BASELINE configs[2]'s size with the METHOD the Fe2S2 example runs (semi-stochastic REDUCE, 1000 draws): 8192 walkers at sorb 120 through
            # total_energy (fused-aware chunks, look-ahead stream; the draws read the drawn tiles back from the row's float32 copy)
            h1c, h2c = (t.to(dev) for t in synth_integrals(120))
            xc = synth_walkers(8192, 120, 30, 30, 4321).to(dev)
            g6 = torch.Generator().manual_seed(1)
            m6 = RealRBM6(0.02 * (torch.rand(120, 120, generator=g6) - 0.5), 0.02 * (torch.rand(120, generator=g6) - 0.5), 0.05 * (torch.rand(120, generator=g6) - 0.5)).to(dev)
            ab120 = lambda xx, func: pf6.ansatz_batch(func, xx, 1 << 22, 120, dev, torch.float64)  # noqa: E731
            fin6 = torch.cat([torch.isfinite(E6.local_energy(xc[b:b + 1024].contiguous(), h1c, h2c, m6, ab120, 120, 60, 30, 30, reduce_psi=True, eps=0.4995)[0]) for b in range(0, 8192, 1024)])
            xs6 = xc[fin6].contiguous()   # (walkers whose diagonal falls below eps are NaN, as in the reference: total_energy refuses them)
            E6._FRONTS.clear()
            fn = lambda: E6.total_energy(xs6, 0, -1, h1c, h2c, m6, 120, 60, 30, 30, reduce_psi=True, eps=0.4995, eps_sample=1000)[0]  # noqa: E731
            fn(); fn(); torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(3):
                e6 = fn()
            torch.cuda.synchronize(dev)
            el6 = (time.perf_counter() - t0) / 3
            nb6 = E6.auto_nbatch(xs6, h1c, 120, 60, 30, 30, m6, None, torch.double, True, 1000, False, False, False, False)
            extra["syn120_reduce_sample1000_total_energy_8192_walkers"] = {
                "value": xs6.size(0) / el6, "unit": "local energies/s", "walkers": int(xs6.size(0)), "ncomb": 1190251, "eps": 0.4995, "eps_sample": 1000,
                "ms_per_step": el6 * 1e3, "walkers_per_local_energy_call": int(nb6), "finite": int(torch.isfinite(e6).sum()),
                "parity": "tests/test_gpu_reduce_route.py::test_semi_stochastic_flushing_form, ::test_long_row_forms_against_the_oracle[120-30-16-0.4995-200-True]"}
            del h1c, h2c, xc, xs6, e6
            E6._FRONTS.clear()
            torch.cuda.empty_cache()
            torch.set_default_dtype(old_default6)
        except Exception as e:  # pragma: no cover
            extra["reduce_local_energy_large"] = {"error": repr(e)}
        # fused-aware chunking (public_function.get_nbatch(fused=...), total_energy(nbatch=0)): the example's batch of 2048 walkers per
        # local_energy call against chunks sized for what the fused path allocates, on 65 536 walkers (C4's global batch)
        try:
            from pynqs_amd import energy as E3, public_function as pf3

            d3 = load_fe2s2()
            sorb3, nele3, noA3, noB3 = int(d3["sorb"]), int(d3["nele"]), int(d3["noA"]), int(d3["noB"])
            ci3 = d3["ci_space"]
            h1c, h2c = torch.from_numpy(d3["h1e"]).to(dev), torch.from_numpy(d3["h2e"]).to(dev)
            x65 = torch.from_numpy(np.ascontiguousarray(ci3[np.arange(65536) % ci3.shape[0]])).to(dev)
            g3 = torch.Generator().manual_seed(7)
            wf3 = torch.polar(torch.exp(-3.0 * torch.rand(ci3.shape[0], generator=g3, dtype=torch.float64)), 2 * np.pi * torch.rand(ci3.shape[0], generator=g3, dtype=torch.float64))
            lut3 = pf3.WavefunctionLUT(torch.from_numpy(ci3.copy()).to(dev), wf3.to(dev), sorb3, device=dev)
            res = {}
            for tag, nb in (("nbatch_2048_as_in_the_example", 2048), ("nbatch_auto_fused_aware", 0)):
                fn = lambda: E3.total_energy(x65, nb, -1, h1c, h2c, None, sorb3, nele3, noA3, noB3, WF_LUT=lut3, use_sample_space=True, dtype=torch.complex128)
                fn(); torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(5):
                    e3, _, _ = fn()
                torch.cuda.synchronize(dev)
                el5 = (time.perf_counter() - t0) / 5
                res[tag] = {"value": 65536 / el5, "unit": "local energies/s", "ms_per_call": el5 * 1e3, "mean_eloc_re": float(e3.mean().real)}
            res["walkers_per_call_auto"] = E3.auto_nbatch(x65, h1c, sorb3, nele3, noA3, noB3, None, lut3, torch.complex128, False, 0, True, False, False, False)
            extra["fe2s2_total_energy_sample_space_65536_walkers_chunking"] = res
            del x65, lut3, h1c, h2c
            torch.cuda.empty_cache()
        except Exception as e:  # pragma: no cover
            extra["chunking"] = {"error": repr(e)}
        # the generic amplitude path: psi(x') by a PyTorch-ROCm module (real RBM, alpha = 2) through
        # pynqs_amd.energy.local_energy -- SIMPLE (every column) and REDUCE (eps = 1e-2, the Fe2S2 example's setting)
        try:
            from pynqs_amd import energy as E, public_function as pf
            from pynqs_amd.rbm import RealRBM

            d = load_fe2s2()
            sorb, nele, noA, noB = int(d["sorb"]), int(d["nele"]), int(d["noA"]), int(d["noB"])
            g = torch.Generator().manual_seed(7)
            rbm = RealRBM(0.01 * (torch.rand(2 * sorb, sorb, generator=g, dtype=torch.float64) - 0.5),
                          0.01 * (torch.rand(2 * sorb, generator=g, dtype=torch.float64) - 0.5),
                          0.1 * (torch.rand(sorb, generator=g, dtype=torch.float64) - 0.5)).to(dev)
            h1g, h2g = torch.from_numpy(d["h1e"]).to(dev), torch.from_numpy(d["h2e"]).to(dev)
            old_default = torch.get_default_dtype()
            torch.set_default_dtype(torch.float64)
            old_fused_rbm, E.FUSED_RBM = E.FUSED_RBM, False  # this line measures the generic module path
            for tag, nw, kw in (("fe2s2_eloc_simple_rbm_torch", 512, {}), ("fe2s2_eloc_reduce_eps1e-2_rbm_torch", 8192, {"reduce_psi": True, "eps": 1e-2}),
                                ("fe2s2_eloc_reduce_eps1e-2_sample1000_rbm_torch", 8192, {"reduce_psi": True, "eps": 1e-2, "eps_sample": 1000})):
                xg = torch.from_numpy(np.ascontiguousarray(d["ci_space"][:nw])).to(dev)
                fn = lambda: E.total_energy(xg, nw, 2_000_000, h1g, h2g, rbm, sorb, nele, noA, noB, use_unique=True, **kw)
                fn(); fn(); torch.cuda.synchronize(dev)
                times = []
                for _ in range(5):  # median of five: a step that has to grow the caching allocator's pool costs milliseconds once
                    t0 = time.perf_counter()
                    e_, _, _ = fn()
                    torch.cuda.synchronize(dev)
                    times.append(time.perf_counter() - t0)
                el3 = sorted(times)[2]
                extra[tag] = {"value": nw / el3, "unit": "local energies/s", "walkers": nw, "ms_per_step": el3 * 1e3,
                              "mean_eloc": float(e_.mean().item())}
            # BASELINE config C3: the same REDUCE local energies with a Transformer-decoder amplitude (stand-in, see DecoderAmplitude)
            torch.manual_seed(7)
            dec = DecoderAmplitude(sorb).to(dev).double().eval()
            xg = torch.from_numpy(np.ascontiguousarray(d["ci_space"][:8192])).to(dev)
            fn = lambda: E.total_energy(xg, 8192, 200_000, h1g, h2g, dec, sorb, nele, noA, noB, use_unique=True, reduce_psi=True, eps=1e-2)
            fn(); torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            e_, _, _ = fn()
            torch.cuda.synchronize(dev)
            el3 = time.perf_counter() - t0
            t0 = time.perf_counter()
            row_, col_, onv_, h_, cnt_ = E.reduce_compact(xg, h1g, h2g, sorb, nele, noA, noB, 1e-2)
            torch.cuda.synchronize(dev)
            el4 = time.perf_counter() - t0
            extra["fe2s2_eloc_reduce_eps1e-2_decoder_torch"] = {
                "value": 8192 / el3, "unit": "local energies/s", "walkers": 8192, "ms_per_step": el3 * 1e3, "mean_eloc": float(e_.mean().item()),
                "ansatz": "autoregressive Transformer decoder, d_model 32, 6 layers, 8 heads, f64, random weights (stand-in)",
                "determinant_part_ms": el4 * 1e3}
            # the reference's other real-parameter RBM amplitudes on the fused kernel, and one GFMC step (fixed-node Green's-function row + move)
            # with the real RBM as trial function: fused kernels against comb + module
            from pynqs_amd import C_extension as CXm, gfmc as GF

            xg = torch.from_numpy(np.ascontiguousarray(d["ci_space"][:8192])).to(dev)
            tab = CXm.RBMTable(rbm.weights.detach(), rbm.hidden_bias.detach(), rbm.visible_bias.detach())

            def _timed(fn, reps):
                fn(); torch.cuda.synchronize(dev)
                t0_ = time.perf_counter()
                for _ in range(reps):
                    r_ = fn()
                torch.cuda.synchronize(dev)
                return (time.perf_counter() - t0_) / reps, r_

            for kind in ("tanh", "pRBM"):
                el5, (e5, _) = _timed(lambda: CXm.eloc_rbm(xg, h1g, h2g, tab, sorb, nele, noA, noB, rbm_type=kind), 20)
                extra[f"fe2s2_eloc_rbm_{kind}"] = {"value": 8192 / el5, "unit": "local energies/s", "walkers": 8192, "ms_per_step": el5 * 1e3,
                                                   "mean_eloc": [float(e5.mean().real), float(e5.mean().imag) if e5.is_complex() else 0.0]}
            # complex128 parameters in the kernel (alpha = 1, the size of the default step's module)
            gc = torch.Generator().manual_seed(13)
            ctab = CXm.CRBMTable((0.02 * (torch.rand(sorb, sorb, 2, generator=gc, dtype=torch.float64) - 0.5)).to(dev),
                                 (0.02 * (torch.rand(sorb, 2, generator=gc, dtype=torch.float64) - 0.5)).to(dev),
                                 (0.05 * (torch.rand(sorb, 2, generator=gc, dtype=torch.float64) - 0.5)).to(dev))
            el5, (e5, _) = _timed(lambda: CXm.eloc_crbm(xg, h1g, h2g, ctab, sorb, nele, noA, noB), 10)
            extra["fe2s2_eloc_crbm"] = {"value": 8192 / el5, "unit": "local energies/s", "walkers": 8192, "ms_per_step": el5 * 1e3, "num_hidden": sorb,
                                        "mean_eloc": [float(e5.mean().real), float(e5.mean().imag)]}
            ab_ = lambda xx, func: pf.ansatz_batch(func, xx, 2_000_000, sorb, dev, torch.double)  # noqa: E731
            wgt = torch.ones(8192, dtype=torch.float64, device=dev)
            for tag, nw, fused in (("fe2s2_gfmc_step_rbm_fused", 8192, True), ("fe2s2_gfmc_step_rbm_module", 512, False)):
                GF.FUSED_GREEN = fused

                def gstep():
                    el_, gk_, comb_, _, _ = GF.green_kernel(xg[:nw], -100.0, h1g, h2g, rbm, ab_, sorb, nele, noA, noB, torch.double, None, True)
                    return GF.sample_update(xg[:nw], wgt[:nw], comb_, gk_)

                el6, (_, _, beta_, acc_) = _timed(gstep, 5)
                extra[tag] = {"value": nw / el6, "unit": "walker moves/s", "walkers": nw, "ms_per_step": el6 * 1e3, "accepted": int(acc_),
                              "mean_beta": float(beta_.mean().item())}
            GF.FUSED_GREEN = True
            torch.set_default_dtype(old_default)
            E.FUSED_RBM = old_fused_rbm
        except Exception as e:  # pragma: no cover
            extra["fe2s2_eloc_rbm_torch"] = {"error": repr(e)}
        out["extra"] = extra
    if rank == 0:
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    if dist is not None:
        barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
