"""Table-backed modules for tests that must feed energy.local_energy GIVEN amplitudes: psi(x) (or f(x) of the multi-psi form) by look-up
of the determinant, so that nothing of a network's forward pass enters a comparison.  (tests/test_gpu_reduce_golden_r3.py keeps its own
copy of the same two classes.)"""
import types

import torch


class Holder:
    """what local_energy(use_multi_psi=True) expects of its ansatz: .module.sample (psi) and .module.extra (f)"""

    def __init__(self, sample, extra):
        self.module = types.SimpleNamespace(sample=sample, extra=extra)


class TableAmplitude(torch.nn.Module):
    """forward(+-1 rows [n, sorb]) -> the table's value of every row; a row the table does not hold is an error"""

    def __init__(self, keys, values, sorb):
        super().__init__()
        from pynqs_amd import public_function as pf

        self.lut = pf.WavefunctionLUT(keys, values, sorb, device=keys.device)
        self.sorb = sorb

    def forward(self, x):
        from pynqs_amd import C_extension as cx

        onv = cx.tensor_to_onv((x > 0).to(torch.uint8), self.sorb)
        pos, found = self.lut.find(onv)
        assert bool(found.all()), "a determinant without an amplitude was asked for"
        return self.lut.wf_value[pos]
