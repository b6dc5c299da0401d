"""The wave sums of the REDUCE front end (pynqs_amd/csrc/reduce_common.h) lane by lane: op_wave_sum reaches the partner lane ^ d of every
butterfly step by cross-lane moves of a fixed pattern (v_permlane32_swap, v_permlane16_swap, DPP row_ror:8, ds_swizzle xor 4, DPP quad_perm),
op_wave_sum_shfl by __shfl_xor.  A pattern that reached the wrong partner would still sum to nearly the same number, so the inputs are chosen
for the order of the additions to show in the last bits, and all 64 lanes of both forms must equal the butterfly emulated in numpy bit for bit.
The integer forms (sum and inclusive scan) are exact in any order and are held to numpy's sums."""
import ctypes as C

import numpy as np
import pytest
import torch

NWAVES = 6


def _doubles():
    """NWAVES x 64 doubles, exponents over ~40 binades, mixed signs"""
    g = np.random.default_rng(20291)  # (the first seed from 20250 on at which every wave tells the trees apart: test_the_inputs_tell_trees_apart)
    return (g.choice([-1.0, 1.0], (NWAVES, 64)) * (1.0 + g.random((NWAVES, 64))) * 2.0 ** g.integers(-20, 21, (NWAVES, 64))).astype(np.float64)


def _butterfly(v):
    v = v.copy()
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ d]
    return v


def _run(what, a):
    from pynqs_amd import _native as N

    x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = torch.empty_like(x)
    N.check(N.lib().pynqs_debug_wave_sum(x.data_ptr(), out.data_ptr(), a.shape[0], what, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "pynqs_debug_wave_sum")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_the_inputs_tell_trees_apart():
    """host only: on every wave the butterfly differs from a left-to-right sum and from a butterfly with another partner order"""
    a = _doubles()
    want = _butterfly(a)
    ltr = np.zeros(NWAVES)
    for i in range(64):
        ltr = ltr + a[:, i]
    assert bool((want[:, 0] != ltr).all())
    other = a.copy()
    lane = np.arange(64)
    for d in (1, 2, 4, 8, 16, 32):
        other = other + other[:, lane ^ d]
    assert bool((want[:, 0] != other[:, 0]).all())
    assert bool((want == want[:, :1]).all())  # every lane ends with the same bits


@pytest.mark.gpu
@pytest.mark.parametrize("what", [0, 1], ids=["fixed_pattern", "shfl_xor"])
def test_double_sum_is_the_butterfly_bit_for_bit(what):
    a = _doubles()
    got = _run(what, a)
    want = _butterfly(a)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"lanes differ: {np.argwhere(got != want)[:8].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("what", [2, 3], ids=["fixed_pattern", "shfl_xor"])
def test_uint32_sum(what):
    g = np.random.default_rng(7)
    a = g.integers(0, 2**32, (NWAVES, 64), dtype=np.uint64).astype(np.uint32)
    a[0] = np.arange(64, dtype=np.uint32) ** 2  # (small, all different: a lane counted twice or not at all shows)
    got = _run(what, a)
    want = (a.astype(np.uint64).sum(1) & 0xFFFFFFFF).astype(np.uint32)
    assert np.array_equal(got, np.repeat(want[:, None], 64, 1))


@pytest.mark.gpu
def test_uint32_scan():
    g = np.random.default_rng(8)
    a = g.integers(0, 2**32, (NWAVES, 64), dtype=np.uint64).astype(np.uint32)
    a[0] = 1
    a[1] = np.arange(64, dtype=np.uint32) ** 2
    got = _run(4, a)
    want = (np.cumsum(a.astype(np.uint64), axis=1) & 0xFFFFFFFF).astype(np.uint32)
    assert np.array_equal(got, want)
