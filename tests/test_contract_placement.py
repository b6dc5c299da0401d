"""pynqs_reduce_contract_group (include/pynqs_amd.h: the walker group workgroup b of B serves under PYNQS_CONTRACT_BY_XCD), on the host:
a permutation of 0 .. B-1 for every B, each class b % 8 on one contiguous range of groups, the classes' ranges in order."""
import pytest

SIZES = list(range(1, 71)) + [2047, 2048, 2049]


def _groups(B):
    from pynqs_amd import _native as N

    f = N.lib().pynqs_reduce_contract_group
    return [int(f(b, B)) for b in range(B)]


@pytest.mark.parametrize("B", SIZES)
def test_placement_is_a_permutation(B):
    assert sorted(_groups(B)) == list(range(B))


@pytest.mark.parametrize("B", SIZES)
def test_each_class_gets_a_contiguous_range(B):
    g = _groups(B)
    start = 0
    for j in range(8):
        mine = g[j::8]  # workgroups j, j + 8, ...: in this order
        assert len(mine) == B // 8 + (1 if j < B % 8 else 0)
        assert mine == list(range(start, start + len(mine))), f"B={B} class {j}"
        start += len(mine)
    assert start == B


@pytest.mark.parametrize("B", SIZES)
def test_placement_is_the_documented_formula(B):
    g = _groups(B)
    for b in range(B):
        j = b & 7
        assert g[b] == j * (B >> 3) + min(j, B & 7) + (b >> 3)


def test_outside_the_grid():
    from pynqs_amd import _native as N

    f = N.lib().pynqs_reduce_contract_group
    assert f(-1, 8) == -1 and f(8, 8) == -1 and f(0, 0) == -1 and f(0, 1 << 33) == -1
