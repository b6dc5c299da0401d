"""Keys of the host-side caches in front of the kernels, checked without a GPU.

* The content key of the integral plan cache (C_extension._fingerprint) must change with any change of the integrals, element order
  included (a relabelling of the orbitals permutes the same values), and must stay the same for the same values in another tensor object.
* total_energy's call token (what local_energy's per-parameter-state caches are valid for) is per thread and is restored when the call
  raises.
* The keys index of a sample-space table is rebuilt when the keys tensor is rewritten in place or replaced."""
import threading
import types

import numpy as np
import pytest
import torch

from conftest import synth_integrals


def _fp(h1, h2):
    from pynqs_amd import C_extension as cx

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a  # noqa: E731
    return cx._fingerprint(T(h1), T(h2))


def _reversed(h1, h2, sorb):
    """The integrals with the spin-orbital order reversed (new orbital i = old orbital sorb - 1 - i; for even sorb alpha and beta swap)."""
    from oracle import oracle as O

    a, b = O.decompress_h1e_h2e(h1, h2, sorb)
    p = np.arange(sorb)[::-1]
    return O.compress_h1e_h2e(a[np.ix_(p, p)], b[np.ix_(p, p, p, p)], sorb)


def test_fingerprint_sees_element_order():
    sorb = 12
    h1, h2 = (torch.from_numpy(a) for a in synth_integrals(sorb))
    base = _fp(h1, h2)
    h1n = h1.view(sorb, sorb) + torch.triu(torch.full((sorb, sorb), 0.125, dtype=torch.float64), 1)   # not symmetric
    assert _fp(h1n.t(), h2) != _fp(h1n, h2)
    assert _fp(h1, h2.flip(0)) != base
    g = np.random.default_rng(0)
    for t, which in ((h2, 1), (h1, 0)):
        for _ in range(50):
            i, j = (int(v) for v in g.choice(t.numel(), 2, replace=False))
            if t[i] == t[j]:
                continue
            s = t.clone()
            s[[i, j]] = s[[j, i]]
            assert (_fp(h1, s) if which else _fp(s, h2)) != base, (which, i, j)


@pytest.mark.parametrize("sorb", [12, 40])
def test_fingerprint_of_the_orbital_reversal(sorb):
    """Reversing the spin orbitals is the same physics with other labels: the packed h2e holds the same values in another order (so two
    order-blind sums cannot tell the systems apart), and the plan of one must not serve the other."""
    h1, h2 = synth_integrals(sorb)
    r1, r2 = _reversed(h1, h2, sorb)
    assert not np.array_equal(r2, h2) and np.array_equal(np.sort(r2), np.sort(h2))
    assert np.array_equal(np.sort(r1), np.sort(h1))
    assert _fp(r1, r2) != _fp(h1, h2)
    assert _fp(h1, r2) != _fp(h1, h2) and _fp(r1, h2) != _fp(h1, h2)


def test_fingerprint_of_integrals_exchanged_between_systems():
    (a1, a2), (b1, b2) = synth_integrals(12, 1), synth_integrals(12, 2)
    assert len({_fp(a1, a2), _fp(b1, b2), _fp(a1, b2), _fp(b1, a2)}) == 4


def test_fingerprint_is_equal_for_equal_content():
    sorb = 12
    h1, h2 = (torch.from_numpy(a) for a in synth_integrals(sorb))
    base = _fp(h1, h2)
    assert _fp(h1.clone(), h2.clone()) == base
    # non-contiguous tensors holding the same values in the same logical order
    h1s = h1.view(sorb, sorb).t().contiguous().t()
    assert not h1s.is_contiguous() and _fp(h1s, h2) == _fp(h1.view(sorb, sorb), h2)
    h2s = torch.stack([h2, torch.zeros_like(h2)], 1)[:, 0]
    assert not h2s.is_contiguous() and _fp(h1, h2s) == base
    f1, f2 = h1.float(), h2.float()
    assert _fp(f1, f2) == _fp(f1.clone(), f2.clone()) and _fp(f1, f2) != base


def test_fingerprint_does_not_depend_on_the_chunk_size(monkeypatch):
    from pynqs_amd import C_extension as cx

    h1, h2 = (torch.from_numpy(a) for a in synth_integrals(12))
    f1, f2 = h1.float(), h2.float()
    want = _fp(h1, h2), _fp(f1, f2)
    for chunk in (1, 7, 64, 2211):
        monkeypatch.setattr(cx, "_FINGERPRINT_CHUNK", chunk)
        assert (_fp(h1, h2), _fp(f1, f2)) == want, chunk


def test_fingerprint_has_no_collision_over_random_permutations():
    """200 seeded permutations of the 2211-element h2e of sorb 12 (and of h1e with it): 201 different keys."""
    h1, h2 = (torch.from_numpy(a) for a in synth_integrals(12, 5))
    g = torch.Generator().manual_seed(11)
    keys = {_fp(h1, h2)}
    for _ in range(200):
        keys.add(_fp(h1[torch.randperm(h1.numel(), generator=g)], h2[torch.randperm(h2.numel(), generator=g)]))
    assert len(keys) == 201


def _fake_total_energy_run(monkeypatch, raise_on=None, hold=None):
    """total_energy on host tensors (two chunks) with local_energy replaced: records the call token every chunk sees."""
    from pynqs_amd import energy as E

    seen = []

    def fake(x, *a, **k):
        seen.append(E._call_token())
        if hold is not None:
            hold()
        if raise_on is not None and len(seen) == raise_on:
            raise RuntimeError("ansatz failed")
        n = x.size(0)
        return torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.ones(n, dtype=torch.float64), (0, 0, 0)

    monkeypatch.setattr(E, "local_energy", fake)
    x = torch.zeros((4, 8), dtype=torch.uint8)
    return seen, lambda: E.total_energy(x, 2, -1, torch.zeros(64, dtype=torch.float64), torch.zeros(1, dtype=torch.float64), None, 8, 4, 2, 2)


def test_call_token_is_restored_when_total_energy_raises(monkeypatch):
    from pynqs_amd import energy as E

    assert E._call_token() is None
    seen, run = _fake_total_energy_run(monkeypatch, raise_on=2)
    with pytest.raises(RuntimeError, match="ansatz failed"):
        run()
    assert len(seen) == 2 and seen[0] is not None and seen[0] is seen[1]
    assert E._call_token() is None
    seen2, run2 = _fake_total_energy_run(monkeypatch)
    run2()
    assert len(seen2) == 2 and seen2[0] is not None and seen2[0] is not seen[0] and E._call_token() is None


def test_call_token_is_per_thread(monkeypatch):
    """Two threads inside total_energy at once: each chunk sees its own call's token, and neither clears the other's."""
    from pynqs_amd import energy as E

    barrier = threading.Barrier(2, timeout=30)
    seen, run = _fake_total_energy_run(monkeypatch, hold=barrier.wait)
    errors = []

    def worker():
        try:
            run()
        except Exception as e:  # (reported below)
            errors.append(e)

    threads = [threading.Thread(target=worker) for _ in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not errors and len(seen) == 4
    assert len({id(s) for s in seen}) == 2 and all(s is not None for s in seen)
    assert E._call_token() is None


def test_keys_index_is_rebuilt_when_the_keys_change(monkeypatch):
    """_keys_index_for keys the index on the keys tensor object and its version counter: an in-place rewrite of the keys (same object,
    same address) or another keys tensor is a new index; an unchanged table keeps its index."""
    from pynqs_amd import C_extension as cx, energy as E

    built = []

    def fake_build(keys, sorb):
        built.append(keys.clone())
        return types.SimpleNamespace(nkeys=keys.size(0), index=torch.zeros(1, device=keys.device), per_walker=1.0)

    monkeypatch.setattr(cx, "keys_index_build", fake_build)
    monkeypatch.setattr(E, "SS_INDEX", True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    keys = torch.arange(64, dtype=torch.uint8).reshape(8, 8)
    lut = types.SimpleNamespace(bra_key=keys)
    ki = E._keys_index_for(lut, 4, 40)
    assert len(built) == 1 and E._keys_index_for(lut, 4, 40) is ki and len(built) == 1
    keys.copy_(keys.flip(0))
    k2 = E._keys_index_for(lut, 4, 40)
    assert len(built) == 2 and k2 is not ki and torch.equal(built[-1], keys)
    assert E._keys_index_for(lut, 4, 40) is k2 and len(built) == 2
    lut.bra_key = keys.clone()
    assert E._keys_index_for(lut, 4, 40) is not k2 and len(built) == 3
