"""bench.py's plain run and --dump-outputs: the timed path's last step written as float32 / float64 .npy files, the same from run to run
(the semi-stochastic draws are re-seeded after the clock-dependent pre-heat), at most 64 MB in all (a seeded sample of the walkers beyond)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(args):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, f"exactly one JSON line expected on stdout, got {len(lines)}"
    return json.loads(lines[0])


def _arrays(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_default_step_dumps_the_same_outputs_twice(tmp_path):
    runs = []
    for tag in ("a", "b"):
        out = _bench(["--steps", "3", "--warmup", "2", "--walkers", "1024", "--dump-outputs", str(tmp_path / tag)])
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["unit"] == "local energies/s" and out["dtype"] == "f64"
        assert not {"parity", "cpu_baseline", "extra"} & set(out), "a plain run measures only its headline figure"
        runs.append(_arrays(tmp_path / tag))
    a, b = runs
    assert set(a) == set(b) and {"eloc", "psi_x", "stats", "loss"} <= set(a) and any(k.startswith("grad_") for k in a)
    assert a["eloc"].shape == (1024, 2) and "sample_walkers" not in a
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and a[k].shape == b[k].shape, k
        assert np.isfinite(a[k]).all(), k
        np.testing.assert_allclose(a[k], b[k], rtol=1e-10, atol=1e-12 * max(1.0, float(np.abs(b[k]).max())), err_msg=k)


def test_large_outputs_are_sampled_below_64_mb(tmp_path):
    # the drop-in call on 8192 walkers returns 0.5 GB of Hmat and comb: a seeded sample of the walkers, the same rows of both
    out = _bench(["--workload", "fe2s2_dropin", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    a = _arrays(tmp_path)
    assert set(a) == {"hmat", "comb", "sample_walkers"}
    assert sum(os.path.getsize(tmp_path / f"{k}.npy") for k in a) <= 64 * 1000 * 1000
    idx = a["sample_walkers"].astype(np.int64)
    assert len(idx) > 100 and np.all(np.diff(idx) > 0) and idx[-1] < 8192
    assert a["hmat"].shape == (len(idx), out["config"]["ncomb"]) and a["comb"].shape == (len(idx), out["config"]["ncomb"], 8)
    assert a["comb"].dtype == np.float32 and a["hmat"].dtype == np.float64
    # column 0 of a row of comb is the sampled walker itself
    ci = np.load(os.path.join(ROOT, "tests", "golden", "fe2s2_inputs.npz"))["ci_space"]
    np.testing.assert_array_equal(a["comb"][:, 0, :], ci[idx % ci.shape[0]].astype(np.float32))
