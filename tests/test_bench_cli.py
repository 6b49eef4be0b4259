"""bench.py's command line and output writer, without a GPU: the options a plain and a --full run rest on, and the
files --dump-outputs writes (float32, less than 64 MB in all, a fixed sample of larger outputs)."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("hsflow_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in r.stdout, opt


def test_dump_outputs_small_arrays_as_they_are(tmp_path):
    b = _bench()
    u = np.arange(12, dtype=np.float64).reshape(3, 4) / 7
    v = -np.arange(12, dtype=np.float32).reshape(3, 4)
    b.dump_outputs(str(tmp_path / "out"), {"u": u, "v": v})
    assert sorted(os.listdir(tmp_path / "out")) == ["u.npy", "v.npy"]
    gu, gv = np.load(tmp_path / "out" / "u.npy"), np.load(tmp_path / "out" / "v.npy")
    assert gu.dtype == np.float32 and gv.dtype == np.float32
    assert np.array_equal(gu, u.astype(np.float32)) and np.array_equal(gv, v)


def test_dump_outputs_samples_large_arrays_the_same_way_every_time(tmp_path):
    b = _bench()
    big = np.random.default_rng(5).standard_normal((9, 1080, 1920), dtype=np.float32)  # 75 MB: past the budget alone
    outs = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        b.dump_outputs(str(d), {"u": big, "v": big[::-1]})
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) < 64 * 10 ** 6
        outs.append((np.load(d / "u.npy"), np.load(d / "v.npy")))
    assert outs[0][0].size == b.DUMP_BYTES // 2 // 4
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    # the sample: the elements at fixed flat indices (seed 0, sorted), whatever the data
    idx = np.sort(np.random.default_rng(0).integers(0, big.size, b.DUMP_BYTES // 2 // 4))
    assert np.array_equal(outs[0][0], big.reshape(-1)[idx]) and np.array_equal(outs[0][1], big[::-1].reshape(-1)[idx])
