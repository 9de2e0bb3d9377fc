"""bench.py --dump-outputs: what the timed path computed goes to DIR/<name>.npy within a 64 MiB budget, the same bytes for
the same arrays; the command line refuses what it cannot honour.  CPU only: dump_outputs() is fed arrays directly."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _total(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_headline_outputs_fit_in_full_precision_or_float32(tmp_path):
    rng = np.random.default_rng(1)
    h, w = 1080, 1920
    arrays = {"vx": rng.random((h, w)), "vy": rng.random((h, w)), "warpI2": rng.random((h, w, 3))}
    how = bench.dump_outputs(str(tmp_path), arrays)
    assert how == {"vx": "float64", "vy": "float64", "warpI2": "float32"}
    assert _total(tmp_path) <= bench.DUMP_BUDGET_BYTES
    for name in ("vx", "vy"):
        assert np.array_equal(np.load(tmp_path / (name + ".npy")), arrays[name])
    wi = np.load(tmp_path / "warpI2.npy")
    assert wi.dtype == np.float32 and np.array_equal(wi, arrays["warpI2"].astype(np.float32))


def test_larger_outputs_are_sampled_within_the_budget_and_the_same_every_time(tmp_path):
    rng = np.random.default_rng(2)
    arrays = {k: rng.random((3000, 3000)) for k in ("a", "b", "c")}
    d1, d2 = tmp_path / "1", tmp_path / "2"
    how = bench.dump_outputs(str(d1), arrays)
    assert bench.dump_outputs(str(d2), arrays) == how
    assert how["a"] == "float32" and how["b"].startswith("float64 sample of ") and how["c"] == "not written (budget spent)"
    assert _total(d1) <= bench.DUMP_BUDGET_BYTES
    assert sorted(os.listdir(d1)) == sorted(os.listdir(d2)) == ["a.npy", "b.npy", "b_sample_index.npy"]
    for f in os.listdir(d1):
        assert (d1 / f).read_bytes() == (d2 / f).read_bytes(), f
    idx, b = np.load(d1 / "b_sample_index.npy"), np.load(d1 / "b.npy")
    assert len(idx) == len(b) > 0 and np.all(np.diff(idx) > 0)
    assert np.array_equal(b, arrays["b"].ravel()[idx])


def test_a_small_budget_writes_what_fits_and_nothing_more(tmp_path):
    arrays = {"x": np.arange(10.0), "y": np.arange(1000.0)}
    how = bench.dump_outputs(str(tmp_path), arrays, budget=400)
    assert how["x"] == "float64" and how["y"] == "not written (budget spent)"
    assert _total(tmp_path) <= 400


@pytest.mark.parametrize("extra", [["--steps", "0"], ["--simulate-step-ms", "1", "--dump-outputs", "out"]])
def test_the_command_line_refuses_what_it_cannot_honour(tmp_path, extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, cwd=str(tmp_path), capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 2 and "error:" in out.stderr, out.stderr[-2000:]
    assert not os.listdir(tmp_path)
