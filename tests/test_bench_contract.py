"""The driver's bench.py contract: one JSON line with the agreed keys (run on a small configuration)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_bench_json_line():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C2", "--steps", "3", "--warmup", "1",
                          "--cpu-stride", "16"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "spectral-points/s" and d["dtype"] == "f64" and d["vs_baseline"] is None and "workload" in d["config"]
    assert d["value"] == pytest.approx(10_000 * 40 / (d["ms_per_step"] * 1e-3), rel=1e-9)
    r = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r, key
    assert r["bound"] in ("hbm", "mfma", "valu_issue") and r["frac"] == pytest.approx(r["achieved"] / r["peak"])
    c = d["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in c, key
    assert c["kind"] in ("port", "reference") and c["value"] > 0
    assert abs(d["olr_wm2"] - c["olr_sample"]) < 5.0          # the CPU leg ran a 1/16 sample of the same column


def _bench_dump(tmp_path, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C2", "--steps", "2", "--warmup", "1", "--no-cpu",
                          "--dump-outputs", str(tmp_path)] + list(extra), env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    arrays = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert set(arrays) == {"Fup", "Fdn", "tau", "Mup", "Mdn", "nu"} and sorted(d["dumped_outputs"]["files"]) == sorted(f + ".npy" for f in arrays)
    assert all(a.dtype == np.float64 and np.all(np.isfinite(a)) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64e6
    return d, arrays


@pytest.mark.gpu
def test_bench_dump_outputs_whole_grid(tmp_path):
    """--dump-outputs on a grid small enough to be written whole: the arrays are the timed step's -- the band fluxes are the
    trapezoid integrals of the dumped M+ / M- and OLR is the one of the result line."""
    import clearsky_jl_amd as cs
    d, a = _bench_dump(tmp_path)
    nl, nnu = 40, 10_000
    assert a["tau"].shape == (nl, nnu) and a["Mup"].shape == a["Mdn"].shape == (nl + 1, nnu) and a["Fup"].shape == a["Fdn"].shape == (nl + 1,)
    assert np.array_equal(a["nu"], np.linspace(1.0, 2500.0, nnu)) and d["dumped_outputs"]["wavenumbers"] == nnu
    assert a["Fup"][0] == d["olr_wm2"] and np.all(a["tau"] > 0)
    w = cs.trapz_weights(a["nu"])
    scale = np.max(a["Fup"])
    assert np.max(np.abs(a["Mup"] @ w - a["Fup"])) < 1e-10 * scale and np.max(np.abs(a["Mdn"] @ w - a["Fdn"])) < 1e-10 * scale


@pytest.mark.gpu
def test_bench_dump_outputs_sampled(tmp_path):
    """--dump-outputs on a grid larger than the budget: a fixed seeded sample of wavenumbers, the same one from run to run."""
    nnu = 100_000
    d, a = _bench_dump(tmp_path, "--nnu", str(nnu))
    m = d["dumped_outputs"]["wavenumbers"]
    assert 1000 < m < nnu and d["dumped_outputs"]["of"] == nnu
    assert a["tau"].shape == (40, m) and a["Mup"].shape == a["Mdn"].shape == (41, m) and a["nu"].shape == (m,)
    grid = np.linspace(1.0, 2500.0, nnu)
    assert np.all(np.diff(a["nu"]) > 0) and np.all(np.isin(a["nu"], grid)) and np.all(a["tau"] > 0)
    import bench
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(nnu, m, replace=False))
    assert np.array_equal(a["nu"], grid[idx])


@pytest.mark.gpu
def test_bench_dump_outputs_across_ranks(tmp_path):
    """Two ranks (gloo, on this box's card) dump the whole grid too: every wavenumber filled by the rank whose shard holds it, the band
    fluxes all-reduced -- the same arrays as one rank's, whatever partition the calibration chose."""
    _, one = _bench_dump(tmp_path / "one")
    d, two = _bench_dump(tmp_path / "two", "--gpus", "2", "--dist-backend", "gloo")
    assert d["n_gpus"] == 2 and d["dumped_outputs"]["wavenumbers"] == 10_000
    assert np.array_equal(one["nu"], two["nu"]) and all(one[k].shape == two[k].shape for k in one)
    assert np.max(np.abs(two["tau"] - one["tau"]) / one["tau"]) < 1e-12
    for k, scale in (("Mup", one["Mup"].max()), ("Mdn", one["Mup"].max()), ("Fup", one["Fup"].max()), ("Fdn", one["Fup"].max())):
        assert np.max(np.abs(two[k] - one[k])) < 1e-12 * scale, k
