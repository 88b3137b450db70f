"""bench.py prints ONE JSON line with the fields the driver reads (run on the small workload so that it takes seconds):
the headline alone by default, the measurements beyond it with --full."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_line_contract(native_libs):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "n2_pbe_small", "--steps", "2", "--warmup", "1",
                        "--full"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is False and d["vs_baseline"] is None
    assert d["unit"] == "ms" and d["dtype"] == "f64" and d["value"] == d["ms_per_step"] > 0.0
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] == "port+lapack" and c["cores"] >= 1 and c["value"] > 0.0


def _bench_dump(tmp_path, name, *args):
    """bench.py on the small workload with --dump-outputs: (the result line, {name: array})"""
    out = tmp_path / name
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "n2_pbe_small"] + list(args) +
                       ["--dump-outputs", str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), {f[:-4]: np.load(str(out / f)) for f in os.listdir(str(out))}


def test_bench_plain_line_and_dump_outputs(native_libs, tmp_path):
    d, got = _bench_dump(tmp_path, "outputs", "--steps", "3", "--warmup", "1")
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "ms" and d["dtype"] == "f64" and d["higher_is_better"] is False
    assert d["value"] == d["ms_per_step"] > 0.0 and d["metric"] == "scf_iteration_wall_time_n2_pbe_small"
    for k in ("roofline", "stages_ms", "check", "cpu_baseline"):  # --full only
        assert k not in d, k
    assert sorted(got) == ["density_sample", "eigenvalues", "fock_sample", "xc_scalars"]
    assert all(a.dtype == np.float64 and np.all(np.isfinite(a)) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    N = int(re.search(r"Nbf=(\d+)", d["config"]["workload"]).group(1))
    assert got["eigenvalues"].shape == (N,) and got["eigenvalues"].min() < 0.0 and got["xc_scalars"].shape == (3,)
    assert got["fock_sample"].shape == got["density_sample"].shape and got["fock_sample"].size > 0
    assert abs(got["xc_scalars"][1] - 14.0) < 1e-3  # Nel of the XC quadrature: N2 has 14 electrons


def test_bench_dump_is_the_last_timed_step(native_libs, tmp_path):
    """the timed steps start from the guess density whatever the warm-up did, so with one timed step the dump is the
    step --full's `check` repeats; with two it is the second, the same for any warm-up and not the first"""
    nocc = 7  # bench.WORKLOADS["n2_pbe_small"]
    one, d1 = _bench_dump(tmp_path, "one", "--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline")
    c = one["check"]
    assert abs(d1["eigenvalues"][:nocc].sum() - c["sum_lowest_eigenvalues_after_one_step"]) <= 1e-10 * abs(c["sum_lowest_eigenvalues_after_one_step"])
    assert abs(d1["eigenvalues"].sum() - c["sum_all_eigenvalues_after_one_step"]) <= 1e-10 * abs(c["sum_all_eigenvalues_after_one_step"])
    assert abs(d1["xc_scalars"][0] - c["xc_energy_after_one_step"]) <= 1e-10 * abs(c["xc_energy_after_one_step"])
    _, d2 = _bench_dump(tmp_path, "two", "--steps", "2", "--warmup", "0")
    _, d2w = _bench_dump(tmp_path, "two_w", "--steps", "2", "--warmup", "2")
    for k in d2:
        scale = np.max(np.abs(d2[k]))
        assert np.max(np.abs(d2[k] - d2w[k])) <= 1e-10 * scale, k
    assert np.max(np.abs(d2["density_sample"] - d1["density_sample"])) > 1e-6 * np.max(np.abs(d1["density_sample"]))
    assert abs(d2["xc_scalars"][0] - d1["xc_scalars"][0]) > 1e-8 * abs(d1["xc_scalars"][0])
