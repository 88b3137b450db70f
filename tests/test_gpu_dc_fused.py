"""Divide and conquer with the column-mapped merge product (default) against LAPACK and against the level-by-level path it
replaced (HELFEM_DC=levels), on tridiagonal matrices that stress what changed: the order of the roots taken before the
product, the two eigenvector buffers alternating by tree depth (trees whose leaves lie at different depths: orders that
are no power of two times the leaf size), the zero blocks written by the children instead of a cleared buffer, edge
tiles of the mapped product, heavy deflation and many rotations.

Bounds: the single matrices hold the bounds of test_gpu_parity.py::test_eig_sym_hard_spectra, the batch of the
benchmark's block orders (1380 / 1470 / 1380, through eig_gsym_sub with X = 1) those of test_eig_sym_vs_lapack with n
the largest block.  Both paths must meet them; their mutual difference is printed.  Two runs of the default path must
agree bitwise.  The switch is read once per process, so every run is a process of its own (tests/dc_fused_worker.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dc_fused_worker as wk  # noqa: E402

CASES = dict(wk.cases())


def _run(path, env):
    e = dict(os.environ)
    e.pop("HELFEM_DC", None)
    e.update(env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dc_fused_worker.py"), path], env=e, cwd=ROOT,
                         timeout=900, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0 and b"ok" in out.stdout, out.stdout.decode()[-2000:]
    return np.load(path)


@pytest.fixture(scope="module")
def runs(native_libs, tmp_path_factory):
    d = tmp_path_factory.mktemp("dc_fused")
    return dict(default=_run(str(d / "a.npz"), {}), again=_run(str(d / "b.npz"), {}),
                levels=_run(str(d / "c.npz"), dict(HELFEM_DC="levels")))


def _figures(A, E, C, Eref):
    n = A.shape[0]
    return (np.max(np.abs(E - Eref)), np.max(np.abs(C.T @ C - np.eye(n))), np.max(np.abs(A @ C - C * E)))


@pytest.mark.parametrize("name", list(CASES))
def test_dc_single_matrices(runs, name):
    A = CASES[name]
    n = A.shape[0]
    Eref = np.linalg.eigh(A)[0]
    scale = max(np.max(np.abs(Eref)), 1e-300)
    for path in ("default", "levels"):
        E, C = runs[path]["E_" + name], runs[path]["C_" + name]
        dE, orth, res = _figures(A, E, C, Eref)
        print("%s %s: |E - Eref| / scale %.3e, |C^T C - 1| %.3e, |A C - C E| / scale %.3e" % (name, path, dE / scale, orth, res / scale))
        assert dE < 5e-14 * scale * max(np.sqrt(n), 10), (name, path)
        assert orth < 1e-12, (name, path)
        assert res < 1e-12 * scale * max(np.sqrt(n), 10), (name, path)
    print("%s default - levels: max |dE| %.3e" % (name, np.max(np.abs(runs["default"]["E_" + name] - runs["levels"]["E_" + name]))))


def test_dc_batch_of_the_benchmark_orders(runs):
    F, blocks = wk.batch_problem()
    n = max(wk.BATCH)
    Eref = np.sort(np.concatenate([np.linalg.eigh(F[np.ix_(b, b)])[0] for b in blocks]))
    scale = max(1.0, np.max(np.abs(Eref)))
    for path in ("default", "levels"):
        E, C = runs[path]["E_batch"], runs[path]["C_batch"]
        dE, orth, res = _figures(F, E, C, Eref)
        print("batch %s: |E - Eref| %.3e, |C^T C - 1| %.3e, |F C - C E| %.3e" % (path, dE, orth, res))
        assert dE < 1e-12 * scale * max(n, 10), path
        assert orth < 1e-12 * max(n, 10), path
        assert res < 1e-11 * scale * max(n, 10), path
        # no eigenvector leaves its symmetry block
        for b in blocks:
            cols = np.nonzero(np.any(C[b, :] != 0.0, axis=0))[0]
            assert len(cols) == len(b), path
    print("batch default - levels: max |dE| %.3e" % np.max(np.abs(runs["default"]["E_batch"] - runs["levels"]["E_batch"])))


def test_dc_default_path_repeats_bitwise(runs):
    a, b = runs["default"], runs["again"]
    for key in a.files:
        assert np.array_equal(a[key], b[key]), key


def test_dc_many_rotations_case_rotates(native_libs):
    """The many_rotations matrix must reach the rotation branch of the deflation, or it adds nothing over the random cases.
    Its top merge joins two mirror-image halves of order 128: 128 pairs of equal poles.  At least a quarter of them (32)
    must be removed by rotations; the count is the one HELFEM_DC_DBG prints for the top merge (order 256)."""
    import re
    e = dict(os.environ)
    e.pop("HELFEM_DC", None)
    e["HELFEM_DC_DBG"] = "1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dc_fused_worker.py"), "-", "many_rotations"], env=e,
                         cwd=ROOT, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = out.stdout.decode()
    assert out.returncode == 0 and "ok" in text, text[-2000:]
    stats = [tuple(map(int, m)) for m in re.findall(r"dc level \d+ node \d+: n (\d+), roots (\d+), rotations (\d+)", text)]
    print("many_rotations (n, roots, rotations):", stats)
    top = [st for st in stats if st[0] == 256]
    assert top and top[0][2] >= 32, stats
