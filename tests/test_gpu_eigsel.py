"""Selected eigenpairs (hfg_eig_sym_sel, hfg_eig_gsym_sub_sel): the lowest nev pairs per block, through both paths of the
tridiagonal stage -- multisection and inverse iteration (HELFEM_EIGSEL=stein), the full divide and conquer followed by
taking the lowest columns (HELFEM_EIGSEL=dc) -- and with the switch unset (the crossover chooses).  The switch is read once
per process, so every path is a process of its own (tests/eigsel_worker.py); every test checks all three.

Size switches the selected path introduces, each with the order or count just below and just above it:
  - the crossover: measured at 0 (every fraction goes to dc when the switch is unset), so it has no two sides; its first
    value, 1/8 of the columns, keeps its cases (n, nev) = (64, 8) and (64, 9);
  - four eigenvalues per workgroup of the multisection kernel: nev = 4 and 5 at n = 130;
  - rows staged in LDS up to n = 3072, global memory beyond (both kernels): n = 3072 and 3073, tridiagonal input, nev = 4;
  - the inverse-iteration kernel asks for more than 64 KB of LDS from n = 1599: n = 1598 and 1599, tridiagonal input.
The bounds are those of test_gpu_parity.py (test_eig_sym_vs_lapack, test_eig_sym_hard_spectra, test_eig_gsym_sub_parity);
LAPACK's dstebz + dstein stay below 0.05 of the hard-spectra bounds on every case used here."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eigsel_worker as wk  # noqa: E402

PATHS = ("stein", "dc", "unset")


def _run(path, env):
    e = dict(os.environ)
    e.pop("HELFEM_EIGSEL", None)
    e.update(env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "eigsel_worker.py"), path], env=e, cwd=ROOT, timeout=900,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0 and b"ok" in out.stdout, out.stdout.decode()[-3000:]
    return np.load(path)


@pytest.fixture(scope="module")
def runs(native_libs, tmp_path_factory):
    d = tmp_path_factory.mktemp("eigsel")
    return dict(stein=_run(str(d / "s.npz"), dict(HELFEM_EIGSEL="stein")), dc=_run(str(d / "d.npz"), dict(HELFEM_EIGSEL="dc")),
                unset=_run(str(d / "u.npz"), {}))


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    if helfem_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the hot path has no CPU fallback")
    return helfem_amd


_EREF = {}


def _eref(key, make):
    if key not in _EREF:
        _EREF[key] = make()
    return _EREF[key]


def _figures(A, E, C, Eref):
    nev = len(E)
    return (np.max(np.abs(E - Eref[:nev])), np.max(np.abs(C.T @ C - np.eye(nev))), np.max(np.abs(A @ C - C * E)))


@pytest.mark.parametrize("name,n,nev,kind", list(wk.dense_cases()), ids=[c[0] for c in wk.dense_cases()])
def test_dense_against_lapack(runs, name, n, nev, kind):
    if kind == "dense":
        A = wk.dense_matrix(n)
        Eref = _eref(("dense", n), lambda: np.linalg.eigvalsh(A))
    else:
        from scipy.linalg import eigvalsh_tridiagonal
        d, e = wk.big_tridiag(n)
        A = wk.tridiag(d, e)
        Eref = _eref(("tridiag", n), lambda: eigvalsh_tridiagonal(d, e))
    scale = max(1.0, np.max(np.abs(Eref)))
    for path in PATHS:
        E, C = runs[path]["E_" + name], runs[path]["C_" + name]
        assert E.shape == (nev,) and C.shape == (n, nev), path
        dE, orth, res = _figures(A, E, C, Eref)
        print("%s %s: |E - Eref| %.3e, |C^T C - 1| %.3e, |A C - C E| %.3e" % (name, path, dE, orth, res))
        assert dE < 1e-12 * scale * max(n, 10), path
        assert orth < 1e-12 * max(n, 10), path
        assert res < 1e-11 * scale * max(n, 10), path


@pytest.mark.parametrize("name,A,nev", list(wk.hard_cases()), ids=[c[0] for c in wk.hard_cases()])
def test_hard_spectra(runs, name, A, nev):
    n = A.shape[0]
    Eref = _eref(("hard", name.rsplit("_", 1)[0]), lambda: np.linalg.eigvalsh(A))
    scale = max(np.max(np.abs(Eref)), 1e-300)
    for path in PATHS:
        E, C = runs[path]["E_" + name], runs[path]["C_" + name]
        assert E.shape == (nev,) and C.shape == (n, nev), path
        dE, orth, res = _figures(A, E, C, Eref)
        print("%s %s: |E - Eref| / scale %.3e, |C^T C - 1| %.3e, |A C - C E| / scale %.3e" % (name, path, dE / scale, orth, res / scale))
        assert dE < 5e-14 * scale * max(np.sqrt(n), 10), path
        assert orth < 1e-12, path
        assert res < 1e-12 * scale * max(np.sqrt(n), 10), path


@pytest.mark.parametrize("name,A,nev", list(wk.aufbau_cases()), ids=[c[0] for c in wk.aufbau_cases()])
def test_first_pairs_are_the_lowest_of_the_full_spectrum(runs, name, A, nev):
    """the gap above level nev is more than 1e-6 scale (aufbau_nev chooses nev so), so the span of the first nev
    eigenvectors is well defined and the two solvers must agree on it"""
    n = A.shape[0]
    for path in PATHS:
        r = runs[path]
        E, C, Ef, Cf = r["E_" + name], r["C_" + name], r["Efull_" + name], r["Cfull_" + name]
        scale = max(np.max(np.abs(Ef)), 1e-300)
        gap = Ef[nev] - Ef[nev - 1]
        print("%s %s: nev %d, gap above it %.3e scale" % (name, path, nev, gap / scale))
        assert gap > 1e-6 * scale
        assert np.max(np.abs(E - Ef[:nev])) < 5e-14 * scale * max(np.sqrt(n), 10), path
        assert np.max(np.abs(Cf[:, :nev] @ Cf[:, :nev].T - C @ C.T)) < 1e-10, path


@pytest.mark.parametrize("name,pname,nev", list(wk.gen_cases()), ids=[c[0] for c in wk.gen_cases()])
def test_generalized_blocked(runs, name, pname, nev):
    from scipy.linalg import eigh
    F, S, blocks = wk.gen_problem(pname)
    N = F.shape[0]
    per = [eigh(F[np.ix_(b, b)], S[np.ix_(b, b)], eigvals_only=True) for b in blocks]
    Eref = np.sort(np.concatenate([e[:min(nev, len(e))] for e in per]))
    scale = max(1.0, max(np.max(np.abs(e)) for e in per))
    K = sum(min(nev, len(b)) for b in blocks)
    block_of = np.zeros(N, dtype=int)
    for i, b in enumerate(blocks):
        block_of[b] = i
    for path in PATHS:
        E, C = runs[path]["E_" + name], runs[path]["C_" + name]
        assert int(runs[path]["K_" + name][0]) == K and E.shape == (K,) and C.shape == (N, K), path
        print("%s %s: |E - Eref| %.3e" % (name, path, np.max(np.abs(E - Eref))))
        assert np.max(np.abs(E - Eref)) < 1e-10 * scale, path
        assert np.all(np.diff(E) >= 0), path
        assert np.max(np.abs(C.T @ S @ C - np.eye(K))) < 1e-10, path
        assert np.max(np.abs(F @ C - S @ C * E)) < 1e-9 * scale, path
        for j in range(K):  # zero rows outside the column's block
            rows = np.nonzero(C[:, j])[0]
            assert len(set(block_of[rows])) == 1, (path, j)
    if nev >= max(len(b) for b in blocks):  # everything asked for: the eigenvalues of the full solver
        assert K == N


def test_device_pointer_entry_is_bitwise_the_host_pointer_one(runs):
    for path in PATHS:
        r = runs[path]
        assert np.array_equal(r["E_dev"], r["E_gen_sigma_pi_3"]) and np.array_equal(r["C_dev"], r["C_gen_sigma_pi_3"]), path


def test_two_calls_repeat_bitwise(runs):
    for path in PATHS:
        r = runs[path]
        assert r["E_repeat_a"].shape == (wk.REPEAT[1],)
        assert np.array_equal(r["E_repeat_a"], r["E_repeat_b"]) and np.array_equal(r["C_repeat_a"], r["C_repeat_b"]), path


def test_errors(hf):
    A = wk.dense_matrix(17)
    for nev in (0, -1):
        with pytest.raises(RuntimeError, match="nev must be at least 1"):
            hf.scf.eig_sym_sel(A, nev)
        with pytest.raises(RuntimeError, match="nev must be at least 1"):
            hf.scf.eig_gsym_sub_sel(A, np.eye(17), [np.arange(17)], nev)
    with pytest.raises(RuntimeError, match="empty symmetry block"):
        hf.scf.eig_gsym_sub_sel(A, np.eye(17), [np.arange(17), np.arange(0)], 2)
    assert hf.scf.eig_sel_count([np.arange(17)], 0) == 0
