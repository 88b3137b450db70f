"""A stage's workspace lives in its context (eigensolver stages) or its table set (Fock and exchange builds) and dies with
it: nothing survives under a recycled address, two live contexts never see each other's cached task lists, and a table
set that is rebuilt or destroyed takes its workspaces along.  tests/ownership_worker.py makes the calls in a child
process (twice: once with HELFEM_EIGSEL=stein for the selected solve, a switch read once per process); repeated runs are
compared bitwise (fixed summation orders, no atomics on these paths), everything else against NumPy or the oracle at the
bounds of test_gpu_parity.py (test_eig_sym_vs_lapack, test_eig_gsym_sub_parity, test_coulomb_parity, test_exchange_parity),
test_gpu_eigsel.py (test_dense_against_lapack) and test_gpu_rs.py (test_rs_exchange_parity)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ownership_worker as wk  # noqa: E402


def _run(mode, path, env):
    e = dict(os.environ)
    e.pop("HELFEM_EIGSEL", None)
    e.pop("HELFEM_EXCHANGE", None)
    e.update(env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ownership_worker.py"), mode, path], env=e, cwd=ROOT, timeout=300,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0 and b"ok" in out.stdout, out.stdout.decode()[-3000:]
    print(out.stdout.decode())
    return np.load(path)


@pytest.fixture(scope="module")
def run_all(native_libs, tmp_path_factory):
    return _run("all", str(tmp_path_factory.mktemp("ownership") / "all.npz"), {})


@pytest.fixture(scope="module")
def run_sel(native_libs, tmp_path_factory):
    return _run("sel", str(tmp_path_factory.mktemp("ownership") / "sel.npz"), dict(HELFEM_EIGSEL="stein"))


def _same(r, a, b):
    return r[a].shape == r[b].shape and np.array_equal(r[a], r[b])


def _check_eig_sym(A, E, C):
    """the bounds of test_eig_sym_vs_lapack / test_dense_against_lapack"""
    n, nev = A.shape[0], len(E)
    Eref = np.linalg.eigh(A)[0]
    scale = max(1.0, np.max(np.abs(Eref)))
    assert C.shape == (n, nev)
    assert np.max(np.abs(E - Eref[:nev])) < 1e-12 * scale * max(n, 10)
    assert np.max(np.abs(C.T @ C - np.eye(nev))) < 1e-12 * max(n, 10)
    assert np.max(np.abs(A @ C - C * E)) < 1e-11 * scale * max(n, 10)


def test_context_lifetime(run_all):
    r = run_all
    for n in (wk.N_SMALL, wk.N_PERSISTENT):
        assert _same(r, "a_E%d" % n, "b_E%d" % n) and _same(r, "a_C%d" % n, "b_C%d" % n), n
        _check_eig_sym(wk.dense_matrix(n), r["b_E%d" % n], r["b_C%d" % n])
    assert _same(r, "a_Eg", "b_Eg") and _same(r, "a_Cg", "b_Cg")
    # the bounds of test_eig_gsym_sub_parity, against numpy.linalg.eigh of the blocks reduced with Cholesky factors
    F, S, blocks = wk.block_problem()
    E, C = r["b_Eg"], r["b_Cg"]
    per = []
    for b in blocks:
        Linv = np.linalg.inv(np.linalg.cholesky(S[np.ix_(b, b)]))
        per.append(np.linalg.eigh(Linv @ F[np.ix_(b, b)] @ Linv.T)[0])
    Eref = np.sort(np.concatenate(per))
    scale = max(1.0, np.max(np.abs(Eref)))
    assert np.max(np.abs(E - Eref)) < 1e-10 * scale
    assert np.all(np.diff(E) >= 0)
    assert np.max(np.abs(C.T @ S @ C - np.eye(len(E)))) < 1e-9
    assert np.max(np.abs(F @ C - S @ C * E)) < 1e-9 * scale


def test_context_lifetime_of_the_selected_solve(run_sel):
    r = run_sel
    assert r["a_Esel"].shape == (wk.SEL[1],)
    for k in ("Esel", "Csel", "E%d" % wk.N_SMALL, "C%d" % wk.N_SMALL):
        assert _same(r, "a_" + k, "b_" + k), k
    _check_eig_sym(wk.dense_matrix(wk.SEL[0]), r["b_Esel"], r["b_Csel"])
    _check_eig_sym(wk.dense_matrix(wk.N_SMALL), r["b_E%d" % wk.N_SMALL], r["b_C%d" % wk.N_SMALL])


def test_two_live_contexts_interleaved(run_all):
    r = run_all
    assert _same(r, "i_E1", "i_E1again") and _same(r, "i_C1", "i_C1again")
    _check_eig_sym(wk.dense_matrix(wk.N_OTHER), r["i_E2"], r["i_C2"])
    _check_eig_sym(wk.dense_matrix(wk.N_PERSISTENT), r["i_E1"], r["i_C1"])


def test_table_set_lifetime(run_all):
    import common
    r = run_all
    for k in ("J", "K", "Kgen", "H"):
        assert _same(r, "t1_" + k, "t2_" + k), k
    assert np.max(np.abs(r["t1_H"])) > 0.0
    # the fast path and the general kernels are two routes to the same matrix (test_exchange_general_kernels_parity's bound
    # holds for each against the oracle, so twice that between them)
    assert common.relerr(r["t1_Kgen"], r["t1_K"]) < 2e-12
    # a new basis after the old one was destroyed: against the oracle
    _, ob = common.make_bases(*wk.DIATOMIC_2, product=False)
    ob.compute_tei(True)
    gshape, _ = common.make_bases(*wk.DIATOMIC_2, oracle=False)
    P = wk.diatomic_density(gshape)
    assert r["t3_J"].shape == P.shape and r["t3_J"].shape != r["t1_J"].shape
    assert common.relerr(r["t3_J"], ob.coulomb(P)) < 1e-12
    assert common.relerr(r["t3_K"], ob.exchange(P)) < 1e-12


def test_range_separated_table_set_lifetime(run_all):
    import common
    r = run_all
    assert _same(r, "r1_K", "r2_K")
    ga, oa = common.make_atomic_bases(*wk.ATOMIC)
    oa.compute_tei(True)
    oa.compute_erfc(wk.OMEGA)
    P = wk.atomic_density(ga)
    assert common.relerr(r["r2_K"], oa.rs_exchange(P)) < 1e-12
    assert common.relerr(r["r2_Kfull"], oa.exchange(P)) < 1e-12  # the first table set beside it
