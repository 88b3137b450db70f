"""hfg_cuhf_update_devptr (Context.cuhf_update), the CUHF constraint of ROHF on device pointers, against the longdouble
dense restatement of tests/rohf_restatement.py on seeded inputs: random SPD S of condition about 5, S-orthonormal occupied
orbitals per spin, the smaller set a perturbed rotation of a subset of the larger (both boundary occupation gaps >= 0.1,
asserted below from NumPy's eigenvalues of C^T S C), random symmetric Fa and Fb.

Shapes, N x (na, nb): 61 (2, 1) small odd order; 61 (3, 0) must leave Fa and Fb untouched; 130 (1, 3) nb > na; 130 (5, 2);
257 (4, 1) order just past a tile multiple; 257 (40, 33) more than 64 columns; 200 (70, 60) more than 128 columns, the dense
route.  tests/cuhf_worker.py runs them all in a child process with the default switches and again with
HELFEM_CUHF_LOWRANK=0, where every shape takes the dense route.

Bound (the issue's).  The error of a device route against the longdouble result is compared with the error of the float64
NumPy dense evaluation against the same longdouble result on the same inputs: at most ten times that (the summation orders
differ), with the floor N eps max|lambda_ref|, the bound of a dot product of length N.  lambda is read as Fa_out - Fa_in
and as Fb_in - Fb_out.

Measured on the MI355X, device error / float64 NumPy error (default route, then HELFEM_CUHF_LOWRANK=0): 0.13 to 0.21 on the
low-rank route, 0.75 to 1.86 on the dense one."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rohf_restatement as rr  # noqa: E402

LD = np.longdouble
FAULT_LIKE = (134, 139, -6, -11)
ROUTES = ["default", "dense"]
LOWRANK = [(N, o) for N, o in rr.SHAPES if sum(o) <= 128 and min(o) > 0]
ids = lambda shapes: ["N%d-na%d-nb%d" % (N, o[0], o[1]) for N, o in shapes]


@pytest.fixture(scope="module")
def runs(native_libs, tmp_path_factory):
    """both settings, one GPU process at a time; nothing more is started after a fault-like end"""
    d = tmp_path_factory.mktemp("cuhf")
    res, stopped = {}, None
    for route in ROUTES:
        if stopped:
            res[route] = "not run: " + stopped
            continue
        e = dict(os.environ)
        e.pop("HELFEM_CUHF_LOWRANK", None)
        if route == "dense":
            e["HELFEM_CUHF_LOWRANK"] = "0"
        path = str(d / (route + ".npz"))
        try:
            out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cuhf_worker.py"), path], env=e, cwd=ROOT, timeout=300,
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        except subprocess.TimeoutExpired:
            stopped = "the worker of '%s' ran into its time limit" % route
            res[route] = stopped
            continue
        text = out.stdout.decode(errors="replace")[-3000:]
        if out.returncode in FAULT_LIKE:
            stopped = "the worker of '%s' ended with status %d" % (route, out.returncode)
        if out.returncode != 0 or "ok" not in text.split():
            res[route] = "status %d\n%s" % (out.returncode, text)
            continue
        res[route] = dict(np.load(path))
    return res


def _run(runs, route):
    if isinstance(runs[route], str):
        pytest.fail("worker of '%s': %s" % (route, runs[route]))
    return runs[route]


def _key(N, o):
    return "%d_%d_%d" % (N, o[0], o[1])


def test_the_child_saw_the_switch(runs):
    assert bool(_run(runs, "default")["switch"][0]) and not bool(_run(runs, "dense")["switch"][0])


@pytest.mark.parametrize("N,occ", LOWRANK + [(200, (70, 60))], ids=ids(LOWRANK + [(200, (70, 60))]))
def test_inputs_have_the_occupation_gaps(N, occ):
    gaps = rr.boundary_gaps(rr.case(N, *occ)["pb"])
    print("gaps at the core / active and active / virtual boundaries: %.3f %.3f" % gaps)
    assert min(gaps) >= 0.1
    assert rr.case(N, *occ)["residual"] < 1e-17, "the longdouble reference's subspaces are decoupled"


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("N,occ", rr.SHAPES, ids=ids(rr.SHAPES))
def test_update_against_the_longdouble_restatement(runs, route, N, occ):
    r, c = _run(runs, route), rr.case(N, *occ)
    k = _key(N, occ)
    if min(occ) == 0 or occ[0] == occ[1]:
        assert bool(r[k + "_untouched"][0]), "Fa and Fb must come back bit for bit"
        return
    assert not bool(r[k + "_untouched"][0])
    for which in ("lamA", "lamB"):
        err = float(np.max(np.abs(r[k + "_" + which].astype(LD) - c["ref"])))
        print("%s %s %s: device error %.3e, float64 NumPy error %.3e, ratio %.2f, floor %.3e, bound %.3e" %
              (route, k, which, err, c["e64"], err / c["e64"], c["floor"], c["bound"]))
        assert err <= c["bound"]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("N,occ", LOWRANK + [(200, (70, 60))], ids=ids(LOWRANK + [(200, (70, 60))]))
def test_two_contexts_give_equal_bits(runs, route, N, occ):
    assert bool(_run(runs, route)[_key(N, occ) + "_same_bits"][0])


@pytest.mark.parametrize("N,occ", LOWRANK, ids=ids(LOWRANK))
def test_lambda_is_bitwise_symmetric_on_the_lowrank_route(runs, N, occ):
    lam = _run(runs, "default")[_key(N, occ) + "_lamA"]
    assert np.array_equal(lam, lam.T)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("N,occ", LOWRANK, ids=ids(LOWRANK))
def test_core_virtual_coupling_vanishes(runs, route, N, occ):
    """Y_c^T (Delta + lambda) Y_v = 0 with the core and virtual natural orbitals of NumPy's dense evaluation"""
    c = rr.case(N, *occ)
    pb = c["pb"]
    lam = _run(runs, route)[_key(N, occ) + "_lamA"].astype(LD)
    Delta = (pb["Fa"].astype(LD) - pb["Fb"].astype(LD)) / 2
    fig = float(np.max(np.abs(c["Yc"].astype(LD).T @ (Delta + lam) @ c["Yv"].astype(LD))))
    print("%s %s: core-virtual coupling left %.3e (bound %.3e)" % (route, _key(N, occ), fig, c["bound"]))
    assert fig <= c["bound"]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("N,occ", [s for s in LOWRANK if s[1][0] > 1], ids=ids([s for s in LOWRANK if s[1][0] > 1]))
def test_rotating_the_occupied_orbitals_changes_nothing(runs, route, N, occ):
    """Ca_o U for an orthogonal U spans the same space: lambda moves by no more than the bound"""
    r, c = _run(runs, route), rr.case(N, *occ)
    fig = float(np.max(np.abs(r[_key(N, occ) + "_lamA_rotated"] - r[_key(N, occ) + "_lamA"])))
    print("%s %s: lambda moved by %.3e (bound %.3e)" % (route, _key(N, occ), fig, c["bound"]))
    assert fig <= c["bound"]
