"""DeviceSCFStep.run / DeviceUSCFStep.run: the step objects' converging loop (DeviceDIIS on top of the stage methods)
against the product driver (scf_diatomic, core guess) and the oracle's scf_diatomic on the smallest diatomic bases of
tests/test_gpu_parity.py.

Bounds.  All three loops stop on max |err| < convthr and |dE| < convthr with convthr = 1e-7, and the energy is stationary
in the density: a density that is within the stopping test of the fixed point has an energy error of second order, far
below convthr.  So the total energies agree to convthr; the components are first order in the density error and agree to
10 convthr.  Iteration counts are not compared (the loops order their reductions differently); DESIGN.md records them."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scf_run_common as common  # noqa: E402

CONVTHR = 1e-7
CONTROL = "HeH_PBE"  # the case of the control below (chosen by running all five)


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    return helfem_amd


@pytest.fixture(scope="module")
def results(hf):
    """every case once: run(), the driver and the oracle"""
    import oracle_lib as orc
    out = {}
    hf.scf_set_iguess(0)
    for name, kw in common.CASES.items():
        step, S, Enucr = common.make_step(hf, kw)
        seen = []
        r = step.run(S, maxit=50, convthr=CONVTHR, Enucr=Enucr, callback=lambda it, E, err: seen.append((it, E, err)))
        g = hf.scf_diatomic(convthr=CONVTHR, maxit=50, **kw)
        o = orc.scf_diatomic(convthr=CONVTHR, maxit=50, **kw)
        print("%s: run %d iterations Etot % .10f, driver %d % .10f, oracle %d % .10f" %
              (name, r["iterations"], r["Etot"], g["iterations"], g["Etot"], o["iterations"], o["Etot"]))
        out[name] = (r, g, o, seen)
    return out


@pytest.mark.parametrize("name", list(common.CASES))
def test_run_against_the_driver_and_the_oracle(results, name):
    r, g, o, seen = results[name]
    assert r["converged"] and g["converged"] and o["converged"]
    assert r["iterations"] <= 50 and len(r["trace"]) == r["iterations"]
    assert [(it, E, err) for it, (E, err) in enumerate(r["trace"], 1)] == seen, "the callback sees every iteration"
    assert r["trace"][-1][0] == r["Etot"] and r["trace"][-1][1] < CONVTHR
    for who, ref in (("driver", g), ("oracle", o)):
        assert abs(r["Etot"] - ref["Etot"]) <= CONVTHR, (name, who, r["Etot"], ref["Etot"])
        comps = dict(E1=ref["Ekin"] + ref["Epot"], Ecoul=ref["Ecoul"], Exx=ref["Exx"], Exc=ref["Exc"], Enucr=ref["Enucr"])
        for k, v in comps.items():
            assert abs(r[k] - v) <= 10 * CONVTHR, (name, who, k, r[k], v)
    assert abs(r["Etot"] - (r["E1"] + r["Ecoul"] + r["Exx"] + r["Exc"] + r["Enucr"])) < 1e-12


def test_bare_steps_do_not_get_there(hf, results):
    """control: as many bare step() iterations from the same core guess as run() needed leave the energy further than
    convthr from the driver's -- the acceleration is what converges the loop, not the iteration count"""
    r, g, _, _ = results[CONTROL]
    step, S, Enucr = common.make_step(hf, common.CASES[CONTROL])
    step._core_guess(None, None)
    for _ in range(r["iterations"] - 1):
        step.step()
    step._fock_stage(None)
    e = step.energy(Enucr)
    print("%s: %d bare steps leave Etot % .10f, driver % .10f" % (CONTROL, r["iterations"], e["Etot"], g["Etot"]))
    assert abs(e["Etot"] - g["Etot"]) > CONVTHR


def test_run_keeps_to_its_density_when_one_is_set(hf, results):
    """a density set by the caller is the starting point (no core guess): from the converged density the loop needs the
    one iteration the |dE| test of the driver costs after it (Eold starts at zero), or two"""
    r0 = results["H2_PBE"][0]
    step, S, Enucr = common.make_step(hf, common.CASES["H2_PBE"])
    first = step.run(S, Enucr=Enucr)
    N = step.N
    step.set_density(step.numpy(step.P, (N, N)), step.numpy(step.C, (N, N)))
    again = step.run(S, Enucr=Enucr)
    assert again["converged"] and again["iterations"] <= 2 and abs(again["Etot"] - r0["Etot"]) <= CONVTHR
    assert first["iterations"] == r0["iterations"] and first["Etot"] == r0["Etot"], "a fresh object repeats the run bit for bit"


def _ranks(nranks, prefix, names):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", HELFEM_NUM_THREADS="4")
    worker = os.path.join(ROOT, "tests", "scf_run_worker.py")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks),
           "--master-addr", "127.0.0.1", "--master-port", str(29540 + nranks), worker, prefix, names]
    subprocess.run(cmd, check=True, env=env, cwd=ROOT, timeout=600, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return [json.load(open("%s.rank%d.json" % (prefix, r))) for r in range(nranks)]


def test_two_ranks_converge_together(native_libs, results, tmp_path):
    """two gloo ranks on the one device, each with its own DeviceDIIS and no collective for it: both ranks end on the same
    iteration with the same energy, which is the single-rank run's (the exchange matrix and the eigenvector blocks are
    summed / gathered over the ranks, so the last bits of F differ from one rank's own build: 1e-10)"""
    names = ["H2_PBE0", "HeH_PBE"]  # restricted with the sharded exchange, unrestricted
    two = _ranks(2, str(tmp_path / "two"), ",".join(names))
    for name in names:
        a, b, one = two[0][name], two[1][name], results[name][0]
        assert a["converged"] and b["converged"]
        assert a["Etot"] == b["Etot"] and a["iterations"] == b["iterations"], (name, a["Etot"], b["Etot"])
        assert a["trace"] == b["trace"]
        assert abs(a["Etot"] - one["Etot"]) <= 1e-10 and a["iterations"] == one["iterations"], (name, a["Etot"], one["Etot"])
