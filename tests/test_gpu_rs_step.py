"""Range-separated hybrids in the step objects: run() of DeviceSCFStep, DeviceUSCFStep and DeviceROHFStep with
kshort != 0 against the atomic driver (scf_run_atomic / hfg_scf_run) for the same options, on the mixed-kernel table set
(HELFEM_EXL_MIX=1: one exchange build per spin and iteration) and on the two-build route (HELFEM_EXL_MIX=0, the checker).

  He  CAM-LDA0     DeviceSCFStep        Be  CAM-B3LYP   DeviceSCFStep
  Li  CAMY-B3LYP   DeviceUSCFStep       Li  CAM-B3LYP   DeviceROHFStep

at 4 elements x 6 nodes, lmax = 0, convthr = 1e-7 (the drivers' default).  Bounds: Etot and Exx within 1e-8 Eh of the
driver's, the same number of iterations; the two routes within 1e-9 Eh of each other; two ranks on one device give the
single-rank energy to 1e-10.

"The same options" includes the damping of the Fock matrix: the atomic program scales the occupied-virtual blocks by 0.7
while the DIIS error is above 0.1 unless told otherwise, run() leaves damping to the drivers (it refuses dampfock != 1),
so the driver runs with dampfock = 1 here (tests/rs_step_common.py run_driver).  The two loops then take the same
iterations and agree to about 1e-13 Eh; against the DAMPED driver run() would be one iteration short in two of the four
cases and Exx, first order in the density error the stopping test leaves, up to 2.6e-8 off."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rs_step_common as common  # noqa: E402

CONVTHR = 1e-7


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    return helfem_amd


@pytest.fixture(scope="module")
def results(hf):
    """every case once: run() on both routes and the driver"""
    out = {}
    hf.scf_set_iguess(0)
    old = os.environ.get("HELFEM_EXL_MIX")
    try:
        for name in common.CASES:
            runs = {}
            for route in ("1", "0"):
                os.environ["HELFEM_EXL_MIX"] = route  # (a live switch: read when the step object is set up)
                step, S, Enucr = common.make_step(hf, name)
                assert step.mix == (route == "1") and step.kshort != 0.0 and step.rs_kind in (1, 2)
                runs[route] = step.run(S, maxit=50, convthr=CONVTHR, Enucr=Enucr)
            g = common.run_driver(hf, name, CONVTHR)
            print("%s: mixed %d iterations Etot % .10f Exx % .10f, two builds %d % .10f, driver %d % .10f % .10f" %
                  (name, runs["1"]["iterations"], runs["1"]["Etot"], runs["1"]["Exx"], runs["0"]["iterations"], runs["0"]["Etot"],
                   g["iterations"], g["Etot"], g["Exx"]))
            out[name] = (runs["1"], runs["0"], g)
    finally:
        if old is None:
            os.environ.pop("HELFEM_EXL_MIX", None)
        else:
            os.environ["HELFEM_EXL_MIX"] = old
    return out


@pytest.mark.parametrize("name", list(common.CASES))
def test_run_against_the_driver(results, name):
    mixed, two, g = results[name]
    assert mixed["converged"] and two["converged"] and g["converged"]
    assert abs(g["Exx"]) > 1e-2, "a run without exact exchange would prove nothing"
    for who, r in (("mixed", mixed), ("two builds", two)):
        assert abs(r["Etot"] - g["Etot"]) <= 1e-8, (name, who, r["Etot"], g["Etot"])
        assert abs(r["Exx"] - g["Exx"]) <= 1e-8, (name, who, r["Exx"], g["Exx"])


@pytest.mark.parametrize("name", list(common.CASES))
def test_run_takes_as_many_iterations_as_the_driver(results, name):
    """measured on an MI355X, run() on either route and the driver alike: He 6, Be 8, Li CAMY-B3LYP 9, Li CAM-B3LYP ROHF 9"""
    mixed, two, g = results[name]
    for who, r in (("mixed", mixed), ("two builds", two)):
        assert r["iterations"] == g["iterations"], (name, who, r["iterations"], g["iterations"])


@pytest.mark.parametrize("name", list(common.CASES))
def test_the_two_routes_agree(results, name):
    mixed, two, _ = results[name]
    for k in ("Etot", "Exx", "E1", "Ecoul", "Exc"):
        assert abs(mixed[k] - two[k]) <= 1e-9, (name, k, mixed[k], two[k])


@pytest.mark.parametrize("route", ["1", "0"], ids=["mixed", "two-builds"])
def test_both_spins_through_the_batched_entries(hf, results, route, monkeypatch):
    """HELFEM_USCF_KBATCH=1 with a screened term: K[Pa] and K[Pb] through hfg_mix_exchange_occ_batch_devptr (mixed set), or
    through hfg_exchange_occ_batch_devptr and hfg_rs_exchange_batch_devptr added on the device (two builds).  Every batched
    entry gives bitwise what its single entry gives: on the mixed set the whole run repeats the unbatched one bit for bit;
    the two-build run is held to the same iterations and to the 1e-9 between the routes.  Then the entries' other form, for
    densities set without their orbitals: exchange() batched against unbatched, within N eps max|K|."""
    name = "Li_CAMY-B3LYP"
    monkeypatch.setenv("HELFEM_EXL_MIX", route)
    monkeypatch.setenv("HELFEM_USCF_KBATCH", "1")
    step, S, Enucr = common.make_step(hf, name)
    assert step.kbatch and step.mix == (route == "1")
    r = step.run(S, maxit=50, convthr=CONVTHR, Enucr=Enucr)
    ref = results[name][0 if route == "1" else 1]
    print("%s route %s batched: %d iterations Etot % .12f, unbatched %d % .12f" % (name, route, r["iterations"], r["Etot"], ref["iterations"], ref["Etot"]))
    assert r["converged"] and r["iterations"] == ref["iterations"]
    for k in ("Etot", "Exx", "E1", "Ecoul", "Exc"):
        assert abs(r[k] - ref[k]) <= 1e-9, (k, r[k], ref[k])
    if route == "1":
        assert r["trace"] == ref["trace"]
    # the densities alone (no orbitals handed over): batched against unbatched, one step each
    N = step.N
    Pa, Pb = step.numpy(step.Pa, (N, N)).copy(), step.numpy(step.Pb, (N, N)).copy()
    Ks = []
    for kb in ("1", "0"):
        monkeypatch.setenv("HELFEM_USCF_KBATCH", kb)
        s2, _, _ = common.make_step(hf, name)
        assert s2.kbatch == (kb == "1")
        s2.set_density(Pa, Pb)
        s2.exchange()
        Ks.append(s2.numpy(s2.K, (2 * N * N,)).copy())
    scale = float(abs(Ks[1]).max())
    assert scale > 1e-3 and float(abs(Ks[0] - Ks[1]).max()) <= N * 2.0 ** -52 * scale


def test_two_ranks_converge_together(native_libs, results, tmp_path):
    """two gloo ranks on the one device, the mixed build sharded over them (the pair path deals the table slots out) and
    all-reduced: the traces of both ranks are equal bit for bit, and the energy is the single-rank run's"""
    name = "Be_CAM-B3LYP"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", HELFEM_NUM_THREADS="4", HELFEM_EXL_MIX="1")
    prefix = str(tmp_path / "two")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29553", os.path.join(ROOT, "tests", "rs_step_worker.py"), prefix, name]
    subprocess.run(cmd, check=True, env=env, cwd=ROOT, timeout=600, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    a, b = [json.load(open("%s.rank%d.json" % (prefix, r)))[name] for r in range(2)]
    one = results[name][0]
    assert a["mix"] and b["mix"] and a["converged"] and b["converged"]
    assert a["trace"] == b["trace"] and a["Etot"] == b["Etot"] and a["iterations"] == b["iterations"]
    assert abs(a["Etot"] - one["Etot"]) <= 1e-10, (a["Etot"], one["Etot"])
