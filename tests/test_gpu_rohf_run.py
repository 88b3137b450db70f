"""DeviceROHFStep.run: the step objects' converging loop with the CUHF constraint (hfg_cuhf_update_devptr between energy()
and the DIIS update) against the product driver (scf_atomic / scf_diatomic with M < 0, core guess) and the oracle's driver,
for Li and N at the bases of Li_ROHF and N_ROHF of tests/test_gpu_parity.py and the HeH doublet at the small basis of
tests/scf_run_common.py.

Bounds: those of tests/test_gpu_scf_run.py.  All three loops stop on max |err| < convthr and |dE| < convthr with
convthr = 1e-7 and the energy is stationary in the density, so the total energies agree to convthr and the components, first
order in the density error, to 10 convthr.  The literature values and tolerances are those of Li_ROHF and N_ROHF."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rohf_run_common as common  # noqa: E402

CONVTHR = 1e-7
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    return helfem_amd


@pytest.fixture(scope="module")
def results(hf):
    """every case once: run(), the driver and the oracle; the converged step object is kept"""
    import oracle_lib as orc
    out = {}
    hf.scf_set_iguess(0)
    for name, (program, _, _, _) in common.CASES.items():
        step, S, Enucr = common.make_step(hf, name)
        r = step.run(S, maxit=50, convthr=CONVTHR, Enucr=Enucr)
        kw = common.driver_keywords(name)
        g = getattr(hf, "scf_" + program)(convthr=CONVTHR, maxit=50, **kw)
        o = getattr(orc, "scf_" + program)(convthr=CONVTHR, maxit=50, **kw)
        print("%s: run %d iterations Etot % .10f, driver %d % .10f, oracle %d % .10f" %
              (name, r["iterations"], r["Etot"], g["iterations"], g["Etot"], o["iterations"], o["Etot"]))
        out[name] = (r, g, o, step, S, Enucr)
    return out


@pytest.mark.parametrize("name", list(common.CASES))
def test_run_against_the_driver_and_the_oracle(results, name):
    r, g, o = results[name][:3]
    lit, littol = common.CASES[name][2:]
    assert r["converged"] and g["converged"] and o["converged"]
    assert r["iterations"] <= 50 and len(r["trace"]) == r["iterations"] and r["trace"][-1][1] < CONVTHR
    for who, ref in (("driver", g), ("oracle", o)):
        assert abs(r["Etot"] - ref["Etot"]) <= CONVTHR, (name, who, r["Etot"], ref["Etot"])
        comps = dict(E1=ref["Ekin"] + ref["Epot"], Ecoul=ref["Ecoul"], Exx=ref["Exx"], Exc=ref["Exc"], Enucr=ref["Enucr"])
        for k, v in comps.items():
            assert abs(r[k] - v) <= 10 * CONVTHR, (name, who, k, r[k], v)
    if lit is not None:
        assert abs(r["Etot"] - lit) <= littol, (name, r["Etot"], lit)


def test_the_constraint_acts(hf, results):
    """Li: the restricted open-shell energy lies above the unrestricted one by more than 10 convthr"""
    r = results["Li"][0]
    step, S, Enucr = common.make_step(hf, "Li", cls=hf.DeviceUSCFStep)
    u = step.run(S, maxit=50, convthr=CONVTHR, Enucr=Enucr)
    print("Li: ROHF % .10f, UHF % .10f" % (r["Etot"], u["Etot"]))
    assert u["converged"] and r["Etot"] - u["Etot"] > 10 * CONVTHR


@pytest.mark.parametrize("name", list(common.CASES))
def test_natural_occupations_are_two_one_zero(results, name):
    step, S = results[name][3:5]
    N = step.N
    P = step.numpy(step.Pa, (N, N)) + step.numpy(step.Pb, (N, N))
    s, U = np.linalg.eigh(S)
    Sh = (U * np.sqrt(s)) @ U.T
    occ = np.linalg.eigvalsh(Sh @ P @ Sh)[::-1]
    want = np.zeros(N)
    want[:step.nela] = 1.0
    want[:step.nelb] = 2.0
    print("%s: natural occupations off by %.3e" % (name, np.max(np.abs(occ - want))))
    assert np.max(np.abs(occ - want)) <= 1e-6


@pytest.mark.parametrize("name", ["Li", "N"])
def test_lambda_stays_inside_the_symmetry_blocks(results, name):
    """the orbitals are block diagonal, so lambda is up to rounding: its part between the blocks is below N eps max|lambda|
    (the eigensolve and the blocked DIIS error read the diagonal blocks only)"""
    step = results[name][3]
    N = step.N
    step._fock_stage(None)
    before = step.numpy(step.Fa, (N, N)).copy()
    step._constrain()
    lam = step.numpy(step.Fa, (N, N)) - before
    bid = np.zeros(N, dtype=int)
    for ib, b in enumerate(step.blocks):
        bid[b] = ib
    off = bid[:, None] != bid[None, :]
    fig, scale = (float(np.max(np.abs(lam[off]))) if off.any() else 0.0), float(np.max(np.abs(lam)))
    print("%s: %d blocks, max|lambda| %.3e, between the blocks %.3e (bound %.3e)" % (name, len(step.blocks), scale, fig, N * EPS * scale))
    assert scale > 0.0 and fig <= N * EPS * scale


def test_step_applies_the_constraint_too(hf, results):
    """from the converged density one step() of the restricted open-shell object stays there (an unconstrained step would
    fall towards the unrestricted energy, which test_the_constraint_acts shows to lie more than 10 convthr lower); without
    the overlap matrix step() refuses"""
    r, _, _, step, S, Enucr = results["Li"]
    step.step()
    step._fock_stage(None)
    e = step.energy(Enucr)
    print("Li: one more step % .10f, converged % .10f" % (e["Etot"], r["Etot"]))
    assert abs(e["Etot"] - r["Etot"]) <= CONVTHR
    fresh = common.make_step(hf, "Li")[0]
    with pytest.raises(RuntimeError, match="set_overlap"):
        fresh._core_guess(None, None)
        fresh.step()


def test_density_without_orbitals_is_refused(hf, results):
    step, S, Enucr = results["HeH"][3:6]
    N = step.N
    fresh = common.make_step(hf, "HeH")[0]
    fresh.set_density(step.numpy(step.Pa, (N, N)), step.numpy(step.Pb, (N, N)))
    with pytest.raises(RuntimeError, match="needs the orbitals"):
        fresh.run(S, Enucr=Enucr)
    for opt in (dict(readocc=0), dict(maverage=True), dict(dampfock=0.7)):
        with pytest.raises(NotImplementedError):
            fresh.run(S, Enucr=Enucr, **opt)


def test_two_ranks_converge_together(native_libs, results, tmp_path):
    """two gloo ranks on the one device, each applying the constraint to identical inputs with no collective for it: the
    traces of both ranks are equal bit for bit, and the energy is the single-rank run's (1e-10, as in test_gpu_scf_run.py:
    the exchange matrix and the eigenvector blocks are summed / gathered over the ranks)"""
    names = ["Li", "HeH"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", HELFEM_NUM_THREADS="4")
    prefix = str(tmp_path / "two")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29547", os.path.join(ROOT, "tests", "rohf_run_worker.py"), prefix, ",".join(names)]
    subprocess.run(cmd, check=True, env=env, cwd=ROOT, timeout=600, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    two = [json.load(open("%s.rank%d.json" % (prefix, r))) for r in range(2)]
    for name in names:
        a, b, one = two[0][name], two[1][name], results[name][0]
        assert a["converged"] and b["converged"]
        assert a["trace"] == b["trace"] and a["Etot"] == b["Etot"] and a["iterations"] == b["iterations"]
        assert abs(a["Etot"] - one["Etot"]) <= 1e-10, (name, a["Etot"], one["Etot"])


def test_adapter_program_on_the_device(native_libs):
    """scf::ROHF_update of include/helfem_gpu_arma.hpp on a problem with a closed-form answer (tests/cpp/rohf_adapter_check.cpp):
    lambda is one row and column of -Delta, each element one rounded product chain of identity matrices"""
    p = subprocess.run([os.path.join(ROOT, "tests", "cpp", "rohf_adapter_check"), "run"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = p.stdout.decode()
    print(text)
    assert p.returncode == 0 and "adapter ok" in text
    figs = dict(line.split()[i:i + 2] for line in text.splitlines() if line.startswith("deviation") for i in (0, 2))
    assert float(figs["deviation"]) <= 37 * EPS and float(figs["opposite"]) <= 4 * EPS
    assert "untouched 1" in text and "logic_error_on_shape 1" in text
