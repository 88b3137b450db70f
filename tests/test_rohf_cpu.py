"""The CUHF constraint of the step objects (hfg_cuhf_update_devptr, Context.cuhf_update, DeviceROHFStep): what can be checked
without a GPU -- the exported symbols and their declarations, the argument checks that come before any device call, the
Python interface, the switch, the adapter program, and the algebra: the rank-(na + nb) form that hip/cuhf_dev.hip evaluates
equals the dense natural-orbital form of the reference (tests/rohf_restatement.py, NumPy against numpy.longdouble)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import rohf_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    return helfem_amd


def test_symbols_exported_and_declared(hf):
    L = hf.lib()
    header = open(os.path.join(ROOT, "include", "helfem_gpu.h")).read()
    for name in ("hfg_cuhf_update_devptr", "hfg_rohf_update"):
        assert hasattr(L, name), name
        assert re.search(r"\bint %s\(" % name, header), name
    # entries named *_dev are the plan of tests/stream_order_worker.py: this one has its own stream-order test
    assert not re.search(r"\bhfg_cuhf\w*_dev\(", header)


def test_argument_checks_come_before_any_device_call(hf):
    L = hf.lib()
    f = L.hfg_cuhf_update_devptr
    f.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                  ctypes.c_void_p, ctypes.c_void_p]
    fake = ctypes.c_void_p(8)  # never dereferenced
    assert f(None, 10, fake, fake, 2, fake, 1, fake, fake) == 1 and b"null context" in L.hfg_last_error()
    assert f(fake, 0, fake, fake, 2, fake, 1, fake, fake) == 1
    assert f(fake, 10, fake, fake, 11, fake, 1, fake, fake) == 1 and b"nocc" in L.hfg_last_error()
    assert f(fake, 10, fake, fake, -1, fake, 1, fake, fake) == 1
    assert f(fake, 10, None, fake, 2, fake, 1, fake, fake) == 1 and b"null pointer" in L.hfg_last_error()
    # nothing to constrain: returns before it looks at a pointer or the device
    assert f(fake, 10, None, None, 3, None, 0, None, None) == 0
    assert f(fake, 10, None, None, 2, None, 2, None, None) == 0


def test_python_interface_exists(hf):
    assert callable(hf.Context.cuhf_update)
    assert list(inspect.signature(hf.Context.cuhf_update).parameters) == ["self", "S", "Ca", "na", "Cb", "nb", "Fa", "Fb"]
    assert inspect.isclass(hf.DeviceROHFStep) and issubclass(hf.DeviceROHFStep, hf.DeviceUSCFStep)
    for name in ("run", "step", "set_overlap", "energy"):
        assert callable(getattr(hf.DeviceROHFStep, name)), name
    assert hf.DeviceROHFStep.run is hf.DeviceSCFStep.run
    # step() is the base class's composition; what makes it ROHF is the hook between the Fock build and the eigensolve
    assert hf.DeviceROHFStep._constrain is not hf.DeviceSCFStep._constrain and hf.DeviceROHFStep._applies_cuhf


def test_step_applies_the_constraint_after_the_fock_stage(hf):
    step = object.__new__(hf.DeviceROHFStep)
    step.S, calls = None, []
    step._fock_stage = lambda allreduce: calls.append("fock")
    step._eig_stage = lambda allreduce, exchange_blocks: calls.append("eig")
    with pytest.raises(RuntimeError, match="set_overlap first"):
        step.step()
    assert calls == ["fock"]


@pytest.mark.parametrize("opt", [dict(readocc=0), dict(maverage=True), dict(dampfock=0.7)])
def test_run_still_refuses_what_stays_with_the_drivers(hf, opt):
    step = object.__new__(hf.DeviceROHFStep)
    with pytest.raises(NotImplementedError, match="not supported by the step objects"):
        step.run(None, **opt)


def test_switch_is_in_the_table(hf):
    rows = {r["name"]: r for r in hf.tuning_table()}
    r = rows["HELFEM_CUHF_LOWRANK"]
    assert (r["kind"], r["default"], r["read"]) == ("off if 0", "on", "live")


def test_adapter_program_compiles_and_links(native_libs):
    from helfem_amd import build
    exe = build._build_adapter_program("rohf_adapter_check", False)
    p = subprocess.run([exe, "compile-only"], stdout=subprocess.PIPE, timeout=60)
    assert p.returncode == 0 and b"adapter compiled" in p.stdout
    text = open(os.path.join(ROOT, "include", "helfem_gpu_arma.hpp")).read()
    assert re.search(r"void ROHF_update\(const Context &ctx, Mat &Fa, Mat &Fb, const Mat &P, const Mat &Sh, const Mat &Sinvh, size_t nocca, size_t noccb\)", text)


@pytest.mark.parametrize("N,occ", rr.SHAPES, ids=["N%d-na%d-nb%d" % (N, o[0], o[1]) for N, o in rr.SHAPES])
def test_lowrank_form_equals_the_dense_form(N, occ):
    """the proof of the algebra: error of the NumPy low-rank form against the longdouble dense form, within ten times the
    error of the float64 dense form against it (floor N eps max|lambda|)"""
    c = rr.case(N, *occ)
    lam = rr.lowrank(c["pb"])
    if min(occ) == 0 or occ[0] == occ[1]:
        assert not np.any(lam) and not np.any(c["ref"]) and not np.any(c["lam64"])
        return
    assert min(rr.boundary_gaps(c["pb"])) >= 0.1 and c["residual"] < 1e-17
    err = float(np.max(np.abs(lam.astype(LD) - c["ref"])))
    print("low-rank error %.3e, float64 dense error %.3e, floor %.3e, bound %.3e" % (err, c["e64"], c["floor"], c["bound"]))
    assert float(np.max(np.abs(c["ref"]))) > 0.1, "a reference that is zero would prove nothing"
    assert err <= c["bound"]
    assert np.array_equal(c["ref"], c["ref"].T)
