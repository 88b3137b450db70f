"""The device-resident DIIS object and the step objects' run(): what can be checked without a GPU -- the exported symbols
and their declarations, the refusals of hfg_diis_create that come before any device call, and the refusal of the options
run() leaves to the drivers."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["hfg_diis_create", "hfg_diis_destroy", "hfg_diis_set_metric_devptr", "hfg_diis_set_blocks", "hfg_diis_update_devptr",
           "hfg_diis_solve_devptr", "hfg_diis_size", "hfg_diis_get"]


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    return helfem_amd


def test_symbols_exported_and_declared(hf):
    L = hf.lib()
    header = open(os.path.join(ROOT, "include", "helfem_gpu.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\bint %s\(" % name, header), name
    assert "typedef struct hfg_diis hfg_diis;" in header
    # entries named *_dev are the plan of the stream-order worker: the new ones end in _devptr
    assert not [n for n in SYMBOLS if n.endswith("_dev")]


def test_create_refusals(hf):
    L = hf.lib()
    h = ctypes.c_void_p()
    fake = ctypes.c_void_p(8)  # never dereferenced: the argument checks come first
    assert L.hfg_diis_create(None, 10, 1, 5, 1e-2, 1e-3, 0, ctypes.byref(h)) == 1 and b"null" in L.hfg_last_error()
    assert L.hfg_diis_create(fake, 10, 1, 5, 1e-2, 1e-3, 0, None) == 1 and b"null" in L.hfg_last_error()
    for N, nspin, order in ((10, 1, 0), (10, 1, -3), (10, 0, 5), (10, 3, 5), (0, 1, 5), (-4, 2, 5)):
        h = ctypes.c_void_p()
        assert L.hfg_diis_create(fake, N, nspin, order, 1e-2, 1e-3, 0, ctypes.byref(h)) != 0, (N, nspin, order)
        assert not h.value


def test_null_object(hf):
    L = hf.lib()
    assert L.hfg_diis_size(None) == 0
    assert L.hfg_diis_destroy(None) == 0
    out = np.zeros(4)
    assert L.hfg_diis_get(None, 0, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 4) == 1
    assert L.hfg_diis_solve_devptr(None, None, None, None) == 1 and b"null object" in L.hfg_last_error()


def test_python_interface_exists(hf):
    assert inspect.isclass(hf.DeviceDIIS)
    for name in ("set_metric", "set_blocks", "update", "solve", "size", "B", "T", "weights", "error"):
        assert hasattr(hf.DeviceDIIS, name), name
    for cls in (hf.DeviceSCFStep, hf.DeviceUSCFStep):
        assert callable(cls.run) and callable(cls.energy)
        pars = inspect.signature(cls.run).parameters
        for name in ("S", "maxit", "convthr", "Enucr", "allreduce", "exchange_blocks", "diis", "callback"):
            assert name in pars, name
        assert pars["maxit"].default == 50 and pars["convthr"].default == 1e-7


@pytest.mark.parametrize("cls", ["DeviceSCFStep", "DeviceUSCFStep"])
@pytest.mark.parametrize("opt", [dict(rohf=True), dict(cuhf=True), dict(readocc=0), dict(maverage=True), dict(dampfock=0.7)])
def test_run_refuses_what_stays_with_the_drivers(hf, cls, opt):
    """before any attribute of the step (context, tables, buffers) is touched: the object here has none"""
    step = object.__new__(getattr(hf, cls))
    with pytest.raises(NotImplementedError, match="not supported by the step objects"):
        step.run(None, **opt)
