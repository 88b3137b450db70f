"""The batched Coulomb build's host side: the C ABI declares the three entries, the device-pointer one stays out of the
hfg_*_dev plan of tests/stream_order_worker.py, the argument refusals need no device, the chunk switch is in the one table,
and the C++ adapter overload compiles against the stand-in matrix class.  No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hf(native_libs):
    os.environ.setdefault("HELFEM_NO_TORCH", "1")
    import helfem_amd
    from helfem_amd import build
    helfem_amd.lib()
    build.build_adapter_test(verbose=False)
    return helfem_amd


def _header():
    with open(os.path.join(ROOT, "include", "helfem_gpu.h")) as fh:
        return fh.read()


def test_header_declares_the_three_entries():
    text = _header()
    args = r"\(hfg_ctx \*ctx, hfg_basis \*basis, int64_t nP, const double \*%s, double \*%s\);"
    assert re.search(r"^int hfg_coulomb_batch" + args % ("P", "J"), text, flags=re.M)
    assert re.search(r"^int hfg_coulomb_batch_devptr" + args % ("dP", "dJ"), text, flags=re.M)
    assert re.search(r"^int hfg_coulomb_energy_matrix" + args % ("P", "W"), text, flags=re.M)


def test_device_pointer_entry_is_not_in_the_dev_plan():
    text = _header()
    dev = re.findall(r"^\s*(?:int|int64_t)\s+(hfg_\w+_dev)\s*\(", text, flags=re.M)
    assert "hfg_coulomb_dev" in dev and not [n for n in dev if "batch" in n]
    assert not re.match(r"hfg_\w+_dev\(", "hfg_coulomb_batch_devptr(")
    # the declaration says why
    at = text.index("int hfg_coulomb_batch_devptr(")
    assert "stream_order_worker.py" in text[at - 600:at] and "test_gpu_coulomb_batch.py" in text[at - 600:at]


def test_refusals_without_a_device(hf):
    L = hf.lib()
    one = (ctypes.c_double * 1)()
    for name in ("hfg_coulomb_batch", "hfg_coulomb_energy_matrix", "hfg_coulomb_batch_devptr"):
        f = getattr(L, name)
        assert f(None, None, -1, None, None) == 1 and b"negative number of densities" in L.hfg_last_error(), name
        assert f(None, None, 2, None, None) == 1 and b"null context or basis" in L.hfg_last_error(), name
    assert L.hfg_coulomb_batch(None, None, 3, one, one) == 1 and b"null context or basis" in L.hfg_last_error()


def test_chunk_switch_is_in_the_table(hf):
    rows = {r["name"]: r for r in hf.tuning_table()}
    r = rows["HELFEM_COULOMB_BATCH_CHUNK"]
    assert r["default"] == "0" and r["read"] == "live" and r["kind"] == "int"


def test_adapter_overload_compiles_against_the_stand_in_matrix_class(hf):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = os.path.join(ROOT, "tests", "cpp", "coulomb_batch_adapter_test.cpp")
    with open(src) as fh:
        assert "basis.coulomb(P)" in fh.read()
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-fsyntax-only", src])
    p = subprocess.run([os.path.join(ROOT, "tests", "cpp", "coulomb_batch_adapter_test"), "compile-only"], stdout=subprocess.PIPE, timeout=60)
    assert p.returncode == 0 and b"adapter compiled" in p.stdout
