"""The device build of the range-separated exchange tables (hip/rs_tei_dev.hip), what can be checked without a GPU: the entry
points exist and are declared, refuse what hfg_compute_rs_tei refuses, the switch is in the table, and the Python layer asks
for a context instead of picking one."""
import ctypes
import os
import re

import pytest

import common

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    helfem_amd.lib()
    return helfem_amd


def test_entry_points_are_exported_and_declared(hf):
    L = hf.lib()
    with open(os.path.join(ROOT, "include", "helfem_gpu.h")) as fh:
        header = fh.read()
    for name in ("hfg_compute_rs_tei_dev", "hfg_rs_special_dev", "hfg_set_erfc_binomial_mode"):
        assert hasattr(L, name), name
        assert re.search(r"^(int|void) %s\(" % name, header, flags=re.M), name
    with open(os.path.join(ROOT, "include", "helfem_gpu_arma.hpp")) as fh:
        assert fh.read().count("hfg_compute_rs_tei_dev(this->context()") == 2  # compute_yukawa and compute_erfc overloads
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        assert "`hfg_compute_rs_tei_dev(" in fh.read()


@pytest.mark.parametrize("kind", [1, 2])
def test_diatomic_handle_is_refused_with_the_reference_text(hf, kind):
    gb, _ = common.make_bases(oracle=False)
    L = hf.lib()
    assert L.hfg_compute_rs_tei(gb.h, kind, 0.4) != 0
    host_text = L.hfg_last_error().decode()
    assert L.hfg_compute_rs_tei_dev(None, gb.h, kind, 0.4) != 0  # refused before the context is looked at
    assert L.hfg_last_error().decode() == host_text == "Range separated functionals are not supported.\n"


def test_bad_arguments_fail_with_an_error_not_a_crash(hf):
    gb, _ = common.make_atomic_bases(oracle=False)
    L = hf.lib()
    assert L.hfg_compute_rs_tei_dev(None, gb.h, 3, 0.4) != 0 and "unknown range-separation kernel" in L.hfg_last_error().decode()
    assert L.hfg_compute_rs_tei_dev(None, gb.h, 1, 0.4) != 0 and "context" in L.hfg_last_error().decode()
    out = (ctypes.c_double * 1)()
    assert L.hfg_rs_special_dev(None, 0, 0, out, out, 1, out) != 0 and "context" in L.hfg_last_error().decode()


def test_switch_is_in_the_table_with_default_host(hf):
    rows = {r["name"]: r for r in hf.tuning_table()}
    r = rows["HELFEM_RS_TEI"]
    assert r["default"] == "host" and r["read"] == "once" and "dev" in r["meaning"]


def test_device_build_needs_a_context(hf):
    gb, _ = common.make_atomic_bases(oracle=False)
    for call in (gb.compute_yukawa, gb.compute_erfc):
        with pytest.raises(ValueError, match="context"):
            call(0.4, device=True)
    gb.compute_yukawa(0.4)  # the default is the host build, as before
    assert gb.atomic_table("rs_tei", 0, 0).shape[0] > 0
