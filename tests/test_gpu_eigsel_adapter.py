"""helfem::gpu::scf::eig_gsym_sub_sel of include/helfem_gpu_arma.hpp on the GPU: tests/cpp/eigsel_adapter_test.cpp solves a
two-block problem (orders 40 and 25, nev = 6) through it and through the full adapter call."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_selected_solver_through_the_cpp_adapter_header(native_libs):
    exe = os.path.join(ROOT, "tests", "cpp", "eigsel_adapter_test")
    p = subprocess.run([exe, "run"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0 and "adapter ok" in out, out
    assert re.search(r"^K 12 cols 12 rows 65$", out, flags=re.M), out
    val = dict(zip(*[iter(re.search(r"^dE .*$", out, flags=re.M).group(0).split())] * 2))
    # |F| is about 10: the bounds of test_gpu_eigsel.py::test_generalized_blocked with scale 10
    assert float(val["dE"]) < 1e-9 and float(val["aufbau"]) < 1e-9, out
    assert float(val["res"]) < 1e-8 and float(val["orth"]) < 1e-10 and float(val["leak"]) == 0.0, out
    assert "logic_error_on_nev_0 1" in out
