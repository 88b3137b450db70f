"""The selected eigensolver's host side: the C ABI declares it, the count needs no device, the path switch is in the one
table of switches, and the C++ adapter compiles with the host compiler."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hf(native_libs):
    os.environ.setdefault("HELFEM_NO_TORCH", "1")
    import helfem_amd
    helfem_amd.lib()
    return helfem_amd


def test_header_declares_the_four_functions():
    with open(os.path.join(ROOT, "include", "helfem_gpu.h")) as fh:
        text = fh.read()
    assert re.search(r"int64_t hfg_eig_sel_count\(int nblk, const int64_t \*blk_ptr, int64_t nev\);", text)
    for name in ("hfg_eig_sym_sel", "hfg_eig_gsym_sub_sel", "hfg_eig_gsym_sub_sel_dev"):
        assert re.search(r"^int %s\(hfg_ctx \*ctx," % name, text, flags=re.M), name
    assert "Aufbau" in text


def test_count_clamps_and_sums_without_a_device(hf):
    for sizes, nev, want in (([1380, 1470, 1380], 32, 96), ([1, 2, 3, 5, 31, 33], 2, 11), ([7], 100, 7), ([4, 4], 4, 8), ([3], 0, 0)):
        blocks, o = [], 0
        for sz in sizes:
            blocks.append(np.arange(o, o + sz))
            o += sz
        assert hf.scf.eig_sel_count(blocks, nev) == want, (sizes, nev)
    f = hf.lib().hfg_eig_sel_count
    f.restype = ctypes.c_int64
    assert f(0, None, ctypes.c_int64(3)) == 0


def test_count_function_under_the_host_sanitizers(tmp_path):
    """the host-only helper of the selected solver, compiled with a stand-alone main under ASan + UBSan and run on the CPU"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "eigsel_count_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "eigsel_count_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert p.returncode == 0 and b"count ok" in p.stdout, p.stdout.decode()


def test_switch_is_in_the_table(hf):
    rows = {r["name"]: r for r in hf.tuning_table()}
    assert rows["HELFEM_EIGSEL"]["default"] == "crossover" and rows["HELFEM_EIGSEL"]["read"] == "once"
    assert "stein" in rows["HELFEM_EIGSEL"]["meaning"] and "dc" in rows["HELFEM_EIGSEL"]["meaning"]


def test_adapter_header_compiles_with_the_host_compiler(hf):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = os.path.join(ROOT, "tests", "cpp", "eigsel_adapter_test.cpp")
    with open(src) as fh:
        assert "eig_gsym_sub_sel" in fh.read()
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-fsyntax-only", src])
    # and the program that build() links against the library, as tests/test_cli_cpu.py runs adapter_test
    p = subprocess.run([os.path.join(ROOT, "tests", "cpp", "eigsel_adapter_test"), "compile-only"], stdout=subprocess.PIPE, timeout=60)
    assert p.returncode == 0 and b"adapter compiled" in p.stdout
