"""The choices of the low-rank exchange build, host side (helfem_amd/csrc/host/exl_plan.h): every rule on both sides of its
threshold and under every value of its switches as a stand-alone program under the address and undefined-behaviour
sanitizers (tests/cpp/exl_plan_check.cpp), the C ABI entry that returns the record of a build, its refusals, and that both
builds of hip/exchange_lr.hip ask the header and keep no copy of a rule.  No GPU needed."""
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
    helfem_amd.lib()
    return helfem_amd


def test_rules_stand_alone_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "exl_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "exl_plan_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert p.returncode == 0 and b"exl plan check ok" in p.stdout, p.stdout.decode()


def test_header_declares_the_entry():
    with open(os.path.join(ROOT, "include", "helfem_gpu.h")) as fh:
        text = fh.read()
    assert re.search(r"^int hfg_exl_last_plan\(hfg_basis \*basis, const char \*which, char \*buf, size_t cap\);", text, flags=re.M)
    with open(os.path.join(ROOT, "helfem_amd", "csrc", "hip", "internal.h")) as fh:
        assert len(re.findall(r"\bexl_last_plan_json\(", fh.read())) == 1  # declared once


def test_refusals_and_an_empty_record_without_a_device(hf):
    L = hf.lib()
    assert L.hfg_exl_last_plan.argtypes == [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    buf = ctypes.create_string_buffer(256)
    assert L.hfg_exl_last_plan(None, b"coulomb", buf, 256) == 1 and b"null basis" in L.hfg_last_error()
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import common
    gb, _ = common.make_bases(1, 1, 1.4, (1,), 1, 4, oracle=False)
    assert L.hfg_exl_last_plan(gb.h, b"other", buf, 256) == 1 and b"coulomb, screened or mix" in L.hfg_last_error()
    assert L.hfg_exl_last_plan(gb.h, b"coulomb", buf, 8) == 1 and b"buffer too small" in L.hfg_last_error()
    for which in ("coulomb", "screened", "mix"):  # nothing uploaded, nothing built: null records, no error
        assert gb.exchange_last_plan(which) == {"single": None, "batch": None}
    assert callable(hf.AtomicTwoDBasis.exchange_last_plan)


def test_both_builds_ask_the_header_and_keep_no_copy():
    with open(os.path.join(ROOT, "helfem_amd", "csrc", "hip", "exchange_lr.hip")) as fh:
        src = fh.read()
    host = src[src.index("struct ExLRAux"):]  # the launchers; the kernels above them read no switch
    # the switches of the rules are read in one place, exl_switches(), and the thresholds stand in the header alone
    for field in ("exl_rb", "exl_mgroups", "exl_rect", "exl_wl", "exl_splitk", "exl_crect"):
        assert len(re.findall(r"tuning\(\)\.%s\b" % field, src)) == 1, field
    for literal in (r"\b1500\.0\b", r"\b2048\b", r">= 512\b", r"150 \* 1024", r"> 256\b"):
        assert not re.search(literal, host), literal
    for fn in ("exl_cross", "exl_elem", "exl_grouped", "exl_alpha_lds"):
        assert len(re.findall(r"helfem::%s\(" % fn, host)) == 2, fn  # the single build and the batched one
    assert len(re.findall(r"helfem::exl_batch_takes\(", host)) == 1 and len(re.findall(r"helfem::exl_rb_kernel\(", host)) == 1
