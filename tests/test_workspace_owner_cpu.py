"""The workspace owner of the HIP side (helfem_amd/csrc/hip/workspace_owner.h) is host-only: a stand-alone program with
counting dummy workspaces checks it under ASan + UBSan and, with one owner per thread, under TSan.  Nothing of it is loaded
into Python.  And the structure it replaces stays gone: no map keyed by a context or a table set, no *_release function."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "helfem_amd", "csrc", "hip")


@pytest.mark.parametrize("sanitize", ["address,undefined", "thread"])
def test_owner_under_the_host_sanitizers(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "workspace_owner_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "workspace_owner_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0 and b"owner ok" in p.stdout, p.stdout.decode()


def test_owner_header_has_no_hip_in_it():
    with open(os.path.join(HIP, "workspace_owner.h")) as fh:
        text = fh.read()
    assert not re.search(r"#include\s*[<\"]hip/|\bhip[A-Z]\w*\(", text)
    with open(os.path.join(HIP, "common.h")) as fh:
        assert '#include "workspace_owner.h"' in fh.read()


def test_nothing_is_keyed_by_a_context_or_a_table_set():
    csrc = os.path.join(ROOT, "helfem_amd", "csrc")
    for d, _, files in os.walk(csrc):
        for f in files:
            with open(os.path.join(d, f)) as fh:
                text = fh.read()
            assert not re.search(r"std::map<\s*(hfg_ctx|hfg_dev_tables)\s*\*", text), f
            assert not re.search(r"\b(eig|dc|stsel|trd|trdp|fock|exchange|exchange_lr)_release\b", text), f
    with open(os.path.join(HIP, "internal.h")) as fh:
        assert "_release(" not in fh.read()
