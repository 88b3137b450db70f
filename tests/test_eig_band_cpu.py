"""The banded F X of the blocked eigensolve, host side: the planner (helfem_amd/csrc/host/eig_band_plan.h) against brute
force -- through the library and as a stand-alone program under the address and undefined-behaviour sanitizers -- the C ABI
entries, their refusals, and the switch in the one table.  No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K0_ALIGN, KSTEP, TILE = 4, 16, 64  # what the tile engine needs: a step starts at a group of four columns of one MFMA, 16 columns long


@pytest.fixture(scope="module")
def hf(native_libs):
    os.environ.setdefault("HELFEM_NO_TORCH", "1")
    import helfem_amd
    helfem_amd.lib()
    return helfem_amd


def block_nodes(E, p, shells, skip=0):
    """radial nodes of one symmetry block in the callers' order: shell-major, the first node missing in `skip` shells, the
    boundary function at the far end not in the basis"""
    R = E * (p - 1)
    return [n for s in range(shells) for n in range(1 if s < skip else 0, R)]


def share(n, m, pm, E):
    return any(e * pm <= n <= e * pm + pm and e * pm <= m <= e * pm + pm for e in range(E))


BASES = [(3, 8, 7, 0), (3, 8, 7, 3), (5, 15, 3, 0), (5, 15, 3, 1), (5, 8, 5, 0), (4, 9, 13, 5)]  # orders 147 144 210 209 175 411


@pytest.mark.parametrize("E,p,shells,skip", BASES)
def test_planner_against_brute_force(hf, E, p, shells, skip):
    pm = p - 1
    node = np.array(block_nodes(E, p, shells, skip))
    n = len(node)
    perm, steps, banded = hf.eig_band_plan(node, pm, E)
    assert sorted(perm.tolist()) == list(range(n))
    key = list(zip(node[perm].tolist(), perm.tolist()))
    assert key == sorted(key)  # rows radial-major: node first, then the position in the caller's list
    assert banded and len(steps) == (n + TILE - 1) // TILE >= 2
    for t, ks in enumerate(steps):
        ks = ks.tolist()
        # aligned, inside [0, n), ascending without overlap: every column keeps its place in the dense summation
        assert ks and all(0 <= k < n and k % K0_ALIGN == 0 for k in ks) and all(b - a >= KSTEP for a, b in zip(ks, ks[1:]))
        covered = np.zeros(n, dtype=bool)
        for k in ks:
            covered[k:k + KSTEP] = True
        lo = TILE * t
        for i in perm[lo:lo + TILE]:  # the tile's rows; the columns are in the caller's order
            need = np.array([share(int(node[i]), int(m), pm, E) for m in node])
            assert np.all(covered[need]), (t, int(i))
    # the steps leave work out: that is the point
    assert sum(len(ks) for ks in steps) <= 0.9 * len(steps) * ((n + KSTEP - 1) // KSTEP)


def test_benchmark_block_takes_about_a_third_of_the_steps(hf):
    node = np.array(block_nodes(5, 15, 21, 7))  # a 21-shell block of the flagship basis
    n = len(node)
    _, steps, banded = hf.eig_band_plan(node, 14, 5)
    assert banded and sum(len(ks) for ks in steps) < 0.4 * len(steps) * ((n + KSTEP - 1) // KSTEP)
    assert max(len(ks) for ks in steps) <= 3 * 21 and min(len(ks) for ks in steps) >= 21  # one to three steps per shell


@pytest.mark.parametrize("E,p,shells", [(2, 4, 1), (3, 8, 3), (1, 15, 9), (4, 5, 13)])
def test_dense_blocks(hf, E, p, shells):
    """a single row tile (orders 6 and 63), one element that everything shares, elements finer than a k step: all steps"""
    node = block_nodes(E, p, shells)
    n = len(node)
    _, steps, banded = hf.eig_band_plan(node, p - 1, E)
    assert not banded and all(ks.tolist() == list(range(0, n, KSTEP)) for ks in steps)


def test_planner_stand_alone_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "eig_band_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "eig_band_plan_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert p.returncode == 0 and b"band plan check ok" in p.stdout, p.stdout.decode()


def test_header_declares_the_entries():
    with open(os.path.join(ROOT, "include", "helfem_gpu.h")) as fh:
        text = fh.read()
    assert re.search(r"^int hfg_ctx_declare_fock_band\(hfg_ctx \*ctx, hfg_basis \*basis, const double \*dH0, const int \*dBlockId, int \*state\);", text, flags=re.M)
    assert re.search(r"^int hfg_ctx_declare_band\(hfg_ctx \*ctx, int64_t N, const int \*node, int pm, int E, const double \*dH0, const int \*dBlockId, int \*state\);",
                     text, flags=re.M)
    assert re.search(r"^int hfg_ctx_fock_band_state\(hfg_ctx \*ctx, int \*state\);", text, flags=re.M)
    assert re.search(r"^int hfg_eig_band_plan\(int64_t n, const int \*node, int pm, int E, int64_t \*perm, int \*toff, int \*kstart, int64_t cap, int \*banded\);",
                     text, flags=re.M)


def test_refusals_without_a_device(hf):
    L = hf.lib()
    one = (ctypes.c_int * 1)(0)
    big = (ctypes.c_int64 * 1)(0)
    f = L.hfg_eig_band_plan
    f.argtypes = [ctypes.c_int64, hf.c_int_p, ctypes.c_int, ctypes.c_int, hf.c_i64_p, hf.c_int_p, hf.c_int_p, ctypes.c_int64, hf.c_int_p]
    two = (ctypes.c_int * 2)(0, 0)
    assert f(0, one, 7, 3, big, two, one, 1, one) == 1 and b"empty block" in L.hfg_last_error()
    assert f(1, None, 7, 3, big, two, one, 1, one) == 1 and b"null pointer" in L.hfg_last_error()
    bad = (ctypes.c_int * 1)(22)  # 3 elements of 7: nodes 0 ... 21
    assert f(1, bad, 7, 3, big, two, one, 1, one) == 1 and b"outside the elements" in L.hfg_last_error()
    assert f(1, one, 7, 3, big, two, one, 0, one) == 1 and b"capacity" in L.hfg_last_error()
    g = L.hfg_ctx_declare_fock_band
    g.argtypes = [ctypes.c_void_p] * 4 + [hf.c_int_p]
    assert g(None, None, None, None, one) == 1 and b"null context or basis" in L.hfg_last_error()


def test_switch_is_in_the_table(hf, monkeypatch):
    monkeypatch.delenv("HELFEM_EIG_BAND", raising=False)
    r = {r["name"]: r for r in hf.tuning_table()}["HELFEM_EIG_BAND"]
    assert r["default"] == "on" and r["value"] == "on" and r["read"] == "live" and r["kind"] == "off if 0"
    monkeypatch.setenv("HELFEM_EIG_BAND", "0")
    assert {r["name"]: r["value"] for r in hf.tuning_table()}["HELFEM_EIG_BAND"] == "off"
