"""Fractional occupations by symmetry block, the parts that need no GPU: spherical_occupations against hand-written lists
and each of its refusals; the refusals of hfg_occupy_blocks_devptr that come before the context is touched (nblk < 1,
ncols < N, an occupation outside [0, 1]) -- the fourth, more occupations than a block has rows, needs the device's block ids
and is tested in tests/test_gpu_frac_occ.py; the launch rules of host/occ_plan.h against their limits for N = 1, 64, 65, 4230
and 6102 as a stand-alone program under the address and undefined-behaviour sanitizers (tests/cpp/occ_plan_check.cpp); and
that the existing step objects still leave forced occupations to the drivers."""
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
    import helfem_amd
    helfem_amd.lib()
    return helfem_amd


def atom(hf, Z, lmax, mmax, nelem=2, nnodes=4):
    lval, mval = hf.angular_basis(lmax, mmax)
    return hf.AtomicTwoDBasis(Z, nnodes, 5 * nnodes, hf.atomic_grid(nelem), lval, mval)


def by_lm(basis, occ):
    assert len(occ) == len(basis.lval) == len(basis.get_sym_idx(2))
    return {(l, m): o for l, m, o in zip(basis.lval, basis.mval, occ)}


def test_hydrogen(hf):
    b = atom(hf, 1, 0, 0)
    assert hf.spherical_occupations(b, {0: [1]}) == [[0.5]]


def test_carbon(hf):
    b = atom(hf, 6, 1, 1)
    got = by_lm(b, hf.spherical_occupations(b, {0: [2, 2], 1: [2]}))
    third = 2.0 / 6.0
    assert got == {(0, 0): [1.0, 1.0], (1, -1): [third], (1, 0): [third], (1, 1): [third]}


def test_neon(hf):
    b = atom(hf, 10, 1, 1)
    got = by_lm(b, hf.spherical_occupations(b, {0: [2, 2], 1: [6]}))
    assert got == {(0, 0): [1.0, 1.0], (1, -1): [1.0], (1, 0): [1.0], (1, 1): [1.0]}


def test_scandium_has_a_d_shell(hf):
    b = atom(hf, 21, 2, 2)
    got = by_lm(b, hf.spherical_occupations(b, {0: [2, 2, 2, 2], 1: [6, 6], 2: [1]}))
    want = {(0, 0): [1.0, 1.0, 1.0, 1.0]}
    for m in (-1, 0, 1):
        want[(1, m)] = [1.0, 1.0]
    for m in (-2, -1, 0, 1, 2):
        want[(2, m)] = [0.1]
    assert got == want
    assert abs(2 * sum(sum(o) for o in got.values()) - 21) < 1e-14


def test_an_l_without_electrons_gets_an_empty_list(hf):
    b = atom(hf, 2, 1, 1)
    got = by_lm(b, hf.spherical_occupations(b, {0: [2]}))
    assert got == {(0, 0): [1.0], (1, -1): [], (1, 0): [], (1, 1): []}


def test_refuses_an_l_beyond_the_basis(hf):
    with pytest.raises(ValueError, match="beyond the basis"):
        hf.spherical_occupations(atom(hf, 21, 1, 1), {0: [2], 2: [1]})


def test_refuses_an_incomplete_m_range(hf):
    b = atom(hf, 6, 1, 0)  # l = 1 with m = 0 only
    assert (1, 0) in zip(b.lval, b.mval) and (1, 1) not in zip(b.lval, b.mval)
    with pytest.raises(ValueError, match="lacks m = -1, 1 of l = 1"):
        hf.spherical_occupations(b, {0: [2, 2], 1: [2]})


def test_refuses_an_overfull_shell(hf):
    with pytest.raises(ValueError, match="7 electrons in a shell of l = 1"):
        hf.spherical_occupations(atom(hf, 10, 1, 1), {0: [2, 2], 1: [7]})
    with pytest.raises(ValueError, match="3 electrons in a shell of l = 0"):
        hf.spherical_occupations(atom(hf, 10, 1, 1), {0: [3]})


def test_refuses_a_diatomic_basis(hf):
    lval, mval = hf.lm_to_l_m([2])
    b = hf.TwoDBasis(1, 1, 0.7, 4, 20, hf.get_grid(4.0, 2, 4, 1.0), lval, mval)
    with pytest.raises(ValueError, match="diatomic"):
        hf.spherical_occupations(b, {0: [2]})


# ---- hfg_occupy_blocks_devptr: what is refused before the context is touched (a null context reaches it) ---------------
def occupy(hf, N, ncols, nblk, occ_ptr, occ):
    f = hf.lib().hfg_occupy_blocks_devptr
    f.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                  ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)] + [ctypes.c_void_p] * 3
    p = np.asarray(occ_ptr, dtype=np.int64)
    o = np.asarray(list(occ) + [0.0], dtype=np.float64)
    rc = f(None, N, ncols, None, None, None, nblk, p.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
           o.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None, None)
    return rc, hf.lib().hfg_last_error().decode()


@pytest.mark.parametrize("args,text", [
    ((8, 8, 0, [0], []), "nblk < 1"),
    ((8, 8, -3, [0], []), "nblk < 1"),
    ((8, 7, 2, [0, 1, 2], [1.0, 1.0]), "ncols < N"),
    ((8, 8, 2, [0, 1, 2], [1.0, 1.5]), "occupation 1 outside [0, 1]"),
    ((8, 8, 2, [0, 1, 2], [-1e-300, 1.0]), "occupation 0 outside [0, 1]"),
    ((8, 8, 2, [0, 1, 2], [1.0, float("nan")]), "occupation 1 outside [0, 1]"),
], ids=["nblk-0", "nblk-negative", "ncols-below-N", "above-1", "below-0", "nan"])
def test_host_side_refusals(hf, args, text):
    rc, msg = occupy(hf, *args)
    assert rc == 1 and text in msg, (rc, msg)


def test_valid_arguments_get_as_far_as_the_context(hf):
    """the same call with nothing wrong in the lists is refused for its null context, not for the lists"""
    rc, msg = occupy(hf, 8, 8, 2, [0, 1, 2], [0.0, 1.0])
    assert rc == 1 and "null context" in msg, (rc, msg)


# ---- launch rules -----------------------------------------------------------------------------------------------------
def test_launch_rules_stand_alone_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "occ_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "occ_plan_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0 and b"occ plan check ok" in p.stdout, p.stdout.decode()
    m = re.search(rb"(\d+) cases in the sweep", p.stdout)
    assert m and int(m.group(1)) >= 1100, p.stdout.decode()


def test_header_is_host_only():
    with open(os.path.join(ROOT, "helfem_amd", "csrc", "host", "occ_plan.h")) as fh:
        text = fh.read()
    assert "namespace helfem" in text and "hip" not in "".join(re.findall(r"#include.*", text))


# ---- what stays -------------------------------------------------------------------------------------------------------
def test_the_restricted_step_still_leaves_forced_occupations_to_the_drivers(hf):
    with pytest.raises(NotImplementedError, match="readocc"):
        hf._refuse_out_of_scope("DeviceSCFStep", False, False, 0, False, 1.0)
    assert issubclass(hf.DeviceFracSCFStep, hf.DeviceSCFStep)
    # step() and run() are the restricted step's own
    assert hf.DeviceFracSCFStep.run is hf.DeviceSCFStep.run and hf.DeviceFracSCFStep.step is hf.DeviceSCFStep.step
