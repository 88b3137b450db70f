"""The host-side rules of the Fock build (helfem_amd/csrc/host/fock_plan.h): every rule against the expressions the launchers
held before, over a sweep and on both sides of each threshold, as a stand-alone program under the address and
undefined-behaviour sanitizers (tests/cpp/fock_plan_check.cpp), and that the launchers of hip/fock.hip ask the header and
keep no copy of a rule, raise the LDS attribute in one place, drive J beside XC in one function and share the device pieces
of the two grid kernels.  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fock():
    with open(os.path.join(ROOT, "helfem_amd", "csrc", "hip", "fock.hip")) as fh:
        return fh.read()


def test_rules_stand_alone_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "fock_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "fock_plan_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0 and b"fock plan check ok" in p.stdout, p.stdout.decode()
    m = re.search(rb"(\d+) cases in the sweep", p.stdout)
    assert m and int(m.group(1)) >= 78400, p.stdout.decode()  # the theta plan alone: 140 nth x 70 groups x 4 limits x lapl


def test_header_is_host_only():
    with open(os.path.join(ROOT, "helfem_amd", "csrc", "host", "fock_plan.h")) as fh:
        text = fh.read()
    assert "namespace helfem" in text and "hip" not in "".join(re.findall(r"#include.*", text)) and "tables.h" not in text


def test_launchers_ask_the_header_and_keep_no_copy():
    src = _fock()
    host = src[src.index("// launchers"):]
    assert '#include "../host/fock_plan.h"' in src
    assert len(re.findall(r"hipFuncAttributeMaxDynamicSharedMemorySize", host)) == 1
    assert len(re.findall(r"tuning\(\)\.xc_lds_limit", host)) <= 2  # the restricted and the polarised plan
    assert len(re.findall(r"tuning\(\)\.fock_overlap", host)) == 1
    for literal in (r"64 \* 1024", r"150 \* 1024", r"160 \* 1024"):
        assert not re.search(literal, host), literal
    assert "round_up64" not in host and "CB_MAX_NT = " not in src and "XC_FT_MAXPP = " not in src
    for fn in ("fock_block_threads", "coulomb_radial_lds", "xc_density_radial_lds", "xc_density_theta_lds", "xc_fock_radial_lds",
               "xc_fock_theta_plan", "xc_grid_lds", "xc_grid_pol_plan", "coulomb_batch_chunk", "coulomb_batch_tile_bytes",
               "coulomb_batch_tei", "fock_lds_raise"):
        assert re.search(r"\b%s\(" % fn, host), fn
    # the theta launcher takes the plan and the skip flags: no trailing defaults to count
    m = re.search(r"static void launch_xc_fock_theta\(([^)]*)\)", host)
    assert m and "=" not in m.group(1) and "XCPlan" in m.group(1) and "FockSkip" in m.group(1)
    # the model potential goes through the Fock stage of the XC builds
    mp = host[host.index("void model_potential_dev("):host.index("size_t fock_compact_size(")]
    assert "xc_fock_stage(" in mp and "hipLaunchKernelGGL(k_xc_fock_radial" not in mp and "launch_xc_fock_theta" not in mp
    assert len(re.findall(r"h_grp_off\[g \+ 1\]", host)) == 1  # the largest m group is found in one place


def _function_bodies(text):
    """(name, body) of every function definition at namespace level: a line that does not start with a blank and ends in '{',
    up to the next line that is '}' alone"""
    out = []
    for m in re.finditer(r"^(?![ }/#])[^\n;]*?(\w+)\([^;{]*\)\s*\{\n(.*?)^\}", text, flags=re.M | re.S):
        out.append((m.group(1), m.group(2)))
    return out


def test_one_driver_for_j_beside_xc():
    src = _fock()
    host = src[src.index("// launchers"):]
    owners = [name for name, body in _function_bodies(host) if "hipEventRecord(ctx->side_ev" in body]
    assert owners == ["fock_j_beside_xc"], owners
    assert len(re.findall(r"hipEventRecord\(ctx->side_ev", host)) == 2  # the two events, both there
    driver = dict(_function_bodies(host))["fock_j_beside_xc"]
    assert "try" in driver and driver.count("try") == 1 and "~OnStream()" in driver  # the stream comes back through a guard
    assert re.search(r"catch \(\.\.\.\) \{[^}]*hipStreamWaitEvent\(main, ctx->side_ev\[1\], 0\);\s*throw;", driver)
    for fn in ("fock_compact_dev", "fock_compact_pol_dev"):
        body = dict(_function_bodies(host))[fn]
        assert "fock_j_beside_xc(" in body and "ctx->stream = " not in body and "side_ev" not in body, fn


def test_grid_kernels_share_their_device_pieces():
    src = _fock()
    kernels = src[:src.index("// launchers")]
    grid = kernels[kernels.index("__global__ void k_xc_grid("):kernels.index("__global__ void k_xc_grid_pol(")]
    pol = kernels[kernels.index("__global__ void k_xc_grid_pol("):kernels.index("xc_fock_theta_zero(")]
    for helper in ("xc_scale_factors_weight", "xc_reduce_partials", "xc_phi_transform"):
        assert re.search(r"__device__ __forceinline__ void %s\(" % helper, kernels), helper
        assert len(re.findall(r"\b%s\(" % helper, grid)) == 1 and len(re.findall(r"\b%s\(" % helper, pol)) == 1, helper
    # the scale factors without the weight: inside the phi transform, which both kernels call
    assert re.search(r"__device__ __forceinline__ void xc_scale_factors\(", kernels)
    for body in (grid, pol):
        assert "__shfl_down" not in body and "sqrt(" not in body
    assert kernels.count("template <bool EXT>") == 2  # two kernels, flags stay arguments
