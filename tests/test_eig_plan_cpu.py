"""The rules of the blocked eigensolve's products, host side (helfem_amd/csrc/host/eig_plan.h): every rule on both sides of
its threshold, the benchmark's shapes and the equivalence with the expressions the driver used to carry, as a stand-alone
program under the address and undefined-behaviour sanitizers (tests/cpp/eig_plan_check.cpp); and that hip/eig.hip and
hip/gemm.hip ask the header and keep no copy of a rule, with the driver cut into stages.  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "helfem_amd", "csrc")
STAGES = ("block_supports", "band_lists", "block_lists", "fill_chunk", "build_tasks", "build_row_tasks", "reduce_stage", "publish_direct",
          "publish_slots", "last_product", "wait_status", "eig_blocks_multi_dev", "eig_assemble_sel_dev", "eig_gsym_sub_multi_dev")


def read(*rel):
    with open(os.path.join(CSRC, *rel)) as fh:
        return fh.read()


def test_rules_stand_alone_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "eig_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "eig_plan_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0 and b"eig plan check ok" in p.stdout, p.stdout.decode()


def test_the_driver_asks_the_header_and_keeps_no_copy():
    eig, gemm, header, internal = read("hip", "eig.hip"), read("hip", "gemm.hip"), read("host", "eig_plan.h"), read("hip", "internal.h")
    # the switches of the rules are read in one place of eig.hip, the thresholds stand in the header alone
    for field in ("gemm_tile", "gemm_splitk", "gemm_rect", "mfma_4x4x4"):
        assert len(re.findall(r"tuning\(\)\.%s\b" % field, eig)) == 1, field
    assert len(re.findall(r"tuning\(\)\.gemm_tile\b", gemm)) == 1
    for literal in (r"\b0\.85\b", r"nm >= 256\b"):
        assert len(re.findall(literal, header)) >= 1, literal
        assert not re.search(literal, eig) and not re.search(literal, gemm), literal
    assert not re.search(r">= 256\b", eig)
    for fn in ("eig_product_plan", "eig_last_product"):
        assert len(re.findall(r"helfem::%s\(" % fn, eig)) == 1, fn
    assert len(re.findall(r"helfem::eig_value_offsets\(", eig)) == 2 and len(re.findall(r"helfem::eig_block_nmax\(", eig)) == 3
    assert len(re.findall(r"helfem::gemm_prefers_128\(", gemm)) == 1 and "gemm_prefers_128" not in eig
    # the types of the launcher live in the host header, which internal.h includes
    assert re.search(r"^enum class GemmTile \{", header, flags=re.M) and re.search(r"^struct GemmHow \{", header, flags=re.M)
    assert "enum class GemmTile" not in internal and "struct GemmHow" not in internal and '#include "../host/eig_plan.h"' in internal
    assert set(re.findall(r'^#include ["<]([^">]+)[">]', header, flags=re.M)) == {"algorithm", "cstddef", "cstdint"}  # host only
    # one slot count per process, one launch site of the support kernel, one builder of the copy lists
    for text in (eig, gemm, internal, read("hip", "common.h")):
        assert "eig_num_cus" not in text
    assert len(re.findall(r"hipDeviceAttributeMultiprocessorCount", gemm)) == 1 and "multiProcessorCount" not in eig
    assert len(re.findall(r"hipLaunchKernelGGL\(k_col_support\b", eig)) == 1
    assert len(re.findall(r"hipLaunchKernelGGL\(k_copy_slices\b", eig)) == 1 and len(re.findall(r"\bpublish_values\(", eig)) == 4
    assert "catch (...)" not in eig[eig.index("static void eig_gsym_sub_multi_dev("):]  # the shard comes back through the guard


def test_no_stage_of_the_blocked_driver_is_long():
    eig = read("hip", "eig.hip")
    lengths = {}
    for name in STAGES:
        starts = [m.start() for m in re.finditer(r"^static [^\n;]*\b%s\(" % name, eig, flags=re.M)]
        assert len(starts) == 1, name  # defined once, no forward declaration
        body = eig[starts[0]:]
        lengths[name] = body[:body.index("\n}\n")].count("\n") + 2
    assert max(lengths.values()) <= 80, lengths
    assert lengths["eig_blocks_multi_dev"] > 30  # (the scan found the driver itself, not a stub)
