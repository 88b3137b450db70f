"""The HELFEM_* run-time switches have one home (helfem_amd/csrc/host/tuning.h): nothing else in the library reads the
environment, DESIGN.md's switch table lists exactly what the library reports, and the values follow the rules the table
states.  No GPU needed."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "helfem_amd", "csrc")
# read by the Python side where they are used; only listed in DESIGN.md
PYTHON_SIDE = {"HELFEM_AMD_LIB", "HELFEM_NO_TORCH", "HELFEM_FOCK_SHARD", "HELFEM_DIST_BACKEND", "HELFEM_DIST_FORCE", "HELFEM_HIPCC_FLAGS",
               "HELFEM_BENCH_DEVICE"}
# switches of the two-stage probe (tests/gpu_probe/two_stage.hip, driven by tools/sb_debug.py), not of the library
PROBE = {"HELFEM_SB_NPANEL", "HELFEM_SB_STEP"}

CHILD = """
import json, os, sys
import helfem_amd as hf
out = [{r["name"]: r["value"] for r in hf.tuning_table()}]
for step in json.loads(sys.argv[1]):
    for k, v in step.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    out.append({r["name"]: r["value"] for r in hf.tuning_table()})
print("TABLES" + json.dumps(out))
"""


def tables(env, steps=()):
    """the switch values a fresh process with these HELFEM_* variables reports: at start, and after each of the steps
    (dicts of variables it sets, None = unsets, in its own environment)"""
    e = {k: v for k, v in os.environ.items() if not k.startswith("HELFEM_")}
    e.update(env)
    e["HELFEM_NO_TORCH"] = "1"
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-c", CHILD, json.dumps(list(steps))], env=e, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    return json.loads(p.stdout.decode().split("TABLES")[1])


def value(name, text):
    """reported value of switch `name` in a process started with name=text (None: unset)"""
    return tables({} if text is None else {name: text})[0][name]


@pytest.fixture(scope="module", autouse=True)
def hf(native_libs):
    import helfem_amd
    helfem_amd.lib()
    return helfem_amd


def test_only_the_table_reads_the_environment():
    hits = []
    for d, _, files in os.walk(CSRC):
        for f in files:
            path = os.path.join(d, f)
            if os.path.relpath(path, CSRC) == os.path.join("host", "tuning.cpp"):
                continue
            with open(path, errors="ignore") as fh:
                hits += ["%s:%d" % (os.path.relpath(path, ROOT), i + 1) for i, line in enumerate(fh) if "getenv(" in line]
    assert hits == []


def test_design_table_lists_what_the_library_reports(hf):
    rows = hf.tuning_table()
    assert all(set(r) == {"name", "kind", "default", "value", "read", "meaning"} for r in rows)
    reported = {r["name"] for r in rows}
    assert len(reported) == len(rows) and all(n.startswith("HELFEM_") for n in reported)
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        text = fh.read()
    section = text[text.index("## 6a. Run-time switches"):text.index("## 7. Out of scope")]
    documented = set(re.findall(r"^\| `(HELFEM_[A-Z0-9_]+)` \|", section, flags=re.M))
    assert documented == reported | PYTHON_SIDE
    # the documented default is the library's
    for r in rows:
        shown = "`%s`" % r["default"] if r["default"] else "unset"
        assert re.search(r"^\| `%s` \| %s \| %s \| %s \|" % (r["name"], re.escape(r["kind"]), re.escape(shown), r["read"]), section, flags=re.M), r["name"]
    used = set()
    files = [os.path.join(ROOT, "bench.py")] + [os.path.join(ROOT, "helfem_amd", f) for f in os.listdir(os.path.join(ROOT, "helfem_amd")) if f.endswith(".py")]
    for top in ("tests", "tools"):
        for d, _, fs in os.walk(os.path.join(ROOT, top)):
            files += [os.path.join(d, f) for f in fs if f.endswith((".py", ".hip", ".cpp", ".h", ".hpp", ".sh"))]
    for path in files:
        with open(path, errors="ignore") as fh:
            used |= set(re.findall(r"HELFEM_[A-Z0-9_]*[A-Z0-9]", fh.read()))
    assert used - (reported | PYTHON_SIDE | PROBE) == set()


def test_defaults():
    t = tables({})[0]
    assert t["HELFEM_TRD"] == "persistent" and t["HELFEM_BT_FOLD"] == "on" and t["HELFEM_BT_SIDE"] == "off"
    assert t["HELFEM_EXL_GROUPS"] == "4" and t["HELFEM_TRDP_STEP"] == "96" and t["HELFEM_TRD_TAIL"] == "2" and t["HELFEM_DC_DBG"] == "off"
    assert t["HELFEM_XC_LDS_LIMIT"] == str(150 * 1024) and t["HELFEM_TRDP_LIMIT_MS"] == "200" and t["HELFEM_TRDP_MIN"] == "256"
    assert t["HELFEM_TRDF_SYM"] == "-1" and t["HELFEM_GEMM_SPLITK"] == "-1" and t["HELFEM_EXL_RECT"] == "-1" and t["HELFEM_EXL_RB"] == "0"
    assert t["HELFEM_SCF"] == "off" and t["HELFEM_EXCHANGE"] == "off" and t["HELFEM_MFMA"] == "off" and t["HELFEM_TRDP_STAMPS_FILE"] == ""
    on_by_default = ["BT_FOLD", "TRDP_PHASES", "TRDP_COOP", "EXL_SPLITK", "EXL_CRECT", "EXL_PAIR", "EXL_HINT", "EXL_MGROUPS", "EXL_WL", "FOCK_OVERLAP",
                     "EIG_PAIR", "DIIS_BLOCKS", "DIIS_LOWRANK", "TRD_BAND_UPDATE"]
    assert [t["HELFEM_" + n] for n in on_by_default] == ["on"] * len(on_by_default)


@pytest.mark.parametrize("text,mode", [("chain", "chain"), ("twokernel", "twokernel"), ("unblocked", "unblocked"), ("persistent", "persistent"),
                                       ("graph", "chain"), ("", "chain")])
def test_trd_mode(text, mode):
    assert value("HELFEM_TRD", text) == mode  # any other text behaves as the chain


@pytest.mark.parametrize("name,text,shown", [
    ("HELFEM_BT_FOLD", "0", "off"), ("HELFEM_BT_FOLD", "1", "on"), ("HELFEM_BT_FOLD", "x", "off"), ("HELFEM_BT_FOLD", "", "off"), ("HELFEM_BT_FOLD", "7", "on"),
    ("HELFEM_BT_SIDE", "1", "on"), ("HELFEM_BT_SIDE", "2", "off"),
    ("HELFEM_GEMM_RECT", "2", "on"), ("HELFEM_GEMM_RECT", "0", "off"),
    ("HELFEM_EXL_GROUPS", "0", "1"), ("HELFEM_EXL_GROUPS", "99", "16"), ("HELFEM_EXL_GROUPS", "3", "3"),
    ("HELFEM_TRDP_STEP", "0", "1"), ("HELFEM_TRDP_STEP", "40", "40"),
    ("HELFEM_TRD_TAIL", "0", "0"), ("HELFEM_TRD_TAIL", "1", "1"), ("HELFEM_TRD_TAIL", "2", "2"), ("HELFEM_TRD_TAIL", "7", "7"),
    ("HELFEM_DC_DBG", "", "on"), ("HELFEM_DC_DBG", "0", "on"),
    ("HELFEM_TRIDIAG", "ql", "on"), ("HELFEM_TRIDIAG", "QL", "off"), ("HELFEM_MFMA", "4x4x4", "on"), ("HELFEM_MFMA", "16x16x4", "off"),
    ("HELFEM_EXL_RB", "4", "4"), ("HELFEM_XC_LDS_LIMIT", "4096", "4096"), ("HELFEM_TRDP_LIMIT_MS", "5000000000", "5000000000"),
    ("HELFEM_NUM_THREADS", "-3", "0"), ("HELFEM_NUM_THREADS", "5", "5"), ("HELFEM_TRDP_STAMPS_FILE", "/tmp/stamps.txt", "/tmp/stamps.txt"),
])
def test_value_rules(name, text, shown):
    assert value(name, text) == shown


def test_live_switches_follow_the_environment_and_the_snapshot_does_not():
    before, after, back = tables({"HELFEM_GEMM_TILE": "64"}, steps=[
        {"HELFEM_SCF": "host", "HELFEM_EXCHANGE": "general", "HELFEM_NUM_THREADS": "3", "HELFEM_GEMM_TILE": "128", "HELFEM_TRD": "chain", "HELFEM_BT_FOLD": "0"},
        {"HELFEM_SCF": None, "HELFEM_EXCHANGE": "low-rank", "HELFEM_GEMM_TILE": None}])
    assert (before["HELFEM_SCF"], before["HELFEM_EXCHANGE"], before["HELFEM_NUM_THREADS"]) == ("off", "off", "0")
    assert (after["HELFEM_SCF"], after["HELFEM_EXCHANGE"], after["HELFEM_NUM_THREADS"]) == ("on", "on", "3")
    assert (back["HELFEM_SCF"], back["HELFEM_EXCHANGE"], back["HELFEM_NUM_THREADS"]) == ("off", "off", "3")
    for t in (before, after, back):
        assert (t["HELFEM_GEMM_TILE"], t["HELFEM_TRD"], t["HELFEM_BT_FOLD"]) == ("64", "persistent", "on")
