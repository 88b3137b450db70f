"""The plan of tests/stream_order_worker.py (no GPU): every hfg_*_dev function that include/helfem_gpu.h declares is either
in the plan of the stream-ordering test, on every stream kind and under every setting, or in its documented exclusion list."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stream_order_worker as wk  # noqa: E402


def _plan_lines():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stream_order_worker.py"), "--plan"], cwd=ROOT, timeout=60,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()
    return [line.split("\t") for line in out.stdout.decode().splitlines()]


def test_every_dev_symbol_of_the_header_is_planned_or_excluded():
    header = open(os.path.join(ROOT, "include", "helfem_gpu.h")).read()
    declared = set(re.findall(r"\b(hfg_\w+_dev)\s*\(", header))
    assert len(declared) >= 17 and declared == set(wk.header_dev_symbols())
    lines = _plan_lines()
    excluded = {row[1] for row in lines if row[0] == "excluded"}
    cases = [tuple(row[1:]) for row in lines if row[0] == "case"]
    assert excluded == set(wk.EXCLUDED) and excluded <= declared
    assert not [c for c in cases if c[2].startswith("UNCOVERED")], "a device-pointer entry without a case in the worker"
    for setting, _ in wk.SETTINGS:
        for kind in wk.STREAM_KINDS:
            planned = {c[2] for c in cases if c[0] == setting and c[1] == kind and "@" not in c[2]}
            assert planned | excluded == declared, (setting, kind, sorted(declared - planned - excluded))
            assert not planned & excluded
    assert cases == [tuple(p) for p in wk.plan()]


def test_the_exclusions_are_documented_in_the_gpu_module():
    doc = open(os.path.join(ROOT, "tests", "test_gpu_stream_order.py")).read().split('"""')[1]
    for sym, why in wk.EXCLUDED.items():
        assert sym in doc and why
    # every excluded symbol takes no device pointer: no parameter whose name starts with d + capital (dP, dF, dBlockBuf ...)
    header = open(os.path.join(ROOT, "include", "helfem_gpu.h")).read()
    for sym in wk.EXCLUDED:
        args = re.search(r"^int\s+%s\s*\(([^;]*?)\)\s*;" % sym, header, re.S | re.M).group(1)
        assert not re.search(r"\*\s*d[A-Z]\w*", args), (sym, args)
    for sym in wk.entries():
        args = re.search(r"^int\s+%s\s*\(([^;]*?)\)\s*;" % sym, header, re.S | re.M).group(1)
        assert re.search(r"\*\s*d[A-Z]\w*", args), (sym, args)


def test_the_trd_chain_setting_adds_the_give_up_cases():
    extra = [(k, e) for s, k, e in wk.plan() if s == "trd_chain" and "@" in e]
    assert len(extra) == len(wk.STREAM_KINDS) * (1 + len(wk.AFTER_GIVEUP))
    assert min(wk.GIVEUP_SIZES) < 1024 <= max(wk.GIVEUP_SIZES)
    # the block of the protocol sits just above HELFEM_TRDP_MIN and 4 * BT_KB
    eig = open(os.path.join(ROOT, "helfem_amd", "csrc", "hip", "eig.hip")).read()
    kb = int(re.search(r"constexpr int BT_KB = (\d+);", eig).group(1))
    tun = open(os.path.join(ROOT, "helfem_amd", "csrc", "host", "tuning.h")).read()
    trdp_min = int(re.search(r"X\(trdp_min, int, (\d+),", tun).group(1))
    assert max(wk.EIG_SIZES) == max(trdp_min, 4 * kb) + 1
    trdp = open(os.path.join(ROOT, "helfem_amd", "csrc", "hip", "trdp.hip")).read()
    assert re.search(r"ns\[i\] >= 1024 &&", trdp), "the order from which a chained block makes the context give its side stream up"
