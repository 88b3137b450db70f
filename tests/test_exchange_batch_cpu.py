"""The batched exchange build's host side: the C ABI declares the entries with their argument lists, the device-pointer ones
stay out of the hfg_*_dev plan of tests/stream_order_worker.py, the argument refusals need no device, the chunk planner
splits hand-made rank lists as documented (through the library, and as a stand-alone program under the address and
undefined-behaviour sanitizers), and both switches are in the one table.  No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = ("hfg_exchange_batch", "hfg_rs_exchange_batch")
DEVPTR = ("hfg_exchange_batch_devptr", "hfg_rs_exchange_batch_devptr")


@pytest.fixture(scope="module")
def hf(native_libs):
    os.environ.setdefault("HELFEM_NO_TORCH", "1")
    import helfem_amd
    helfem_amd.lib()
    return helfem_amd


def _header():
    with open(os.path.join(ROOT, "include", "helfem_gpu.h")) as fh:
        return fh.read()


def test_header_declares_the_entries():
    text = _header()
    args = r"\(hfg_ctx \*ctx, hfg_basis \*basis, int64_t nP, const double \*%s, double \*%s\);"
    for name in HOST:
        assert re.search(r"^int %s" % name + args % ("P", "K"), text, flags=re.M), name
    for name in DEVPTR:
        assert re.search(r"^int %s" % name + args % ("dP", "dK"), text, flags=re.M), name
    assert re.search(r"^int hfg_exchange_occ_batch_devptr\(hfg_ctx \*ctx, hfg_basis \*basis, int64_t nP, const double \*dP, const double \*dC,\s+"
                     r"const int64_t \*nocc, int64_t ldc_cols, double \*dK\);", text, flags=re.M)
    assert re.search(r"^int hfg_exchange_batch_plan\(int64_t nP, const int \*ranks, int max_members, int \*chunk_of, int \*nchunks\);", text, flags=re.M)
    dev = re.findall(r"^\s*(?:int|int64_t)\s+(hfg_\w+_dev)\s*\(", text, flags=re.M)
    assert "hfg_exchange_dev" in dev and not [n for n in dev if "batch" in n]


def test_symbols_and_argtypes(hf):
    L = hf.lib()
    five = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, hf.c_double_p, hf.c_double_p]
    for name in HOST:
        assert getattr(L, name).argtypes == five, name
    for name in DEVPTR:
        assert getattr(L, name).argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p], name
    assert L.hfg_exchange_occ_batch_devptr.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                        hf.c_i64_p, ctypes.c_int64, ctypes.c_void_p]
    for cls in (hf.TwoDBasis, hf.AtomicTwoDBasis):
        assert callable(cls.exchange_batch) and callable(cls.exchange_batch_torch)
    assert callable(hf.AtomicTwoDBasis.rs_exchange_batch)


@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("have_C", [False, True])
@pytest.mark.parametrize("kfrac,kshort", [(0.25, 0.0), (0.19, 0.46), (0.0, 1.0)], ids=["coulomb", "both", "screened"])
@pytest.mark.parametrize("mix", [False, True])
def test_exchange_route(hf, mix, kfrac, kshort, have_C, batch):
    """the step objects' exchange router over its whole contract: which entries one exchange build calls, in which order and
    into which matrix, for the mixed table set or not, each case of the two weights, with and without the occupied orbitals,
    for one density and for the batch of HELFEM_USCF_KBATCH.  The table is written out here, not derived."""
    if mix:  # one build returns the weighted sum, whatever the weights; the batched entry also serves without orbitals
        want = [({(False, False): "hfg_mix_exchange_devptr", (True, False): "hfg_mix_exchange_occ_devptr",
                  (False, True): "hfg_mix_exchange_occ_batch_devptr", (True, True): "hfg_mix_exchange_occ_batch_devptr"}[have_C, batch], "K")]
    else:
        coulomb = {(False, False): "hfg_exchange_dev", (True, False): "hfg_exchange_occ_dev",
                   (False, True): "hfg_exchange_batch_devptr", (True, True): "hfg_exchange_occ_batch_devptr"}[have_C, batch]
        screened = "hfg_rs_exchange_batch_devptr" if batch else "hfg_rs_exchange_dev"  # never takes the orbitals
        want = {"coulomb": [(coulomb, "K")], "both": [(coulomb, "K"), (screened, "Krs")], "screened": [(screened, "Krs")]}[
            "coulomb" if kshort == 0.0 else "both" if kfrac != 0.0 else "screened"]
    got = hf._exchange_route(mix, kfrac, kshort, have_C, batch)
    assert [tuple(r) for r in got] == want
    L = hf.lib()
    for name, _ in got:  # every entry is exported and declared once, by lib()
        assert getattr(L, name).argtypes is not None, name


def test_refusals_without_a_device(hf):
    L = hf.lib()
    one = (ctypes.c_double * 1)()
    for name in HOST + DEVPTR:
        f = getattr(L, name)
        assert f(None, None, -1, None, None) == 1 and b"negative number of densities" in L.hfg_last_error(), name
        assert f(None, None, 2, None, None) == 1 and b"null context or basis" in L.hfg_last_error(), name
    assert L.hfg_exchange_batch(None, None, 3, one, one) == 1 and b"null context or basis" in L.hfg_last_error()
    n = (ctypes.c_int64 * 2)(1, 1)
    f = L.hfg_exchange_occ_batch_devptr
    assert f(None, None, -1, None, None, n, 1, None) == 1 and b"negative number of densities" in L.hfg_last_error()
    assert f(None, None, 2, None, None, n, 1, None) == 1 and b"null context or basis" in L.hfg_last_error()


def test_planner_on_hand_made_rank_lists(hf, monkeypatch):
    monkeypatch.delenv("HELFEM_EXCHANGE_BATCH_CHUNK", raising=False)
    plan = hf.exchange_batch_plan
    assert plan([21, 21, 30]) == ([0, 0, 1], 2)  # 42 + 30 > 64: splits after the second density
    assert plan([32, 0, 32, 1]) == ([0, -1, 0, 1], 2)  # a rank of 0 takes no columns and belongs to no chunk
    assert plan([5, 70, 5, 5]) == ([0, 1, 2, 2], 3)  # a rank above 64 is routed alone
    assert plan([5, -1, 5]) == ([0, 1, 2], 3)  # so is a density that one group of factors does not reproduce
    assert plan([2, 5, 1], max_members=1) == ([0, 1, 2], 3)
    assert plan([]) == ([], 0)
    monkeypatch.setenv("HELFEM_EXCHANGE_BATCH_CHUNK", "1")  # a live switch
    assert {r["name"]: r["value"] for r in hf.tuning_table()}["HELFEM_EXCHANGE_BATCH_CHUNK"] == "1"
    assert plan([2, 5, 1]) == ([0, 1, 2], 3)  # singletons
    assert plan([2, 5, 1], max_members=2) == ([0, 0, 1], 2)  # an explicit limit wins
    monkeypatch.delenv("HELFEM_EXCHANGE_BATCH_CHUNK")
    rng = __import__("numpy").random.RandomState(3)
    for _ in range(50):  # no chunk exceeds 64 columns
        ranks = rng.randint(0, 80, size=rng.randint(1, 40)).tolist()
        chunk_of, n = plan(ranks)
        cols = [0] * n
        for r, c in zip(ranks, chunk_of):
            assert (c == -1) == (r == 0)
            if 0 < r <= 64:
                cols[c] += r
        assert max(cols + [0]) <= 64 and sorted(set(c for c in chunk_of if c >= 0)) == list(range(n))
        assert [c for c in chunk_of if c >= 0] == sorted(c for c in chunk_of if c >= 0)  # runs of consecutive densities
    L = hf.lib()
    assert L.hfg_exchange_batch_plan(-1, None, 0, None, None) == 1 and b"negative" in L.hfg_last_error()
    assert L.hfg_exchange_batch_plan(2, None, 0, None, None) == 1 and b"null" in L.hfg_last_error()


def test_planner_stand_alone_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "exchange_batch_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "exchange_batch_plan_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert p.returncode == 0 and b"plan check ok" in p.stdout, p.stdout.decode()


def test_adapter_overloads_compile_against_the_stand_in_matrix_class():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-fsyntax-only", os.path.join(ROOT, "tests", "cpp", "exchange_batch_adapter_check.cpp")])
    # the existing batched Coulomb overload goes through the same helper now: its own test file still compiles
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-fsyntax-only", os.path.join(ROOT, "tests", "cpp", "coulomb_batch_adapter_test.cpp")])


def test_switches_are_in_the_table(hf):
    rows = {r["name"]: r for r in hf.tuning_table()}
    r = rows["HELFEM_EXCHANGE_BATCH_CHUNK"]
    assert r["default"] == "0" and r["read"] == "live" and r["kind"] == "int"
    r = rows["HELFEM_USCF_KBATCH"]
    assert r["default"] == "off" and r["value"] == "off" and r["kind"] == "=1"  # off by default
