"""The low-rank exchange build (hip/exchange_lr.hip) launch variant by launch variant: the tasks the build really makes, with
their pointers, leading dimensions and slack, under every kernel, tile and launcher its rules (host/exl_plan.h) can pick,
against the oracle's K at shapes where the oracle sees all of K, and with the record of what ran (hfg_exl_last_plan) to tell
which variant a case went through.

One child process per setting (tests/exchange_variants_worker.py; the switches are read once per process), one after the
other, each under its own time limit; after a fault-like end (status 134, 139, -6, -11 or a timeout) no further child is
started and the remaining cases fail with "not run" (the protocol of test_gpu_eig_direct.py).  The parent computes the
oracle's K once per (basis, table set, density) on the CPU and hands it to the workers in an .npz.

Settings: default, EXL_RECT=0, EXL_RECT=1, EXL_WL=0, EXL_WL=0 EXL_RECT=0, EXL_WL=0 EXL_RECT=1, EXL_SPLITK=0, EXL_CRECT=0,
EXL_MGROUPS=0 (the names without the library's prefix), every other switch of the exchange builds (the worker's SWITCHES) removed
from the environment first.

Bases (host-built tables):
  B1  sigma + pi of the parity suite, N = 60: cross blocks of 10 and 20 rows, pair lists of at most 36 columns -- every block
      far below every tile, the edge of the over-read flags of the element tasks
  B2  hetero_sigma_pi_delta, N = 100: three element pairs, five runs with differing M intervals, so grouped tasks of
      differing K (no block is skipped: M = 0 lies in the interval of every run, and the plans record cross_skipped = 0)
  B3  sigma only, lmmax = (8,), 2 elements of 15 nodes, N = 252: one run (not grouped), A p = 135 crosses the 128 edge of
      the split 128 x 128 tiles, p = 15 leaves a padding row in the matrix-core RB tiles
  B4  lmmax = (5, 4), 2 elements of 13 nodes, N = 328: a sigma run of 78 rows (an edge tile of the 128 x 64 work list) beside
      pi runs of 52 (below a tile)
  B5  the atomic "sp" basis of test_gpu_rs.py, N = 44: Coulomb, Yukawa(0.4) and erfc(0.4) tables through rs_exchange; the erfc
      set runs k_exl_RB_pair, element tasks without over-read flags and k_exl_reduce_pair.  N = 44 is below r_hi = 57 and
      below 64: there the densities "r_hi", "rank64" and "multigroup" have rank 44 and one group, the split is out of reach
      (the assertion on it is made from the recorded rank) -- the diatomic bases carry those cases
  The oracle's exchange() on this CPU: B1 0.01 s, B2 0.05 s, B3 0.60 s, B4 1.08 s, B5 below 0.01 s per call.

Densities (common.random_density; NLM from the plan of a first build, r_hi = ceil(512 / NLM), r_lo = r_hi - 1): ranks r_lo
and r_hi on both sides of the split threshold of the cross products, rank 1, rank 2 (the plain member of the batch), rank 64
(a full group), an indefinite one with signed factors, and rank 64 + r_hi minus a rank-5 part (two groups of differing
rank, the second accumulating into K; on B1 and B5 N caps it at one group).

Asserted per (setting, basis, density): relerr(K, oracle) < 1e-12 (1e-11 for the indefinite and the multi-group density: the
bounds test_gpu_parity.py holds these inputs to), |K - K^T| <= 1e-13 max|K|, K of the zero matrix exactly zero; from the
plans: r_lo not split, r_hi split (except under EXL_SPLITK=0), and per setting the variant it is there for.  Batches
(r_hi, 2, r_lo) on B1 and B4 under every setting: every K_b bitwise the single build of the same process and within 1e-12
of the oracle, split and plain members in one chunk, bitwise again under HELFEM_EXCHANGE_BATCH_CHUNK=2.  Shards 0, 1, 2 of 3
of hfg_exchange_dev on B2 under default, EXL_WL=0 and EXL_RECT=0 sum to the full matrix within 1e-12.  The table of reached
variants (test_every_variant_is_reached) must be complete.  Every deviation is printed; the differences between settings
are printed and not bounded.

Observed on the MI355X: the worst deviation from the oracle is 1.27e-15 over the 1e-12 cases and 1.33e-15 over the 1e-11
cases under every one of the nine settings (WORST_SEEN below); the batches deviate by at most 1.1e-15; the shards sum to
the full matrix within 4.4e-16.  K under EXL_RECT, EXL_WL and EXL_CRECT is bitwise K under the default (the tiles of one
k order), under EXL_SPLITK=0 it differs by at most 9.8e-19 and under EXL_MGROUPS=0 by 7.3e-17 of max|K|.  The whole module
takes 27 s, 2 to 3 s per worker process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import exchange_variants_worker as wk  # noqa: E402

FAULT_LIKE = (134, 139, -6, -11)
WORKER_TIMEOUT_S = 240
# worst relerr(K, oracle) over all bases and densities of a setting as observed on the MI355X (single builds: the 1e-12 cases,
# the 1e-11 cases), for the reader: nothing is asserted against these
WORST_SEEN = {s: (1.27e-15, 1.33e-15) for s, _ in wk.SETTINGS}
KEYS = ["%s/%s" % (b, t) for b in sorted(wk.BASES) for t in wk.TABLES[b]]
DIATOMIC = ("B1", "B2", "B3", "B4")


def _child(args, env, path):
    """(result or None, error text or None, fault-like)"""
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "exchange_variants_worker.py")] + args, env=env, cwd=ROOT,
                             timeout=WORKER_TIMEOUT_S, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    except subprocess.TimeoutExpired as x:
        return None, "ran into its time limit\n" + (x.stdout or b"").decode(errors="replace")[-3000:], True
    text = out.stdout.decode(errors="replace")[-3000:]
    if out.returncode != 0 or "ok" not in text.split():
        return None, "status %d\n%s" % (out.returncode, text), out.returncode in FAULT_LIKE
    return json.load(open(path)), None, False


@pytest.fixture(scope="module")
def runs(native_libs, tmp_path_factory):
    """the probe, the oracle's matrices, then one GPU process per setting; after a fault-like end nothing more is started"""
    import common
    d = tmp_path_factory.mktemp("exchange_variants")
    base_env = {k: v for k, v in os.environ.items() if k not in wk.SWITCHES}
    res = {}
    info, err, fault = _child(["probe", str(d / "probe.json")], base_env, str(d / "probe.json"))
    if info is None:
        return dict(info=None, error="probe: " + err, settings={s: dict(error="not run: the probe failed") for s, _ in wk.SETTINGS})
    data = {}
    for name in sorted(wk.BASES):
        ob = wk.make(name, True)
        for which in wk.TABLES[name]:
            key = "%s/%s" % (name, which)
            ex, _ = wk.set_tables(ob, which)
            Ps = wk.densities(info[key]["N"], info[key]["plan"]["NLM"])
            if name == wk.SHARD_BASIS:
                gb = common.make_bases(*wk.BASES[name][1], oracle=False)[0]  # (host object: the symmetry blocks)
                Ps["m_blocked"] = wk.shard_density(gb)
            for tag, P in Ps.items():
                data["P/%s/%s" % (key, tag)] = P
                data["K/%s/%s" % (key, tag)] = ex(P)
    np.savez(str(d / "in.npz"), **data)
    stopped = None
    for setting, env in wk.SETTINGS:
        if stopped:
            res[setting] = dict(error="not run: %s" % stopped)
            continue
        e = dict(base_env)
        e.update(env)
        path = str(d / (setting + ".json"))
        r, err, fault = _child(["run", setting, str(d / "in.npz"), path, str(d / (setting + ".npz"))], e, path)
        if fault:
            stopped = "the worker of '%s' %s" % (setting, err.split("\n")[0])
        res[setting] = r if r is not None else dict(error=err)
        if r is not None:
            r["K"] = str(d / (setting + ".npz"))
    return dict(info=info, settings=res)


def _records(runs, setting, **match):
    r = runs["settings"][setting]
    if "error" in r:
        pytest.fail("worker of '%s': %s" % (setting, r["error"]))
    return [x for x in r["records"] if all(x[k] == v for k, v in match.items())]


def _one(runs, setting, **match):
    recs = _records(runs, setting, **match)
    assert len(recs) == 1, (setting, match, len(recs))
    return recs[0]


SINGLE = [(s, k) for s, _ in wk.SETTINGS for k in KEYS]


@pytest.mark.parametrize("setting,key", SINGLE, ids=["%s-%s" % (s, k.replace("/", "-")) for s, k in SINGLE])
def test_k_against_the_oracle(runs, setting, key):
    basis, tables = key.split("/")
    assert runs["settings"][setting].get("tuning", {}).get("HELFEM_EXCHANGE", "off") == "off" or "error" in runs["settings"][setting]
    bad = []
    for tag in sorted(wk.BOUND):
        rec = _one(runs, setting, kind="single", basis=basis, tables=tables, density=tag)
        print("%-10s %-12s %-10s dev %.2e asym %.2e ranks %s" % (setting, key, tag, rec["dev"], rec["asym"], rec["plan"]["ranks"]))
        assert rec["plan"] is not None and not rec["plan"]["declined"], (tag, rec["plan"])  # the low-rank build ran, not the general kernels
        if not rec["dev"] < wk.BOUND[tag]:
            bad.append((tag, "dev", rec["dev"]))
        if not rec["asym"] <= 1e-13:
            bad.append((tag, "asym", rec["asym"]))
        if not rec["zero"]:
            bad.append((tag, "K of the zero matrix is not zero"))
    assert not bad, bad


STRADDLE = [(s, k) for s, _ in wk.SETTINGS for k in KEYS]


@pytest.mark.parametrize("setting,key", STRADDLE, ids=["%s-%s" % (s, k.replace("/", "-")) for s, k in STRADDLE])
def test_ranks_on_both_sides_of_the_split_threshold(runs, setting, key):
    basis, tables = key.split("/")
    N, NLM = runs["info"][key]["N"], runs["info"][key]["plan"]["NLM"]
    r_lo, r_hi = wk.ranks_for(NLM)
    assert 8 <= NLM and r_hi <= 64 and NLM * r_lo < 512 <= NLM * r_hi
    lo = _one(runs, setting, kind="single", basis=basis, tables=tables, density="r_lo")["plan"]
    hi = _one(runs, setting, kind="single", basis=basis, tables=tables, density="r_hi")["plan"]
    print(setting, key, "NLM", NLM, "r_lo", lo["ranks"], lo["cross_split"], "r_hi", hi["ranks"], hi["cross_split"])
    assert lo["ranks"] == [min(r_lo, N)] and hi["ranks"] == [min(r_hi, N)]
    assert lo["cross_split"] == [0] and lo["n_cross_split"] == 0
    if basis in DIATOMIC:
        assert N > r_hi and lo["n_cross_plain"] > 0
        assert hi["cross_split"] == [0 if setting == "splitk0" else 1]
        assert (hi["n_cross_split"] > 0) == (setting != "splitk0") and (hi["n_cross_plain"] > 0) == (setting == "splitk0")
    else:  # N < r_hi: the density has rank N, below the threshold (module docstring); pair tables have no cross products
        reach = NLM * hi["ranks"][0] >= 512 and tables != "erfc" and setting != "splitk0"
        assert not reach and hi["cross_split"] == [0]
        assert (hi["n_cross_plain"] == 0) == (tables == "erfc")
    full = _one(runs, setting, kind="single", basis=basis, tables=tables, density="rank64")["plan"]
    multi = _one(runs, setting, kind="single", basis=basis, tables=tables, density="multigroup")["plan"]
    one = _one(runs, setting, kind="single", basis=basis, tables=tables, density="rank1")["plan"]
    assert one["ranks"] == [1] and full["ranks"] == [min(64, N)]
    if N > 64 + r_hi + 5:  # two groups of differing rank, the second accumulating into K
        assert len(multi["ranks"]) == 2 and multi["ranks"][0] == 64 and 0 < multi["ranks"][1] != 64, multi["ranks"]
    assert basis not in ("B2", "B3", "B4") or N > 64 + r_hi + 5


def _tile(plan, part):
    return (plan[part + "_tile"], plan[part + "_launcher"]) if part == "elem" else (plan["cross_split_tile"], plan["cross_launcher"])


@pytest.mark.parametrize("setting", [s for s, _ in wk.SETTINGS])
def test_the_plan_shows_the_variant_the_setting_is_there_for(runs, setting):
    for key in KEYS:
        basis, tables = key.split("/")
        hi = _one(runs, setting, kind="single", basis=basis, tables=tables, density="r_hi")["plan"]
        print(setting, key, json.dumps(hi))
        elem_want = {"default": ("T64", "worklist"), "rect0": ("T128", "worklist"), "rect1": ("T128x64", "worklist"),
                     "wl0": ("T128x64", "tasklist"), "wl0_rect0": ("Auto", "tasklist"), "wl0_rect1": ("T128x64", "tasklist")}.get(setting, ("T64", "worklist"))
        assert _tile(hi, "elem") == elem_want, (key, hi)  # (every basis here averages far fewer than 1500 pairs per task)
        assert hi["n_elem"] > 0 and hi["max_pairs"] > 0
        if tables == "erfc":
            assert hi["rb"] == "pair" and not hi["elem_over"] and not hi["grouped"] and hi["n_cross_split"] == hi["n_cross_plain"] == 0
            continue
        assert hi["rb"] == "mfma" and hi["alpha"] == "k_exl_alpha" and hi["elem_over"]
        runs_n = len(hi["run_shells"])
        assert hi["grouped"] == (runs_n > 1 and setting != "mgroups0")
        if basis == "B3":
            assert runs_n == 1 and not hi["grouped"]
        if basis not in DIATOMIC or setting == "splitk0":
            continue
        if hi["grouped"]:
            want = ("T128", "tasklist") if setting == "crect0" else ("T128x64", "tasklist") if setting.startswith("wl0") else ("T128x64", "worklist")
        else:
            want = ("T128", "tasklist")
        assert _tile(hi, "cross") == want, (key, hi)


def test_the_shapes_the_bases_are_there_for(runs):
    if runs["info"] is None:
        pytest.fail(runs["error"])
    plan = {k: runs["info"][k]["plan"] for k in KEYS}
    b1, b2, b3, b4 = (plan[b + "/coulomb"] for b in DIATOMIC)
    rows = lambda p: [n * p["p"] for n in p["run_shells"]]
    print({k: (runs["info"][k]["N"], p["NLM"], p["A"], p["p"], p["E"], p["run_shells"], p["max_pairs"]) for k, p in plan.items()})
    assert max(rows(b1)) <= 20 and min(rows(b1)) >= 10 and b1["max_pairs"] <= 36 and b1["elem_over"]  # far below every tile
    assert b2["E"] == 3 and len(b2["run_shells"]) == 5
    assert len(b3["run_shells"]) == 1 and b3["A"] * b3["p"] > 128 and b3["p"] == 15  # crosses the 128 edge; a padding row of the 16 x 16 RB tiles
    assert max(rows(b4)) > 64 and min(rows(b4)) < 64 and len(b4["run_shells"]) > 1  # an edge tile beside a sub-tile block
    assert plan["B5/erfc"]["rb"] == "pair" and plan["B5/yukawa"]["rb"] == "mfma"
    for k in KEYS:
        assert 100 <= runs["info"][k]["N"] <= 400 or k.split("/")[0] in ("B1", "B5")


BATCH = [(s, b) for s, _ in wk.SETTINGS for b in wk.BATCH_BASES]


@pytest.mark.parametrize("setting,basis", BATCH, ids=["%s-%s" % sb for sb in BATCH])
def test_batch_is_bitwise_the_single_builds(runs, setting, basis):
    rec = _one(runs, setting, kind="batch", basis=basis)
    plan = rec["plan"]
    print(setting, basis, rec["members"], "dev", rec["dev"], "bitwise", rec["bitwise"], rec["bitwise_chunk2"], json.dumps(plan))
    NLM = plan["NLM"]
    r_lo, r_hi = wk.ranks_for(NLM)
    want = {"r_hi": r_hi, "rank2": 2, "r_lo": r_lo}
    assert rec["members"] == list(wk.batch_ranks(NLM)) and plan["ranks"] == [want[t] for t in rec["members"]] and sum(plan["ranks"]) <= 64
    assert plan["batch"] and plan["chunks"] == 1  # one chunk holds them all
    assert all(rec["bitwise"]), rec["bitwise"]
    assert all(dv < 1e-12 for dv in rec["dev"]), rec["dev"]
    # a member that splits beside members that do not: h_csplit and h_cplain both filled in one launch sequence
    assert plan["cross_split"] == [0 if setting == "splitk0" or t != "r_hi" else 1 for t in rec["members"]]
    assert plan["n_cross_plain"] > 0 and (plan["n_cross_split"] > 0) == (setting != "splitk0")
    # every member got the tiles of its single build
    for t, split in zip(rec["members"], plan["cross_split"]):
        single = _one(runs, setting, kind="single", basis=basis, tables="coulomb", density=t)["plan"]
        assert single["cross_split"] == [split] and single["elem_tile"] == plan["elem_tile"] and single["elem_launcher"] == plan["elem_launcher"]
        if split:
            assert _tile(single, "cross") == _tile(plan, "cross")
    assert rec["bitwise_chunk2"] and rec["plan_chunk2"]["chunks"] == 1 and len(rec["plan_chunk2"]["ranks"]) == 2


@pytest.mark.parametrize("setting", wk.SHARD_SETTINGS)
def test_shards_sum_to_the_full_matrix(runs, setting):
    rec = _one(runs, setting, kind="shards", basis=wk.SHARD_BASIS)
    print(setting, rec["dev"], rec["dev_oracle"], rec["parts"], [p["n_elem"] for p in rec["plans"]])
    assert rec["dev"] < 1e-12 and rec["dev_oracle"] < 1e-12
    assert all(part > 1e-3 for part in rec["parts"])  # a shard is not the whole
    assert len(rec["plans"]) == wk.NSHARDS and all(0 < p["n_elem"] for p in rec["plans"])
    full = _one(runs, setting, kind="single", basis=wk.SHARD_BASIS, tables="coulomb", density="rank2")["plan"]
    assert sum(p["n_elem"] for p in rec["plans"]) == full["n_elem"]  # the slots are dealt out, none twice


def test_every_variant_is_reached(runs):
    """the launch variants of the build, each with the cases whose recorded plan shows it; none may be empty"""
    reached = {v: [] for v in (
        "elem worklist T64", "elem worklist T128", "elem worklist T128x64", "elem tasklist T128x64", "elem tasklist Auto",
        "elem over-read flags, at most 36 pair columns under a 128-wide tile", "elem without over-read flags (pair tables), every launcher",
        "cross plain, default tiles", "cross split T128x64 worklist, grouped", "cross split T128x64 tasklist split2, grouped",
        "cross split T128 split2, grouped", "cross split T128 split2, not grouped",
        "cross split T128 split2, block across the 128 edge", "cross split T128x64 worklist, edge tile beside a sub-tile block",
        "cross grouped, five runs, tasks of differing K", "rb pair", "rb mfma with a padding row (p = 15)",
        "second group of another rank accumulates", "signed factors",
        "batch: split and plain members in one chunk", "batch: no member split", "batch bitwise under non-default switches",
        "shards under the task-list grid", "shards under 128 x 128 tiles")}
    pair_launchers = set()
    for setting, _ in wk.SETTINGS:
        for rec in _records(runs, setting):
            where = "%s %s/%s %s" % (setting, rec["basis"], rec["tables"], rec["density"])
            if rec["kind"] == "shards":
                if rec["plans"][0]["elem_launcher"] == "tasklist":
                    reached["shards under the task-list grid"].append(where)
                if rec["plans"][0]["elem_tile"] == "T128":
                    reached["shards under 128 x 128 tiles"].append(where)
                continue
            p = rec["plan"]
            if rec["kind"] == "batch":
                if 0 < sum(p["cross_split"]) < len(p["cross_split"]) and p["n_cross_split"] and p["n_cross_plain"]:
                    reached["batch: split and plain members in one chunk"].append(where)
                if not sum(p["cross_split"]):
                    reached["batch: no member split"].append(where)
                if setting != "default" and all(rec["bitwise"]):
                    reached["batch bitwise under non-default switches"].append(where)
                continue
            rows = [n * p["p"] for n in p["run_shells"]]
            reached["elem %s %s" % (p["elem_launcher"], p["elem_tile"])].append(where)
            if p["elem_over"] and p["max_pairs"] <= 36 and p["elem_tile"] in ("T128", "T128x64"):  # 128 rows or 128 columns wide
                reached["elem over-read flags, at most 36 pair columns under a 128-wide tile"].append(where)
            if p["rb"] == "pair":
                reached["rb pair"].append(where)
                if not p["elem_over"]:
                    pair_launchers.add((p["elem_launcher"], p["elem_tile"]))
            if p["rb"] == "mfma" and p["p"] == 15:
                reached["rb mfma with a padding row (p = 15)"].append(where)
            if p["n_cross_plain"]:
                reached["cross plain, default tiles"].append(where)
            if p["n_cross_split"]:
                tile, launcher, g = p["cross_split_tile"], p["cross_launcher"], p["grouped"]
                if (tile, launcher, g) == ("T128x64", "worklist", True):
                    reached["cross split T128x64 worklist, grouped"].append(where)
                    if max(rows) > 64 > min(rows):
                        reached["cross split T128x64 worklist, edge tile beside a sub-tile block"].append(where)
                if (tile, launcher, g) == ("T128x64", "tasklist", True):
                    reached["cross split T128x64 tasklist split2, grouped"].append(where)
                if (tile, launcher) == ("T128", "tasklist"):
                    reached["cross split T128 split2, %sgrouped" % ("" if g else "not ")].append(where)
                    if p["cross_maxM"] > 128:
                        reached["cross split T128 split2, block across the 128 edge"].append(where)
                # (a block that no channel reaches cannot occur: M = 0 lies in the interval of every run, cross_skipped is 0)
                if g and len(p["run_shells"]) == 5 and p["cross_minK"] < p["cross_maxK"] and p["cross_skipped"] == 0:
                    reached["cross grouped, five runs, tasks of differing K"].append(where)
            if len(p["ranks"]) == 2 and p["ranks"][0] != p["ranks"][1]:
                reached["second group of another rank accumulates"].append(where)
            if rec["density"] == "indefinite":
                reached["signed factors"].append(where)
    if {("worklist", "T64"), ("worklist", "T128"), ("worklist", "T128x64"), ("tasklist", "T128x64"), ("tasklist", "Auto")} <= pair_launchers:
        reached["elem without over-read flags (pair tables), every launcher"].append(sorted(pair_launchers))
    for v in sorted(reached):
        print("%-75s %3d  %s" % (v, len(reached[v]), reached[v][:3]))
    missing = [v for v in sorted(reached) if not reached[v]]
    assert not missing, missing


def test_differences_between_the_settings_are_printed(runs):
    """K of every setting against the default's: printed for the reader, not bounded (other tiles sum in another order)"""
    ref = runs["settings"]["default"]
    if "error" in ref:
        pytest.fail("worker of 'default': %s" % ref["error"])
    K0 = np.load(ref["K"])
    worst = {}
    for setting, _ in wk.SETTINGS[1:]:
        r = runs["settings"][setting]
        if "error" in r:
            pytest.fail("worker of '%s': %s" % (setting, r["error"]))
        K = np.load(r["K"])
        assert sorted(K.files) == sorted(K0.files)
        for name in K.files:
            d = float(np.max(np.abs(K[name] - K0[name])) / np.max(np.abs(K0[name])))
            worst[setting] = max(worst.get(setting, 0.0), d)
            print("%-10s %-24s %.2e" % (setting, name, d))
    print("largest difference from the default per setting:", worst)
    for setting, _ in wk.SETTINGS:  # and the worst deviation from the oracle per setting (the figures of WORST_SEEN)
        recs = _records(runs, setting, kind="single")
        print("worst deviation from the oracle under %-10s: %.2e (1e-12 cases), %.2e (1e-11 cases)" % (
            setting, max(x["dev"] for x in recs if wk.BOUND[x["density"]] == 1e-12), max(x["dev"] for x in recs if wk.BOUND[x["density"]] == 1e-11)))
