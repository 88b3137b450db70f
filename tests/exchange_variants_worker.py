"""Worker of test_gpu_exchange_variants.py, in a process of its own: the switches of the exchange build it is started under are
read once, at start-up.  Also holds what the parent shares with it: the bases, the settings and the densities.

Usage: exchange_variants_worker.py probe OUT.json           NLM, A, p and the runs of every basis and table set, from the plan
                                                            of one rank-1 build (the parent derives the ranks from them)
       exchange_variants_worker.py run SETTING IN.npz OUT.json OUT.npz
                                                            every density of IN.npz through hfg_exchange / hfg_rs_exchange, the
                                                            batches and (SETTING names who runs them) the shards, under the
                                                            switches of the environment: deviations and plans into OUT.json,
                                                            the matrices into OUT.npz

The process exits non-zero at the first error and does nothing on the GPU after it."""
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWITCHES = ("HELFEM_EXL_RB", "HELFEM_EXL_MGROUPS", "HELFEM_EXL_RECT", "HELFEM_EXL_WL", "HELFEM_EXL_SPLITK", "HELFEM_EXL_CRECT",
            "HELFEM_EXL_GROUPS", "HELFEM_EXL_HINT", "HELFEM_EXL_PAIR", "HELFEM_EXL_MIX", "HELFEM_EXCHANGE", "HELFEM_EXCHANGE_BATCH_CHUNK")
SETTINGS = (("default", {}),
            ("rect0", {"HELFEM_EXL_RECT": "0"}),
            ("rect1", {"HELFEM_EXL_RECT": "1"}),
            ("wl0", {"HELFEM_EXL_WL": "0"}),
            ("wl0_rect0", {"HELFEM_EXL_WL": "0", "HELFEM_EXL_RECT": "0"}),
            ("wl0_rect1", {"HELFEM_EXL_WL": "0", "HELFEM_EXL_RECT": "1"}),
            ("splitk0", {"HELFEM_EXL_SPLITK": "0"}),
            ("crect0", {"HELFEM_EXL_CRECT": "0"}),
            ("mgroups0", {"HELFEM_EXL_MGROUPS": "0"}))

# diatomic: (Z1, Z2, Rbond, lmmax, nelem, nnodes); atomic: (Z, lmax, mmax, nelem, nnodes)
BASES = {
    "B1": ("diatomic", (7, 7, 2.068, (3, 2), 2, 5)),     # sigma + pi of test_gpu_parity.py: every block far below a tile
    "B2": ("diatomic", (3, 9, 2.955, (3, 3, 2), 3, 4)),  # hetero_sigma_pi_delta: three element pairs, five runs
    "B3": ("diatomic", (1, 1, 1.4, (8,), 2, 15)),        # sigma only: one run, A p = 135, 15 nodes
    "B4": ("diatomic", (7, 7, 2.068, (5, 4), 2, 13)),    # sigma run of 78 rows, pi runs of 52
    "B5": ("atomic", (10, 1, 1, 3, 5)),                  # "sp" of test_gpu_rs.py: Coulomb, Yukawa and erfc (pair) tables
}
OMEGA = 0.4
TABLES = {"B1": ("coulomb",), "B2": ("coulomb",), "B3": ("coulomb",), "B4": ("coulomb",), "B5": ("coulomb", "yukawa", "erfc")}
BATCH_BASES = ("B1", "B4")
SHARD_BASIS, SHARD_SETTINGS, NSHARDS = "B2", ("default", "wl0", "rect0"), 3
# bounds of test_gpu_parity.py on these inputs
BOUND = {"r_lo": 1e-12, "r_hi": 1e-12, "rank1": 1e-12, "rank2": 1e-12, "rank64": 1e-12, "indefinite": 1e-11, "multigroup": 1e-11}


def ranks_for(NLM):
    """ranks on both sides of the split threshold NLM * r >= 512"""
    assert NLM >= 8  # so that r_hi <= 64: one group
    r_hi = -(-512 // NLM)
    return r_hi - 1, r_hi


def batch_ranks(NLM):
    r_lo, r_hi = ranks_for(NLM)
    return ("r_hi", "rank2", "r_lo") if r_hi + 2 + r_lo <= 64 else ("r_hi", "rank2")


def densities(N, NLM):
    """tag -> density; seeds fixed, so that the parent and every worker mean the same matrices"""
    import common
    r_lo, r_hi = ranks_for(NLM)
    return {
        "r_lo": common.random_density(N, r_lo, seed=101),
        "r_hi": common.random_density(N, r_hi, seed=102),
        "rank1": common.random_density(N, 1, seed=103),
        "rank2": common.random_density(N, 2, seed=104),  # the plain member of the batch
        "rank64": common.random_density(N, 64, seed=105),
        "indefinite": common.random_density(N, 3, seed=31) - common.random_density(N, 2, seed=32),
        "multigroup": common.random_density(N, 64 + r_hi, seed=41) - 0.5 * common.random_density(N, 5, seed=48),
    }


def shard_density(gb):
    import common
    return common.random_density(gb.Nbf(), 2, seed=12, blocks=gb.get_sym_idx(1))


def make(name, oracle):
    """(product basis, oracle basis) with host-built tables; the product one uploaded"""
    import common
    kind, args = BASES[name]
    gb, ob = (common.make_bases if kind == "diatomic" else common.make_atomic_bases)(*args, product=not oracle, oracle=oracle)
    b = ob if oracle else gb
    b.compute_tei(True)
    if not oracle:
        gb.upload()
    return b


def set_tables(b, which):
    """the table set `which` of basis b ready; returns (exchange function, name of the set in hfg_exl_last_plan)"""
    if which == "coulomb":
        return b.exchange, "coulomb"
    (b.compute_yukawa if which == "yukawa" else b.compute_erfc)(OMEGA)
    return b.rs_exchange, "screened"


def probe(out_path):
    res = {}
    for name in sorted(BASES):
        gb = make(name, False)
        N = gb.Nbf()
        for which in TABLES[name]:
            ex, pname = set_tables(gb, which)
            P = np.zeros((N, N), order="F")
            P[0, 0] = 1.0
            ex(P)
            plan = gb.exchange_last_plan(pname)["single"]
            assert plan is not None and not plan["declined"], (name, which, plan)
            res["%s/%s" % (name, which)] = dict(N=N, plan=plan)
    json.dump(res, open(out_path, "w"))


def run(setting, in_path, out_path, k_path):
    import common
    import helfem_amd as hf
    data = np.load(in_path)
    records, mats = [], {}
    tuning = {r["name"]: r["value"] for r in hf.tuning_table() if r["name"] in SWITCHES}
    for name in sorted(BASES):
        gb = make(name, False)
        N = gb.Nbf()
        for which in TABLES[name]:
            ex, pname = set_tables(gb, which)
            key = "%s/%s" % (name, which)
            K0 = ex(np.zeros((N, N), order="F"))
            single = {}
            for tag in sorted(BOUND):
                P, Ko = data["P/%s/%s" % (key, tag)], data["K/%s/%s" % (key, tag)]
                K = ex(P)
                plan = gb.exchange_last_plan(pname)["single"]
                single[tag] = K
                mats["%s/%s" % (key, tag)] = K
                records.append(dict(kind="single", basis=name, tables=which, density=tag, dev=float(common.relerr(K, Ko)),
                                    asym=float(np.max(np.abs(K - K.T)) / np.max(np.abs(K))), zero=bool(np.all(K0 == 0.0)), plan=plan))
            if name in BATCH_BASES:
                NLM = records[-1]["plan"]["NLM"]
                tags = batch_ranks(NLM)
                Ps = [data["P/%s/%s" % (key, t)] for t in tags]
                rec = dict(kind="batch", basis=name, tables=which, density="+".join(tags), members=list(tags))
                Kb = gb.exchange_batch(Ps)
                rec["plan"] = gb.exchange_last_plan(pname)["batch"]
                rec["bitwise"] = [bool(np.array_equal(Kb[i], single[t])) for i, t in enumerate(tags)]
                rec["dev"] = [float(common.relerr(Kb[i], data["K/%s/%s" % (key, t)])) for i, t in enumerate(tags)]
                os.environ["HELFEM_EXCHANGE_BATCH_CHUNK"] = "2"  # a live switch
                try:
                    K2 = gb.exchange_batch(Ps)
                finally:
                    os.environ.pop("HELFEM_EXCHANGE_BATCH_CHUNK")
                rec["bitwise_chunk2"] = bool(np.array_equal(K2, Kb))
                rec["plan_chunk2"] = gb.exchange_last_plan(pname)["batch"]
                records.append(rec)
        if name == SHARD_BASIS and setting in SHARD_SETTINGS:
            import ctypes
            import torch
            P = shard_density(gb)
            full = gb.exchange(P)
            dP = torch.from_numpy(np.ascontiguousarray(P.T)).cuda()  # symmetric: layout does not matter
            dK = torch.zeros((N, N), dtype=torch.float64, device="cuda")
            acc, parts, plans = np.zeros_like(full), [], []
            try:
                for rk in range(NSHARDS):
                    gb.ctx.set_shard(rk, NSHARDS)
                    rc = hf.lib().hfg_exchange_dev(gb.ctx.h, gb.h, ctypes.c_void_p(dP.data_ptr()), ctypes.c_void_p(dK.data_ptr()))
                    assert rc == 0, hf.lib().hfg_last_error()
                    torch.cuda.synchronize()
                    part = dK.cpu().numpy().T
                    parts.append(float(common.relerr(part, full)))
                    plans.append(gb.exchange_last_plan("coulomb")["single"])
                    acc += part
            finally:
                gb.ctx.set_shard(0, 1)
            records.append(dict(kind="shards", basis=name, tables="coulomb", density="m_blocked", dev=float(common.relerr(acc, full)),
                                dev_oracle=float(common.relerr(full, data["K/%s/coulomb/m_blocked" % name])), parts=parts, plans=plans))
    np.savez(k_path, **mats)
    json.dump(dict(setting=setting, tuning=tuning, records=records), open(out_path, "w"))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        {"probe": probe, "run": run}[sys.argv[1]](*sys.argv[2:])
        print("ok")
    except BaseException:  # the first error ends the process: nothing more is enqueued, no destructor runs on the GPU
        traceback.print_exc()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(1)
