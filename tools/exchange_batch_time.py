"""Time of hfg_exchange_batch_devptr beside nP calls of hfg_exchange_dev on one basis, both on device buffers, from the
context's profile scopes (hfg_profile_get): "exchange" (the single calls), "exchange_batch" (the batched call) and
"exl_batch_element_gemm" (its in-element GEMM alone, with its useful work in "exl_batch_element_gemm_gflop").  Single and
batched rounds alternate in one process; medians, and the range of the rounds as the run-to-run noise.  The comparison is
always the loop over the single build in the same process, never the batch against itself.

  python tools/exchange_batch_time.py [--workload n2_pbe0_nbf4230 | atomic] [--np 1,2,4,8] [--rank 7] [--warmup 3] [--repeat 10]

Densities: nP matrices C C^T of `rank` random orbitals, each inside one of the first three symmetry blocks of equal m
(--rank 7 with nP = 2 is the unrestricted shape of the bench; 8 x 7 = 56 factors still share one chunk).  "atomic" is the atomic basis of BASELINE config 2 (Ar, lmax = mmax = 1, 20 elements of 15 nodes).
Table stream: bytes of the exchange-ordered element tables / time of the element GEMM, against 8 TB/s (HBM3E data sheet);
useful flops of the element GEMM against 78.6 TFLOP/s (FP64 matrix data sheet)."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_TBS, MFMA_TFLOPS = 8.0, 78.6
ATOMIC = dict(Z=18, lmax=1, mmax=1, nelem=20, nnodes=15)

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="n2_pbe0_nbf4230")
    ap.add_argument("--np", default="1,2,4,8")
    ap.add_argument("--rank", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=10)
    a = ap.parse_args()
    import torch
    import bench
    import helfem_amd as hf
    ctx = hf.Context(0, stream=0)
    if a.workload == "atomic":
        import common
        basis, _ = common.make_atomic_bases(ATOMIC["Z"], ATOMIC["lmax"], ATOMIC["mmax"], ATOMIC["nelem"], ATOMIC["nnodes"], oracle=False)
        p, ntt = ATOMIC["nnodes"], 1
    else:
        w = bench.WORKLOADS[a.workload]
        basis, *_ = bench.build_basis(hf, w)
        p, ntt = w["nnodes"], 4
    basis.compute_tei(True, device=True, ctx=ctx)
    basis.upload(ctx=ctx)
    N, E, pp = basis.Nbf(), basis.Nel(), p * p
    blocks = basis.get_sym_idx(1)
    print("%s: Nbf %d, %d elements of %d nodes, %d symmetry blocks, %d factors per density" % (a.workload, N, E, p, len(blocks), a.rank), flush=True)
    L = hf.lib()
    L.hfg_exchange_dev.argtypes = [ctypes.c_void_p] * 4
    V = ctypes.c_void_p
    rng = np.random.RandomState(3)
    for nP in [int(v) for v in a.np.split(",")]:
        Ps = []
        for b in range(nP):
            C = np.zeros((N, a.rank))
            for k in range(a.rank):  # every orbital lives in one symmetry block, as the occupied orbitals of an SCF run do
                idx = blocks[k % min(len(blocks), 3)]
                C[idx, k] = rng.uniform(-1, 1, size=len(idx))
            Ps.append(C @ C.T)
        dP = torch.from_numpy(np.array(Ps)).cuda().contiguous()
        dK1, dKb = torch.empty_like(dP), torch.empty_like(dP)

        def singles():
            for b in range(nP):
                hf._check(L.hfg_exchange_dev(ctx.h, basis.h, V(dP[b].data_ptr()), V(dK1[b].data_ptr())))

        def batched():
            basis.exchange_batch_torch(dP, out=dKb, ctx=ctx)
        for _ in range(a.warmup):
            singles()
            batched()
        ctx.synchronize()
        same = bool(torch.equal(dKb, dK1))
        ts, tb, tg, t1 = [], [], [], []
        gf = chunks = 0.0
        ctx.profile(True)
        for _ in range(a.repeat):  # alternating: a drift of the clock reaches both alike
            ctx.profile_reset()
            singles()
            ctx.synchronize()
            ts.append(ctx.profile_get("exchange")[0])
            t1.append(ctx.profile_get("exl_element_gemm")[0])
            ctx.profile_reset()
            batched()
            ctx.synchronize()
            tb.append(ctx.profile_get("exchange_batch")[0])
            if "exl_batch_element_gemm" in ctx.profile_names():
                tg.append(ctx.profile_get("exl_batch_element_gemm")[0])
                gf, chunks = ctx.profile_get("exl_batch_element_gemm_gflop")
        ctx.profile(False)
        ms, mb = float(np.median(ts)), float(np.median(tb))
        spread = max(ts) - min(ts)
        verdict = "faster" if mb < ms - spread else "slower" if mb > ms + spread else "within the loop's spread"
        line = "nP %2d  loop %.3f ms (min %.3f max %.3f, its element GEMMs %.3f)  batched %.3f ms (min %.3f max %.3f)  ratio %.3f  %s  bitwise %s" % (
            nP, ms, min(ts), max(ts), float(np.median(t1)), mb, min(tb), max(tb), ms / mb, verdict, same)
        if tg:
            mg = float(np.median(tg))
            # every chunk streams every (slot, element) table once: rows padded to 128, columns to 16 (exlr_setup)
            try:
                ntab = len(basis.lm_map())
            except Exception:  # (no channel map for this basis class: the flop rate alone)
                ntab = 0
            tbytes = chunks * ntab * E * ((pp + 127) // 128 * 128) * ((ntt * pp + 15) // 16 * 16) * 8
            line += "  %d chunk(s): element GEMM %.3f ms, %.1f useful TFLOP/s (%.0f %% of %.1f)" % (chunks, mg, gf / mg, 100 * gf / mg / MFMA_TFLOPS, MFMA_TFLOPS)
            if ntab:
                line += ", tables %.2f TB/s (%.0f %% of %.1f)" % (tbytes / (mg * 1e-3) / 1e12, 100 * tbytes / (mg * 1e-3) / 1e12 / HBM_TBS, HBM_TBS)
        print(line, flush=True)
        del dP, dK1, dKb
        torch.cuda.empty_cache()
