"""Time of hfg_coulomb_batch_devptr beside nP calls of hfg_coulomb_dev on one basis, both on device buffers, from the context's
profile scopes (hfg_profile_get): "coulomb" (the single calls), "coulomb_batch" (the batched call) and "coulomb_batch_tei"
(its pass over the in-element tables alone).  Single and batched rounds alternate in one process; medians, and the spread
of the alternating rounds as the run-to-run noise.

  python tools/coulomb_batch_time.py [--workload n2_pbe_nbf4230] [--np 1,4,16,64] [--warmup 3] [--repeat 10]

Fractions: table bytes / time against 8 TB/s (HBM3E data sheet) and useful flops 2 p^4 per (table type, channel (L, M),
element, density) against 78.6 TFLOP/s (FP64 matrix data sheet)."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS, MFMA_TFLOPS = 8.0, 78.6

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="n2_pbe_nbf4230")
    ap.add_argument("--np", default="1,4,16,64")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=10)
    a = ap.parse_args()
    import torch
    import bench
    import helfem_amd as hf
    w = bench.WORKLOADS[a.workload]
    ctx = hf.Context(0, stream=0)
    basis, *_ = bench.build_basis(hf, w)
    basis.compute_tei(False, device=True, ctx=ctx)
    basis.upload(ctx=ctx)
    N, E, pp = basis.Nbf(), basis.Nel(), w["nnodes"] ** 2
    lm = basis.lm_map()
    NLM = sum(1 if M == 0 else 2 for _, M in lm)
    table_bytes = 4 * len(lm) * E * pp * pp * 8
    # the rule is coulomb_batch_chunk of helfem_amd/csrc/host/fock_plan.h (it owns it; this restates it for the printout)
    tile = ((pp + 3) // 4 * 4) * 16 * 8  # LDS column tiles of eight densities
    chunk = 8 * (min(4, 65536 // tile) or min(4, 163840 // tile))
    print("%s: Nbf %d, %d elements of %d nodes, %d (L,|M|) channels, tables %.3f GB, %d densities per pass" % (
        a.workload, N, E, w["nnodes"], len(lm), table_bytes / 1e9, chunk))
    L = hf.lib()
    L.hfg_coulomb_dev.argtypes = [ctypes.c_void_p] * 4
    V = ctypes.c_void_p
    gen = torch.Generator(device="cuda").manual_seed(3)
    for nP in [int(v) for v in a.np.split(",")]:
        dP = torch.rand((nP, N, N), dtype=torch.float64, device="cuda", generator=gen)
        dP = (dP + dP.transpose(1, 2)).contiguous()
        dJ1, dJb = torch.empty_like(dP), torch.empty_like(dP)

        def singles():
            for b in range(nP):
                hf._check(L.hfg_coulomb_dev(ctx.h, basis.h, V(dP[b].data_ptr()), V(dJ1[b].data_ptr())))

        def batched():
            basis.coulomb_batch_torch(dP, out=dJb, ctx=ctx)
        for _ in range(a.warmup):
            singles()
            batched()
        ctx.synchronize()
        err = float((dJb - dJ1).abs().max() / dJ1.abs().max())
        ts, tb, tt = [], [], []
        ctx.profile(True)
        for _ in range(a.repeat):  # alternating: a drift of the clock reaches both alike
            ctx.profile_reset()
            singles()
            ctx.synchronize()
            ts.append(ctx.profile_get("coulomb")[0])
            ctx.profile_reset()
            batched()
            ctx.synchronize()
            tb.append(ctx.profile_get("coulomb_batch")[0])
            tt.append(ctx.profile_get("coulomb_batch_tei")[0])
        ctx.profile(False)
        ms, mb, mt = float(np.median(ts)), float(np.median(tb)), float(np.median(tt))
        line = "nP %3d  %d single calls %.3f ms (min %.3f max %.3f)  batched %.3f ms (min %.3f max %.3f)  ratio %.2f  max|dJ|/max|J| %.1e" % (
            nP, nP, ms, min(ts), max(ts), mb, min(tb), max(tb), ms / mb, err)
        if mt > 0.0:  # (one density goes through the single build's kernels: no batched pass)
            passes = -(-nP // chunk)
            tbs, tfl = passes * table_bytes / (mt * 1e-3) / 1e12, 2.0 * pp * pp * 4 * NLM * E * nP / (mt * 1e-3) / 1e12
            line += "  %d pass(es) over the tables %.3f ms: %.2f TB/s (%.0f %% of %.1f), %.1f TFLOP/s (%.0f %% of %.1f)" % (
                passes, mt, tbs, 100 * tbs / HBM_TBS, HBM_TBS, tfl, 100 * tfl / MFMA_TFLOPS, MFMA_TFLOPS)
        print(line, flush=True)
        del dP, dJ1, dJb
        torch.cuda.empty_cache()
