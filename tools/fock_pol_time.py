"""Time of the Fock matrices of one unrestricted iteration, device buffers in and out, three ways in one process:

  (i)   the sequence of the device SCF loop (hip/scf_device.hip): P = Pa + Pb, hfg_coulomb_dev, hfg_xc_fock_pol_dev, and per spin
        F = mask(H0 + J + XC) as dense passes (torch operations on the context's stream stand in for the loop's axpby and mask
        kernels: three launches per spin where the loop has four)
  (ii)  hfg_fock_compact_pol_devptr + hfg_fock_finish_pol_devptr with the symmetry blocks declared (DeviceUSCFStep)
  (iii) (ii) with HELFEM_FOCK_SKIP=0

Densities: Pa = half the core-guess density, Pb = 0.8 Pa.  The three alternate round by round, each between two events on the
stream; medians, minima and maxima over the rounds.  A second set of rounds runs with the context's profile scopes on and
prints the stage times of (i) and (ii) (hfg_profile_get: coulomb, xc, scatter).

  python tools/fock_pol_time.py [--workloads n2_pbe_nbf4230,n2_pbe_small] [--warmup 5] [--repeat 30]"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
V = ctypes.c_void_p


def run(hf, torch, bench, name, warmup, repeat):
    w = bench.WORKLOADS[name]
    basis, _, _, _, ldft, mdft = bench.build_basis(hf, w)
    nocc = w["nocc"]
    step = hf.DeviceUSCFStep(basis, w["x"], w["c"], ldft, mdft, (nocc, nocc), symmetry=1, device=0, device_tei=True)
    ctx, L, N = step.ctx, hf.lib(), step.N
    S, H0 = basis.overlap(), basis.kinetic() + basis.nuclear()
    X = hf.scf.form_Sinvh(S, False, step.blocks, ctx=ctx)
    _, C = hf.scf.eig_gsym_sub(H0, X, step.blocks, ctx=ctx)
    Pa = hf.scf.form_density(C, nocc, ctx=ctx)
    step.set_matrices(H0, X)
    step.set_density(Pa, 0.8 * Pa)
    f64 = dict(dtype=torch.float64, device=step.dev)
    P, J, XCa, XCb, Fa, Fb = (torch.zeros(N * N, **f64) for _ in range(6))
    scal = torch.zeros(3, **f64)
    bid = step.blockid
    mask = (bid[:, None] == bid[None, :]).to(torch.float64).reshape(-1).contiguous()
    L.hfg_coulomb_dev.argtypes = [V] * 4
    L.hfg_xc_fock_pol_dev.argtypes = [V, V, ctypes.c_int, ctypes.c_int, V, V, V, V, V, ctypes.c_double]
    p = lambda t: V(t.data_ptr())

    def parent():
        torch.add(step.Pa, step.Pb, out=P)
        hf._check(L.hfg_coulomb_dev(ctx.h, basis.h, p(P), p(J)))
        hf._check(L.hfg_xc_fock_pol_dev(ctx.h, basis.h, w["x"], w["c"], p(step.Pa), p(step.Pb), p(XCa), p(XCb), p(scal), step.thr))
        for F, XC in ((Fa, XCa), (Fb, XCb)):
            torch.add(step.H0, J, out=F)
            F.add_(XC)
            F.mul_(mask)

    def fused():
        step.fock_partial()
        step.fock_finish()

    def fused_noskip():
        os.environ["HELFEM_FOCK_SKIP"] = "0"
        try:
            fused()
        finally:
            os.environ.pop("HELFEM_FOCK_SKIP", None)

    seqs = (("(i) coulomb_dev + xc_fock_pol_dev + dense passes", parent), ("(ii) fused build + finish", fused),
            ("(iii) fused, HELFEM_FOCK_SKIP=0", fused_noskip))
    for _ in range(warmup):
        for _, f in seqs:
            f()
    torch.cuda.synchronize()
    err = max(float((a - b).abs().max() / b.abs().max()) for a, b in ((step.Fa, Fa), (step.Fb, Fb)))
    times = {tag: [] for tag, _ in seqs}
    for _ in range(repeat):  # alternating: a drift of the clock reaches all alike
        for tag, f in seqs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            times[tag].append(e0.elapsed_time(e1))
    print("%s: Nbf %d, Nang %d, %d elements of %d nodes; max|F fused - F dense| / max|F| = %.1e" % (
        name, N, basis.Nang(), basis.Nel(), w["nnodes"], err))
    for tag, _ in seqs:
        t = np.array(times[tag])
        print("  %-50s median %.3f ms  min %.3f  max %.3f  (quartiles %.3f %.3f)" % (
            tag, np.median(t), t.min(), t.max(), np.percentile(t, 25), np.percentile(t, 75)), flush=True)
    ctx.profile(True)
    for tag, f in seqs[:2]:
        stage = {n: [] for n in ("coulomb", "xc", "scatter")}
        for _ in range(repeat):
            ctx.profile_reset()
            f()
            ctx.synchronize()
            for n in stage:
                stage[n].append(ctx.profile_get(n)[0])
        print("  stages of %s: %s" % (tag, ", ".join("%s %.3f ms" % (n, float(np.median(v))) for n, v in stage.items())), flush=True)
    ctx.profile(False)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="n2_pbe_nbf4230,n2_pbe_small")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=30)
    a = ap.parse_args()
    import torch
    import bench
    import helfem_amd as hf
    for name in a.workloads.split(","):
        run(hf, torch, bench, name, a.warmup, a.repeat)
