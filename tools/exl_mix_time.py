"""Times the exact exchange of a range-separated hybrid from the mixed-kernel table set against the two builds it replaces, at
BASELINE config 2's basis (Ar, 15 nodes, lmax = mmax = 1) with 10 and 20 elements, for both screened kernels:
   python tools/exl_mix_time.py [OUT.txt]      (default: profiles/exl_mix_time.txt)
Per case: the mixing, once per run (hfg_mix_exchange_tables: HIP events around k_exl_mix_tables alone, "exchange_mix_kernel";
around the whole call with the set's shells and couplings, their uploads and synchronisations, "exchange_mix_tables"; and
the wall time of the call), then one K build for the nine occupied orbitals of argon per spin --
  mixed   hfg_mix_exchange_occ_devptr
  two     hfg_exchange_occ_dev + hfg_rs_exchange_dev + the weighted sum on the device (the code paths before the mixed set)
alternating, 3 warm-up and 10 timed rounds, time between two events on the context's stream; medians and the spread
(max - min) of each.  Every build synchronises its stream before it returns, so an interval is the latency of the build
as a step object pays it, host work between its launches included, not the sum of its kernels' times.  Also the bytes of
the mixed set, N_L E^2 p^4 8, and of the exchange-ordered copy the pair path keeps beside it."""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import helfem_amd as hf  # noqa: E402
import common  # noqa: E402

OMEGA, LMAX, NNODES, NOCC = 0.4, 1, 15, 9
ALPHA, BETA = 0.19, 0.46
WARM, ROUNDS = 3, 10
V = ctypes.c_void_p


def run(nelem, kind, ctx):
    gb, _ = common.make_atomic_bases(18, LMAX, 1, nelem, NNODES, oracle=False)
    gb.ctx = ctx
    gb.compute_tei(True, device=True)
    getattr(gb, "compute_" + kind)(OMEGA, device=True)
    gb.upload()
    N = gb.Nbf()
    C, _ = np.linalg.qr(np.random.RandomState(3).uniform(-1, 1, (N, NOCC)))
    dC = torch.zeros(N * N, dtype=torch.float64, device="cuda")
    dC[:N * NOCC].copy_(torch.from_numpy(np.asfortranarray(C).ravel(order="F")))
    dP = torch.from_numpy(np.asfortranarray(C @ C.T).ravel(order="F")).cuda()
    K, Krs, Kmix = (torch.zeros(N * N, dtype=torch.float64, device="cuda") for _ in range(3))
    ctx.profile(True)
    ctx.profile_reset()
    ctx.synchronize()
    t0 = time.perf_counter()
    assert gb.mix_exchange_tables(ALPHA, BETA)
    wall = time.perf_counter() - t0
    mix_ms, kern_ms = ctx.profile_get("exchange_mix_tables")[0], ctx.profile_get("exchange_mix_kernel")[0]
    ctx.profile(False)
    L = hf.lib()
    L.hfg_exchange_occ_dev.argtypes = [V, V, V, V, ctypes.c_int64, V]
    L.hfg_mix_exchange_occ_devptr.argtypes = [V, V, V, V, ctypes.c_int64, V]
    L.hfg_rs_exchange_dev.argtypes = [V, V, V, V]
    p = lambda t: V(t.data_ptr())

    def mixed():
        assert L.hfg_mix_exchange_occ_devptr(ctx.h, gb.h, p(dP), p(dC), NOCC, p(Kmix)) == 0, L.hfg_last_error()

    def two():
        assert L.hfg_exchange_occ_dev(ctx.h, gb.h, p(dP), p(dC), NOCC, p(K)) == 0, L.hfg_last_error()
        assert L.hfg_rs_exchange_dev(ctx.h, gb.h, p(dP), p(Krs)) == 0, L.hfg_last_error()
        K.mul_(ALPHA).add_(Krs, alpha=BETA)

    times = {"mixed": [], "two": []}
    for it in range(WARM + ROUNDS):
        for tag, fn in (("mixed", mixed), ("two", two)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if it >= WARM:
                times[tag].append(a.elapsed_time(b))
    dev = float((Kmix - K).abs().max() / K.abs().max())
    nbytes = (2 * LMAX + 1) * nelem ** 2 * NNODES ** 4 * 8
    return dict(N=N, wall=wall, mix_ms=mix_ms, kern_ms=kern_ms, times=times, dev=dev, nbytes=nbytes)


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "exl_mix_time.txt")
    ctx = hf.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    lines = ["# tools/exl_mix_time.py: Ar, %d nodes, lmax = mmax = %d, omega = %.1f, alpha = %.2f, beta = %.2f, %d occupied orbitals; "
             "%d warm-up and %d timed rounds, alternating; ms" % (NNODES, LMAX, OMEGA, ALPHA, BETA, NOCC, WARM, ROUNDS)]
    for nelem in (10, 20):
        for kind in ("yukawa", "erfc"):
            r = run(nelem, kind, ctx)
            med = {k: float(np.median(v)) for k, v in r["times"].items()}
            spr = {k: float(np.max(v) - np.min(v)) for k, v in r["times"].items()}
            lines.append("nelem %2d  %-6s  Nbf %4d  mix kernel %7.3f ms  mix call %7.3f ms (%6.1f ms wall)  mixed K %7.3f (spread %.3f)  two builds %7.3f (spread %.3f)  "
                         "ratio %.2f  mixed set %7.1f MB (+ as much exchange-ordered)  mixed vs two %.1e" %
                         (nelem, kind, r["N"], r["kern_ms"], r["mix_ms"], 1e3 * r["wall"], med["mixed"], spr["mixed"], med["two"], spr["two"],
                          med["two"] / med["mixed"], r["nbytes"] / 1e6, r["dev"]))
            print(lines[-1], flush=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
