"""Times the set-up of the range-separated exchange tables, host path (hfg_compute_rs_tei + hfg_basis_upload) against device
path (hfg_compute_rs_tei_dev + hfg_basis_upload), for both kernels, at BASELINE config 2's basis (Ar, 20 x 15 nodes,
lmax = mmax = 1, omega = 0.4) and at half as many elements:
   python tools/rs_tei_time.py [OUT.txt]      (default: profiles/rs_tei_time.txt)
Wall times are measured (one run each, after a warm-up build on a tiny basis that loads the code objects).  The byte counts are
computed from the table shapes: "host tables" is what rs_tei, rs_ktei and the disjoint tables hold in host memory at their
peak; "uploaded" is what crosses to the device (host path: the padded tables; device path: the polynomial operands)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helfem_amd as hf  # noqa: E402
import common  # noqa: E402

OMEGA, LMAX, NNODES = 0.4, 1, 15
NL = 2 * LMAX + 1


def sizes(nelem, kind, path):
    """(bytes of the host table vectors, bytes uploaded)"""
    p, nq = NNODES, 5 * NNODES
    Np = [(p - 1) ** 2 if e in (0, nelem - 1) else p * p for e in range(nelem)]
    if kind == "yukawa":
        host = NL * sum(2 * n * n + 2 * n for n in Np) * 8
        up_host = NL * nelem * (p ** 4 + 2 * p * p) * 8
        up_dev = sum(n * (2 * nq + nq * nq) + 2 * nq + 2 * nq * nq for n in Np) * 8
    else:
        host = NL * 2 * sum(a * b for a in Np for b in Np) * 8
        up_host = NL * nelem * nelem * p ** 4 * 8
        up_dev = (nelem * (p * p * nq + nq + nq * nq) + nelem * p * p * nq * nq) * 8  # (a diagonal operand may be sent in two batches)
    return (host, up_host) if path == "host" else (0, up_dev)


def run(nelem, kind, path, ctx):
    gb, _ = common.make_atomic_bases(18, LMAX, 1, nelem, NNODES, oracle=False)
    gb.ctx = ctx
    gb.compute_tei(True, device=True)
    gb.upload()
    ctx.synchronize()
    t0 = time.perf_counter()
    getattr(gb, "compute_" + kind)(OMEGA, device=(path == "dev"))
    t1 = time.perf_counter()
    gb.upload()
    ctx.synchronize()
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rs_tei_time.txt")
    ctx = hf.default_context()
    for kind in ("yukawa", "erfc"):
        run(2, kind, "dev", ctx)
    lines = ["# tools/rs_tei_time.py: Ar, %d nodes, lmax = mmax = %d (N_L = %d), omega = %.1f; threads of the host path: %s" %
             (NNODES, LMAX, NL, OMEGA, os.environ.get("HELFEM_NUM_THREADS", "one per core"))]
    for nelem in (10, 20):
        for kind in ("yukawa", "erfc"):
            for path in ("host", "dev"):
                tb, tu = run(nelem, kind, path, ctx)
                hb, ub = sizes(nelem, kind, path)
                lines.append("nelem %2d  %-6s  %-4s  tables %9.3f s  upload %7.3f s  total %9.3f s  host tables %8.1f MB  uploaded %8.1f MB" %
                             (nelem, kind, path, tb, tu, tb + tu, hb / 1e6, ub / 1e6))
                print(lines[-1], flush=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
