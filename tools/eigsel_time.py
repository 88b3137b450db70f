"""Stage times of the selected eigensolver (hfg_eig_gsym_sub_sel) beside the full one (hfg_eig_gsym_sub) on one blocked
problem, from the context's profile scopes (hfg_profile_get): eig_tridiag, eig_tridiag_solve / eig_tridiag_sel,
eig_backtransform, eig_products.  Both paths of the selected solver are timed, each in a child process (HELFEM_EIGSEL is
read once per process); the rounds of the full and the selected call alternate inside every process.

  python tools/eigsel_time.py [--blocks 1380,1470,1380] [--nev 32[,NEV...]] [--warmup 3] [--repeat 10]

The matrices are the random tridiagonal blocks of tests/dc_fused_worker.py with X = 1 (no basis set-up)."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCOPES = ("eig_tridiag", "eig_tridiag_solve", "eig_tridiag_sel", "eig_backtransform", "eig_products")


def problem(sizes):
    rng = np.random.RandomState(77)
    N = sum(sizes)
    F = np.zeros((N, N), order="F")
    blocks, off = [], 0
    for n in sizes:
        d, e = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n - 1)
        F[off:off + n, off:off + n] = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
        blocks.append(np.arange(off, off + n))
        off += n
    return F, blocks


def child(sizes, nevs, warmup, repeat):
    import time
    import helfem_amd as hf
    ctx = hf.default_context()
    F, blocks = problem(sizes)
    X = np.eye(F.shape[0], order="F")
    calls = [("full", lambda: hf.scf.eig_gsym_sub(F, X, blocks))] + [("sel nev=%d" % v, lambda v=v: hf.scf.eig_gsym_sub_sel(F, X, blocks, v))
                                                                  for v in nevs]
    for _, f in calls:
        for _ in range(warmup):
            f()
    acc = {name: {s: [] for s in SCOPES} for name, _ in calls}
    ctx.profile(True)
    for _ in range(repeat):
        for name, f in calls:  # alternating: a drift of the clock reaches every call alike
            ctx.profile_reset()
            f()
            for s in SCOPES:
                acc[name][s].append(ctx.profile_get(s)[0])
    ctx.profile(False)
    path = os.environ.get("HELFEM_EIGSEL", "unset")
    for name, _ in calls:
        row = "  ".join("%s %.3f (min %.3f)" % (s, float(np.median(acc[name][s])), float(np.min(acc[name][s]))) for s in SCOPES)
        total = np.median(np.sum([acc[name][s] for s in SCOPES if s != "eig_products"], axis=0))
        print("HELFEM_EIGSEL=%s  %-12s  median ms: %s  stages total %.3f" % (path, name, row, total), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="1380,1470,1380")
    ap.add_argument("--nev", default="32")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    sizes = [int(v) for v in a.blocks.split(",")]
    nevs = [int(v) for v in a.nev.split(",")]
    if a.child:
        child(sizes, nevs, a.warmup, a.repeat)
        sys.exit(0)
    for path in ("stein", "dc"):
        env = dict(os.environ, HELFEM_EIGSEL=path)
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--child", "--blocks", a.blocks, "--nev", a.nev, "--warmup",
                              str(a.warmup), "--repeat", str(a.repeat)], env=env, cwd=ROOT)
        if rc != 0:
            sys.exit(rc)
