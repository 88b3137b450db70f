"""Worker of tests/test_gpu_eig_direct.py: the one-call blocked eigensolve (hfg_eig_gsym_sub_dev, hfg_eig_gsym_sub_sel_dev) with
HELFEM_EIG_DIRECT on (ranking ahead of the last product, which stores straight into C) against the same call with the switch
off (block slots, then hfg_eig_assemble_dev) and against numpy.linalg.eigh per block.  The switch is read at every call, the
GEMM switches that pick the last product's kernel once per process: the test starts one worker per setting of those.

Problems: block-diagonal F (random symmetric inside the blocks) and Sinvh = S^-1/2 per block of a random SPD overlap, on
interleaved index lists.  Also usable as a module: problem(), solve(), reference()."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# edge tiles, a 1 x 1 block, sizes straddling 64 and 128, eigenvalue ties across identical blocks (m = +-1 of the workload)
CASES = (("one", [1], False), ("edge", [5, 70, 64], False), ("straddle", [65, 1, 129], False), ("ties", [130, 130], True))
NEVS = (1, 3, 200)  # below, inside and beyond the block sizes
SWITCH = "HELFEM_EIG_DIRECT"
GEMM_SWITCHES = ("HELFEM_GEMM_TILE", "HELFEM_GEMM_SPLITK", "HELFEM_GEMM_RECT", "HELFEM_MFMA")  # they pick the last product's kernel
I64P = ctypes.POINTER(ctypes.c_int64)


def problem(sizes, seed, identical=False):
    """F, S, X = S^-1/2 (N x N, block diagonal on `blocks`), blocks: sorted index lists dealt out by a seeded permutation"""
    r = np.random.RandomState(seed)
    N = sum(sizes)
    perm = r.permutation(N)
    blocks, o = [], 0
    for n in sizes:
        blocks.append(np.sort(perm[o:o + n]))
        o += n
    if len(sizes) > 1:  # interleaved: no block is one contiguous run (a 1 x 1 block aside)
        assert all(len(b) == 1 or np.any(np.diff(b) != 1) for b in blocks)
    F, S, X = np.zeros((N, N)), np.zeros((N, N)), np.zeros((N, N))
    Fb = Sb = None
    for b in blocks:
        n = len(b)
        if Fb is None or not identical:
            A, B = r.uniform(-1, 1, (n, n)), r.uniform(-1, 1, (n, n))
            Fb, Sb = A + A.T, B @ B.T + n * np.eye(n)
        w, V = np.linalg.eigh(Sb)
        F[np.ix_(b, b)], S[np.ix_(b, b)], X[np.ix_(b, b)] = Fb, Sb, (V / np.sqrt(w)) @ V.T
    return F, S, X, blocks


def reference(F, X, blocks, nev=None):
    """eigenvalues by numpy.linalg.eigh per block, the lowest min(nev, n) of each, sorted over all"""
    E = []
    for b in blocks:
        Xb = X[np.ix_(b, b)]
        w = np.linalg.eigh(Xb.T @ F[np.ix_(b, b)] @ Xb)[0]
        E.append(w if nev is None else w[:min(nev, len(b))])
    return np.sort(np.concatenate(E))


def up(torch, M, dev):
    return torch.from_numpy(np.asfortranarray(M).ravel(order="F").copy()).to(dev)


def solve(hf, torch, ctx, Fd, Xd, N, blocks, nev=None, direct=True):
    """E (K), C (N x K) of the device-pointer entry, outputs pre-filled with NaN; the switch is set for this call"""
    ptr, idx = hf.scf._blocks(blocks)
    K = N if nev is None else sum(min(nev, len(b)) for b in blocks)
    dev = Fd.device
    Ed = torch.full((K,), float("nan"), dtype=torch.float64, device=dev)
    Cd = torch.full((N * K,), float("nan"), dtype=torch.float64, device=dev)
    os.environ[SWITCH] = "1" if direct else "0"
    try:
        L = hf.lib()
        args = [ctx.h, ctypes.c_int64(N), ctypes.c_void_p(Fd.data_ptr()), ctypes.c_void_p(Xd.data_ptr()), len(blocks),
                ptr.ctypes.data_as(I64P), idx.ctypes.data_as(I64P)]
        out = [ctypes.c_void_p(Ed.data_ptr()), ctypes.c_void_p(Cd.data_ptr())]
        if nev is None:
            rc = L.hfg_eig_gsym_sub_dev(*(args + out))
        else:
            rc = L.hfg_eig_gsym_sub_sel_dev(*(args + [ctypes.c_int64(nev)] + out))
        assert rc == 0, L.hfg_last_error(ctx.h)
        ctx.synchronize()
    finally:
        os.environ.pop(SWITCH, None)
    return Ed.cpu().numpy(), Cd.cpu().numpy().reshape((N, K), order="F")


def maxdiff(a, b):
    """max |a - b|; NaN anywhere (a word the call did not write) gives NaN, which no bound passes"""
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def figures(F, S, blocks, E, C, Eref):
    K = len(E)
    scale = max(1.0, float(np.max(np.abs(F))))
    outside = np.ones(C.shape, dtype=bool)  # rows outside the column's block: exactly zero
    owner = np.empty(C.shape[0], dtype=int)
    for ib, b in enumerate(blocks):
        owner[b] = ib
    for j in range(K):
        outside[blocks[owner[int(np.argmax(np.abs(C[:, j])))]], j] = False
    return dict(E=maxdiff(E, Eref) / max(1.0, float(np.max(np.abs(Eref)))), orth=maxdiff(C.T @ S @ C, np.eye(K)),
                resid=maxdiff(F @ C, S @ C * E) / scale, outside=float(np.max(np.abs(C[outside]))) if outside.any() else 0.0,
                ascending=bool(np.all(np.diff(E) >= 0)))


def main(out_path):
    import torch
    import helfem_amd as hf
    dev = torch.device("cuda", 0)
    ctx = hf.default_context()
    recs = []
    for name, sizes, identical in CASES:
        F, S, X, blocks = problem(sizes, 11 + len(sizes) + sizes[0], identical)
        N = F.shape[0]
        Fd, Xd = up(torch, F, dev), up(torch, X, dev)
        for nev in (None,) + NEVS:
            E1, C1 = solve(hf, torch, ctx, Fd, Xd, N, blocks, nev, direct=True)
            E0, C0 = solve(hf, torch, ctx, Fd, Xd, N, blocks, nev, direct=False)
            rec = dict(case=name, nev=nev, dE=maxdiff(E1, E0), dC=maxdiff(C1, C0))
            rec.update(figures(F, S, blocks, E1, C1, reference(F, X, blocks, nev)))
            recs.append(rec)
    json.dump(dict(records=recs, tuning={r["name"]: r["value"] for r in hf.tuning_table() if r["name"] in GEMM_SWITCHES}),
              open(out_path, "w"))
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
