"""Worker of test_gpu_dc_fused.py: eigen-decompositions of the test's tridiagonal matrices in a process of its own (the
HELFEM_DC switch is read once per process).  Usage: dc_fused_worker.py OUT.npz; writes E_<case> and C_<case>.  With a case name as second argument: that case
alone, nothing written."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import helfem_amd as hf  # noqa: E402

BATCH = (1380, 1470, 1380)


def tridiag(d, e):
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def mirrored(rng, levels):
    """d and e of a tridiagonal matrix that is its own mirror image at every level of the bisection tree: the two children
    of every merge have the same spectrum, so that every pole pair is close and the deflation rotates (many rotations).
    Weak disorder (diagonal +-0.05 beside couplings of about 1): the eigenvectors extend over the whole matrix, so the
    components of z are not small and the close pairs are removed by rotations, not by the small-z test."""
    d = rng.uniform(-0.05, 0.05, 16)
    e = rng.uniform(0.95, 1.05, 15)
    for _ in range(levels):
        d = np.concatenate([d, d[::-1]])
        e = np.concatenate([e, [rng.uniform(0.95, 1.05)], e[::-1]])
    return d, e


def cases():
    """(name, matrix) in a fixed order; all from seeded generators"""
    rng = np.random.RandomState(2024)
    # orders around the leaf size (16), around 48 and 96 (roots of the lowest merge levels) and around the 64-wide tiles
    # of the product; most are not multiples of 16
    for n in (15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 129, 191, 193, 385, 777):
        yield "random_%d" % n, tridiag(rng.uniform(-1, 1, n), rng.uniform(-1, 1, n - 1))
    n = 300
    yield "constant_diagonal", tridiag(np.zeros(n), np.ones(n - 1))
    yield "wilkinson", tridiag(np.abs(np.arange(n) - n // 2).astype(float), np.ones(n - 1))
    yield "near_identity", tridiag(np.ones(n), np.full(n - 1, 1e-9))
    yield "many_rotations", tridiag(*mirrored(rng, 4))


def batch_problem():
    rng = np.random.RandomState(77)
    N = sum(BATCH)
    F = np.zeros((N, N), order="F")
    blocks, off = [], 0
    for n in BATCH:
        F[off:off + n, off:off + n] = tridiag(rng.uniform(-1, 1, n), rng.uniform(-1, 1, n - 1))
        blocks.append(np.arange(off, off + n))
        off += n
    return F, blocks


if __name__ == "__main__":
    if len(sys.argv) > 2:  # one named case alone (the test reads the merge statistics of HELFEM_DC_DBG from stderr)
        hf.scf.eig_sym(dict(cases())[sys.argv[2]])
        print("ok")
        sys.exit(0)
    out = {}
    for name, A in cases():
        E, C = hf.scf.eig_sym(A)
        out["E_" + name], out["C_" + name] = E, C
    F, blocks = batch_problem()
    E, C = hf.scf.eig_gsym_sub(F, np.eye(F.shape[0], order="F"), blocks)
    out["E_batch"], out["C_batch"] = E, C
    np.savez(sys.argv[1], **out)
    print("ok")
