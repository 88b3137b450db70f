"""Worker of test_gpu_eigsel.py: the selected eigensolver on the test's inputs in a process of its own (HELFEM_EIGSEL is
read once per process).  Usage: eigsel_worker.py OUT.npz; writes E_<case> and C_<case> for every case of dense_cases(),
hard_cases(), aufbau_cases() and gen_cases(), the second run of the repeatability case and the device-pointer call."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helfem_amd as hf  # noqa: E402

# orders of test_eig_sym_vs_lapack that the issue names, and 65
DENSE_N = (1, 2, 3, 17, 64, 65, 130, 257, 333)
# (n, nev) next to the size switches of the selected path, see the docstring of test_gpu_eigsel.py
DENSE_EXTRA = ((64, 8), (64, 9), (130, 4), (130, 5))
TRIDIAG_EXTRA = ((1598, 4), (1599, 4), (3072, 4), (3073, 4))
REPEAT = (333, 40)


def dense_matrix(n):
    rng = np.random.RandomState(n)
    A = rng.uniform(-1, 1, size=(n, n))
    return A + A.T + np.diag(np.linspace(0, 50.0, n))


def tridiag(d, e):
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def big_tridiag(n):
    rng = np.random.RandomState(n)
    return rng.uniform(-1, 1, n), rng.uniform(-1, 1, n - 1)


def dense_cases():
    """(name, n, nev, matrix maker)"""
    for n in DENSE_N:
        for nev in sorted({1, 2, -(-n // 4), n}):
            if nev <= n:
                yield "dense_%d_%d" % (n, nev), n, nev, "dense"
    for n, nev in DENSE_EXTRA:
        yield "dense_%d_%d" % (n, nev), n, nev, "dense"
    for n, nev in TRIDIAG_EXTRA:
        yield "tridiag_%d_%d" % (n, nev), n, nev, "tridiag"


def hard_matrices():
    """the generator of test_gpu_parity.py::test_eig_sym_hard_spectra"""
    rng = np.random.RandomState(42)
    n = 300
    yield "near_identity", tridiag(np.ones(n), np.full(n - 1, 1e-9))
    yield "graded", tridiag(np.arange(n, dtype=float) ** 3, rng.uniform(0, 1, n - 1))
    yield "wilkinson", tridiag(np.abs(np.arange(n) - n // 2).astype(float), np.ones(n - 1))
    yield "toeplitz", tridiag(np.zeros(n), np.ones(n - 1))
    yield "decoupled", tridiag(rng.uniform(-1, 1, n), np.where(rng.rand(n - 1) < 0.3, 0.0, rng.uniform(-1, 1, n - 1)))
    dd = rng.uniform(-1, 1, n)
    dd[100:140] = 0.5
    yield "clustered", tridiag(dd, rng.uniform(-1, 1, n - 1) * 1e-8)
    yield "dynamic_range", tridiag(np.exp(rng.uniform(-20, 15, n)), np.exp(rng.uniform(-20, 10, n - 1)))
    for m in (33, 65, 97, 129, 513, 1000):
        yield "random_%d" % m, tridiag(rng.uniform(-1, 1, m), rng.uniform(-1, 1, m - 1))
    A = rng.uniform(-1, 1, (40, 40))
    A = A + A.T
    Z = np.zeros_like(A)
    yield "degenerate_pairs", np.block([[A, Z], [Z, A]])


def hard_cases():
    for name, A in hard_matrices():
        n = A.shape[0]
        for nev in sorted({1, 2, 8, n // 4, n // 2}):
            yield "hard_%s_%d" % (name, nev), A, nev


def aufbau_nev(A, start, step):
    """the first nev >= start (in steps of `step`) below which the full spectrum has a gap of more than 1e-6 scale"""
    E = np.linalg.eigvalsh(A)
    scale = max(np.max(np.abs(E)), 1e-300)
    nev = start
    while E[nev] - E[nev - 1] <= 1e-6 * scale:
        nev += step
    return nev


def aufbau_cases():
    deg = dict(hard_matrices())["degenerate_pairs"]
    yield "aufbau_degenerate_pairs", deg, aufbau_nev(deg, 8, 2)  # its levels come in equal pairs: an even count
    A = dense_matrix(130)
    yield "aufbau_random_130", A, aufbau_nev(A, 20, 1)


GEN_BASES = {
    # test_gpu_parity.py: CASES
    "sigma_only": (1, 1, 1.4, (4,), 2, 6),
    "sigma_pi": (7, 7, 2.068, (3, 2), 2, 5),
    "hetero_sigma_pi_delta": (3, 9, 2.955, (3, 3, 2), 3, 4),
}


def gen_problem(name):
    """(F, S, blocks) of a generalized, blocked problem"""
    if name == "small_odd_blocks":
        rng = np.random.RandomState(3)
        sizes = [1, 2, 3, 5, 31, 33]
        N = sum(sizes)
        perm = rng.permutation(N)
        blocks, o = [], 0
        for sz in sizes:
            blocks.append(np.sort(perm[o:o + sz]))
            o += sz
        A = rng.uniform(-1, 1, (N, N))
        S = A @ A.T + N * np.eye(N)
    else:
        import common
        Z1, Z2, R, lmmax, nelem, nnodes = GEN_BASES[name]
        gb, _ = common.make_bases(Z1, Z2, R, lmmax, nelem, nnodes, oracle=False)
        S = gb.overlap()
        blocks = [np.asarray(b) for b in gb.get_sym_idx(1)]
        N = S.shape[0]
        rng = np.random.RandomState(N)
    F = rng.uniform(-1, 1, (N, N))
    F = F + F.T
    mask = np.zeros((N, N), dtype=bool)
    for b in blocks:
        mask[np.ix_(b, b)] = True
    return np.where(mask, F, 0.0), np.where(mask, S, 0.0), blocks


def gen_cases():
    for name in sorted(GEN_BASES):
        _, _, blocks = gen_problem(name)
        for nev in sorted({1, 3, max(len(b) for b in blocks)}):
            yield "gen_%s_%d" % (name, nev), name, nev
    yield "gen_small_odd_blocks_2", "small_odd_blocks", 2


def sel_dev(F, X, blocks, nev):
    """hfg_eig_gsym_sub_sel_dev on device pointers"""
    import torch
    ctx = hf.default_context()
    dev = torch.device("cuda", 0)
    N = F.shape[0]
    K = hf.scf.eig_sel_count(blocks, nev)
    ptr, idx = hf.scf._blocks(blocks)
    Fd = torch.from_numpy(np.asfortranarray(F).ravel(order="F").copy()).to(dev)
    Xd = torch.from_numpy(np.asfortranarray(X).ravel(order="F").copy()).to(dev)
    Ed, Cd = torch.zeros(K, dtype=torch.float64, device=dev), torch.zeros(N * K, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    i64p = ctypes.POINTER(ctypes.c_int64)
    f = hf.lib().hfg_eig_gsym_sub_sel_dev
    f.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, i64p, i64p, ctypes.c_int64,
                  ctypes.c_void_p, ctypes.c_void_p]
    rc = f(ctx.h, N, Fd.data_ptr(), Xd.data_ptr(), len(blocks), ptr.ctypes.data_as(i64p), idx.ctypes.data_as(i64p), nev, Ed.data_ptr(),
           Cd.data_ptr())
    assert rc == 0, hf.lib().hfg_last_error()
    ctx.synchronize()
    return Ed.cpu().numpy(), Cd.cpu().numpy().reshape((N, K), order="F")


if __name__ == "__main__":
    out = {}
    for name, n, nev, kind in dense_cases():
        A = dense_matrix(n) if kind == "dense" else tridiag(*big_tridiag(n))
        out["E_" + name], out["C_" + name] = hf.scf.eig_sym_sel(A, nev)
    for name, A, nev in hard_cases():
        out["E_" + name], out["C_" + name] = hf.scf.eig_sym_sel(A, nev)
    for name, A, nev in aufbau_cases():
        out["E_" + name], out["C_" + name] = hf.scf.eig_sym_sel(A, nev)
        out["Efull_" + name], out["Cfull_" + name] = hf.scf.eig_sym(A)
    probs = {}
    for name, pname, nev in gen_cases():
        if pname not in probs:
            F, S, blocks = gen_problem(pname)
            probs[pname] = (F, S, blocks, hf.scf.form_Sinvh(S, False, blocks))
        F, S, blocks, X = probs[pname]
        out["E_" + name], out["C_" + name] = hf.scf.eig_gsym_sub_sel(F, X, blocks, nev)
        out["K_" + name] = np.array([hf.scf.eig_sel_count(blocks, nev)])
    F, S, blocks, X = probs["sigma_pi"]
    out["E_dev"], out["C_dev"] = sel_dev(F, X, blocks, 3)
    A = dense_matrix(REPEAT[0])
    out["E_repeat_a"], out["C_repeat_a"] = hf.scf.eig_sym_sel(A, REPEAT[1])
    out["E_repeat_b"], out["C_repeat_b"] = hf.scf.eig_sym_sel(A, REPEAT[1])
    np.savez(sys.argv[1], **out)
    print("ok")
