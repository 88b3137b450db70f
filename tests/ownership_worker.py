"""Worker of test_gpu_ownership.py: workspaces live in their context or table set and die with it.  One thread, no
concurrency; every result goes into OUT.npz and the test compares.  Usage: ownership_worker.py all|sel OUT.npz

  all  context lifetime (A, destroyed, then B: often at A's address), two live contexts interleaved, table-set lifetime
       (re-upload, a new basis after the old one is destroyed, the erfc table set of an atomic basis)
  sel  context lifetime of the selected solve (run with HELFEM_EIGSEL=stein: the fifth workspace of a context)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helfem_amd as hf  # noqa: E402

N_SMALL, N_PERSISTENT, N_OTHER = 70, 300, 333  # below the compact-WY and persistent thresholds; persistent; another tile shape
BLOCK_SIZES = (50, 121, 187)
SEL = (300, 5)
DIATOMIC = (1, 1, 1.4, (4,), 2, 6)    # test_gpu_parity.py: CASES["sigma_only"], the smallest there
DIATOMIC_2 = (1, 1, 1.4, (4,), 2, 5)  # the same with another number of nodes
ATOMIC = (2, 0, 0, 3, 6)              # test_gpu_rs.py: RS_CASES["s_only"], the smallest there
OMEGA = 0.4
PBE = (101, 130)


def dense_matrix(n):
    """the matrices of test_gpu_parity.py::test_eig_sym_vs_lapack"""
    rng = np.random.RandomState(n)
    A = rng.uniform(-1, 1, size=(n, n))
    return A + A.T + np.diag(np.linspace(0, 50.0, n))


def block_problem():
    """(F, S, blocks): three symmetry blocks of unequal order, scattered over the index range"""
    rng = np.random.RandomState(7)
    N = sum(BLOCK_SIZES)
    perm = rng.permutation(N)
    blocks, o = [], 0
    for sz in BLOCK_SIZES:
        blocks.append(np.sort(perm[o:o + sz]))
        o += sz
    A = rng.uniform(-1, 1, (N, N))
    S = A @ A.T + N * np.eye(N)
    F = rng.uniform(-1, 1, (N, N))
    F = F + F.T
    mask = np.zeros((N, N), dtype=bool)
    for b in blocks:
        mask[np.ix_(b, b)] = True
    return np.where(mask, F, 0.0), np.where(mask, S, 0.0), blocks


def diatomic_ldft_mdft(case):
    lmmax = case[3]
    return 4 * max(lmmax) + 12, 4 * len(lmmax) + 5


def diatomic_density(gb):
    import common
    return common.random_density(gb.Nbf(), 2, seed=12, blocks=gb.get_sym_idx(1))  # test_gpu_parity.py: "m_blocked"


def atomic_density(gb):
    import common
    return common.random_density(gb.Nbf(), 3, seed=11)  # test_gpu_rs.py: "general"


def context_lifetime(out, calls):
    """calls(ctx) -> dict of arrays; on context A, then, A destroyed, on a new context B"""
    a = hf.Context(0)
    addr_a = a.h.value
    for k, v in calls(a).items():
        out["a_" + k] = v
    a.close()
    b = hf.Context(0)
    print("context B %s context A's address" % ("has" if b.h.value == addr_a else "does not have"))
    for k, v in calls(b).items():
        out["b_" + k] = v
    b.close()


def full_calls(ctx):
    r = {}
    for n in (N_SMALL, N_PERSISTENT):
        r["E%d" % n], r["C%d" % n] = hf.scf.eig_sym(dense_matrix(n), ctx)
    F, S, blocks = block_problem()
    X = hf.scf.form_Sinvh(S, False, blocks, ctx)
    r["Eg"], r["Cg"] = hf.scf.eig_gsym_sub(F, X, blocks, ctx)
    return r


def sel_calls(ctx):
    r = {}
    r["Esel"], r["Csel"] = hf.scf.eig_sym_sel(dense_matrix(SEL[0]), SEL[1], ctx)
    r["E%d" % N_SMALL], r["C%d" % N_SMALL] = hf.scf.eig_sym(dense_matrix(N_SMALL), ctx)
    return r


def interleaved(out):
    a, b = hf.Context(0), hf.Context(0)
    M1, M2 = dense_matrix(N_PERSISTENT), dense_matrix(N_OTHER)
    out["i_E1"], out["i_C1"] = hf.scf.eig_sym(M1, a)
    out["i_E2"], out["i_C2"] = hf.scf.eig_sym(M2, b)
    out["i_E1again"], out["i_C1again"] = hf.scf.eig_sym(M1, a)
    a.close()
    b.close()


def fock_parts(gb, ldft, mdft):
    P = diatomic_density(gb)
    J, K = gb.coulomb(P), gb.exchange(P)
    os.environ["HELFEM_EXCHANGE"] = "general"  # a live switch: read at every call
    try:
        Kgen = gb.exchange(P)
    finally:
        del os.environ["HELFEM_EXCHANGE"]
    H = hf.DFTGrid(gb, ldft, mdft).eval_Fxc(PBE[0], PBE[1], P)[0]
    return dict(J=J, K=K, Kgen=Kgen, H=H)


def table_lifetime(out):
    import common
    ctx = hf.Context(0)
    gb, _ = common.make_bases(*DIATOMIC, oracle=False)
    gb.compute_tei(True)
    ldft, mdft = diatomic_ldft_mdft(DIATOMIC)
    gb.upload(ldft, mdft, ctx=ctx)
    for k, v in fock_parts(gb, ldft, mdft).items():
        out["t1_" + k] = v
    gb.upload(ldft, mdft)  # the table set and its three workspaces are rebuilt
    for k, v in fock_parts(gb, ldft, mdft).items():
        out["t2_" + k] = v
    del gb  # hfg_basis_destroy
    gb, _ = common.make_bases(*DIATOMIC_2, oracle=False)
    gb.compute_tei(True)
    gb.upload(*diatomic_ldft_mdft(DIATOMIC_2), ctx=ctx)
    P = diatomic_density(gb)
    out["t3_J"], out["t3_K"] = gb.coulomb(P), gb.exchange(P)
    del gb
    # the second table set (dev_rs) of an atomic basis: erfc tables
    ga, _ = common.make_atomic_bases(*ATOMIC, oracle=False)
    ga.compute_tei(True)
    ga.compute_erfc(OMEGA)
    ga.upload(ctx=ctx)
    P = atomic_density(ga)
    out["r1_K"] = ga.rs_exchange(P)
    ga.upload()
    out["r2_K"] = ga.rs_exchange(P)
    out["r2_Kfull"] = ga.exchange(P)
    del ga
    ctx.close()


if __name__ == "__main__":
    mode, path = sys.argv[1], sys.argv[2]
    out = {}
    if mode == "all":
        context_lifetime(out, full_calls)
        interleaved(out)
        table_lifetime(out)
    elif mode == "sel":
        context_lifetime(out, sel_calls)
    else:
        raise SystemExit("unknown mode " + mode)
    np.savez(path, **out)
    print("ok")
