"""The CUHF form of ROHF (scf::ROHF_update, scf_helpers.cpp:470-523) stated twice in NumPy, for tests/test_rohf_cpu.py,
tests/test_gpu_cuhf.py and their workers.

  dense_longdouble   the reference's sequence in numpy.longdouble: P in an orthonormal basis, its natural orbitals, Delta in
                     the natural-orbital basis, the core-virtual blocks back in the AO basis.  NumPy has no longdouble
                     eigensolver and the update needs none: lambda depends on the core, active and virtual SUBSPACES only.
                     The float64 eigenvectors are orthonormalised in longdouble (one Newton step) and the three subspaces
                     decoupled by one first-order rotation K_ij = M_ij / (d_j - d_i) between clusters, M = V^T Porth V
                     (quadratically convergent: the float64 vectors are already good to 1e-16 and the occupation gaps are
                     at least 0.1); the residual coupling is returned and asserted by the callers.  The orthonormal basis is
                     the Cholesky one, Sh = L, Sinvh = L^-T (Sh^T Sinvh = 1, Sh Sh^T = S): lambda does not depend on it.
  dense_float64      the same sequence in float64 with NumPy's eigh and the symmetric S^(1/2), as the oracle's cuhf_update
                     and the device driver evaluate it: the yardstick of the error bound
  lowrank            the rank-(na + nb) form of hip/cuhf_dev.hip from the occupied orbitals: G = C^T S C = R L R^T,
                     Y = C R L^(-1/2), T = S Y, lambda = -(B + B^T), B = T_c [A - (A Y_w) T_w^T], A = Y_c^T Delta

Matrices are plain two-dimensional NumPy arrays.  bound() is the issue's: ten times the error of dense_float64 against
dense_longdouble on the same inputs, with the floor N eps max|lambda_ref| of a dot product of length N."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52

# N, (na, nb): the issue's shapes; r = na + nb > 128 takes the dense route on the device
SHAPES = [(61, (2, 1)), (61, (3, 0)), (130, (1, 3)), (130, (5, 2)), (257, (4, 1)), (257, (40, 33)), (200, (70, 60))]


def problem(N, na, nb, seed):
    """S (random SPD, condition about 5), S-orthonormal occupied orbitals per spin -- the smaller set a perturbed rotation of
    a subset of the larger, so that the natural occupations are close to 2, 1 and 0 -- and random symmetric Fa, Fb"""
    rng = np.random.RandomState(seed)
    A = rng.randn(N, N)
    S = A @ A.T / N + np.eye(N)
    s, U = np.linalg.eigh(S)
    X = (U / np.sqrt(s)) @ U.T
    nbig, nsmall = max(na, nb), min(na, nb)
    Qbig = np.linalg.qr(rng.randn(N, nbig))[0]
    Qsmall = np.zeros((N, 0))
    if nsmall:
        subset = rng.choice(nbig, nsmall, replace=False)
        rot = np.linalg.qr(rng.randn(nsmall, nsmall))[0]
        Qsmall = np.linalg.qr(Qbig[:, subset] @ rot + 0.3 * rng.randn(N, nsmall) / np.sqrt(N))[0]
    Cbig, Csmall = X @ Qbig, X @ Qsmall
    Ca, Cb = (Cbig, Csmall) if na >= nb else (Csmall, Cbig)
    Fa, Fb = rng.randn(N, N), rng.randn(N, N)
    return dict(N=N, na=na, nb=nb, S=S, Ca=Ca, Cb=Cb, Fa=0.5 * (Fa + Fa.T), Fb=0.5 * (Fb + Fb.T))


def occupations(pb):
    """non-zero natural occupations of Pa + Pb, descending: the eigenvalues of C^T S C"""
    C = np.hstack([pb["Ca"], pb["Cb"]])
    return np.linalg.eigvalsh(C.T @ pb["S"] @ C)[::-1]


def boundary_gaps(pb):
    """occupation gaps at the core / active and the active / virtual boundary"""
    lam = np.concatenate([occupations(pb), np.zeros(1)])  # (the virtual space of an N > r problem holds exact zeros)
    Nc, Nw = min(pb["na"], pb["nb"]), max(pb["na"], pb["nb"])
    return lam[Nc - 1] - lam[Nc], lam[Nw - 1] - lam[Nw]


def _cholesky_ld(S):
    N = S.shape[0]
    L = np.zeros((N, N), dtype=LD)
    for j in range(N):
        d = S[j, j] - np.dot(L[j, :j], L[j, :j])
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _lower_inverse_ld(L):
    N = L.shape[0]
    X = np.zeros((N, N), dtype=LD)
    for i in range(N):  # row i of L X = 1
        X[i, :] = -(L[i, :i] @ X[:i, :])
        X[i, i] += LD(1)
        X[i, :] /= L[i, i]
    return X


def dense_longdouble(pb):
    """lambda (longdouble) and the residual coupling between the subspaces, relative to the largest occupation"""
    N, na, nb = pb["N"], pb["na"], pb["nb"]
    Nc, Nw = min(na, nb), max(na, nb)
    if Nc == 0 or na == nb:
        return np.zeros((N, N), dtype=LD), 0.0
    S, Ca, Cb = pb["S"].astype(LD), pb["Ca"].astype(LD), pb["Cb"].astype(LD)
    P = Ca @ Ca.T + Cb @ Cb.T
    L = _cholesky_ld(S)
    Linv = _lower_inverse_ld(L)
    Porth = L.T @ P @ L
    V = np.linalg.eigh(Porth.astype(np.float64))[1].astype(LD)  # ascending: virtual, active, core
    one = np.eye(N, dtype=LD)
    V = V @ (3 * one - V.T @ V) / 2
    cluster = np.zeros(N, dtype=int)
    cluster[N - Nw:] = 1
    cluster[N - Nc:] = 2
    cross = cluster[:, None] != cluster[None, :]
    M = V.T @ Porth @ V
    d = np.diag(M)
    den = np.where(cross, d[None, :] - d[:, None], LD(1))
    V = V @ (one + np.where(cross, M / den, LD(0)))
    V = V @ (3 * one - V.T @ V) / 2
    M = V.T @ Porth @ V
    residual = float(np.max(np.abs(np.where(cross, M, LD(0)))) / np.max(np.abs(d)))
    Y, T = Linv.T @ V, L @ V  # AO_to_NO and the transpose of NO_to_AO
    Delta = (pb["Fa"].astype(LD) - pb["Fb"].astype(LD)) / 2
    Yc, Tc, Yv, Tv = Y[:, N - Nc:], T[:, N - Nc:], Y[:, :N - Nw], T[:, :N - Nw]
    B = Tc @ (Yc.T @ Delta @ Yv) @ Tv.T
    return -(B + B.T), residual


def dense_float64(pb):
    """lambda as the oracle's cuhf_update evaluates it, with the AO coefficients of the core and the virtual natural orbitals"""
    N, na, nb = pb["N"], pb["na"], pb["nb"]
    Nc, Nw = min(na, nb), max(na, nb)
    s, U = np.linalg.eigh(pb["S"])
    Sh, Sinvh = (U * np.sqrt(s)) @ U.T, (U / np.sqrt(s)) @ U.T
    P = pb["Ca"] @ pb["Ca"].T + pb["Cb"] @ pb["Cb"].T
    Pv = np.linalg.eigh(Sh.T @ P @ Sh)[1][:, ::-1]  # descending: core first, virtual last
    AO_to_NO, NO_to_AO = Sinvh @ Pv, (Sh @ Pv).T
    Delta = 0.5 * (pb["Fa"] - pb["Fb"])
    Dno = AO_to_NO.T @ Delta @ AO_to_NO
    lam = np.zeros((N, N))
    if Nc and na != nb:
        lam[:Nc, Nw:] = -Dno[:Nc, Nw:]
        lam[Nw:, :Nc] = -Dno[Nw:, :Nc]
    return NO_to_AO.T @ lam @ NO_to_AO, AO_to_NO[:, :Nc], AO_to_NO[:, Nw:]


def lowrank(pb):
    """lambda from the occupied orbitals, float64"""
    N, na, nb = pb["N"], pb["na"], pb["nb"]
    Nc, Nw = min(na, nb), max(na, nb)
    if Nc == 0 or na == nb:
        return np.zeros((N, N))
    C = np.hstack([pb["Ca"], pb["Cb"]])
    SC = pb["S"] @ C
    lam, R = np.linalg.eigh(C.T @ SC)
    Q = R[:, ::-1][:, :Nw] / np.sqrt(lam[::-1][:Nw])
    Y, T = C @ Q, SC @ Q
    A = Y[:, :Nc].T @ (0.5 * (pb["Fa"] - pb["Fb"]))
    A = A - (A @ Y) @ T.T
    B = T[:, :Nc] @ A
    return -(B + B.T)


def bound(pb, ref, lam64):
    """(bound, error of the float64 dense evaluation, floor)"""
    e64 = float(np.max(np.abs(lam64.astype(LD) - ref)))
    floor = pb["N"] * EPS * float(np.max(np.abs(ref)))
    return max(10.0 * e64, floor), e64, floor


_cache = {}


def case(N, na, nb):
    """the problem of one shape with its references, computed once per process: dict with pb, ref (longdouble), residual,
    lam64, Yc, Yv, bound, e64, floor"""
    key = (N, na, nb)
    if key not in _cache:
        pb = problem(N, na, nb, seed=1000 * N + 10 * na + nb)
        ref, residual = dense_longdouble(pb)
        lam64, Yc, Yv = dense_float64(pb)
        b, e64, floor = bound(pb, ref, lam64)
        _cache[key] = dict(pb=pb, ref=ref, residual=residual, lam64=lam64, Yc=Yc, Yv=Yv, bound=b, e64=e64, floor=floor)
    return _cache[key]
