"""The device-resident DIIS object (hfg_diis_*, helfem_amd.DeviceDIIS) against a NumPy restatement in numpy.longdouble.

Data: random SPD S, X = S^{-1/2} from numpy.linalg.eigh (a rectangular Sinvh: n eigenvectors, X = U_n
diag(s_n^{-1/2})), random symmetric F_i, P_i = C_o C_o^T with C_o = X Q for random orthonormal Q.

Tolerances (none of them tuned to what the kernels give).  u = 2^-52 below is twice the unit roundoff, which leaves room
for either accumulation order of a fused multiply-add.

  error matrix   The issue's bound, c k u (product of the operands' max-abs norms), with the operands of the definition
                 err = X^T (F P S - S P F) X:  tol_err = c N u max|X|^2 max|F| max|P| max|S|.  k = N is the longest inner
                 dimension of any route's chain.  c counts the roundings that separate a route from the exact value: the
                 longest chain any route evaluates is X^T F C_o C_o^T S X, five products (F C_o, X^T(.), S C_o, X^T(.),
                 A B^T), one unit of k u each in the forward bound of a product chain (Higham, Accuracy and Stability,
                 section 3.5, first order); the two chains are subtracted (one more); and the dense route reads the float64
                 P where the low-rank route reads C_o (P = fl(C_o C_o^T), one more).  c = 5 + 1 + 1 = 7.
  max |err|      tol_err (the maximum moves by at most the largest elementwise error).
  B(i, j)        sum over spins of <e_i, e_j>, L = n^2 terms each: |dB| <= sum|e_i| tol_j + sum|e_j| tol_i + L tol_i tol_j
                 (errors of the factors) + L u sum|e_i e_j| (the summation, any order), times 2 for nspin = 1.
  T(i, j)        sum over spins of <P_i, F_j>, inputs exact: |dT| <= N^2 u sum|P_i F_j|, times 2 for nspin = 1.
  weights        the same host arithmetic (helfem::DiisMixer) on the same B, T, E: equal bit for bit.
  extrapolation  sum of h terms: |dF| <= (h + 1) u sum_j |w_j| |F_j|.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

U = 2.0 ** -52
LD = np.longdouble
LIMIT = 64  # DIIS_LR_MAXCOLS of hip/internal.h: more occupied columns take the dense route
ADIIS = dict(diiseps=1e-2, diisthr=1e-3)  # random matrices have errors far above both: pure ADIIS
CDIIS = dict(diiseps=1e12, diisthr=1e11)  # ... far below both: pure CDIIS


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    return helfem_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _weights(hf, B, T, E, maxerr, diiseps, diisthr, mode=0):
    L = hf.lib()
    dp = ctypes.POINTER(ctypes.c_double)
    L.hfg_diis_weights.argtypes = [ctypes.c_int, dp, dp, dp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, dp,
                                   ctypes.POINTER(ctypes.c_int)]
    n = len(E)
    B, T, E = (np.ascontiguousarray(a, dtype=np.float64) for a in (B, T, E))
    w = np.zeros(n)
    dr = ctypes.c_int()
    rc = L.hfg_diis_weights(n, B.ctypes.data_as(dp), T.ctypes.data_as(dp), E.ctypes.data_as(dp), float(maxerr), diiseps, diisthr, mode,
                            w.ctypes.data_as(dp), ctypes.byref(dr))
    assert rc == 0, L.hfg_last_error()
    return w, dr.value


class Problem(object):
    """S, X and a sequence of (E, F_s, P_s, C_s) entries; blocks: index lists that S, X, F and the orbitals respect"""

    def __init__(self, N, n, nocc, nspin, nentries, seed, blocks=None):
        rng = np.random.RandomState(seed)
        self.N, self.n, self.nocc, self.nspin, self.blocks = N, n, nocc, nspin, blocks
        mask = np.ones((N, N))
        if blocks is not None:
            bid = np.zeros(N, dtype=int)
            for ib, b in enumerate(blocks):
                bid[b] = ib
            mask = (bid[:, None] == bid[None, :]).astype(float)
        A = rng.randn(N, N) * mask
        self.S = A @ A.T / N + np.eye(N)
        if blocks is None:
            s, Uv = np.linalg.eigh(self.S)
            self.X = (Uv / np.sqrt(s))[:, N - n:]  # the n columns of the largest eigenvalues
        else:  # S^{-1/2} block by block: column j has its support on the block of basis function j
            assert n == N
            self.X = np.zeros((N, N))
            for b in blocks:
                s, Uv = np.linalg.eigh(self.S[np.ix_(b, b)])
                self.X[np.ix_(b, b)] = (Uv / np.sqrt(s)) @ Uv.T
        self.entries = []
        for it in range(nentries):
            Fs, Ps, Cs = [], [], []
            for sp in range(nspin):
                F = rng.randn(N, N) * mask
                F = 0.5 * (F + F.T)
                if blocks is None:
                    Q = np.linalg.qr(rng.randn(n, nocc))[0]
                else:  # every orbital lives in one block: orthonormal columns block by block
                    Q = np.zeros((n, nocc))
                    for ib, b in enumerate(blocks):
                        mine = list(range(ib, nocc, len(blocks)))
                        if mine:
                            Q[np.ix_(b, mine)] = np.linalg.qr(rng.randn(len(b), len(mine)))[0]
                C = self.X @ Q
                Fs.append(F)
                Cs.append(C)
                Ps.append(C @ C.T)
            self.entries.append((-1.0 - 0.01 * it, Fs, Ps, Cs))  # falling energies: no ADIIS cool-off

    def reference(self, it):
        """per spin: error matrix (longdouble) and its tolerance"""
        X, S = self.X.astype(LD), self.S.astype(LD)
        errs, tols = [], []
        for F, P, C in zip(*self.entries[it][1:]):
            M = F.astype(LD) @ P.astype(LD) @ S
            errs.append(X.T @ (M - M.T) @ X)
            amax = lambda M: float(np.max(np.abs(M)))
            tols.append(7 * self.N * U * amax(self.X) ** 2 * amax(F) * amax(P) * amax(self.S))
        return errs, tols


def dev(torch, M):
    return torch.from_numpy(np.asfortranarray(M).ravel(order="F").copy()).cuda()


def host(t, rows, cols):
    return t.cpu().numpy()[:rows * cols].reshape((rows, cols), order="F")


def make(hf, torch, pb, order, ctx=None, blocks=None, **kw):
    ctx = ctx or hf.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    d = hf.DeviceDIIS(ctx, pb.N, pb.nspin, order=order, **kw)
    d.set_metric(dev(torch, pb.S), dev(torch, pb.X))
    if blocks is not None:
        d.set_blocks(blocks)
    return d


def push(d, torch, pb, it, orbitals=True):
    E, Fs, Ps, Cs = pb.entries[it]
    a = [dev(torch, Fs[0]), dev(torch, Ps[0])] + ([dev(torch, Cs[0]), pb.nocc] if orbitals else [None, 0])
    if pb.nspin == 2:
        a += [dev(torch, Fs[1]), dev(torch, Ps[1])] + ([dev(torch, Cs[1]), pb.nocc] if orbitals else [None, 0])
    return d.update(E, *a)


# nocc = LIMIT + 1, the one value just above the low-rank kernel's column limit, needs nocc <= n and so exists at N = 130
# only: the dense routing through update() with orbitals given is exercised there (and without orbitals, at N = 37, in
# test_lowrank_dense_and_blocked_routes_agree)
CASES = [(N, n, nocc, nspin) for N in (37, 130) for n in (N, N - 3) for nocc in (1, 5, LIMIT + 1) if nocc <= n for nspin in (1, 2)]


@pytest.mark.parametrize("N,n,nocc,nspin", CASES, ids=["N%d-n%d-nocc%d-nspin%d" % c for c in CASES])
def test_five_pushes_into_a_ring_of_three(hf, torch, N, n, nocc, nspin):
    """error matrix, max |err|, B and T after every push; weights and extrapolated F after every solve"""
    order, mode = 3, (CDIIS if nocc == 5 else ADIIS)
    pb = Problem(N, n, nocc, nspin, 5, seed=1000 * N + 10 * nocc + nspin)
    d = make(hf, torch, pb, order, **mode)
    fac = 2.0 if nspin == 1 else 1.0
    kept = []  # (entry index, errors, tolerances) of the entries the object still holds, oldest first
    for it in range(5):
        if len(kept) == order:
            kept.pop(0)
        maxerr = push(d, torch, pb, it)
        errs, tols = pb.reference(it)
        kept.append((it, errs, tols))
        assert d.size == len(kept)
        got = d.error
        for sp in range(nspin):
            fig = float(np.max(np.abs(got[sp].astype(LD) - errs[sp])))
            print("push %d spin %d: error matrix off by %.3e (bound %.3e)" % (it, sp, fig, tols[sp]))
            assert fig <= tols[sp]
            if nocc <= LIMIT:
                assert np.array_equal(got[sp], -got[sp].T), "the low-rank kernel's error matrix is antisymmetric bit for bit"
        ref_max = max(float(np.max(np.abs(e))) for e in errs)
        assert abs(maxerr - ref_max) <= max(tols)
        assert maxerr == float(np.max(np.abs(got))), "max |err| is the maximum of the stored matrix"
        B, T = d.B, d.T
        for i, (ii, ei, ti) in enumerate(kept):
            for j, (jj, ej, tj) in enumerate(kept):
                Bref = tolB = Tref = tolT = LD(0)
                for sp in range(nspin):
                    Bref += np.sum(ei[sp] * ej[sp])
                    L = ei[sp].size
                    tolB += np.sum(np.abs(ei[sp])) * tj[sp] + np.sum(np.abs(ej[sp])) * ti[sp] + L * ti[sp] * tj[sp] + \
                        L * U * np.sum(np.abs(ei[sp] * ej[sp]))
                    Pi, Fj = pb.entries[ii][2][sp].astype(LD), pb.entries[jj][1][sp].astype(LD)
                    Tref += np.sum(Pi * Fj)
                    tolT += N * N * U * np.sum(np.abs(Pi * Fj))
                print("push %d B(%d,%d) off by %.3e (bound %.3e), T off by %.3e (bound %.3e)" %
                      (it, i, j, abs(B[i, j] - fac * Bref), fac * tolB, abs(T[i, j] - fac * Tref), fac * tolT))
                assert abs(B[i, j] - fac * Bref) <= fac * tolB, (it, i, j, B[i, j], fac * Bref, fac * tolB)
                assert abs(T[i, j] - fac * Tref) <= fac * tolT, (it, i, j, T[i, j], fac * Tref, fac * tolT)
        assert np.array_equal(B, B.T)
        # solve: the weights from the read-back B, T and E, the extrapolation from the test's own copies of F
        Es = [pb.entries[k[0]][0] for k in kept]
        wref, dref = _weights(hf, B, T, Es, maxerr, mode["diiseps"], mode["diisthr"])
        outs = [torch.zeros(N * N, dtype=torch.float64, device="cuda") for _ in range(nspin)]
        dropped = d.solve(*outs)
        assert dropped == dref
        kept = kept[dropped:]
        w = d.weights
        assert d.size == len(kept) and np.array_equal(w, wref[dropped:]), (w, wref)
        assert abs(np.sum(w) - 1.0) < 1e-12
        for sp in range(nspin):
            Fs = [pb.entries[k[0]][1][sp].astype(LD) for k in kept]
            ref = sum(LD(wj) * Fj for wj, Fj in zip(w, Fs))
            tol = (len(kept) + 1) * U * float(np.max(sum(abs(wj) * np.abs(Fj) for wj, Fj in zip(w, Fs))))
            assert float(np.max(np.abs(host(outs[sp], N, N).astype(LD) - ref))) <= tol


def _blocks37():
    perm = np.random.RandomState(7).permutation(37)
    return [sorted(perm[:20].tolist()), sorted(perm[20:31].tolist()), sorted(perm[31:].tolist())]


@pytest.mark.parametrize("nspin", [1, 2])
def test_lowrank_dense_and_blocked_routes_agree(hf, torch, nspin):
    """block-diagonal inputs, three blocks of 20, 11 and 6 interleaved functions: the four routes against the reference"""
    blocks = _blocks37()
    pb = Problem(37, 37, 5, nspin, 1, seed=42 + nspin, blocks=blocks)
    errs, tols = pb.reference(0)
    got = {}
    for name, blk, orb in (("lowrank", None, True), ("dense", None, False), ("lowrank-blocked", blocks, True), ("dense-blocked", blocks, False)):
        d = make(hf, torch, pb, 2, blocks=blk)
        maxerr = push(d, torch, pb, 0, orbitals=orb)
        got[name] = d.error
        for sp in range(nspin):
            fig = float(np.max(np.abs(got[name][sp].astype(LD) - errs[sp])))
            print("%s spin %d: off by %.3e (bound %.3e)" % (name, sp, fig, tols[sp]))
            assert fig <= tols[sp], name
        assert maxerr == float(np.max(np.abs(got[name])))
    for name in got:  # and so against each other within twice the bound
        assert float(np.max(np.abs(got[name] - got["lowrank"]))) <= 2 * max(tols)
    # the blocked routes leave the entries between the blocks exactly zero
    bid = np.zeros(37, dtype=int)
    for ib, b in enumerate(blocks):
        bid[b] = ib
    off = bid[:, None] != bid[None, :]
    assert not np.any(got["lowrank-blocked"][:, off]) and not np.any(got["dense-blocked"][:, off])


def test_blocks_refusals(hf, torch):
    pb = Problem(37, 34, 1, 1, 1, seed=3)
    d = make(hf, torch, pb, 2)
    with pytest.raises(RuntimeError, match="square Sinvh"):
        d.set_blocks(_blocks37())
    pb = Problem(37, 37, 1, 1, 1, seed=3)  # a dense Sinvh is not block structured
    d = make(hf, torch, pb, 2)
    with pytest.raises(RuntimeError, match="not block structured"):
        d.set_blocks(_blocks37())
    push(d, torch, pb, 0)
    with pytest.raises(RuntimeError, match="history is not empty"):
        d.set_blocks(None)


def test_one_spin_counts_twice(hf, torch):
    """nspin = 1 against nspin = 2 fed Fb = Fa, Pb = Pa: B and T within the bounds of the module docstring (the two sum
    their terms in different orders), the CDIIS weights within the first-order perturbation bound of the linear system
    B w = 1, |dw| <= 4 cond(B) |dB| / |B| (two for the solve, two for the normalisation)"""
    N, nocc = 37, 5
    p1 = Problem(N, N, nocc, 1, 3, seed=11)
    p2 = Problem(N, N, nocc, 2, 3, seed=11)
    p2.entries = [(E, [F[0], F[0]], [P[0], P[0]], [C[0], C[0]]) for E, F, P, C in p1.entries]
    d1, d2 = make(hf, torch, p1, 3, mode=1, **CDIIS), make(hf, torch, p2, 3, mode=1, **CDIIS)
    refs = []
    for it in range(3):
        push(d1, torch, p1, it)
        push(d2, torch, p2, it)
        refs.append(p1.reference(it))
    B1, B2, T1, T2 = d1.B, d2.B, d1.T, d2.T
    tolB = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            (ei,), (ti,) = refs[i]
            (ej,), (tj,) = refs[j]
            L = ei.size
            tolB[i, j] = 2 * float(np.sum(np.abs(ei)) * tj + np.sum(np.abs(ej)) * ti + L * ti * tj + L * U * np.sum(np.abs(ei * ej)))
            tolT = 2 * N * N * U * float(np.sum(np.abs(p1.entries[i][2][0] * p1.entries[j][1][0])))
            assert abs(B1[i, j] - B2[i, j]) <= 2 * tolB[i, j] and abs(T1[i, j] - T2[i, j]) <= 2 * tolT
    F1, F2a, F2b = (torch.zeros(N * N, dtype=torch.float64, device="cuda") for _ in range(3))
    assert d1.solve(F1) == d2.solve(F2a, F2b)
    tolw = 4 * np.linalg.cond(B1) * np.linalg.norm(2 * tolB, 2) / np.linalg.norm(B1, 2)
    print("weights differ by %.3e (bound %.3e)" % (np.max(np.abs(d1.weights - d2.weights)), tolw))
    assert np.max(np.abs(d1.weights - d2.weights)) <= tolw
    assert torch.equal(F2a, F2b)


@pytest.mark.parametrize("orbitals,blocked", [(True, False), (False, False), (True, True)])
def test_two_contexts_give_the_same_bits(hf, torch, orbitals, blocked):
    blocks = _blocks37() if blocked else None
    pb = Problem(37, 37, 5, 2, 4, seed=5, blocks=blocks)
    out = []
    for _ in range(2):
        d = make(hf, torch, pb, 3, ctx=hf.Context(0), blocks=blocks)  # a context with a stream of its own
        Fa, Fb = (torch.zeros(37 * 37, dtype=torch.float64, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        rec = []
        for it in range(4):
            push(d, torch, pb, it, orbitals=orbitals)
            d.solve(Fa, Fb)
            d.ctx.synchronize()
            rec += [d.B.copy(), d.T.copy(), d.weights.copy(), Fa.cpu().numpy(), Fb.cpu().numpy()]
        out.append(rec)
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_stream_order_and_the_ring_owning_its_copies(hf, torch):
    """the object on a non-default torch stream.  update: the inputs arrive by copies enqueued right before the call, behind
    a long-running delay, and are overwritten right after it; solve: its output is consumed by a torch copy with no
    synchronisation in between and then overwritten.  The later solve also shows that the ring holds copies: F and P of
    every entry have been overwritten by then."""
    import stream_order_worker as sow
    N, nocc = 130, 5
    pb = Problem(N, N, nocc, 2, 3, seed=77)
    base = make(hf, torch, pb, 3)
    for it in range(3):
        push(base, torch, pb, it)
    Fr = [torch.zeros(N * N, dtype=torch.float64, device="cuda") for _ in range(2)]
    base.solve(*Fr)
    torch.cuda.synchronize()
    Bref, Tref, wref = base.B, base.T, base.weights
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        delay = sow.Delay(torch)
        d = make(hf, torch, pb, 3, ctx=hf.Context(0, stream=s.cuda_stream))
        true = [[dev(torch, M[sp]) for M in pb.entries[it][1:] for sp in range(2)] for it in range(3)]  # Fa Fb Pa Pb Ca Cb
        work = [torch.empty_like(t) for t in true[0]]
        decoy = [torch.full_like(t, 0.37) for t in true[0]]
        res = [torch.empty_like(f) for f in Fr]
        out = [torch.zeros(N * N, dtype=torch.float64, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for it in range(3):
            if it == 2:
                e0.record()
            delay.run()
            if it == 2:
                e1.record()
            for w, t in zip(work, true[it]):
                w.copy_(t)
            d.update(pb.entries[it][0], work[0], work[2], work[4], nocc, work[1], work[3], work[5], nocc)
            for w, t in zip(work, decoy):
                w.copy_(t)
        delay.run()
        d.solve(*out)
        for r, o in zip(res, out):
            r.copy_(o)
        for o in out:
            o.fill_(0.37)
        torch.cuda.synchronize()
        assert e0.elapsed_time(e1) >= sow.DELAY_MIN_MS, "the delay is too short for the run to mean anything"
    assert np.array_equal(d.B, Bref) and np.array_equal(d.T, Tref) and np.array_equal(d.weights, wref)
    for r, f in zip(res, Fr):
        assert torch.equal(r, f)
