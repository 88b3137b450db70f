"""The banded F X of the blocked eigensolve (hfg_ctx_declare_fock_band, HELFEM_EIG_BAND): with the radial-element pattern of
F = H0 + J + XC declared, the rows of every block of F are taken radial-major inside the eigensolve and F X runs as row-tile
tasks over the k steps that meet their non-zero columns.  HELFEM_EIG_BAND=0 (read at every call) ignores the declaration:
the dense task.

Bases: bench.py's n2_pbe_small (3 elements of 8 nodes, blocks of 120 / 147 / 120: two and three row tiles) and the same with
5 elements (blocks of 204 / 245 / 204: row tiles inside one element and tiles that contain a shared node both occur).  F is
the PBE Fock matrix of the core-guess density.

Tolerances.  Eigenvalues: 1e-10, as the existing eigensolver tests.  P = C_occ C_occ^T and the generalized residual
max |F C - S C diag(E)|: the dense path's own distance from a NumPy eigh reference, measured in the same test, times 4,
with the floors below where that distance is at rounding level; the residual also against the backward-error scale
10 N eps |F| (the spectra reach 3e4).  Measured on MI355X, dense path against NumPy, restricted entry:
    3 elements:  |P - P_ref| 8.1e-13,  residual 2.7e-10,  |E - E_ref| 3.6e-12
    5 elements:  |P - P_ref| 3.7e-12,  residual 1.8e-09,  |E - E_ref| 2.8e-11
    pair (beta, core Hamiltonian): |P - P_ref| 1.8e-12 and 2.5e-12, residual 6.9e-10 and 1.3e-09; selected entry (nev = 5):
    residual 4.5e-11 and 4.2e-11
The banded path sits at the same distances because it gives the same bits: the columns keep the caller's order and the
skipped terms are exact zeros, so beyond the tolerances every test asserts E and C equal to the dense path's (difference 0
in every entry measured), and run() reaches -132.680117455144 (3 elements, 14 iterations) and -132.680310323255 (5, 13)
either way.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SWITCH = "HELFEM_EIG_BAND"
I64P = ctypes.POINTER(ctypes.c_int64)
P_FLOOR = 1e-14      # a few ulp of P's largest entries (order 1): below it "four times the dense path" means nothing
RESID_FLOOR = 1e-12  # likewise for the residual, whose terms are of the order of the largest eigenvalue times an entry of C


class band(object):
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        os.environ[SWITCH] = "1" if self.on else "0"

    def __exit__(self, *a):
        os.environ.pop(SWITCH, None)


def make_step(hf, name, nelem=None, cls=None, nocc=None):
    import bench
    w = dict(bench.WORKLOADS[name])
    if nelem:
        w["nelem"] = nelem
    basis, _, _, _, ldft, mdft = bench.build_basis(hf, w)
    basis.compute_tei(w.get("kfrac", 0.0) != 0.0)
    step = (cls or hf.DeviceSCFStep)(basis, w["x"], w["c"], ldft, mdft, nocc or w["nocc"], symmetry=1, device=0, kfrac=w.get("kfrac", 0.0))
    S = basis.overlap()
    H0 = basis.kinetic() + basis.nuclear()
    Sinvh = hf.scf.form_Sinvh(S, False, step.blocks, ctx=step.ctx)
    return dict(w=w, basis=basis, step=step, S=S, H0=H0, Sinvh=Sinvh)


@pytest.fixture(scope="module")
def gpu(native_libs):
    import torch
    import helfem_amd as hf
    return hf, torch


@pytest.fixture(scope="module", params=[3, 5], ids=["3elem", "5elem"])
def pbe(gpu, request):
    """the step with its matrices set, F = the PBE Fock matrix of the core guess, and the NumPy reference: computed once"""
    hf, torch = gpu
    d = make_step(hf, "n2_pbe_small", nelem=request.param)
    step, w = d["step"], d["w"]
    step.set_matrices(d["H0"], d["Sinvh"])
    assert step.ctx.fock_band_state() == "declared"
    E0, C0 = hf.scf.eig_gsym_sub(d["H0"], d["Sinvh"], step.blocks, ctx=step.ctx)
    d["P0"], d["C0"] = 2.0 * hf.scf.form_density(C0, w["nocc"], ctx=step.ctx), C0
    step.set_density(d["P0"], C0)
    step.fock_partial()
    step.fock_finish()
    torch.cuda.synchronize()
    N = step.N
    F = step.F.cpu().numpy().reshape(N, N, order="F").copy()
    d["F"], d["Fdev"] = F, step.F.clone()
    X = d["Sinvh"]
    Eref, V = np.linalg.eigh(X.T @ F @ X)
    d["Eref"], d["Pref"] = Eref, (X @ V[:, :w["nocc"]]) @ (X @ V[:, :w["nocc"]]).T
    Eh, Vh = np.linalg.eigh(X.T @ d["H0"] @ X)
    # (the core Hamiltonian's lowest nocc orbitals may end inside a degenerate pi pair, where P is not defined: the largest
    # count up to nocc that ends at a gap)
    nh = max(k for k in range(1, w["nocc"] + 1) if Eh[k] - Eh[k - 1] > 1e-6)
    d["nocc_h"], d["Eref_h"], d["Pref_h"] = nh, Eh, (X @ Vh[:, :nh]) @ (X @ Vh[:, :nh]).T
    return d


def figures(d, F, E, C, Eref, Pref, nocc):
    S = d["S"]
    K = len(E)
    return dict(E=float(np.max(np.abs(E - Eref[:K]))) if Eref is not None else 0.0,
                resid=float(np.max(np.abs(F @ C - S @ C * E[None, :]))),
                P=float(np.max(np.abs(C[:, :nocc] @ C[:, :nocc].T - Pref))))


def compare(name, d, F, Eref, Pref, on, off, nocc, fnorm=None):
    (E1, C1), (E0, C0) = on, off
    f1, f0 = figures(d, F, E1, C1, Eref, Pref, nocc), figures(d, F, E0, C0, Eref, Pref, nocc)
    dE = float(np.max(np.abs(E1 - E0)))
    print("%s: max |E_band - E_dense| %.2e; dense %s; banded %s" % (name, dE, f0, f1))
    assert dE < 1e-10 and f1["E"] < 1e-10 and f0["E"] < 1e-10
    # beside the dense path's own figure, the backward-error scale of a symmetric eigensolver, c n eps |F| with c = 10 (LAPACK's
    # own test ratios allow more): the spectra here reach 3e4, so an absolute figure taken from other matrices says nothing
    # (|F| in the orthonormal basis = its largest eigenvalue in magnitude, of the whole spectrum also where few pairs are asked for)
    scale = 10.0 * F.shape[0] * np.finfo(float).eps * float(np.max(np.abs(d["Eref"] if fnorm is None else fnorm)))
    assert f1["resid"] <= 4.0 * max(f0["resid"], RESID_FLOOR) and f1["resid"] < scale
    assert f1["P"] <= 4.0 * max(f0["P"], P_FLOOR)
    assert np.all(np.diff(E1) >= 0)
    # more than the tolerances ask: the columns keep their order and the skipped terms are exact zeros
    assert np.array_equal(E1, E0) and np.array_equal(C1, C0)


def band_nodes(hf, step, w):
    """radial node of every basis function: the pure basis is shell-major, nodes 0 ... R - 1 per shell, without node 0 in the
    shells with m != 0 (the boundary condition on the axis)"""
    _, mval = hf.lm_to_l_m(w["lmmax"])
    R = step.basis.Nrad()
    nodes = np.concatenate([np.arange(1 if m != 0 else 0, R) for m in mval]).astype(np.int32)
    assert len(nodes) == step.N
    return nodes


def test_plan_of_these_bases_has_partial_ranges(gpu, pbe):
    """the comparison means something: every block of both bases takes row tasks with ranges shorter than the block, and with
    5 elements row tiles inside one element and tiles that contain a shared node both occur"""
    hf, _ = gpu
    step, w = pbe["step"], pbe["w"]
    E, pm = w["nelem"], w["nnodes"] - 1
    assert step.basis.Nrad() == E * pm
    nodes = band_nodes(hf, step, w)
    kinds = set()
    for b in step.blocks:
        perm, steps, banded = hf.eig_band_plan(nodes[b], pm, E)
        assert banded and len(steps) >= 2 and any(len(ks) < (len(b) + 15) // 16 for ks in steps)
        snode = nodes[b][perm]
        for t in range(len(steps)):
            rows = snode[64 * t:64 * (t + 1)]
            kinds.add(bool(np.any((rows % pm == 0) & (rows > 0))))
    if E == 5:
        assert kinds == {True, False}


def test_restricted_entry(gpu, pbe):
    hf, torch = gpu
    step, nocc = pbe["step"], pbe["w"]["nocc"]
    N = step.N

    def solve(on):
        with band(on):
            step.F.copy_(pbe["Fdev"])
            step.E.fill_(float("nan"))
            step.C.fill_(float("nan"))
            step.eig_whole()
            torch.cuda.synchronize()
        return step.E.cpu().numpy().copy(), step.C.cpu().numpy().reshape(N, N, order="F").copy()

    on, off, again = solve(True), solve(False), solve(True)
    assert np.array_equal(on[0], again[0]) and np.array_equal(on[1], again[1])  # the order change and back repeats bitwise
    compare("restricted", pbe, pbe["F"], pbe["Eref"], pbe["Pref"], on, off, nocc)


def test_two_phase_entry(gpu, pbe):
    """block slots, then hfg_eig_assemble_dev: the row tasks feed the slot path as they feed the one-call entry"""
    hf, torch = gpu
    step, nocc = pbe["step"], pbe["w"]["nocc"]
    N = step.N

    def solve(on):
        with band(on):
            step.F.copy_(pbe["Fdev"])
            step.E.fill_(float("nan"))
            step.C.fill_(float("nan"))
            step.eig_partial()
            step.eig_finish()
            torch.cuda.synchronize()
        return step.E.cpu().numpy().copy(), step.C.cpu().numpy().reshape(N, N, order="F").copy()

    compare("two-phase", pbe, pbe["F"], pbe["Eref"], pbe["Pref"], solve(True), solve(False), nocc)


def test_pair_entry(gpu, pbe):
    """both spins in one batch: the PBE Fock matrix and the core Hamiltonian, both inside the pattern"""
    hf, torch = gpu
    step, nocc = pbe["step"], pbe["w"]["nocc"]
    N = step.N
    dev = step.dev
    Fa, Fb = pbe["Fdev"], step.H0
    out = [torch.empty(n, dtype=torch.float64, device=dev) for n in (N, N * N, N, N * N)]
    f = hf.lib().hfg_eig_gsym_sub_pair_devptr

    def solve(on):
        with band(on):
            for t in out:
                t.fill_(float("nan"))
            rc = f(step.ctx.h, ctypes.c_int64(N), step._ptr(Fa), step._ptr(Fb), step._ptr(step.Sinvh), len(step.blocks),
                   step.blk_ptr.ctypes.data_as(I64P), step.blk_idx.ctypes.data_as(I64P), *[step._ptr(t) for t in out])
            assert rc == 0, hf.lib().hfg_last_error()
            torch.cuda.synchronize()
        Ea, Ca, Eb, Cb = [t.cpu().numpy().copy() for t in out]
        return (Ea, Ca.reshape(N, N, order="F")), (Eb, Cb.reshape(N, N, order="F"))

    on, off = solve(True), solve(False)
    compare("pair, alpha", pbe, pbe["F"], pbe["Eref"], pbe["Pref"], on[0], off[0], nocc)
    compare("pair, beta", pbe, pbe["H0"], pbe["Eref_h"], pbe["Pref_h"], on[1], off[1], pbe["nocc_h"], fnorm=pbe["Eref_h"])


def test_selected_entry(gpu, pbe):
    """the lowest nev pairs of every block: nev = 5 holds the 7 occupied orbitals of N2 (5 sigma, one pi pair)"""
    hf, torch = gpu
    step, nocc = pbe["step"], pbe["w"]["nocc"]
    N, nev = step.N, 5
    K = int(hf.lib().hfg_eig_sel_count(len(step.blocks), step.blk_ptr.ctypes.data_as(I64P), ctypes.c_int64(nev)))
    Ed = torch.empty(K, dtype=torch.float64, device=step.dev)
    Cd = torch.empty(N * K, dtype=torch.float64, device=step.dev)
    f = hf.lib().hfg_eig_gsym_sub_sel_dev

    def solve(on):
        with band(on):
            Ed.fill_(float("nan"))
            Cd.fill_(float("nan"))
            rc = f(step.ctx.h, ctypes.c_int64(N), step._ptr(pbe["Fdev"]), step._ptr(step.Sinvh), len(step.blocks),
                   step.blk_ptr.ctypes.data_as(I64P), step.blk_idx.ctypes.data_as(I64P), ctypes.c_int64(nev), step._ptr(Ed), step._ptr(Cd))
            assert rc == 0, hf.lib().hfg_last_error()
            torch.cuda.synchronize()
        return Ed.cpu().numpy().copy(), Cd.cpu().numpy().reshape(N, K, order="F").copy()

    on, off = solve(True), solve(False)
    assert np.max(np.abs(on[0][:nocc] - pbe["Eref"][:nocc])) < 1e-10  # the occupied ones are the lowest of the whole spectrum
    compare("selected", pbe, pbe["F"], None, pbe["Pref"], on, off, nocc)


def _one_step(torch, step, P0, C0, on):
    with band(on):
        for t in (step.E, step.C, step.F):  # outputs of the step, poisoned BEFORE the inputs go in: the exact exchange
            t.fill_(float("nan"))           # reads the occupied columns that set_density stores in C
        step.set_density(P0, C0)
        step.step()
        torch.cuda.synchronize()
    return {k: getattr(step, k).cpu().numpy().copy() for k in ("E", "C", "P", "F", "scal")}


def test_pbe0_makes_no_declaration(gpu):
    hf, torch = gpu
    d = make_step(hf, "n2_pbe0_small")
    step, w = d["step"], d["w"]
    step.set_matrices(d["H0"], d["Sinvh"])
    assert step.anyK and step.ctx.fock_band_state() == "none"
    _, C0 = hf.scf.eig_gsym_sub(d["H0"], d["Sinvh"], step.blocks, ctx=step.ctx)
    P0 = 2.0 * hf.scf.form_density(C0, w["nocc"], ctx=step.ctx)
    on, off = _one_step(torch, step, P0, C0, True), _one_step(torch, step, P0, C0, False)
    for k in on:
        assert np.array_equal(on[k], off[k]), k
    assert np.all(np.isfinite(on["E"]))


def test_h0_outside_the_pattern_refuses_the_declaration(gpu):
    hf, torch = gpu
    d = make_step(hf, "n2_pbe_small")
    step, w = d["step"], d["w"]
    _, C0 = hf.scf.eig_gsym_sub(d["H0"], d["Sinvh"], step.blocks, ctx=step.ctx)
    P0 = 2.0 * hf.scf.form_density(C0, w["nocc"], ctx=step.ctx)
    R = step.basis.Nrad()
    b = np.sort(step.blocks[0])
    i, j = int(b[0]), int(b[0]) + R - 3
    # first and last-but-one function of the block's first shell: consecutive indices, first and last element
    assert np.array_equal(b[:R - 2], np.arange(i, j + 1)) and d["H0"][i, j] == 0.0 and d["S"][i, j] == 0.0
    H0 = d["H0"].copy()
    H0[i, j] = H0[j, i] = 1e-3
    step.set_matrices(H0, d["Sinvh"])
    assert step.ctx.fock_band_state() == "refused"
    on, off = _one_step(torch, step, P0, C0, True), _one_step(torch, step, P0, C0, False)
    for k in on:
        assert np.array_equal(on[k], off[k]), k
    step.set_matrices(d["H0"], d["Sinvh"])  # the unplanted matrix is taken
    assert step.ctx.fock_band_state() == "declared"


def test_run_converges_to_the_same_energy(gpu, pbe):
    hf, torch = gpu
    step = pbe["step"]
    convthr = 1e-7

    def run(on):
        with band(on):
            step.have_density = step.have_C = False  # from the core guess, through this step's own eigensolver
            return step.run(pbe["S"], maxit=60, convthr=convthr)

    r1, r0 = run(True), run(False)
    print("Etot banded %.12f (%d iterations), dense %.12f (%d)" % (r1["Etot"], r1["iterations"], r0["Etot"], r0["iterations"]))
    assert r1["converged"] and r0["converged"]
    assert abs(r1["Etot"] - r0["Etot"]) < convthr
