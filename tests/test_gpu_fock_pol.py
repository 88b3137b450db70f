"""The fused Fock build of an unrestricted iteration: hfg_fock_compact_pol_devptr (J[Pa + Pb] + XC_a | XC_b in the compact
layout, J beside the XC kernels, skipped shell pairs, shards), hfg_fock_finish_pol_devptr, hfg_eig_gsym_sub_pair_devptr and
DeviceUSCFStep on top of them.

Shapes: (a) the basis of tests/test_gpu_fock_skip.py (N2, lmmax (6, 6), nelem 3, nnodes 8: three m groups, shared element
nodes, N = 387); (b) diatomic lmmax (2, 1), nnodes 4, nelem 17; (c) diatomic lmmax (0,), nnodes 17, nelem 2 (p * p = 289: the
gather's second pass); (d) atomic Z = 10, lmax 2, mmax 1, nnodes 4, nelem 17 (the Laplacian planes).

Bounds, the project's own (tests/test_gpu_parity.py, test_gpu_fock_shapes.py): J relative 1e-12; XC H relative 1e-10; Exc and
Nel 1e-11 max(1, |.|), Ekin 1e-10 max(1, |.|); eigenvalues 1e-10 max(1, |E|); shards 1e-11 of the largest entry.  Every
deviation is printed (pytest -s).

The oracle's polarised call at (a) takes 11 s (101-130), 5 s (1-7) and 31 s (202-231) on 8 cores, so there the XC part is
compared on the radial points Q % 8 == 1 (Context.set_shard against eval_Fxc_points, as test_gpu_fock_shapes.py does for its
largest shapes; the points lie in every element): XC = the sharded build minus the sharded Hartree-Fock build, whose J is
the same kernels on the same flags; the whole J is compared unsharded."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import common
import fock_pol_worker as wk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = wk.W
PBE, TPSS, LDA, BR89, HF = (101, 130), (202, 231), (1, 7), (206, 0), (0, 0)
SHARD = (1, 8)
V = ctypes.c_void_p


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def flatF(M):
    return np.asfortranarray(M).ravel(order="F").copy()


class Pol(object):
    """device buffers of one basis on one context, and the three entries on them"""

    def __init__(self, hf, torch, gb, ctx):
        self.hf, self.torch, self.gb, self.ctx, self.L = hf, torch, gb, ctx, hf.lib()
        self.N, self.A = gb.Nbf(), gb.Nang()
        self.nc = int(self.L.hfg_fock_compact_size(gb.h))
        assert int(self.L.hfg_fock_compact_pol_size(gb.h)) == 2 * self.nc
        f64 = dict(dtype=torch.float64, device="cuda:0")
        n2 = self.N * self.N
        self.Pa, self.Pb, self.Fa, self.Fb, self.X = (torch.zeros(n2, **f64) for _ in range(5))
        self.Fc, self.scal = torch.full((2 * self.nc,), -7.25, **f64), torch.zeros(3, **f64)

    def up(self, t, M):
        t.copy_(self.torch.from_numpy(flatF(M)))

    def mat(self, t):
        return t.cpu().numpy().reshape((self.N, self.N), order="F").copy()

    def build(self, funcs, Pa, Pb, thr=1e-12):
        """(Fc as [spin][x][y][rest], scal) of one build"""
        self.up(self.Pa, Pa)
        self.up(self.Pb, Pb)
        self.torch.cuda.synchronize()
        rc = self.L.hfg_fock_compact_pol_devptr(self.ctx.h, self.gb.h, funcs[0], funcs[1], V(self.Pa.data_ptr()), V(self.Pb.data_ptr()),
                                                V(self.Fc.data_ptr()), V(self.scal.data_ptr()), thr)
        assert rc == 0, self.L.hfg_last_error()
        self.ctx.synchronize()
        return self.Fc.cpu().numpy().reshape(2, self.A, self.A, -1).copy(), self.scal.cpu().numpy().copy()

    def finish(self, H0=None, bid=None):
        """(Fa, Fb) of hfg_fock_finish_pol_devptr on the compact buffer of the last build"""
        self.torch.cuda.synchronize()
        rc = self.L.hfg_fock_finish_pol_devptr(self.ctx.h, self.gb.h, V(self.Fc.data_ptr()), V(H0.data_ptr()) if H0 is not None else None,
                                               V(bid.data_ptr()) if bid is not None else None, V(self.Fa.data_ptr()), V(self.Fb.data_ptr()))
        assert rc == 0, self.L.hfg_last_error()
        self.ctx.synchronize()
        return self.mat(self.Fa), self.mat(self.Fb)

    def finish_slab(self, spin, H0=None, bid=None):
        """hfg_fock_finish_dev on one slab"""
        self.L.hfg_fock_finish_dev.argtypes = [V] * 6
        slab = self.Fc[spin * self.nc:(spin + 1) * self.nc]
        rc = self.L.hfg_fock_finish_dev(self.ctx.h, self.gb.h, V(slab.data_ptr()), V(H0.data_ptr()) if H0 is not None else None,
                                        V(bid.data_ptr()) if bid is not None else None, V(self.X.data_ptr()))
        assert rc == 0, self.L.hfg_last_error()
        self.ctx.synchronize()
        return self.mat(self.X)

    def dense(self, name, P):
        """hfg_coulomb_dev / hfg_exchange_dev of one density"""
        f = getattr(self.L, name)
        f.argtypes = [V] * 4
        self.up(self.Pa, P)
        self.torch.cuda.synchronize()
        assert f(self.ctx.h, self.gb.h, V(self.Pa.data_ptr()), V(self.X.data_ptr())) == 0, self.L.hfg_last_error()
        self.ctx.synchronize()
        return self.mat(self.X)


class Env(object):
    pass


@pytest.fixture(scope="module")
def env(native_libs):
    """shape (a) with its densities; the references that several tests share are computed once"""
    import torch
    import helfem_amd as hf
    if hf.device_count() < 1:
        pytest.fail("no HIP device visible: the hot path has no CPU fallback")
    e = Env()
    e.hf, e.torch = hf, torch
    e.gb, e.ob = common.make_bases(W["Z1"], W["Z2"], W["Rbond"], W["lmmax"], W["nelem"], W["nnodes"])
    e.gb.compute_tei(True)
    e.ob.compute_tei(False)
    e.ldft, e.mdft = 4 * max(W["lmmax"]) + 12, 4 * len(W["lmmax"]) + 5
    e.gb.upload(e.ldft, e.mdft)
    gb = e.gb
    e.N, e.A, e.R, e.E, e.p = gb.Nbf(), gb.Nang(), gb.Nrad(), W["nelem"], W["nnodes"]
    assert e.N % 64 != 0
    _, mval = hf.lm_to_l_m(list(W["lmmax"]))
    e.mval = np.asarray(mval)
    skip = (e.mval != 0).astype(int)
    e.off = np.concatenate([[0], np.cumsum(e.R - skip)])[:-1] - skip  # pure(a, n) = off[a] + n
    assert len(set(mval)) == 3
    e.need = (e.mval[:, None] == e.mval[None, :])  # symmetry 1: blocks of equal m
    e.blocks = gb.get_sym_idx(1)
    e.S, e.H0 = gb.overlap(), gb.kinetic() + gb.nuclear()
    e.Sinvh = hf.scf.form_Sinvh(e.S, False, e.blocks)
    _, C0 = hf.scf.eig_gsym_sub(e.H0, e.Sinvh, e.blocks)
    e.C0 = C0
    e.Pa = np.asfortranarray(hf.scf.form_density(C0, 7))  # half the core density: block diagonal
    other = common.random_density(e.N, 2, seed=13, blocks=e.blocks)
    e.Pb = np.asfortranarray(0.5 * e.Pa + 0.25 * other)
    assert np.array_equal(e.Pb, masked(e, e.Pb))
    # the pair of the oracle comparisons: spread over the whole grid, rho_b / rho_a bounded below by 0.5
    e.Qa = common.random_density(e.N, 2, seed=12, blocks=e.blocks)
    e.Qb = np.asfortranarray(0.5 * e.Qa + 0.25 * other)
    e.Ma, e.Mb = wk.mixed_pair(gb)  # nothing to skip
    assert np.all(e.Ma != 0.0)
    x, y = int(np.where(e.mval == 0)[0][1]), int(np.where(e.mval != 0)[0][2])
    e.stray = (e.off[x] + e.p - 1, e.off[y] + e.p - 1)  # an off-block pair at the node that elements 0 and 1 share
    e.stray_pair = (x, y)
    e.bid = np.zeros(e.N, dtype=np.int32)
    for ib, b in enumerate(e.blocks):
        e.bid[b] = ib
    e.pol = Pol(hf, torch, gb, gb.ctx)  # the basis' own context: no blocks declared
    os.environ.pop("HELFEM_FOCK_SKIP", None)
    yield e
    os.environ.pop("HELFEM_FOCK_SKIP", None)


def masked(e, M):
    out = np.zeros_like(M)
    for b in e.blocks:
        out[np.ix_(b, b)] = M[np.ix_(b, b)]
    return out


def new_step(e, funcs=PBE, nocc=(8, 6), blocks_set=True, **kw):
    s = e.hf.DeviceUSCFStep(e.gb, funcs[0], funcs[1], e.ldft, e.mdft, nocc, symmetry=1, device=0, **kw)
    if not blocks_set:
        s.ctx.set_fock_blocks(e.gb, None)
    return s


def step_build(e, step, Pa, Pb, skip):
    os.environ["HELFEM_FOCK_SKIP"] = "1" if skip else "0"
    try:
        step.set_density(Pa, Pb)
        step.fock_partial()
        e.torch.cuda.synchronize()
        return step.Fc.cpu().numpy().reshape(2, e.A, e.A, -1).copy(), step.scal.cpu().numpy().copy()
    finally:
        os.environ.pop("HELFEM_FOCK_SKIP", None)


def report(what, err, bound):
    print("%s: %.3e (bound %.0e)" % (what, err, bound))
    return err


def check_scal(what, got, ref):
    eX = report(what + " Exc", abs(got[0] - ref[0]) / max(1.0, abs(ref[0])), 1e-11)
    eN = report(what + " Nel", abs(got[1] - ref[1]) / max(1.0, abs(ref[1])), 1e-11)
    eK = report(what + " Ekin", abs(got[2] - ref[2]) / max(1.0, abs(ref[2])), 1e-10)
    assert eX < 1e-11 and eN < 1e-11 and eK < 1e-10, (what, eX, eN, eK)


# ---- 1. the oracle ---------------------------------------------------------------------------------------------------------
def test_hartree_fock_is_the_coulomb_matrix(env):
    e = env
    Fc, scal = e.pol.build(HF, e.Qa, e.Qb)
    Fa, Fb = e.pol.finish()
    assert same_bits(Fc[0], Fc[1]) and np.all(scal == 0.0)
    J = e.pol.dense("hfg_coulomb_dev", e.Qa + e.Qb)
    ea, eb = report("(a) HF slab a vs hfg_coulomb_dev", common.relerr(Fa, J), 1e-13), report("slab b", common.relerr(Fb, J), 1e-13)
    eo = report("(a) J vs oracle", common.relerr(Fa, e.ob.coulomb(e.Qa + e.Qb)), 1e-12)
    assert ea < 1e-13 and eb < 1e-13 and eo < 1e-12


@pytest.mark.parametrize("funcs", [PBE, LDA, TPSS], ids=["pbe", "lda", "tpss"])
def test_oracle_parity_small_n2(env, funcs):
    """XC on the radial points Q % 8 == 1 (module docstring)"""
    e = env
    rank, n = SHARD
    e.gb.ctx.set_shard(rank, n)
    try:
        e.pol.build(funcs, e.Qa, e.Qb)
        Fa, Fb = e.pol.finish()
        sc = e.pol.scal.cpu().numpy().copy()
        e.pol.build(HF, e.Qa, e.Qb)
        Ja, Jb = e.pol.finish()
    finally:
        e.gb.ctx.set_shard(0, 1)
    pts = [q for q in range(e.E * 5 * e.p) if q % n == rank]
    Hao, Hbo, Exco, Nelo, Ekino = e.ob.eval_Fxc_points(e.ldft, e.mdft, funcs[0], funcs[1], e.Qa, pts, Pb=e.Qb, threads=8)
    assert np.max(np.abs(Hao)) > 0.0 and np.max(np.abs(Hbo)) > 0.0
    tag = "(a) %d-%d points Q %% %d == %d" % (funcs + (n, rank))
    ea, eb = report(tag + " Ha", common.relerr(Fa - Ja, Hao), 1e-10), report(tag + " Hb", common.relerr(Fb - Jb, Hbo), 1e-10)
    assert ea < 1e-10 and eb < 1e-10
    check_scal(tag, sc, (Exco, Nelo, Ekino))
    if funcs == TPSS:
        assert Ekino > 0.0


SHAPES = {"b": ("diatomic", 4, 17, (2, 1)), "c": ("diatomic", 17, 2, (0,)), "d": ("atomic", 4, 17, (2, 1))}


class Shape(object):
    def __init__(self, hf, torch, prog, p, E, ang):
        self.prog, self.p, self.E = prog, p, E
        if prog == "diatomic":
            self.gb, self.ob = common.make_bases(1, 1, 1.4, ang, E, p)
            self.ldft, self.mdft = 4 * max(ang) + 12, 4 * len(ang) + 5
        else:
            self.gb, self.ob = common.make_atomic_bases(10, ang[0], ang[1], E, p)
            self.ldft, self.mdft = 4 * ang[0] + 10, 4 * ang[1] + 5
        self.gb.compute_tei(True)
        self.ob.compute_tei(True)
        self.gb.upload(self.ldft, self.mdft)
        N = self.gb.Nbf()
        blocked = common.random_density(N, 2, seed=12, blocks=self.gb.get_sym_idx(1))
        self.Pa = np.asfortranarray(0.05 * common.random_density(N, 3, seed=11) + blocked)
        self.Pb = np.asfortranarray(0.5 * self.Pa + 0.25 * blocked)
        self.pol = Pol(hf, torch, self.gb, self.gb.ctx)


@pytest.fixture(scope="module", params=sorted(SHAPES), ids=sorted(SHAPES))
def shape(request, native_libs):
    import torch
    import helfem_amd as hf
    s = Shape(hf, torch, *SHAPES[request.param])
    s.tag = "(%s)" % request.param
    return s


def test_oracle_parity_shapes(shape):
    s = shape
    Fc, scal = s.pol.build(PBE, s.Pa, s.Pb)
    if s.tag == "(c)":
        assert s.p * s.p > 256
    Fa, Fb = s.pol.finish()
    Jo = s.ob.coulomb(s.Pa + s.Pb)
    Hao, Hbo, Exco, Nelo, Ekino = s.ob.eval_Fxc_pol(s.ldft, s.mdft, PBE[0], PBE[1], s.Pa, s.Pb)
    # J + XC against the sum of the references: each part at its own bound
    bound = (1e-12 * np.max(np.abs(Jo)) + 1e-10 * max(np.max(np.abs(Hao)), np.max(np.abs(Hbo))))
    ea, eb = np.max(np.abs(Fa - Jo - Hao)), np.max(np.abs(Fb - Jo - Hbo))
    print("%s 101-130 |F - (J + H)| a %.3e b %.3e (bound %.3e = 1e-12 max|J| + 1e-10 max|H|)" % (s.tag, ea, eb, bound))
    assert ea < bound and eb < bound
    check_scal(s.tag + " 101-130", scal, (Exco, Nelo, Ekino))
    # the XC part alone at its relative bound, J taken out with the Hartree-Fock build (both slabs J, the same kernels)
    s.pol.build(HF, s.Pa, s.Pb)
    Ja, Jb = s.pol.finish()
    ej = report(s.tag + " J", common.relerr(Ja, Jo), 1e-12)
    xa, xb = report(s.tag + " Ha", common.relerr(Fa - Ja, Hao), 1e-10), report(s.tag + " Hb", common.relerr(Fb - Jb, Hbo), 1e-10)
    assert ej < 1e-12 and xa < 1e-10 and xb < 1e-10
    if s.prog != "atomic":
        return
    # the Laplacian planes: mgga_x_br89 against the dense restatement of tests/lapl_dense.py, as tests/test_gpu_lapl.py does
    import helfem_amd as hf
    import lapl_dense
    dense = lapl_dense.DenseWorker(hf, s.gb, hf.get_grid(40.0, s.E, 4, 2.0), s.p, s.ldft, s.mdft)
    Fc, scal = s.pol.build(BR89, s.Pa, s.Pb)
    Fa, Fb = s.pol.finish()
    Had, Hbd, Excd, Neld = dense.eval_Fxc_pol(BR89[0], BR89[1], s.Pa, s.Pb)
    ea, eb = report("(d) 206-0 Ha", common.relerr(Fa - Ja, Had), 1e-10), report("(d) 206-0 Hb", common.relerr(Fb - Jb, Hbd), 1e-10)
    eX = report("(d) 206-0 Exc", abs(scal[0] - Excd) / max(1.0, abs(Excd)), 1e-11)
    eN = report("(d) 206-0 Nel", abs(scal[1] - Neld) / max(1.0, abs(Neld)), 1e-11)
    assert ea < 1e-10 and eb < 1e-10 and eX < 1e-11 and eN < 1e-11


# ---- 2. the existing entries ------------------------------------------------------------------------------------------------
def test_against_the_existing_entries(env):
    e = env
    t = e.torch
    Fc, scal = e.pol.build(PBE, e.Ma, e.Mb)
    Fa, Fb = e.pol.finish()
    J = e.pol.dense("hfg_coulomb_dev", e.Ma + e.Mb)
    Ha, Hb, Exc, Nel, Ekin = e.hf.DFTGrid(e.gb, e.ldft, e.mdft).eval_Fxc_dev(PBE[0], PBE[1], e.Ma, e.Mb)
    ea, eb = report("(a) vs J + XC_a of the dense entries", common.relerr(Fa, J + Ha), 1e-12), report("b", common.relerr(Fb, J + Hb), 1e-12)
    assert ea < 1e-12 and eb < 1e-12
    check_scal("(a) vs hfg_xc_fock_pol_dev", scal, (Exc, Nel, Ekin))
    # the finish of each slab: bitwise hfg_fock_finish_dev, with and without H0 and block ids
    H0, bid = t.from_numpy(flatF(e.H0)).cuda(), t.from_numpy(e.bid).cuda()
    for h, b in ((None, None), (H0, None), (H0, bid)):
        Fa, Fb = e.pol.finish(h, b)
        assert same_bits(Fa, e.pol.finish_slab(0, h, b)) and same_bits(Fb, e.pol.finish_slab(1, h, b))
    assert np.array_equal(Fa, masked(e, Fa)) and np.any(Fa != Fb)


# ---- 3. closed shell ----------------------------------------------------------------------------------------------------------
def test_closed_shell(env):
    """Pa = Pb: the two slabs against each other and against the restricted build of P = 2 Pa.

    Bitwise equal slabs are what the new code owes: one J, the same gather, stages and combine for both spins.  They are
    asserted for Hartree-Fock and for the exchange functionals (LDA 1, PBE 101), which the grid kernel evaluates spin by spin
    with one function.  The polarised correlation point code (xc_device.h, shared with hfg_xc_fock_pol_dev, whose results
    may not change) is not symmetric in its last bit: on MI355X, at this shape, hfg_xc_fock_pol_dev(Pa, Pa) itself returns
    Ha != Hb in 54 667 of 149 769 entries for 101-130, max |Ha - Hb| = 5.6e-17 at max |H| = 0.52 (1-7: 2.8e-17, 202-231:
    1.1e-16; 1-0 and 101-0: none), and the slabs of the fused build differ likewise, in 54 903 of 69 312 entries by at most
    1.1e-16 at max |F| = 3440.  With correlation the new code's obligation is pinned in two ways:

      * the finished matrices differ by exactly what hfg_xc_fock_pol_dev(Pa, Pa) shows, Fa - Fb = Ha - Hb, up to the roundings
        of the sums alone.  With c1, c2 the (at most two) compact entries of an element of F, each c = fl(J + XC) and
        F = fl(c1 + c2), H = fl(x1 + x2), so entry by entry, u = 2^-53:
            |(Fa - Fb) - (Ha - Hb)| <= u (|c1a| + |c2a| + |Fa| + |c1b| + |c2b| + |Fb| + |Ha| + |Hb|)
        (|c1| + |c2| is the finish of the slab of absolute values); J, the gather, the stages and the combine contribute nothing;
      * slab against slab: two roundings of J + XC, u max |F| each, beside an XC asymmetry that the first point holds to the
        existing entry's last bit of |H| << |F|: relative to max |F| below 1e-15 (4.5 ulp)."""
    e = env
    for funcs in (HF, (1, 0), (101, 0)):
        Fc, scal = e.pol.build(funcs, e.Pa, e.Pa)
        assert same_bits(Fc[0], Fc[1]), funcs
    P = np.asfortranarray(2.0 * e.Pa)
    Fc, scal = e.pol.build(PBE, e.Pa, e.Pa)
    eab = report("(a) closed shell 101-130, slab a vs slab b", common.relerr(Fc[0], Fc[1]), 1e-15)
    assert eab < 1e-15
    Fa, Fb = e.pol.finish()
    e.pol.Fc.abs_()
    Ta, Tb = e.pol.finish()
    Ha, Hb = e.hf.DFTGrid(e.gb, e.ldft, e.mdft).eval_Fxc_dev(PBE[0], PBE[1], e.Pa, e.Pa)[:2]
    dF, dH = Fa - Fb, Ha - Hb
    u = 2.0 ** -53
    bound = u * (Ta + np.abs(Fa) + Tb + np.abs(Fb) + np.abs(Ha) + np.abs(Hb) + np.abs(dF) + np.abs(dH))
    dev = np.abs(dF - dH)
    print("(a) closed shell 101-130: max |Fa - Fb| %.3e, max |Ha - Hb| %.3e, max |(Fa - Fb) - (Ha - Hb)| %.3e, largest share of "
          "the rounding bound %.3f" % (np.max(np.abs(dF)), np.max(np.abs(dH)), np.max(dev), np.max(dev / np.maximum(bound, 1e-300))))
    assert np.all(dev <= bound)
    Fc, scal = e.pol.build(PBE, e.Pa, e.Pa)
    r = e.hf.DeviceSCFStep(e.gb, PBE[0], PBE[1], e.ldft, e.mdft, 7, symmetry=1, device=0)
    r.ctx.set_fock_blocks(e.gb, None)
    r.set_density(P)
    r.fock_partial()
    e.torch.cuda.synchronize()
    Fr = r.Fc.cpu().numpy().reshape(e.A, e.A, -1)
    ea = report("(a) closed shell slab a vs hfg_fock_compact_dev", common.relerr(Fc[0], Fr), 1e-10)
    eb = report("(a) closed shell slab b vs hfg_fock_compact_dev", common.relerr(Fc[1], Fr), 1e-10)
    assert ea < 1e-10 and eb < 1e-10
    check_scal("(a) closed shell", scal, r.scal.cpu().numpy())


# ---- 4. skipping is invisible -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case1(env):
    """block-diagonal densities with the blocks set, on a fresh context: skipped and unskipped"""
    e = env
    step = new_step(e)
    Fc1, sc1 = step_build(e, step, e.Pa, e.Pb, True)
    Fc0, sc0 = step_build(e, step, e.Pa, e.Pb, False)
    return Fc1, sc1, Fc0, sc0


def test_block_diagonal_densities_with_blocks_set(env, case1):
    e = env
    Fc1, sc1, Fc0, sc0 = case1
    for s in range(2):
        assert same_bits(Fc1[s][e.need], Fc0[s][e.need])
        assert np.all(bits(Fc1[s][~e.need]) == 0)  # exactly +0
        assert np.any(Fc0[s][~e.need] != 0.0)  # without skipping they are computed
    assert same_bits(sc1, sc0)
    assert np.any(Fc1[0] != Fc1[1])


def test_block_diagonal_densities_nothing_set(env, case1):
    e = env
    step = new_step(e, blocks_set=False)
    Fc1, sc1 = step_build(e, step, e.Pa, e.Pb, True)
    Fc0, sc0 = step_build(e, step, e.Pa, e.Pb, False)
    assert same_bits(Fc1[:, e.need], Fc0[:, e.need]) and same_bits(sc1, sc0)
    assert np.array_equal(Fc1[:, ~e.need], Fc0[:, ~e.need])  # values: a sign of zero may differ, nothing else
    assert np.any(Fc1[:, ~e.need] != 0.0)
    assert same_bits(Fc0, case1[2])


def test_dense_densities_skip_nothing(env):
    e = env
    step = new_step(e, blocks_set=False)
    Fc1, sc1 = step_build(e, step, e.Ma, e.Mb, True)
    Fc0, sc0 = step_build(e, step, e.Ma, e.Mb, False)
    assert same_bits(Fc1, Fc0) and same_bits(sc1, sc0)


def with_stray(e, value):
    P = e.Pb.copy()
    i, j = e.stray
    assert P[i, j] == 0.0 and e.Pa[i, j] == 0.0
    P[i, j] = P[j, i] = value
    return P


def test_one_stray_entry_in_one_spin(env, case1):
    """in Pb only: the union flag keeps the pair for both spins and for J"""
    e = env
    step = new_step(e, blocks_set=False)
    Pb = with_stray(e, 0.3)
    Fc1, sc1 = step_build(e, step, e.Pa, Pb, True)
    Fc0, sc0 = step_build(e, step, e.Pa, Pb, False)
    assert same_bits(Fc1, Fc0) and same_bits(sc1, sc0)
    x, y = e.stray_pair
    pp = e.p * e.p
    base = case1[2]
    hf_step = new_step(e, HF, blocks_set=False)  # both slabs J
    Jc, _ = step_build(e, hf_step, e.Pa, Pb, True)
    J0, _ = step_build(e, hf_step, e.Pa, e.Pb, True)
    for el in range(2):  # both elements of the shared node
        sl = slice(el * pp, (el + 1) * pp)
        assert np.any(Jc[0][x, y, sl] != J0[0][x, y, sl]) and np.any(Jc[1][x, y, sl] != J0[1][x, y, sl])  # through J: both slabs
        xc_b = (Fc1[1][x, y, sl] - Jc[1][x, y, sl]) - (base[1][x, y, sl] - J0[1][x, y, sl])
        assert np.max(np.abs(xc_b)) > 1e-8  # through XC: slab b
        assert np.any(Fc1[0][x, y, sl] != base[0][x, y, sl])


def test_nan_in_an_off_block_pair_of_one_spin(env):
    e = env
    step = new_step(e, blocks_set=False)
    Pb = with_stray(e, float("nan"))
    Fc1, _ = step_build(e, step, e.Pa, Pb, True)
    Fc0, _ = step_build(e, step, e.Pa, Pb, False)
    assert np.isnan(Fc0).any()
    assert np.array_equal(np.isnan(Fc1), np.isnan(Fc0))
    assert same_bits(Fc1[~np.isnan(Fc0)], Fc0[~np.isnan(Fc0)])


def test_stale_buffers_of_a_denser_build(env, case1):
    e = env
    step = new_step(e)
    step_build(e, step, e.Ma, e.Mb, True)
    Fc, sc = step_build(e, step, e.Pa, e.Pb, True)
    assert same_bits(Fc, case1[0]) and same_bits(sc, case1[1])


def test_tpss_with_blocks_set(env):
    e = env
    step = new_step(e, TPSS)
    Fc1, sc1 = step_build(e, step, e.Pa, e.Pb, True)
    Fc0, sc0 = step_build(e, step, e.Pa, e.Pb, False)
    assert same_bits(Fc1[:, e.need], Fc0[:, e.need]) and same_bits(sc1, sc0)
    assert np.all(bits(Fc1[:, ~e.need]) == 0)
    assert sc1[2] > 0.0


# ---- 5. shards ------------------------------------------------------------------------------------------------------------------
def test_shards_sum_to_the_unsharded_build(env, case1):
    e = env
    step = new_step(e)
    Fc_sum, sc_sum = np.zeros_like(case1[0]), np.zeros(3)
    try:
        for r in range(2):
            step.ctx.set_shard(r, 2)
            Fc, sc = step_build(e, step, e.Pa, e.Pb, True)
            assert np.all(bits(Fc[:, ~e.need]) == 0)
            Fc_sum += Fc
            sc_sum += sc
    finally:
        step.ctx.set_shard(0, 1)
    eF = report("(a) shards Fc", np.max(np.abs(Fc_sum - case1[0])) / np.max(np.abs(case1[0])), 1e-11)
    eS = report("(a) shards scal", np.max(np.abs(sc_sum - case1[1])) / np.max(np.abs(case1[1])), 1e-11)
    assert eF < 1e-11 and eS < 1e-11


# ---- 6. repeatability -----------------------------------------------------------------------------------------------------------
def _worker(mode, path, **environ):
    child = dict(os.environ)
    child.update(environ)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fock_pol_worker.py"), mode, path], cwd=ROOT, timeout=300,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=child)
    assert out.returncode == 0 and "ok" in out.stdout.decode().split(), out.stdout.decode()[-3000:]


def test_two_builds_in_a_row_repeat_bitwise(env, tmp_path):
    """with J beside the XC kernels (this process), and with HELFEM_FOCK_OVERLAP=0, which is read once: a process of its own"""
    e = env
    assert os.environ.get("HELFEM_FOCK_OVERLAP") is None
    first, second = e.pol.build(PBE, e.Ma, e.Mb), e.pol.build(PBE, e.Ma, e.Mb)
    assert same_bits(first[0], second[0]) and same_bits(first[1], second[1])
    path = str(tmp_path / "repeat.npz")
    _worker("repeat", path, HELFEM_FOCK_OVERLAP="0")
    r = np.load(path)
    assert same_bits(r["Fc1"], r["Fc2"]) and same_bits(r["scal1"], r["scal2"])
    err = report("(a) one stream vs two", common.relerr(r["Fc1"].reshape(first[0].shape), first[0]), 1e-12)
    assert err < 1e-12 and np.max(np.abs(r["scal1"] - first[1])) <= 1e-12 * np.max(np.abs(first[1]))


# ---- 7. the step object -----------------------------------------------------------------------------------------------------------
def start(e, step, nocc):
    step.set_matrices(e.H0, e.Sinvh)
    Pa, Pb = e.hf.scf.form_density(e.C0, nocc[0]), e.hf.scf.form_density(e.C0, nocc[1]) if nocc[1] else np.zeros((e.N, e.N))
    step.set_density(Pa, Pb)
    return Pa, Pb


def test_two_whole_steps(env):
    e = env
    out = []
    for skip in (True, False):
        step = new_step(e)
        start(e, step, (8, 6))
        os.environ["HELFEM_FOCK_SKIP"] = "1" if skip else "0"
        try:
            for _ in range(2):
                step.step(None)
            e.torch.cuda.synchronize()
        finally:
            os.environ.pop("HELFEM_FOCK_SKIP", None)
        out.append([t.cpu().numpy().copy() for t in (step.Ea, step.Eb, step.Fa, step.Fb, step.Pa, step.Pb)])
    for a, b in zip(*out):
        assert same_bits(a, b)
    assert np.any(out[0][0] != out[0][1])  # the spins differ


def test_one_step_against_the_host_pointer_solve_and_the_restricted_step(env):
    e = env
    step = new_step(e)
    start(e, step, (8, 6))
    step.step(None)
    e.torch.cuda.synchronize()
    Fa, Fb = step.numpy(step.Fa, (e.N, e.N)), step.numpy(step.Fb, (e.N, e.N))
    Ea, Ca, Eb, Cb = e.hf.scf.eig_gsym_sub_pair(Fa, Fb, e.Sinvh, e.blocks)
    for tag, E, Eh, C, n, P in (("a", step.Ea, Ea, step.Ca, 8, step.Pa), ("b", step.Eb, Eb, step.Cb, 6, step.Pb)):
        E, C = E.cpu().numpy(), step.numpy(C, (e.N, e.N))
        err = report("(a) step E%s vs hfg_eig_gsym_sub_pair" % tag, np.max(np.abs(E - Eh)) / max(1.0, np.max(np.abs(Eh))), 1e-10)
        assert err < 1e-10
        assert common.relerr(step.numpy(P, (e.N, e.N)), C[:, :n] @ C[:, :n].T) < 1e-12
    # (7, 7) from the closed-shell density: the restricted step's levels
    u = new_step(e, nocc=(7, 7))
    Pa, _ = start(e, u, (7, 7))
    u.step(None)
    r = e.hf.DeviceSCFStep(e.gb, PBE[0], PBE[1], e.ldft, e.mdft, 7, symmetry=1, device=0)
    r.set_matrices(e.H0, e.Sinvh)
    r.set_density(2.0 * Pa)
    r.step(None)
    e.torch.cuda.synchronize()
    Er = r.E.cpu().numpy()
    for tag, E in (("a", u.Ea), ("b", u.Eb)):
        err = report("(a) (7, 7) E%s vs DeviceSCFStep" % tag, np.max(np.abs(E.cpu().numpy() - Er)) / max(1.0, np.max(np.abs(Er))), 1e-10)
        assert err < 1e-10
    assert common.relerr(step.numpy(u.Pa, (e.N, e.N)), step.numpy(r.P, (e.N, e.N))) < 1e-9  # both C_occ C_occ^T


def test_step_with_exact_exchange(env):
    """kfrac = 0.25: F_s = finish(build) + 0.25 K[P_s], K from hfg_exchange_dev"""
    e = env
    step = new_step(e, kfrac=0.25)
    Pa, Pb = start(e, step, (8, 6))
    step.step(None)
    e.torch.cuda.synchronize()
    plain = new_step(e)
    start(e, plain, (8, 6))
    plain.fock_partial()
    plain.fock_finish()
    e.torch.cuda.synchronize()
    for tag, F, F0, P in (("a", step.Fa, plain.Fa, Pa), ("b", step.Fb, plain.Fb, Pb)):
        ref = plain.numpy(F0, (e.N, e.N)) + 0.25 * e.pol.dense("hfg_exchange_dev", P)
        err = report("(a) kfrac 0.25 F%s" % tag, common.relerr(step.numpy(F, (e.N, e.N)), ref), 1e-13)
        assert err < 1e-13


class _Pause(Exception):
    pass


def rehearse_ranks(e, nranks, nocc, **kw):
    """the steps of all ranks in this process, one after the other, with a summing closure for allreduce.  A rank cannot go
    on before the others have reached the same collective, so the step is replayed: every pass starts all ranks anew, feeds
    the collectives whose sums are known and stops each rank at the first one that is not (builds repeat bitwise: section 6);
    that one's sum over the ranks is then known to the next pass."""
    steps = [new_step(e, nocc=nocc, rank=r, nranks=nranks, **kw) for r in range(nranks)]
    sums = []
    while True:
        pending, done = [], 0
        for s in steps:
            start(e, s, nocc)
            calls = [0]

            def allreduce(t, calls=calls):
                i = calls[0]
                calls[0] += 1
                if i == len(sums):
                    pending.append(t.clone())
                    raise _Pause()
                t.copy_(sums[i])
            try:
                s.step(allreduce)
                done += 1
            except _Pause:
                pass
        e.torch.cuda.synchronize()
        if done == nranks:
            return steps, len(sums)
        assert done == 0 and len(pending) == nranks
        sums.append(sum(pending[1:], pending[0]))


@pytest.mark.parametrize("fock_shard,ncoll", [("auto", 3), ("always", 5)])
def test_two_ranks_reproduce_one(env, monkeypatch, fock_shard, ncoll):
    """the several-rank branch of the step (shard policy, all-reduced Fc, scal and K, the two block buffers, eig_blocks and
    eig_assemble per spin) with ranks 0 and 1 of 2 against the one-rank step; kfrac = 0.25 so that K is there.  Collectives:
    K and the two block buffers, with fock_shard = "always" also Fc and scal."""
    e = env
    monkeypatch.delenv("HELFEM_FOCK_SHARD", raising=False)
    one = new_step(e, kfrac=0.25)
    start(e, one, (8, 6))
    one.step(None)
    e.torch.cuda.synchronize()
    steps, n = rehearse_ranks(e, 2, (8, 6), kfrac=0.25, fock_shard=fock_shard)
    assert n == ncoll
    get = lambda s, name: getattr(s, name).cpu().numpy()
    for s in steps:
        for name in ("Fa", "Fb"):  # the sharded step's bound: 1e-11 of the largest entry
            err = report("(a) 2 ranks %s, rank %d %s" % (fock_shard, s.rank, name), common.relerr(get(s, name), get(one, name)), 1e-11)
            assert err < 1e-11
        for name in ("Ea", "Eb"):
            ref = get(one, name)
            err = report("(a) 2 ranks %s, rank %d %s" % (fock_shard, s.rank, name),
                         np.max(np.abs(get(s, name) - ref)) / max(1.0, np.max(np.abs(ref))), 1e-10)
            assert err < 1e-10
        for name in ("Pa", "Pb"):
            assert common.relerr(get(s, name), get(one, name)) < 1e-9
    for name in ("Fa", "Fb", "Ea", "Eb", "Pa", "Pb", "Ca", "Cb"):
        assert same_bits(get(steps[0], name), get(steps[1], name)), name  # every rank ends with the same matrices


def test_one_electron_step(native_libs):
    """H2+ at shape (c), Hartree-Fock (kfrac = 1: hfg_exchange_dev returns -K, as TwoDBasis::exchange does) and nocc = (1, 0):
    J - K vanishes on the occupied orbital and is positive semidefinite, so the core level stays the lowest eigenvalue; Pb and
    K[Pb] stay zero"""
    import torch
    import helfem_amd as hf
    gb, _ = common.make_bases(1, 1, 1.4, (0,), 2, 17, oracle=False)
    gb.compute_tei(True)
    blocks = gb.get_sym_idx(1)
    S, H0 = gb.overlap(), gb.kinetic() + gb.nuclear()
    X = hf.scf.form_Sinvh(S, False, blocks)
    E0, C0 = hf.scf.eig_gsym_sub(H0, X, blocks)
    step = hf.DeviceUSCFStep(gb, 0, 0, 12, 9, (1, 0), symmetry=1, device=0, kfrac=1.0)
    step.set_matrices(H0, X)
    step.set_density(hf.scf.form_density(C0, 1), np.zeros_like(S), Ca=C0)
    for _ in range(2):
        step.step(None)
    torch.cuda.synchronize()
    Ea = step.Ea.cpu().numpy()
    err = report("(c) one electron: lowest level vs the core Hamiltonian's", abs(Ea[0] - E0[0]), 1e-10)
    assert err < 1e-10 * max(1.0, abs(E0[0]))
    assert not step.Pb.any().item() and not step.Kb.any().item()
    Pa = step.numpy(step.Pa, S.shape)
    assert abs(np.sum(Pa * S) - 1.0) < 1e-10


# ---- 8. stream order ------------------------------------------------------------------------------------------------------------
def test_devptr_entries_keep_the_stream_order(native_libs, tmp_path):
    """the protocol of tests/stream_order_worker.py for the three entries: on the null stream and on a non-default torch stream,
    input written by a copy enqueued just before the call, output read by a copy enqueued just after, decoys before and after, no
    host synchronisation; on a stream of the context's own, complete after hfg_ctx_synchronize and equal to the null stream's"""
    import stream_order_worker as sow
    path = str(tmp_path / "stream.json")
    _worker("stream", path)
    recs = json.load(open(path))["records"]
    assert sorted((r["entry"], r["kind"]) for r in recs) == sorted((n, k) for n in wk.ENTRIES for k in sow.STREAM_KINDS)
    for rec in recs:
        print(rec)
        assert rec["decoy_differs"] and rec["repeat"]["ok"], rec
        assert rec["baselines_bitwise"], "results repeat bitwise from call to call"
        if "twin" in rec:
            assert rec["twin"]["ok"], rec
        if rec["kind"] == "own":
            assert rec["own_vs_null"]["ok"], rec
            continue
        assert rec["delay_ms"] >= sow.DELAY_MIN_MS, "the delay is too short for the run to mean anything"
        assert not rec["ordered_is_decoy"], "the call read its inputs before the copy enqueued ahead of it"
        assert rec["ordered"]["ok"] and rec["ordered"]["bitwise"], rec


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(env):
    e = env
    L, p = e.hf.lib(), e.pol
    ctx, gb = e.gb.ctx.h, e.gb.h
    Pa, Pb, Fc, sc, Fa, Fb = (V(t.data_ptr()) for t in (p.Pa, p.Pb, p.Fc, p.scal, p.Fa, p.Fb))
    err = lambda: L.hfg_last_error().decode()
    for args in ((None, gb, 101, 130, Pa, Pb, Fc, sc), (ctx, None, 101, 130, Pa, Pb, Fc, sc), (ctx, gb, 101, 130, None, Pb, Fc, sc),
                 (ctx, gb, 101, 130, Pa, None, Fc, sc), (ctx, gb, 101, 130, Pa, Pb, None, sc), (ctx, gb, 101, 130, Pa, Pb, Fc, None)):
        assert L.hfg_fock_compact_pol_devptr(*(args + (1e-12,))) == 1 and "null" in err()
    for args in ((None, gb, Fc, None, None, Fa, Fb), (ctx, None, Fc, None, None, Fa, Fb), (ctx, gb, None, None, None, Fa, Fb),
                 (ctx, gb, Fc, None, None, None, Fb), (ctx, gb, Fc, None, None, Fa, None)):
        assert L.hfg_fock_finish_pol_devptr(*args) == 1 and "null" in err()
    ptr, idx = e.hf.scf._blocks(e.blocks)
    i64 = ctypes.POINTER(ctypes.c_int64)
    pp, ip = ptr.ctypes.data_as(i64), idx.ctypes.data_as(i64)
    assert L.hfg_eig_gsym_sub_pair_devptr(ctx, e.N, Pa, None, Pb, len(e.blocks), pp, ip, sc, Fa, sc, Fb) == 1 and "null" in err()
    assert L.hfg_eig_gsym_sub_pair_devptr(None, e.N, Pa, Pb, Pb, len(e.blocks), pp, ip, sc, Fa, sc, Fb) == 1 and "null" in err()
    # a basis without uploaded tables: the restricted entry's status and words
    L.hfg_fock_compact_dev.argtypes = [V, V, ctypes.c_int, ctypes.c_int, V, V, V, ctypes.c_double]
    bare, _ = common.make_bases(1, 1, 1.4, (0,), 2, 17, oracle=False)
    assert L.hfg_fock_compact_dev(ctx, bare.h, 101, 130, Pa, Fc, sc, 1e-12) == 1
    words = err()
    assert L.hfg_fock_compact_pol_devptr(ctx, bare.h, 101, 130, Pa, Pb, Fc, sc, 1e-12) == 1 and err() == words
    assert L.hfg_fock_finish_pol_devptr(ctx, bare.h, Fc, None, None, Fa, Fb) == 1 and err() == words
    # a functional without XC tables: the polarised entry's status and words
    L.hfg_xc_fock_pol_dev.argtypes = [V, V, ctypes.c_int, ctypes.c_int, V, V, V, V, V, ctypes.c_double]
    bare.compute_tei(False)
    bare.upload()
    n2 = bare.Nbf() ** 2
    assert n2 <= e.N * e.N and 2 * int(L.hfg_fock_compact_size(bare.h)) <= 2 * p.nc  # the buffers of (a) hold this basis
    assert L.hfg_xc_fock_pol_dev(bare.ctx.h, bare.h, 101, 130, Pa, Pb, Fa, Fb, sc, 1e-12) == 2
    words = err()
    assert L.hfg_fock_compact_pol_devptr(bare.ctx.h, bare.h, 101, 130, Pa, Pb, Fc, sc, 1e-12) == 2 and err() == words
    assert L.hfg_fock_compact_pol_devptr(bare.ctx.h, bare.h, 0, 0, Pa, Pb, Fc, sc, 1e-12) == 0  # Hartree-Fock needs none
    # a diatomic basis with a Laplacian functional
    assert L.hfg_xc_fock_pol_dev(ctx, gb, 206, 0, Pa, Pb, Fa, Fb, sc, 1e-12) == 1
    words = err()
    assert L.hfg_fock_compact_pol_devptr(ctx, gb, 206, 0, Pa, Pb, Fc, sc, 1e-12) == 1 and err() == words
    e.gb.ctx.synchronize()
    # the context works afterwards
    Fc1, sc1 = p.build(PBE, e.Qa, e.Qb)
    assert np.all(np.isfinite(Fc1)) and sc1[1] > 0.0
