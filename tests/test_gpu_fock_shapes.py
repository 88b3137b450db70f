"""The Fock-build kernels (J, K, XC and the table set-up kernels) across element count E = nelem and element order
p = nnodes, against the CPU oracle on the same basis and densities.

The kernels of hip/fock.hip, hip/exchange.hip, hip/exchange_lr.hip, hip/tei_dev.hip and hip/rs_tei_dev.hip size their
workgroups and LDS from p and E.  The boundaries this module stands on, each with a shape on either side:

  element count, k_coulomb_radial: launched with bs = min(256, round_up64(p * p)) threads, its per-element scalars
  (4 * E trace sums, then E prefix / suffix sums) were filled by one thread each.  4 * E = bs is the last shape that
  fits one pass; one element more needs a second pass of the workgroup:
      p = 4, 8   bs =  64   E = 16 | 17
      p = 9      bs = 128   E = 32 | 33
      p = 12     bs = 192   E = 48 | 49
      p = 14     bs = 256   E = 64 | 65       and (15, 65), the production order
  The same shapes straddle E * p = 512, where the low-rank exchange leaves k_exl_alpha (one thread per (element, row))
  for k_exl_alpha_gen: (9, 32) = 288, (8, 17) = 136 below; (12, 48) = 576, (14, 64) = 896 above.
  The angular basis is minimal there (diatomic lmmax = (0,), atomic lmax = 0): the limits depend on p and E only.
  (4, 17) is repeated with a rich angular basis (diatomic lmmax = (2, 1), atomic lmax = 2, mmax = 1): the +-M partner
  channels of k_coulomb_tei and several m groups in the XC kernels at the smallest shape beyond the first limit.

  element order at E = 2: round_up64(p * p) steps at p * p = 64 | 65 (p = 8 | 9), 128 (11 | 12), 192 (13 | 14) and the
  strided loops start their second pass beyond p * p = 256 (16 | 17); the exchange RB kernels change at 16 | 17 too.

Bounds (the project's own, tests/test_gpu_parity.py, test_gpu_rs.py, test_gpu_rs_tei_dev.py, test_gpu_lapl.py): J, K
relative 1e-12; XC: H relative 1e-10, Exc and Nel 1e-11 max(1, |.|), Ekin 1e-10 max(1, |.|); J / K from device-built tables
against host-built tables 1e-13 / 1e-12 (range-separated: 1e-11); model potential 1e-11 (diatomic), 1e-14 (atomic).
Every deviation is printed (pytest -s).

Densities: block-diagonal common.random_density(..., blocks=get_sym_idx(1)) and the mixed one of test_xc_parity
(0.05 general + block-diagonal).  Polarised meta-GGA: Pa = mixed, Pb = 0.5 mixed + 0.25 block-diagonal, so that
rho_b / rho_a stays within [0.5, 0.75] while zeta varies from point to point: where one channel sinks under the density
threshold beside a finite gradient the potentials are ill-conditioned (see _orbital_spin_densities in test_gpu_parity.py)
and two arithmetic routes do not agree to 1e-10 whatever the kernels do.

The Laplacian functional has no counterpart in the oracle library; its reference is tests/lapl_dense.py, as in
tests/test_gpu_lapl.py.

Oracle (CPU) times, seconds on 8 cores, one call, minimal angular basis (tables | J | K | XC 101-130 | XC pol 202-231):
  diatomic (4,16) .01 0 0 .02 .12   (4,17) .02 0 0 .02 .14   (8,16) .08 0 0 .08 .34   (8,17) .09 0 0 .11 .41
           (9,32) .22 .02 .02 .24 .89   (9,33) .20 .01 .02 .30 1.17   (12,48) 1.02 .09 .10 1.01 2.93
           (12,49) .58 .06 .11 1.12 3.56   (14,64) .76 .17 .18 2.16 5.50   (14,65) .74 .14 .26 2.38 6.88
           (15,65) 1.08 .22 .34 3.17 7.94   (4,17) lmmax (2,1) .06 .01 .03 .33 1.76   E = 2, p = 8 ... 17: all < 0.4
  atomic   (9,33) .01 0 0 .16 .57   (12,49) .03 .01 .01 .74 1.70   (14,64) .07 .03 .04 1.96 3.23   (14,65) .06 .03 .03 2.03 3.61
           (15,65) .13 .04 .05 2.90 4.93   (4,17) lmax 2 mmax 1: 0 0 .01 .36 1.50   the smaller shapes and E = 2: all < 0.3
  J and K are whole everywhere, and so is the restricted XC.  The polarised XC of the diatomic (14,64), (14,65) and
  (15,65) exceeds 5 s: there the product runs the radial points Q % 4 == 1 (Context.set_shard, hfg_xc_fock_pol_dev)
  against the oracle's sum over the same points, which lie in every element, the first and the last among them.
  atomic only: lapl_dense set-up + (206, 0): (4,17) .15, lmax 2: 4.1, (9,33) .3, (12,49) .9, (14,65) 1.4, (15,65) 2.1;
  Yukawa tables + K < 0.2 everywhere; erfc pair tables (E^2 blocks of p^4, no restricted form) oracle | product host:
  (4,17) .4 | .3, (9,33) 1.0 | .9, (12,49) 3.8 | 3.5, (14,65) 8.8 | 9.0, (15,65) 11.4 | 11.7, (17,2) 1.1 | 1.1
  (both builds are threaded: on the 16 cores beside an MI355X the slowest test of the module, erfc at (15,65), takes 4.8 s,
  the polarised shards 3.3 - 3.7 s, the whole module 82 s).

Observed on MI355X, worst over all shapes: J 4.8e-16, K 6.8e-16, K general kernels 5.3e-16, device-built tables J 8.5e-16 /
K 1.6e-15, XC 101-130 H 5.1e-14 Exc 4.3e-14 Nel 4.2e-14, XC 202-231 polarised H 1.4e-13 Exc 2.2e-15 Ekin 8.2e-15,
XC 206 H 6.9e-12 Exc 4.3e-16, rs K 1.1e-15 (erfc) 6.7e-16 (Yukawa), model potential 1.2e-15 (diatomic) 0 (atomic).
Before k_coulomb_radial filled its scalars in strided loops, test_coulomb and test_tables_built_on_device failed at the
shapes with 4 * E > bs and at no other: J off by 0.15 - 0.29 of its largest element in the diatomic program, by 2e-9 - 1.75
in the atomic one (whatever the LDS held: at atomic (9,33) and (4,17) lmax 2 one of the two tests met values that passed).
"""
import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

LARGE = [(4, 16), (4, 17), (8, 16), (8, 17), (9, 32), (9, 33), (12, 48), (12, 49), (14, 64), (14, 65), (15, 65)]
ORDERS = [(p, 2) for p in (8, 9, 11, 12, 13, 14, 16, 17)]
ATOMIC = [("atomic", p, E, (0, 0)) for p, E in LARGE] + [("atomic", 4, 17, (2, 1))] + [("atomic", p, E, (0, 0)) for p, E in ORDERS]
DIATOMIC = [("diatomic", p, E, (0,)) for p, E in LARGE] + [("diatomic", 4, 17, (2, 1))] + [("diatomic", p, E, (0,)) for p, E in ORDERS]
# the atomic shapes first: the tests of the atomic program alone then share the parameter indices, hence the cached fixture
SHAPES = ATOMIC + DIATOMIC
# polarised XC of the oracle beyond 5 s (module docstring): a radial shard instead of the whole grid
XC_POL_SHARD = {("diatomic", 14, 64), ("diatomic", 14, 65), ("diatomic", 15, 65)}
SHARD = (1, 4)


def _id(s):
    return "%s-p%d-E%d-ang%s" % (s[0], s[1], s[2], "_".join(str(a) for a in s[3]))


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    if helfem_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the hot path has no CPU fallback")
    return helfem_amd


def _bases(prog, p, E, ang, **kw):
    if prog == "diatomic":
        return common.make_bases(1, 1, 1.4, ang, E, p, **kw)
    return common.make_atomic_bases(10, ang[0], ang[1], E, p, **kw)


def _grid_orders(prog, ang):
    if prog == "diatomic":
        return 4 * max(ang) + 12, 4 * len(ang) + 5
    return 4 * ang[0] + 10, 4 * ang[1] + 5


class Shape(object):
    """product and oracle basis of one shape with host-built tables, uploaded with the XC grid; the two densities"""

    def __init__(self, hf, prog, p, E, ang):
        self.key, self.prog, self.p, self.E, self.ang = (prog, p, E, ang), prog, p, E, ang
        self.gb, self.ob = _bases(prog, p, E, ang)
        self.gb.compute_tei(True)
        self.ob.compute_tei(True)
        self.ldft, self.mdft = _grid_orders(prog, ang)
        self.gb.upload(self.ldft, self.mdft)
        N = self.gb.Nbf()
        self.blocked = common.random_density(N, 2, seed=12, blocks=self.gb.get_sym_idx(1))
        self.mixed = np.asfortranarray(0.05 * common.random_density(N, 3, seed=11) + self.blocked)
        self.ref = {}  # oracle results, computed once and shared by the tests of the shape

    def densities(self):
        return (("blocked", self.blocked), ("mixed", self.mixed))

    def oracle(self, what, tag, P):
        k = (what, tag)
        if k not in self.ref:
            self.ref[k] = self.ob.coulomb(P) if what == "J" else self.ob.exchange(P)
            self.ref[k].setflags(write=False)
        return self.ref[k]


@pytest.fixture(scope="module", params=SHAPES, ids=[_id(s) for s in SHAPES])
def shape(request, hf):
    return Shape(hf, *request.param)


atomic_only = pytest.mark.parametrize("shape", ATOMIC, ids=[_id(s) for s in ATOMIC], indirect=True)


def _report(s, what, err, bound):
    print("%s %s: %.3e (bound %.0e)" % (_id(s.key), what, err, bound))
    return err


def test_coulomb(shape):
    s = shape
    for tag, P in s.densities():
        err = _report(s, "J " + tag, common.relerr(s.gb.coulomb(P), s.oracle("J", tag, P)), 1e-12)
        assert err < 1e-12, (s.key, tag, err)


def test_exchange(shape):
    s = shape
    for tag, P in s.densities():
        err = _report(s, "K " + tag, common.relerr(s.gb.exchange(P), s.oracle("K", tag, P)), 1e-12)
        assert err < 1e-12, (s.key, tag, err)


def test_exchange_general_kernels(shape, monkeypatch):
    """HELFEM_EXCHANGE=general: hip/exchange.hip, one thread per entry of a p x p block"""
    s = shape
    monkeypatch.setenv("HELFEM_EXCHANGE", "general")
    for tag, P in s.densities():
        err = _report(s, "K general kernels " + tag, common.relerr(s.gb.exchange(P), s.oracle("K", tag, P)), 1e-12)
        assert err < 1e-12, (s.key, tag, err)


def _check_xc(s, what, got, ref):
    """got, ref: (H..., Exc, Nel, Ekin)"""
    (Hs, (Exc, Nel, Ekin)), (Hos, (Exco, Nelo, Ekino)) = (got[:-3], got[-3:]), (ref[:-3], ref[-3:])
    eH = max(_report(s, what + " H", common.relerr(H, Ho), 1e-10) for H, Ho in zip(Hs, Hos))
    eX = _report(s, what + " Exc", abs(Exc - Exco) / max(1.0, abs(Exco)), 1e-11)
    eN = _report(s, what + " Nel", abs(Nel - Nelo) / max(1.0, abs(Nelo)), 1e-11)
    eK = _report(s, what + " Ekin", abs(Ekin - Ekino) / max(1.0, abs(Ekino)), 1e-10)
    assert all(np.max(np.abs(Ho)) > 0.0 for Ho in Hos)
    assert eH < 1e-10 and eX < 1e-11 and eN < 1e-11 and eK < 1e-10, (s.key, what, eH, eX, eN, eK)


def test_xc_restricted(shape, hf):
    s = shape
    grid = hf.DFTGrid(s.gb, s.ldft, s.mdft)
    for tag, P in s.densities():
        _check_xc(s, "XC 101-130 " + tag, grid.eval_Fxc(101, 130, P), s.ob.eval_Fxc(s.ldft, s.mdft, 101, 130, P))


def test_xc_polarised(shape, hf):
    s = shape
    grid = hf.DFTGrid(s.gb, s.ldft, s.mdft)
    Pa, Pb = s.mixed, np.asfortranarray(0.5 * s.mixed + 0.25 * s.blocked)
    if s.key[:3] in XC_POL_SHARD:
        rank, n = SHARD
        s.gb.ctx.set_shard(rank, n)
        try:
            got = grid.eval_Fxc_dev(202, 231, Pa, Pb)
        finally:
            s.gb.ctx.set_shard(0, 1)
        pts = [q for q in range(s.E * 5 * s.p) if q % n == rank]  # make_bases: nquad = 5 nnodes points per element
        ref = s.ob.eval_Fxc_points(s.ldft, s.mdft, 202, 231, Pa, pts, Pb=Pb, threads=8)
        what = "XC pol 202-231 points Q %% %d == %d" % (n, rank)
    else:
        got = grid.eval_Fxc_pol(202, 231, Pa, Pb)
        ref = s.ob.eval_Fxc_pol(s.ldft, s.mdft, 202, 231, Pa, Pb)
        what = "XC pol 202-231"
    assert ref[-1] > 0.0  # the kinetic energy density is there
    _check_xc(s, what, got, ref)


def test_tables_built_on_device(shape, hf):
    """hfg_compute_tei_dev: J and K from device-built tables against those from the host-built tables, as
    test_tei_tables_built_on_device_match_host_tables compares them, and against the oracle"""
    s = shape
    gd, _ = _bases(s.prog, s.p, s.E, s.ang, oracle=False)
    gd.compute_tei(True, device=True)
    gd.upload()
    for tag, P in s.densities():
        Jd, Kd = gd.coulomb(P), gd.exchange(P)
        eJ = _report(s, "J device tables vs host tables " + tag, common.relerr(Jd, s.gb.coulomb(P)), 1e-13)
        eK = _report(s, "K device tables vs host tables " + tag, common.relerr(Kd, s.gb.exchange(P)), 1e-12)
        eJo = _report(s, "J device tables vs oracle " + tag, common.relerr(Jd, s.oracle("J", tag, P)), 1e-12)
        eKo = _report(s, "K device tables vs oracle " + tag, common.relerr(Kd, s.oracle("K", tag, P)), 1e-12)
        assert eJ < 1e-13 and eK < 1e-12 and eJo < 1e-12 and eKo < 1e-12, (s.key, tag, eJ, eK, eJo, eKo)


@atomic_only
def test_atomic_xc_laplacian(shape, hf):
    """mgga_x_br89 (206): the Laplacian planes of the XC kernels, against the dense restatement of tests/lapl_dense.py"""
    import lapl_dense
    s = shape
    dense = lapl_dense.DenseWorker(hf, s.gb, hf.get_grid(40.0, s.E, 4, 2.0), s.p, s.ldft, s.mdft)
    grid = hf.DFTGrid(s.gb, s.ldft, s.mdft)
    for tag, P in s.densities():
        H, Exc, Nel, _ = grid.eval_Fxc(206, 0, P)
        Hd, Excd, Neld = dense.eval_Fxc(206, 0, P)
        eH = _report(s, "XC 206-0 H " + tag, common.relerr(H, Hd), 1e-10)
        eX = _report(s, "XC 206-0 Exc " + tag, abs(Exc - Excd) / max(1.0, abs(Excd)), 1e-11)
        eN = _report(s, "XC 206-0 Nel " + tag, abs(Nel - Neld) / max(1.0, abs(Neld)), 1e-11)
        assert eH < 1e-10 and eX < 1e-11 and eN < 1e-11, (s.key, tag, eH, eX, eN)


@atomic_only
@pytest.mark.parametrize("kind", ["yukawa", "erfc"])
def test_atomic_rs_exchange(shape, hf, kind):
    """hfg_rs_exchange as tests/test_gpu_rs.py calls it, with host-built tables against the oracle; then with the tables of
    hfg_compute_rs_tei_dev against the host-built ones (the bound of tests/test_gpu_rs_tei_dev.py) and the oracle"""
    s = shape
    getattr(s.gb, "compute_" + kind)(0.4)
    getattr(s.ob, "compute_" + kind)(0.4)
    gd, _ = _bases(s.prog, s.p, s.E, s.ang, oracle=False)
    gd.ctx = hf.default_context()
    gd.compute_tei(True, device=True)
    getattr(gd, "compute_" + kind)(0.4, device=True)
    for tag, P in s.densities():
        Ko = s.ob.rs_exchange(P)
        Kh, Kd = s.gb.rs_exchange(P), gd.rs_exchange(P)
        eh = _report(s, "rs K %s %s" % (kind, tag), common.relerr(Kh, Ko), 1e-12)
        ed = _report(s, "rs K %s device tables vs host tables %s" % (kind, tag), common.relerr(Kd, Kh), 1e-11)
        edo = _report(s, "rs K %s device tables vs oracle %s" % (kind, tag), common.relerr(Kd, Ko), 1e-12)
        assert eh < 1e-12 and ed <= 1e-11 and edo < 1e-12, (s.key, kind, tag, eh, ed, edo)


@pytest.mark.parametrize("p,E", [(4, 17), (14, 65)])
def test_model_potential_diatomic(hf, p, E):
    """hfg_model_potential (k_mp_fill and the XC Fock kernels) against the oracle's TwoDGrid::model_potential"""
    import oracle_lib as orc
    gb, ob = _bases("diatomic", p, E, (0,))
    gb.compute_tei(False)
    ldft, mdft = _grid_orders("diatomic", (0,))
    gb.upload(ldft, mdft)
    for pots in (((3, 3), (3, 1)), ((1, 3, 0.56), (1, 1, 1.0))):
        err = common.relerr(gb.model_potential(*pots), orc.model_potential(ob, pots[0], pots[1], lang=ldft, mang=mdft))
        print("diatomic-p%d-E%d model potential %s: %.3e (bound 1e-11)" % (p, E, pots, err))
        assert err < 1e-11, (p, E, pots, err)


@pytest.mark.parametrize("p,E", [(4, 17), (14, 65)])
def test_model_potential_atomic(hf, p, E):
    import oracle_lib as orc
    ga, oa = _bases("atomic", p, E, (0, 0))
    ga.compute_tei(False)
    for pot in ((3, 10), (0, 10)):
        err = common.relerr(ga.model_potential(pot), orc.model_potential(oa, pot))
        print("atomic-p%d-E%d model potential %s: %.3e (bound 1e-14)" % (p, E, pot, err))
        assert err < 1e-14, (p, E, pot, err)


def test_general_exchange_refuses_more_than_32_nodes(hf, monkeypatch):
    """k_ex_radial takes one thread per entry of a p x p block: beyond 32 nodes that is more than a workgroup holds, and
    the general kernels say so instead of failing at the launch"""
    gb, _ = _bases("atomic", 33, 1, (0, 0), oracle=False)
    gb.compute_tei(True)
    monkeypatch.setenv("HELFEM_EXCHANGE", "general")
    N = gb.Nbf()
    with pytest.raises(RuntimeError, match="at most 32 nodes per element"):
        gb.exchange(np.eye(N, order="F"))
