"""Short-range GGA exchange and the range-separated GGA hybrids (CAM-B3LYP, CAMY-B3LYP, CAMY-BLYP, LCY-BLYP, LCY-PBE) on the
GPU.  The CPU oracle does not know these functionals and there is no libxc: nothing here is oracle SCF parity.  The XC
kernels are compared with the dense NumPy grid worker of tests/lapl_dense.py, whose point values come from the independent
restatement of tests/rsgga_restatement.py (pinned against 120-digit closed forms in test_rsgga_cpu.py); the Fock matrix with
differences of Exc; shards with the whole; the SCF drivers with each other; and the converged total energy with a sum of
pieces that are pinned elsewhere (T, V, J, K and the screened K against the oracle; Exc by the dense worker)."""
import ctypes
import statistics

import numpy as np
import pytest

import common
import rsgga_restatement as rs

pytestmark = pytest.mark.gpu

CASES = {  # the atomic cases of tests/test_gpu_scan.py: (Z, lmax, mmax, nelem, nnodes)
    "sp": (10, 1, 1, 3, 5),
    "spd_m1": (18, 2, 1, 2, 6),
}
HYB_IDS = [h["id"] for h in rs.HYBRIDS.values()]


@pytest.fixture(scope="module")
def hf():
    import helfem_amd
    if helfem_amd.device_count() < 1:
        pytest.fail("no HIP device visible")
    return helfem_amd


@pytest.fixture(scope="module")
def new_ids(hf):
    return [hf.xc_func_ids(n)[0] for n in rs.PRIMITIVES] + HYB_IDS


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request, hf):
    import lapl_dense
    Z, lmax, mmax, nelem, nnodes = CASES[request.param]
    gb, _ = common.make_atomic_bases(Z, lmax, mmax, nelem, nnodes, oracle=False)
    gb.compute_tei(True)
    ldft, mdft = 4 * lmax + 10, 4 * mmax + 5
    gb.upload(ldft, mdft)
    dense = lapl_dense.DenseWorker(rs.Evaluator(hf), gb, hf.get_grid(40.0, nelem, 4, 2.0), nnodes, ldft, mdft)
    return request.param, gb, dense, ldft, mdft, gb.get_sym_idx(1)


def _pd(gb, blocks, seed):
    return common.random_density(gb.Nbf(), 2, seed=seed, blocks=blocks)


# ---------------------------------------------------------------------------------------------------------------------
# 1. grid parity with the dense worker; the bounds are those of tests/test_gpu_scan.py:55-57 and :67-69
#    (test_atomic_restricted_parity_with_dense_restatement): 1e-11 relative for Exc and Nel, 1e-10 for the Fock matrix
# ---------------------------------------------------------------------------------------------------------------------
def test_atomic_restricted_parity_with_dense_restatement(hf, case, new_ids):
    name, gb, dense, ldft, mdft, blocks = case
    P = _pd(gb, blocks, 3)
    for x, c in [(i, 0) for i in new_ids] + [(529, 131), (new_ids[3], 130)]:
        H, Exc, Nel, _ = hf.DFTGrid(gb, ldft, mdft).eval_Fxc(x, c, P)
        Hd, Excd, Neld = dense.eval_Fxc(x, c, P)
        print("restricted", name, x, c, "Exc %.12f dExc/Exc %.2e dH %.2e" % (Exc, abs(Exc - Excd) / abs(Excd), common.relerr(H, Hd)))
        assert abs(Exc - Excd) <= 1e-11 * abs(Excd), (name, x, c, Exc, Excd)
        assert abs(Nel - Neld) <= 1e-11 * abs(Neld)
        assert common.relerr(H, Hd) <= 1e-10, (name, x, c, common.relerr(H, Hd))


def test_atomic_polarised_parity_with_dense_restatement(hf, case, new_ids):
    """an open-shell density: Pb is not a multiple of Pa"""
    name, gb, dense, ldft, mdft, blocks = case
    Pa, Pb = _pd(gb, blocks, 4), 0.5 * _pd(gb, blocks, 5)
    for x, c in [(i, 0) for i in new_ids] + [(529, 131)]:
        Ha, Hb, Exc, Nel, _ = hf.DFTGrid(gb, ldft, mdft).eval_Fxc_pol(x, c, Pa, Pb)
        Had, Hbd, Excd, Neld = dense.eval_Fxc_pol(x, c, Pa, Pb)
        print("polarised", name, x, c, "Exc %.12f dExc/Exc %.2e dHa %.2e dHb %.2e" % (Exc, abs(Exc - Excd) / abs(Excd), common.relerr(Ha, Had),
                                                                                  common.relerr(Hb, Hbd)))
        assert abs(Exc - Excd) <= 1e-11 * abs(Excd), (name, x, c, Exc, Excd)
        assert abs(Nel - Neld) <= 1e-11 * abs(Neld)
        assert common.relerr(Ha, Had) <= 1e-10 and common.relerr(Hb, Hbd) <= 1e-10, (x, c, common.relerr(Ha, Had), common.relerr(Hb, Hbd))


# ---------------------------------------------------------------------------------------------------------------------
# 2. Fock = dExc/dP (central differences with one Richardson step; step and bound of tests/test_gpu_scan.py:108-116)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ne(hf):
    gb, _ = common.make_atomic_bases(10, 1, 1, 3, 5, oracle=False)
    gb.compute_tei(True)
    ldft, mdft = 14, 9
    gb.upload(ldft, mdft)
    return gb, hf.DFTGrid(gb, ldft, mdft), gb.get_sym_idx(1)


def _directions(gb, blocks, n=3, seed=11):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        D = np.zeros((gb.Nbf(), gb.Nbf()))
        for b in blocks:
            X = rng.uniform(-1, 1, (len(b), len(b)))
            D[np.ix_(b, b)] = X + X.T
        out.append(D)
    return out


def _richardson(f, h):
    c = lambda s: (f(s) - f(-s)) / (2 * s)  # noqa: E731
    return (4 * c(h / 2) - c(h)) / 3


@pytest.mark.parametrize("fid", [433, 468])
def test_fock_matrix_is_the_derivative_of_exc(hf, ne, fid):
    gb, g, blocks = ne
    P = _pd(gb, blocks, 6)
    H, _, _, _ = g.eval_Fxc(fid, 0, P)
    Pa, Pb = _pd(gb, blocks, 7), 0.5 * _pd(gb, blocks, 8)
    Ha, Hb, _, _, _ = g.eval_Fxc_pol(fid, 0, Pa, Pb)
    h = 1e-4
    for D in _directions(gb, blocks):
        fd = _richardson(lambda t: g.eval_Fxc(fid, 0, P + t * D)[1], h)
        an = np.sum(H * D)
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1e-3), (fd, an)
        fda = _richardson(lambda t: g.eval_Fxc_pol(fid, 0, Pa + t * D, Pb)[2], h)
        fdb = _richardson(lambda t: g.eval_Fxc_pol(fid, 0, Pa, Pb + t * D)[2], h)
        assert abs(fda - np.sum(Ha * D)) <= 1e-6 * max(abs(fda), 1e-3), (fda, np.sum(Ha * D))
        assert abs(fdb - np.sum(Hb * D)) <= 1e-6 * max(abs(fdb), 1e-3), (fdb, np.sum(Hb * D))


# ---------------------------------------------------------------------------------------------------------------------
# 3. shards; bitwise repeatability
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", [433, 467])
def test_shards_sum_to_the_unsharded_result(hf, ne, fid):
    gb, g, blocks = ne
    P = _pd(gb, blocks, 10)
    Pa, Pb = _pd(gb, blocks, 12), 0.5 * _pd(gb, blocks, 13)
    H, Exc, _, _ = g.eval_Fxc_dev(fid, 0, P)
    Ha, Hb, Excp, _, _ = g.eval_Fxc_dev(fid, 0, Pa, Pb)
    ctx = gb.ctx
    for n in (2, 3):
        acc, e, accA, accB, ep = np.zeros_like(H), 0.0, np.zeros_like(H), np.zeros_like(H), 0.0
        try:
            for rk in range(n):
                ctx.set_shard(rk, n)
                h, x, _, _ = g.eval_Fxc_dev(fid, 0, P)
                acc += h
                e += x
                ha, hb, xp, _, _ = g.eval_Fxc_dev(fid, 0, Pa, Pb)
                accA += ha
                accB += hb
                ep += xp
        finally:
            ctx.set_shard(0, 1)
        assert common.relerr(acc, H) <= 1e-12 and abs(e - Exc) <= 1e-12 * abs(Exc)
        assert common.relerr(accA, Ha) <= 1e-12 and common.relerr(accB, Hb) <= 1e-12 and abs(ep - Excp) <= 1e-12 * abs(Excp)


def test_restricted_is_reproducible_bitwise(hf, ne, new_ids):
    gb, g, blocks = ne
    P = _pd(gb, blocks, 14)
    for fid in new_ids:
        a, b = g.eval_Fxc(fid, 0, P), g.eval_Fxc(fid, 0, P)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1], fid


# ---------------------------------------------------------------------------------------------------------------------
# 4. omega as an external parameter on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_omega_is_an_external_parameter_of_the_primitives(hf, ne):
    gb, g, blocks = ne
    N = gb.Nbf()
    P = np.asfortranarray(_pd(gb, blocks, 15))
    Pa, Pb = np.asfortranarray(_pd(gb, blocks, 16)), np.asfortranarray(0.5 * _pd(gb, blocks, 17))
    L = hf.lib()
    dp = ctypes.POINTER(ctypes.c_double)
    L.hfg_xc_fock_ext.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, dp, ctypes.c_int, ctypes.c_int, dp, ctypes.c_int, dp, dp,
                                  dp, dp, dp, ctypes.c_double]
    L.hfg_xc_fock_pol_ext.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, dp, ctypes.c_int, ctypes.c_int, dp, ctypes.c_int,
                                      dp, dp, dp, dp, dp, dp, dp, ctypes.c_double]

    def ext(fid, pars):
        xa = np.array(pars, dtype=float)
        H = np.zeros((N, N), order="F")
        exc, nel, ekin = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        rc = L.hfg_xc_fock_ext(gb.ctx.h, gb.h, fid, xa.ctypes.data_as(dp), len(pars), 0, None, 0, P.ctypes.data_as(dp), H.ctypes.data_as(dp),
                               ctypes.byref(exc), ctypes.byref(nel), ctypes.byref(ekin), 1e-12)
        return rc, H, exc.value

    def ext_pol(fid, pars):
        xa = np.array(pars, dtype=float)
        Ha, Hb = np.zeros((N, N), order="F"), np.zeros((N, N), order="F")
        exc, nel, ekin = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        rc = L.hfg_xc_fock_pol_ext(gb.ctx.h, gb.h, fid, xa.ctypes.data_as(dp), len(pars), 0, None, 0, Pa.ctypes.data_as(dp),
                                   Pb.ctypes.data_as(dp), Ha.ctypes.data_as(dp), Hb.ctypes.data_as(dp), ctypes.byref(exc), ctypes.byref(nel),
                                   ctypes.byref(ekin), 1e-12)
        return rc, Ha, Hb, exc.value

    for name, p in rs.PRIMITIVES.items():
        fid = hf.xc_func_ids(name)[0]
        H0, E0, _, _ = g.eval_Fxc(fid, 0, P)
        rc, H1, E1 = ext(fid, [p["omega"]])
        assert rc == 0, L.hfg_last_error()
        assert E1 == E0 and np.array_equal(H1, H0), name  # the default is the functional's own omega, bitwise
        rc, H2, E2 = ext(fid, [0.5])
        assert rc == 0 and abs(E2 - E0) > 1e-3 * abs(E0), (name, E0, E2)
        assert g.eval_Fxc(fid, 0, P)[1] == E0  # in force for its call only
        Ha0, Hb0, Ep0, _, _ = g.eval_Fxc_pol(fid, 0, Pa, Pb)
        rc, Ha1, Hb1, Ep1 = ext_pol(fid, [p["omega"]])
        assert rc == 0 and Ep1 == Ep0 and np.array_equal(Ha1, Ha0) and np.array_equal(Hb1, Hb0), name
        rc, _, _, Ep2 = ext_pol(fid, [0.5])
        assert rc == 0 and abs(Ep2 - Ep0) > 1e-3 * abs(Ep0), name
    assert ext(529, [0.2, 0.3])[0] != 0 and "with 2 values" in L.hfg_last_error().decode()
    assert ext(433, [0.33])[0] != 0
    assert ext(529, [-1.0])[0] != 0 and "omega must be positive" in L.hfg_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------------
# 5. SCF: the basis sizes of RS_SCF_CASES in tests/test_gpu_rs.py
# ---------------------------------------------------------------------------------------------------------------------
SYSTEMS = [("He", dict(Z=2, lmax=0, mmax=0, nelem=5, nnodes=10)), ("Li_M2", dict(Z=3, lmax=0, mmax=0, nelem=5, nnodes=10, M=2)),
           ("Ne", dict(Z=10, lmax=1, mmax=1, nelem=5, nnodes=10))]
METHODS = ["hyb_gga_xc_cam_b3lyp", "hyb_gga_xc_camy_b3lyp", "hyb_gga_xc_lcy_pbe"]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("sysname,kw", SYSTEMS, ids=[s[0] for s in SYSTEMS])
def test_scf_converges_and_the_drivers_agree(hf, sysname, kw, method, monkeypatch):
    """the run converges to convthr; the device-resident and the host-pointer driver agree to the bound of
    tests/test_gpu_scan.py:277 (1e-8 relative to max(1, |E|)); the screened exchange build that ran is the functional's"""
    ctx = hf.default_context()
    kind = hf.xc_rs_kind(hf.xc_func_ids(method)[0])
    mine, other = ("exchange_yukawa", "exchange_erfc") if kind == 1 else ("exchange_erfc", "exchange_yukawa")
    out = {}
    for driver in ("device", "host"):
        if driver == "host":
            monkeypatch.setenv("HELFEM_SCF", "host")
        ctx.profile(True)
        ctx.profile_reset()
        try:
            out[driver] = hf.scf_atomic(method=method, convthr=1e-9, maxit=80, **kw)
            ctx.synchronize()
            calls = {n: ctx.profile_get(n)[1] for n in ctx.profile_names()}
        finally:
            ctx.profile(False)
        print("SCF", sysname, method, driver, "Etot %.10f Exx %.10f Exc %.10f it %d" % (out[driver]["Etot"], out[driver]["Exx"],
                                                                                      out[driver]["Exc"], out[driver]["iterations"]), calls)
        assert out[driver]["converged"], (driver, out[driver])
        assert calls.get(mine, 0) > 0 and calls.get(other, 0) == 0 and calls.get("exchange", 0) > 0, (driver, calls)
    dev, host = out["device"], out["host"]
    for k in ("Etot", "Exc", "Exx"):
        assert abs(dev[k] - host[k]) < 1e-8 * max(1.0, abs(host[k])), (k, dev[k], host[k])
    assert dev["Exx"] < -0.1


# ---------------------------------------------------------------------------------------------------------------------
# 6. the total energy from separately pinned pieces
# ---------------------------------------------------------------------------------------------------------------------
class _Opt(ctypes.Structure):  # hfg_scf_options of include/helfem_gpu.h
    _fields_ = [("program", ctypes.c_int), ("Z1", ctypes.c_int), ("Z2", ctypes.c_int), ("Rbond", ctypes.c_double),
                ("nela", ctypes.c_int), ("nelb", ctypes.c_int), ("Q", ctypes.c_int), ("M", ctypes.c_int),
                ("lmmax", ctypes.c_int * 16), ("nlm", ctypes.c_int), ("lmax", ctypes.c_int), ("mmax", ctypes.c_int),
                ("lpad", ctypes.c_int), ("Rmax", ctypes.c_double), ("grid", ctypes.c_int), ("zexp", ctypes.c_double),
                ("nelem", ctypes.c_int), ("nnodes", ctypes.c_int), ("nquad", ctypes.c_int), ("maxit", ctypes.c_int),
                ("convthr", ctypes.c_double), ("diag", ctypes.c_int), ("method", ctypes.c_char * 128), ("ldft", ctypes.c_int),
                ("mdft", ctypes.c_int), ("dftthr", ctypes.c_double), ("restricted", ctypes.c_int), ("symmetry", ctypes.c_int),
                ("primbas", ctypes.c_int), ("diiseps", ctypes.c_double), ("diisthr", ctypes.c_double), ("diisorder", ctypes.c_int),
                ("iguess", ctypes.c_int), ("x_pars", ctypes.c_void_p), ("n_x_pars", ctypes.c_int), ("c_pars", ctypes.c_void_p),
                ("n_c_pars", ctypes.c_int), ("maverage", ctypes.c_int), ("dampfock", ctypes.c_double), ("dampthr", ctypes.c_double),
                ("save", ctypes.c_char * 512), ("load", ctypes.c_char * 512), ("Ez", ctypes.c_double), ("Qzz", ctypes.c_double),
                ("Bz", ctypes.c_double), ("finitenuc", ctypes.c_int), ("readocc", ctypes.c_int), ("occs", ctypes.c_void_p),
                ("occ_rows", ctypes.c_int), ("occ_cols", ctypes.c_int), ("perturb", ctypes.c_double), ("iconf", ctypes.c_int),
                ("zeroder", ctypes.c_int), ("verbose", ctypes.c_int)]


class _Res(ctypes.Structure):
    _fields_ = [("Etot", ctypes.c_double), ("Ekin", ctypes.c_double), ("Epot", ctypes.c_double), ("Enucr", ctypes.c_double),
                ("Ecoul", ctypes.c_double), ("Exx", ctypes.c_double), ("Exc", ctypes.c_double), ("iterations", ctypes.c_int),
                ("converged", ctypes.c_int), ("nela", ctypes.c_int), ("nelb", ctypes.c_int), ("Nbf", ctypes.c_int64),
                ("tJ", ctypes.c_double), ("tK", ctypes.c_double), ("tXC", ctypes.c_double), ("tdiag", ctypes.c_double)]


@pytest.mark.parametrize("method", ["hyb_gga_xc_cam_b3lyp", "hyb_gga_xc_lcy_pbe"])
def test_total_energy_from_pinned_pieces(hf, method):
    """Ne, restricted: E = Tr P (T + V) + 1/2 Tr P J + Tr Pa [kfrac K(Pa) + kshort K_screened(Pa)] + Exc, with T, V, J, K and the
    screened K from the entry points that are pinned against the oracle and Exc from the dense worker with the restatement,
    at the orbitals the driver returns; against the driver's total to 1e-8 Eh"""
    import lapl_dense
    Z, lmax, mmax, nelem, nnodes = 10, 1, 1, 5, 10
    L = hf.lib()
    o = _Opt()
    L.hfg_scf_options_default.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert L.hfg_scf_options_default(ctypes.byref(o), 1) == 0
    o.Z1, o.lmax, o.mmax, o.nelem, o.nnodes, o.method = Z, lmax, mmax, nelem, nnodes, method.encode()
    o.convthr, o.maxit, o.iguess, o.save, o.verbose = 1e-10, 100, 0, b"", 0
    gb, _ = common.make_atomic_bases(Z, lmax, mmax, nelem, nnodes, oracle=False)
    N = gb.Nbf()
    res = _Res()
    E, C = np.zeros(N), np.zeros((N, N), order="F")
    dp = ctypes.POINTER(ctypes.c_double)
    L.hfg_scf_run.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, dp, dp]
    rc = L.hfg_scf_run(hf.default_context().h, ctypes.byref(o), ctypes.byref(res), E.ctypes.data_as(dp), C.ctypes.data_as(dp))
    assert rc == 0, L.hfg_last_error()
    assert res.converged and res.Nbf == N and res.nela == 5 and res.nelb == 5
    Pa = np.asfortranarray(C[:, :5] @ C[:, :5].T)
    P = 2 * Pa
    fid = hf.xc_func_ids(method)[0]
    omega, kfrac, kshort = hf.xc_exact_exchange(fid)
    gb.compute_tei(True)
    if hf.xc_rs_kind(fid) == 1:
        gb.compute_yukawa(omega)
    else:
        gb.compute_erfc(omega)
    ldft, mdft = 4 * lmax + 10, 4 * mmax + 5
    gb.upload(ldft, mdft)
    e1 = np.sum(P * (gb.kinetic() + gb.nuclear()))
    ej = 0.5 * np.sum(P * gb.coulomb(P))
    ek = np.sum(Pa * (kfrac * gb.exchange(Pa) + kshort * gb.rs_exchange(Pa)))
    dense = lapl_dense.DenseWorker(rs.Evaluator(hf), gb, hf.get_grid(40.0, nelem, 4, 2.0), nnodes, ldft, mdft)
    _, exc, nel = dense.eval_Fxc(fid, 0, P)
    total = e1 + ej + ek + exc
    print("recomposition", method, "driver %.12f pieces %.12f (one-electron %.12f, J %.12f, K %.12f, Exc %.12f) difference %.3e" %
          (res.Etot, total, e1, ej, ek, exc, total - res.Etot))
    print("   driver: Ekin + Epot %.12f Ecoul %.12f Exx %.12f Exc %.12f" % (res.Ekin + res.Epot, res.Ecoul, res.Exx, res.Exc))
    assert abs(nel - 10.0) < 1e-8
    assert abs(total - res.Etot) <= 1e-8, (total, res.Etot)


# ---------------------------------------------------------------------------------------------------------------------
# 7. stage times, recorded, not asserted
# ---------------------------------------------------------------------------------------------------------------------
def test_stage_times_b3lyp_and_cam_b3lyp(hf):
    """Ar at the basis of BASELINE's config 2 (lmax = mmax = 1, 20 elements of 15 nodes): per-call HIP-event times of the XC stage
    and of the exchange builds, three runs each, alternating"""
    ctx = hf.default_context()
    kw = dict(Z=18, lmax=1, mmax=1, nelem=20, nnodes=15, convthr=1e-7, maxit=12)
    rec = {402: [], 433: []}
    for rep in range(3):
        for fid in (402, 433):
            ctx.profile(True)
            ctx.profile_reset()
            try:
                r = hf.scf_atomic(method=hf.xc_func_name(fid), **kw)
                ctx.synchronize()
                t = {}
                for n in ("xc", "exchange", "exchange_erfc", "coulomb"):
                    if n in ctx.profile_names():
                        ms, calls = ctx.profile_get(n)
                        t[n] = ms / max(calls, 1)
            finally:
                ctx.profile(False)
            rec[fid].append(t)
            print("stage times [ms per call]", hf.xc_func_name(fid), "run", rep, {k: round(v, 4) for k, v in t.items()}, "iterations", r["iterations"])
    for fid in rec:
        for n in sorted(set().union(*[set(t) for t in rec[fid]])):
            v = [t[n] for t in rec[fid] if n in t]
            print("stage median [ms per call]", hf.xc_func_name(fid), n, "median %.4f min %.4f max %.4f" % (statistics.median(v), min(v), max(v)))
    assert all("xc" in t for t in rec[402] + rec[433])
