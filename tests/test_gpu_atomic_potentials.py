"""SCF runs of the atomic program with confinement, a finite nucleus and off-centre nuclei on the device, through
hfg_scf_run_ex and the `atomic` executable.  Checkers: a NumPy SCF on the library's host one-electron matrices with the CPU
oracle's Coulomb and exchange matrices (HF on He and H2), and the energy functional recomputed from the converged density
with the host-pointer entry points hfg_coulomb / hfg_exchange / hfg_xc_fock.  Bars: 1e-8 Eh on Etot, 1e-10 relative on Econf."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.linalg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "helfem_amd", "bin")
NN = 10


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    if helfem_amd.device_count() < 1:
        pytest.fail("no gfx950 device: the GPU tests need one")
    from helfem_amd import build
    build.build_cli(verbose=False)
    return helfem_amd


def setup(hf, Z, lmax, mmax, nelem, opts, extras):
    """grid, basis and one-electron matrices of a run, from the same host entry points the driver uses"""
    x = dict(Rrms=0.0, conf_N=0, conf_R=0.0, conf_barrier=0.0, shift_conf=0.0, add_conf=1, Zl=0, Zr=0, Rmid=0.0, nelem0=0)
    x.update(extras)
    g = hf.atomic_grid(nelem, Rmax=40.0, finitenuc=opts.get("finitenuc", 0), Rrms=x["Rrms"], nelem0=x["nelem0"], Z=Z, Zl=x["Zl"],
                       Zr=x["Zr"], Rmid=x["Rmid"], add_conf=bool(x["add_conf"]), shift_conf=x["shift_conf"])
    l, m = hf.angular_basis(lmax, mmax)
    b = hf.AtomicTwoDBasis(Z, NN, 5 * NN, g, l, m, finitenuc=opts.get("finitenuc", 0), Rrms=x["Rrms"], Zl=x["Zl"], Zr=x["Zr"],
                           Rmid=x["Rmid"])
    Vc = b.confinement(opts.get("iconf", 0), x["conf_N"], x["conf_R"], x["conf_barrier"], x["shift_conf"])
    Enucr = (Z * (x["Zl"] + x["Zr"]) / x["Rmid"] + x["Zl"] * x["Zr"] / (2 * x["Rmid"])) if x["Rmid"] > 0 else 0.0
    return g, l, m, b, Vc, Enucr


def run(hf, Z, lmax, mmax, nelem, method, opts, extras, convthr=1e-9):
    g, l, m, b, Vc, Enucr = setup(hf, Z, lmax, mmax, nelem, opts, extras)
    N = b.Nbf()
    E, C = np.zeros(N), np.zeros((N, N), order="F")
    r = hf.scf_run_atomic(Z, lmax, mmax, nelem, NN, method, E=E, C=C, extras=extras, convthr=convthr, maxit=80, **opts)
    assert r["converged"] and r["Nbf"] == N
    return r, C, b, Vc, Enucr


def read_mat(hf, path, name):
    L = hf.lib()
    dp, i64 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    L.hfg_chk_open.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.hfg_chk_read_mat.argtypes = [ctypes.c_void_p, ctypes.c_char_p, dp, i64, i64]
    L.hfg_chk_close.argtypes = [ctypes.c_void_p]
    h, r, c = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
    assert L.hfg_chk_open(path.encode(), 0, ctypes.byref(h)) == 0, L.hfg_last_error()
    assert L.hfg_chk_read_mat(h, name.encode(), None, ctypes.byref(r), ctypes.byref(c)) == 0, L.hfg_last_error()
    M = np.zeros((r.value, c.value), order="F")
    assert L.hfg_chk_read_mat(h, name.encode(), M.ctypes.data_as(dp), ctypes.byref(r), ctypes.byref(c)) == 0, L.hfg_last_error()
    L.hfg_chk_close(h)
    return M


def energy_from_density(hf, b, C, nocc, Vc, Enucr, method, lmax, mmax):
    """E[P] with the host-pointer entry points (unsharded, complete by contract)"""
    P = np.asfortranarray(2.0 * C[:, :nocc] @ C[:, :nocc].T)
    x_func, c_func = hf.xc_func_ids(method)
    dft = x_func > 0 or c_func > 0
    b.compute_tei(True)
    b.upload(4 * lmax + 10 if dft else 0, 4 * mmax + 5 if dft else 0)
    H0 = b.kinetic() + b.nuclear() + Vc
    E = np.sum(P * H0) + 0.5 * np.sum(P * b.coulomb(P)) + Enucr
    if dft:
        _, Exc, _, _ = hf.DFTGrid(b, 4 * lmax + 10, 4 * mmax + 5).eval_Fxc(x_func, c_func, P)
        E += Exc
    else:
        E += 0.5 * np.sum(P * b.exchange(P / 2.0))  # K[Pa] is returned with its sign: Exx = tr(Pa K[Pa]) for a closed shell
    return E, np.sum(P * Vc)


def numpy_hf(H0, S, J_of, K_of, nocc, Enucr, tol=1e-11):
    """closed-shell Roothaan iterations with plain DIIS on host matrices"""
    _, C = scipy.linalg.eigh(H0, S)
    Fs, Es, Eold = [], [], 0.0
    for it in range(200):
        Pa = C[:, :nocc] @ C[:, :nocc].T
        P = 2 * Pa
        J, K = J_of(P), K_of(Pa)
        F = H0 + J + K
        E = np.sum(P * H0) + 0.5 * np.sum(P * J) + np.sum(Pa * K) + Enucr
        err = F @ P @ S - S @ P @ F
        Fs, Es = (Fs + [F])[-8:], (Es + [err])[-8:]
        n = len(Fs)
        B = -np.ones((n + 1, n + 1))
        B[n, n] = 0.0
        for i in range(n):
            for j in range(n):
                B[i, j] = np.sum(Es[i] * Es[j])
        rhs = np.zeros(n + 1)
        rhs[n] = -1.0
        try:
            c = np.linalg.solve(B, rhs)[:n]
        except np.linalg.LinAlgError:
            c = np.zeros(n)
            c[-1] = 1.0
        _, C = scipy.linalg.eigh(sum(ci * Fi for ci, Fi in zip(c, Fs)), S)
        if abs(E - Eold) < tol and np.abs(err).max() < 1e-8:
            return E
        Eold = E
    raise AssertionError("the NumPy SCF did not converge")


HE_BARRIER = dict(opts=dict(iconf=3), extras=dict(conf_barrier=1.0, shift_conf=6.0))


def test_he_hf_in_a_barrier_against_numpy_scf(hf, tmp_path):
    import oracle_lib as orc
    if not hf.lib().hfg_chk_available():
        pytest.fail("no HDF5 library: the density of the last iteration is read from the checkpoint")
    chk = str(tmp_path / "he.chk")
    r, C, b, Vc, Enucr = run(hf, 2, 0, 0, 5, "HF", dict(HE_BARRIER["opts"], save=chk), HE_BARRIER["extras"])
    g, l, m, _, _, _ = setup(hf, 2, 0, 0, 5, **HE_BARRIER)
    ob = orc.OracleAtomicBasis(2, NN, 5 * NN, g, l, m)
    ob.compute_tei(True)
    Eref = numpy_hf(b.kinetic() + b.nuclear() + Vc, b.overlap(), ob.coulomb, ob.exchange, 1, 0.0)
    Erec, _ = energy_from_density(hf, b, C, 1, Vc, Enucr, "HF", 0, 0)
    # Econf belongs to the density of the last iteration, which the checkpoint holds (the returned orbitals are one
    # diagonalisation further: the barrier sees only the tail, where that step still moves tr(P Vconf) by 6e-7 of its value)
    assert np.array_equal(read_mat(hf, chk, "Vconf"), Vc) and np.array_equal(read_mat(hf, chk, "Vuc"), b.nuclear())
    Econf = np.sum(read_mat(hf, chk, "P") * Vc)
    print("He/HF barrier: Etot %.12f NumPy SCF %.12f recomputed %.12f Econf %.6e (%.6e)" % (r["Etot"], Eref, Erec, r["Econf"], Econf))
    assert abs(r["Etot"] - Eref) < 1e-8 and abs(r["Etot"] - Erec) < 1e-8
    assert r["Econf"] > 0.0 and abs(r["Econf"] - Econf) <= 1e-10 * abs(Econf)


def test_h2_hf_single_centre(hf):
    import oracle_lib as orc
    x = dict(Zl=1, Zr=1, Rmid=0.7, nelem0=2)
    # lmax 4: the NumPy SCF, with J and K from the CPU oracle.  The oracle builds them shell pair by shell pair in dense
    # host arithmetic, about 8 s for the twenty-odd iterations at these 5 shells and growing with the fourth power of the
    # shell count, so the fixed point itself is checked here and lmax 12 below through the functional and the diatomic run
    r4, C, b, Vc, Enucr = run(hf, 0, 4, 0, 4, "HF", {}, x)
    g, l, m, _, _, _ = setup(hf, 0, 4, 0, 4, {}, x)
    ob = orc.OracleAtomicBasis(0, NN, 5 * NN, g, l, m)
    ob.compute_tei(True)
    Eref = numpy_hf(b.kinetic() + b.nuclear(), b.overlap(), ob.coulomb, ob.exchange, 1, Enucr)
    print("H2/HF lmax 4: Etot %.12f NumPy SCF %.12f" % (r4["Etot"], Eref))
    assert abs(r4["Enucr"] - 1.0 / 1.4) < 1e-14 and abs(r4["Etot"] - Eref) < 1e-8
    # lmax 12: the functional recomputed from the converged density
    r12, C, b, Vc, Enucr = run(hf, 0, 12, 0, 4, "HF", {}, x)
    Erec, _ = energy_from_density(hf, b, C, 1, Vc, Enucr, "HF", 12, 0)
    print("H2/HF lmax 12: Etot %.12f recomputed %.12f" % (r12["Etot"], Erec))
    assert abs(r12["Etot"] - Erec) < 1e-8 and r12["Etot"] < r4["Etot"]
    # against this repository's diatomic program at the same bond length: the difference is the truncation of the
    # single-centre expansion in l, and it shrinks
    out = hf.scf_diatomic(1, 1, 1.4, [6, 4], 4, NN, "HF", convthr=1e-9)
    assert out["converged"]
    Ed = out["Etot"]
    print("H2/HF diatomic %.10f; single centre above it by %.3e (lmax 4), %.3e (lmax 12)" % (Ed, r4["Etot"] - Ed, r12["Etot"] - Ed))
    assert 0.0 < r12["Etot"] - Ed < r4["Etot"] - Ed


def test_ne_pbe_gaussian_nucleus(hf):
    """Rrms = 1e-3 bohr with one nuclear element, converged to the program's default 1e-7.  The DIIS error
    Sinvh^T (F P S - S P F) Sinvh carries rounding noise of about machine epsilon times the spectral range of F in the
    orthonormal basis, which the elements inside the nucleus set (computed on the host for this basis and the core orbitals:
    range 2.6e8, noise 4.4e-10; two elements inside Rrms = 5.7e-5: range 1.1e12, noise 1.6e-6, above any usable threshold,
    in double precision and with the reference's own error definition).  The energy is stationary, so 1e-7 in the error
    leaves the 1e-8 bar on Etot standing."""
    Rrms = 1e-3
    opts, x = dict(finitenuc=1), dict(Rrms=Rrms, nelem0=1)
    r, C, b, Vc, Enucr = run(hf, 10, 1, 1, 5, "gga_x_pbe-gga_c_pbe", opts, x, convthr=1e-7)
    Erec, _ = energy_from_density(hf, b, C, 5, Vc, Enucr, "gga_x_pbe-gga_c_pbe", 1, 1)
    rp = hf.scf_run_atomic(10, 1, 1, 5, NN, "gga_x_pbe-gga_c_pbe", convthr=1e-9, maxit=80)
    print("Ne/PBE Gaussian nucleus: Etot %.10f recomputed %.10f point nucleus %.10f (%d iterations)"
          % (r["Etot"], Erec, rp["Etot"], r["iterations"]))
    assert abs(r["Etot"] - Erec) < 1e-8
    # a finite nucleus binds less: first order (2 pi / 3) Z rho(0) Rrms^2, and rho(0) is below that of unscreened
    # hydrogen-like 1s^2 2s^2, 2 (1 + 1/8) Z^3 / pi
    assert 0.0 < r["Etot"] - rp["Etot"] < 2.0 / 3.0 * 10 ** 4 * Rrms ** 2 * 2 * (1 + 1.0 / 8)


def test_lih_pbe_unsymmetric(hf):
    x = dict(Zr=1, Rmid=3.015, nelem0=2)
    r, C, b, Vc, Enucr = run(hf, 3, 6, 0, 4, "gga_x_pbe-gga_c_pbe", dict(symmetry=2), x)  # symmetry 2 is lowered to 1
    Erec, _ = energy_from_density(hf, b, C, 2, Vc, Enucr, "gga_x_pbe-gga_c_pbe", 6, 0)
    print("LiH/PBE: Etot %.10f recomputed %.10f" % (r["Etot"], Erec))
    assert abs(r["Enucr"] - 3.0 / 3.015) < 1e-14 and abs(r["Etot"] - Erec) < 1e-8
    R = b.Nrad()
    P = C[:, :2] @ C[:, :2].T
    assert np.abs(P[0:R, R:2 * R]).max() > 1e-3  # s and p mix


def exe(*args, cwd=None):
    p = subprocess.run([os.path.join(BIN, "atomic")] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=cwd)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def table(out, name):
    return float(re.search(r"%s\s+energy:\s+(\S+)" % re.escape(name), out).group(1))


def test_executable_and_checkpoint_round_trip(hf, tmp_path):
    r, C, b, Vc, Enucr = run(hf, 2, 0, 0, 5, "HF", dict(iconf=3, finitenuc=2), dict(conf_barrier=1.0, shift_conf=6.0, Rrms=1e-3, nelem0=2))
    args = ["--Z", "He", "--lmax", "0", "--mmax", "0", "--nelem", "5", "--nnodes", str(NN), "--iconf", "3", "--conf_barrier", "1",
            "--shift_conf", "6", "--finitenuc", "2", "--Rrms", "1e-3", "--nelem0", "2", "--convthr", "1e-9"]
    if not hf.lib().hfg_chk_available():
        pytest.fail("no HDF5 library: the checkpoint round trip needs one")
    rc, out, err = exe(*(args + ["--save", "a.chk"]), cwd=str(tmp_path))
    assert rc == 0, err
    assert "Finite-nucleus grid" in out and "Barrier confinement, V = 1.000000e+00 shift = 6.000000e+00" in out
    assert abs(table(out, "Total") - r["Etot"]) < 1e-8 and abs(table(out, "Confinement potential") - r["Econf"]) <= 1e-10 * r["Econf"] + 1e-16
    rc, out2, err = exe(*(args + ["--load", "a.chk", "--save", ""]), cwd=str(tmp_path))
    assert rc == 0, err
    its = int(re.search(r"after (\d+) iterations", out2).group(1))
    print("reload: %d iterations, dE %.2e" % (its, table(out2, "Total") - table(out, "Total")))
    assert its <= 2 and abs(table(out2, "Total") - table(out, "Total")) < 1e-8


def test_executable_off_centre_in_angstrom(hf, tmp_path):
    """H2 through the executable with --Rmid in angstrom against the library run in bohr, and the lines the set-up prints"""
    x = dict(Zl=1, Zr=1, Rmid=0.7, nelem0=2)
    r, C, b, Vc, Enucr = run(hf, 0, 4, 0, 4, "HF", {}, x)
    rc, out, err = exe("--Z", "", "--Zl", "H", "--Zr", "H", "--Rmid", "%.17g" % (0.7 / 1.8897261254578281), "--angstrom", "1",
                       "--nelem0", "2", "--lmax", "4", "--mmax", "0", "--nelem", "4", "--nnodes", str(NN), "--convthr", "1e-9",
                       "--save", "", cwd=str(tmp_path))
    assert rc == 0, err
    print("H2 executable: Etot %.12f library %.12f" % (table(out, "Total"), r["Etot"]))
    assert abs(table(out, "Total") - r["Etot"]) < 1e-8 and abs(table(out, "Nuclear repulsion") - 1.0 / 1.4) < 1e-12
    assert "Off-center grid" in out and "Left- and right-hand nuclear charges are 1 and 1 at distance  0.700 from center" in out
    # the grid as an arma::vec prints: one cell per line, fixed with four decimals and ten wide once a value reaches 10
    g = hf.atomic_grid(4, Rmax=40.0, nelem0=2, Z=0, Zl=1, Zr=1, Rmid=0.7)
    want = "Grid\n" + "".join(("%10s\n" % "0") if v == 0.0 else ("%10.4f\n" % v) for v in g)
    assert want in out, out[:2000]


def test_zeroder_basis_is_refused_by_the_device_path(hf):
    g = hf.get_grid(40.0, 4, 4, 2.0)
    b = hf.AtomicTwoDBasis(2, NN, 5 * NN, g, [0], [0], zeroder=True)
    b.compute_tei(True)
    with pytest.raises(RuntimeError, match="the device tables have no slot"):
        b.upload()
    with pytest.raises(RuntimeError, match="SCF runs with zero derivative at Rmax are not supported"):
        hf.scf_run_atomic(2, 0, 0, 4, NN, "HF", zeroder=1, extras=dict())
