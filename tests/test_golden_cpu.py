"""CPU tests (no GPU): the host-side setup code and the oracle against the reference's own known answers,
and the C ABI surface.  Sources of every pinned number are cited next to the test."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    return helfem_amd


# ---- reference: src/general/gaunt_test.cpp (275 + 275 known answers) ----------------------------------
def test_gaunt_known_answers(hf):
    data = json.load(open(os.path.join(GOLD, "gaunt_known_answers.json")))
    assert len(data["entries"]) == 550
    worst = 0.0
    for e in data["entries"]:
        fn = hf.gaunt_coefficient if e["fn"] == "gaunt_coefficient" else hf.modified_gaunt_coefficient
        val = fn(*e["args"])
        # the reference's own criterion is DBL_EPSILON*(1+|ref|) for its GSL-3j based values; this
        # implementation integrates in extended precision and is allowed 4 ulp of (1+|ref|)
        tol = 4 * EPS * (1.0 + abs(e["ref"]))
        worst = max(worst, abs(val - e["ref"]) / (1.0 + abs(e["ref"])))
        assert abs(val - e["ref"]) < tol, (e, val)
    assert worst < 4 * EPS


def test_gaunt_nonzero_m_against_sympy(hf):
    # the reference's test only covers M=m=m'=0; pin m != 0 against sympy's exact Gaunt integral:
    # G^{M m m'}_{L l l'} = int conj(Y_L^M) Y_l^m Y_l'^m' = (-1)^M gaunt(L,l,l',-M,m,m')
    from sympy.physics.wigner import gaunt
    for (L, M, l, m, lp, mp) in [(2, 1, 1, 0, 1, 1), (3, -2, 2, -1, 1, -1), (4, 0, 2, 1, 2, -1), (5, 2, 3, 1, 2, 1),
                                 (6, -3, 4, -2, 2, -1), (1, 1, 1, 1, 0, 0), (7, 2, 4, 0, 3, 2)]:
        ref = float((-1) ** M * gaunt(L, l, lp, -M, m, mp, prec=40))
        assert abs(hf.gaunt_coefficient(L, M, l, m, lp, mp) - ref) < 1e-15, (L, M, l, m, lp, mp)


# ---- reference: the Fortran Legendre library (compiled into oracle/_ref, values committed as fixture) ---
def test_legendre_PQ_vs_reference_fortran(hf):
    data = json.load(open(os.path.join(GOLD, "legendre_reference.json")))
    Lmax, Mmax = data["Lmax"], data["Mmax"]
    for c in data["cases"]:
        P, Q = hf.legendre_PQ(Lmax, Mmax, c["xi"])
        Pr, Qr = np.array(c["P"]), np.array(c["Q"])
        # P_L^M: both sides are upward recurrences, agreement to rounding.  Q_L^M: the reference library's
        # continued fraction loses accuracy towards xi -> 1 (measured against 40-digit mpmath: 1.5e-6 at mu=1e-3,
        # 3e-9 at mu=0.05, <1e-12 from mu=0.3 on, even with --lpad 10); the implementation here is accurate to
        # 1e-16 (test_legendre_PQ_vs_mpmath), so the comparison tolerance follows the REFERENCE's error.
        qtol = 5e-6 if c["mu"] < 0.01 else (1e-8 if c["mu"] < 0.1 else 5e-12)
        # P_L^M (M>0) of the reference carries the cancellation of xi*xi-1 near xi=1 (2e-11 at mu=1e-3)
        ptol = 1e-10 if c["mu"] < 0.01 else (1e-12 if c["mu"] < 0.1 else 1e-13)
        for L in range(Lmax + 1):
            for M in range(min(L, Mmax) + 1):
                assert abs(P[L, M] - Pr[L, M]) <= ptol * abs(Pr[L, M]), ("P", c["mu"], L, M)
                assert abs(Q[L, M] - Qr[L, M]) <= qtol * abs(Qr[L, M]), ("Q", c["mu"], L, M, Q[L, M], Qr[L, M])


LEGENDRE_SCF_CASE = dict(Z1=1, Z2=1, Rbond=1.4, lmmax=[3], nelem=2, nnodes=6, method="HF", convthr=1e-9)


def test_reference_legendre_library_does_not_move_energies():
    """Runs the oracle SCF twice: with the product's P/Q implementation and with the values of the reference's own
    Fortran library plugged into compute_tei exactly as LegendreTable::compute does (legendretable.cpp:60-97).  The
    library's values at every xi this SCF asks for are the fixture legendre_reference_scf.npz
    (tests/golden/make_legendre_scf_golden.py).  The converged energies must agree far below the 1e-8 Eh parity bar,
    i.e. the reference library's limited Q accuracy is immaterial."""
    import oracle_lib as orc
    gold = np.load(os.path.join(GOLD, "legendre_reference_scf.npz"))
    gxi, gP, gQ = gold["xi"], gold["P"], gold["Q"]
    dp = ctypes.POINTER(ctypes.c_double)
    CB = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, dp, dp)
    tiny = np.finfo(float).tiny
    misses = []

    def provider(Lmax, Mmax, lpad, xi, P, Q):
        if xi == 1.0:
            for i in range((Lmax + 1) * (Mmax + 1)):
                P[i] = 0.0
                Q[i] = 0.0
            return
        assert (Lmax, Mmax, lpad) == (int(gold["Lmax"]), int(gold["Mmax"]), int(gold["lpad"]))
        k = int(np.clip(np.searchsorted(gxi, xi), 1, len(gxi) - 1))
        k = k if abs(gxi[k] - xi) < abs(gxi[k - 1] - xi) else k - 1
        if abs(gxi[k] - xi) > 1e-14 * xi:
            misses.append(xi)
        a, b = gP[k], gQ[k]
        for M in range(Mmax + 1):
            for L in range(Lmax + 1):
                pv, qv = a[M, L], b[M, L]
                P[M * (Lmax + 1) + L] = pv if (np.isfinite(pv) and abs(pv) >= tiny) else 0.0
                Q[M * (Lmax + 1) + L] = qv if (np.isfinite(qv) and abs(qv) >= tiny) else 0.0

    cb = CB(provider)
    L = orc.lib()
    L.orc_set_legendre_provider.argtypes = [CB]
    L.orc_set_legendre_provider.restype = None
    own = orc.scf_diatomic(**LEGENDRE_SCF_CASE)
    try:
        L.orc_set_legendre_provider(cb)
        viaref = orc.scf_diatomic(**LEGENDRE_SCF_CASE)
    finally:
        L.orc_set_legendre_provider(ctypes.cast(None, CB))
    assert not misses, "xi not in the fixture: %s" % misses[:5]
    assert own["converged"] and viaref["converged"]
    assert abs(own["Etot"] - viaref["Etot"]) < 1e-10, (own["Etot"], viaref["Etot"])


def test_legendre_PQ_vs_mpmath(hf):
    import mpmath as mp
    mp.mp.dps = 40
    for mu in [1e-7, 1e-4, 0.02, 0.3, 1.3, 3.9]:
        xi = float(np.cosh(mu))
        P, Q = hf.legendre_PQ(14, 3, xi)
        for L in [0, 1, 2, 5, 9, 14]:
            for M in range(min(L, 3) + 1):
                pr = mp.legenp(L, M, mp.mpf(xi), type=3)
                qr = mp.legenq(L, M, mp.mpf(xi), type=3)
                assert abs(P[L, M] - float(pr.real)) <= 2e-14 * abs(float(pr.real)), ("P", mu, L, M)
                assert abs(Q[L, M] - float(qr.real)) <= 5e-13 * abs(float(qr.real)), ("Q", mu, L, M)
    # xi == 1 entries stay zero (legendretable.cpp:73)
    P, Q = hf.legendre_PQ(4, 1, 1.0)
    assert not P.any() and not Q.any()


# ---- reference: src/legendre/legendre_test.cpp:59-101 (Neumann expansion of 1/r12) ----------------------
def test_neumann_expansion_identity(hf):
    Rh = 0.2
    eta1, eta2 = 0.3 * np.pi, 0.7 * np.pi
    phi1, phi2 = 0.125 * np.pi, (2.0 - 0.125) * np.pi
    mu1, mu2 = 0.1, 2.4

    def coord(mu, eta, phi):
        return np.array([Rh * np.sinh(mu) * np.sin(eta) * np.cos(phi), Rh * np.sinh(mu) * np.sin(eta) * np.sin(phi),
                         Rh * np.cosh(mu) * np.cos(eta)])

    exact = 1.0 / np.linalg.norm(coord(mu1, eta1, phi1) - coord(mu2, eta2, phi2))
    Lmax = 50
    P, _ = hf.legendre_PQ(Lmax, Lmax, np.cosh(min(mu1, mu2)))
    _, Q = hf.legendre_PQ(Lmax, Lmax, np.cosh(max(mu1, mu2)))
    from math import factorial
    s = 0.0 + 0.0j
    for L in range(Lmax + 1):
        for M in range(-L, L + 1):
            aM = abs(M)
            y1 = hf.theta_lm(L, M, np.cos(eta1)) * np.exp(1j * M * phi1)
            y2 = hf.theta_lm(L, M, np.cos(eta2)) * np.exp(1j * M * phi2)
            ratio = factorial(L + aM) / factorial(L - aM)
            s += (-1.0) ** M * P[L, aM] * Q[L, aM] * y1 * np.conj(y2) / ratio * (4.0 * np.pi / Rh)
    assert abs(s.real - exact) < 1e-10 * exact and abs(s.imag) < 1e-10


# ---- reference: src/general/sphtest.cpp (orthonormality of Y_lm under the product rule) ------------------
def test_spherical_harmonics_orthonormal(hf):
    # (cos theta Chebyshev) x (uniform phi) rule of angular.cpp:22-45,64-71, as the XC grid uses it
    lmax = 5
    x, w = hf.chebyshev(4 * lmax + 12)
    nphi = 2 * lmax + 5
    phis = 2 * np.pi * np.arange(nphi) / nphi
    lm = [(l, m) for l in range(lmax + 1) for m in range(-l, l + 1)]
    Y = np.array([[hf.theta_lm(l, m, xi) * np.exp(1j * m * ph) for xi in x for ph in phis] for (l, m) in lm])
    W = np.repeat(w, nphi) * (2 * np.pi / nphi)
    Smat = (Y * W) @ Y.conj().T
    assert np.max(np.abs(Smat - np.eye(len(lm)))) < 1e-10


# ---- reference: libhelfem/src/chebyshev.cpp:22-53 and lobatto.cpp tables ---------------------------------
def test_quadrature_rules(hf):
    for n in (5, 20, 75):
        x, w = hf.chebyshev(n)
        assert np.all(np.diff(x) > 0) and abs(w.sum() - 2.0) < 1e-12
        # the modified Gauss-Chebyshev rule is not Gaussian: it converges geometrically with n instead
        assert abs((w * x ** 2).sum() - 2.0 / 3.0) < {5: 1e-3, 20: 1e-9, 75: 1e-14}[n]
    # Gauss-Lobatto nodes: a few tabulated 30-digit values of lobatto.cpp (orders 4 and 5)
    x4 = hf.lobatto_nodes(4)
    assert np.allclose(x4, [-1, -0.447213595499957939281834733746, 0.447213595499957939281834733746, 1], atol=1e-16)
    x5 = hf.lobatto_nodes(5)
    assert np.allclose(x5, [-1, -0.654653670707977143798292456247, 0, 0.654653670707977143798292456247, 1], atol=1e-16)
    for n in (15, 25):
        xn = hf.lobatto_nodes(n)
        assert np.allclose(xn, -xn[::-1], atol=0) and xn[0] == -1.0 and xn[-1] == 1.0
        # interior nodes are the roots of P'_{n-1}
        from numpy.polynomial import legendre as Lg
        c = np.zeros(n)
        c[-1] = 1.0
        assert np.max(np.abs(Lg.legval(xn[1:-1], Lg.legder(c)))) < 1e-9


# ---- run-time identities of the reference driver used as known answers ----------------------------------
def test_grid_overlap_and_kinetic_identity(hf):
    """diatomic/main.cpp:439-467: overlap through the XC grid within 1e-10 (normalised), kinetic relative 1e-8"""
    import common
    gb, ob = common.make_bases(1, 1, 1.4, (3, 2), 2, 6)
    S, T = gb.overlap(), gb.kinetic()
    # the cos(theta) rule converges geometrically (1.7e-9 at 24 points, 1e-11 at 40, 2e-13 at 60 for this basis);
    # the reference's default 4*lmax+12 is sized for lmax ~ 20, so the identity is checked at 40 points here
    ldft, mdft = 40, 4 * 2 + 5
    Sg, Tg = ob.grid_overlap(ldft, mdft), ob.grid_kinetic(ldft, mdft)
    nrm = 1.0 / np.sqrt(np.diag(S))
    assert np.linalg.norm((Sg - S) * np.outer(nrm, nrm)) < 1e-10
    assert np.linalg.norm(np.abs(Tg - T) / (1 + np.abs(T))) < 1e-8


def test_oracle_eig_and_sinvh_identities(hf):
    import common
    import oracle_lib as orc
    gb, ob = common.make_bases(3, 9, 2.955, (3, 3, 2), 3, 4)
    S = gb.overlap()
    for symm in (0, 1):
        blocks = gb.get_sym_idx(symm)
        X = orc.form_Sinvh(S, False, blocks)
        # main.cpp:475-479: orbital orthonormality deviation
        assert np.linalg.norm(X.T @ S @ X - np.eye(S.shape[0])) < 1e-9
    rng = np.random.RandomState(3)
    A = rng.uniform(-1, 1, (120, 120))
    A = A + A.T
    E, C = orc.eig_sym(A)
    assert np.max(np.abs(E - np.linalg.eigvalsh(A))) < 1e-12
    assert np.max(np.abs(A @ C - C * E)) < 1e-11


def test_oracle_xc_functionals_consistency():
    """vrho/vsigma of the oracle's analytic formulas against numerical differentiation of its own rho*exc"""
    import oracle_lib as orc
    rho = np.array([1e-6, 1e-3, 0.05, 0.3, 2.0, 40.0])
    sig = np.array([1e-14, 1e-7, 1e-3, 0.2, 5.0, 3000.0])
    for fid in (1, 7, 8, 12, 101, 130, 106, 131, 402):
        e, vr, vs = orc.xc_unpolarized(fid, rho, sig)
        h = 1e-5
        ep, _, _ = orc.xc_unpolarized(fid, rho * (1 + h), sig)
        em, _, _ = orc.xc_unpolarized(fid, rho * (1 - h), sig)
        num = (rho * (1 + h) * ep - rho * (1 - h) * em) / (2 * h * rho)
        assert np.all(np.abs(num - vr) < 1e-7 * (1 + np.abs(vr))), fid
        if fid in (101, 130, 106, 131, 402):
            ep, _, _ = orc.xc_unpolarized(fid, rho, sig * (1 + h))
            em, _, _ = orc.xc_unpolarized(fid, rho, sig * (1 - h))
            num = rho * (ep - em) / (2 * h * sig)
            noise = 8 * np.finfo(float).eps * np.abs(rho * e) / (2 * h * sig)  # rounding of the difference quotient itself
            assert np.all(np.abs(num - vs) < 1e-6 * (np.abs(vs) + 1e-12) + noise), fid
    # below the density threshold everything is zero (xc_func_set_dens_threshold, dftgrid.cpp:393)
    e, vr, vs = orc.xc_unpolarized(101, np.array([1e-13]), np.array([1.0]), 1e-12)
    assert e[0] == 0 and vr[0] == 0 and vs[0] == 0


# ---- literature anchors for the end-to-end oracle (external values) ----------------------
def test_oracle_h2_hf_energy_literature():
    import oracle_lib as orc
    r = orc.scf_diatomic(1, 1, 1.4, [6], 3, 10, "HF", convthr=1e-8)
    assert r["converged"]
    assert abs(r["Etot"] - (-1.13362957)) < 2e-7  # H2 HF limit at R=1.4 a0


@pytest.mark.slow
def test_oracle_he_lda_energy_nist():
    import oracle_lib as orc
    r = orc.scf_diatomic(2, 0, 2.0, [8], 4, 10, "lda_x-lda_c_vwn", convthr=1e-8)
    assert r["converged"]
    assert abs(r["Etot"] - (-2.834836)) < 2e-6  # NIST LDA (VWN) total energy of He


# ---- the C ABI ---------------------------------------------------------------------------------------------
def test_abi_exports_every_declared_symbol(hf):
    hdr = open(os.path.join(ROOT, "include", "helfem_gpu.h")).read()
    names = sorted(set(re.findall(r"\b(hfg_[a-z_0-9A-Z]+)\s*\(", hdr)))
    assert len(names) > 40
    L = hf.lib()
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    assert b"gfx950" in L.hfg_version()


def test_host_side_basis_api_without_gpu(hf):
    lval, mval = hf.lm_to_l_m([2, 1])
    assert lval == [0, 1, 2, 1, 1] and mval == [0, 0, 0, 1, -1]
    import common
    gb, _ = common.make_bases(7, 7, 2.068, (3, 2), 2, 5, oracle=False)
    assert gb.Nrad() == 2 * 4 and gb.Nang() == 4 + 2 * 2
    assert gb.Nbf() == gb.Ndummy() - 4  # non-sigma shells drop their first radial function (basis.cpp:482)
    S = gb.overlap()
    assert np.allclose(S, S.T, atol=1e-14) and np.all(np.linalg.eigvalsh(S) > 0)
    blocks = gb.get_sym_idx(1)
    assert sorted(len(b) for b in blocks) == sorted([4 * 8, 2 * 7, 2 * 7])
    assert sorted(np.concatenate(blocks).tolist()) == list(range(gb.Nbf()))


def test_compute_paths_fail_loudly_without_gpu(hf):
    if hf.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError):
        hf.Context(0)
    with pytest.raises(RuntimeError):
        hf.scf.eig_sym(np.eye(3))


# ---------------------------------------------------------------------------------------------------
# atomic program: the reference's own known answers and literature energies
# ---------------------------------------------------------------------------------------------------
import oracle_lib as orc  # noqa: E402


def test_atomic_twoe_integral_maple_rationals():
    """src/atomic/inttest.cpp:57-96: the 16 in-element integrals of the linear LIP pair on [0,R] for L=0, as Maple
    rationals in units of R (the reference multiplies by 4 pi, the tables here carry that factor separately)."""
    import ctypes
    L = orc.lib()
    L.orc_atomic_twoe_integral.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           orc.c_double_p]
    m = np.array([[47 / 180, 11 / 360, 11 / 360, 1 / 90], [1 / 10, 1 / 40, 1 / 40, 1 / 60],
                  [1 / 10, 1 / 40, 1 / 40, 1 / 60], [3 / 20, 7 / 120, 7 / 120, 1 / 15]])
    for R in (0.5, 2.3, 40.0):
        ref = (m + m.T) * R
        for nq, tol in ((10, 1e-6), (50, 1e-13), (200, 1e-13)):
            out = np.zeros(16)
            assert L.orc_atomic_twoe_integral(0.0, R, 2, nq, 0, orc._p(out)) == 0
            err = np.abs(out.reshape(4, 4, order="F") - ref).max() / R
            assert err < tol, (R, nq, err)


def test_atomic_twoe_integral_higher_L_against_mpmath():
    """same routine for L = 1, 2 on an element away from the origin, against adaptive quadrature"""
    import ctypes
    import mpmath as mp
    L = orc.lib()
    L.orc_atomic_twoe_integral.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           orc.c_double_p]
    a, b = 0.7, 1.9
    nodes = [-1.0, 0.0, 1.0]

    def lip(i, r):
        x = (2 * r - (a + b)) / (b - a)
        v = mp.mpf(1)
        for k, xk in enumerate(nodes):
            if k != i:
                v *= (x - xk) / (nodes[i] - xk)
        return v

    for Lq in (1, 2):
        out = np.zeros(81)
        assert L.orc_atomic_twoe_integral(a, b, 3, 60, Lq, orc._p(out)) == 0
        t = out.reshape(9, 9, order="F")
        for (i, j, k, l) in [(0, 0, 0, 0), (0, 1, 2, 2), (1, 2, 0, 1), (2, 2, 1, 1)]:
            def inner(r1):
                lo = mp.quad(lambda r2: lip(k, r2) * lip(l, r2) * r2 ** Lq, [a, r1]) / r1 ** (Lq + 1)
                hi = mp.quad(lambda r2: lip(k, r2) * lip(l, r2) / r2 ** (Lq + 1), [r1, b]) * r1 ** Lq
                return lip(i, r1) * lip(j, r1) * (lo + hi)
            ref = float(mp.quad(inner, [a, b]))
            assert abs(t[j * 3 + i, l * 3 + k] - ref) < 1e-12, (Lq, i, j, k, l, t[j * 3 + i, l * 3 + k], ref)


def test_atomic_hydrogenic_one_electron_spectrum():
    """T + V of the atomic basis reproduces the hydrogen-like levels -Z^2/(2 n^2) (1s, 2s, 2p, 3d)"""
    import common
    import scipy.linalg
    Z = 3
    _, ob = common.make_atomic_bases(Z, 2, 0, 5, 15, product=False)
    S, T, V = ob.onebody("overlap"), ob.onebody("kinetic"), ob.onebody("nuclear")
    nr = ob.Nrad
    for l, levels in ((0, [1, 2, 3]), (1, [2, 3]), (2, [3])):
        sl = slice(l * nr, (l + 1) * nr)
        E = scipy.linalg.eigh(T[sl, sl] + V[sl, sl], S[sl, sl], eigvals_only=True)
        for k, n in enumerate(levels):
            assert abs(E[k] + Z * Z / (2.0 * n * n)) < 1e-9, (l, n, E[k])


ATOMIC_LITERATURE = [
    # closed-shell total energies: HF limits (numerical HF) and the NIST atomic reference data LDA (VWN) values
    ("He_HF", dict(Z=2, lmax=0, mmax=0, nelem=5, nnodes=15, method="HF"), -2.8616799956, 1e-8),
    ("Be_HF", dict(Z=4, lmax=0, mmax=0, nelem=5, nnodes=15, method="HF"), -14.573023168, 1e-7),
    ("Ne_HF", dict(Z=10, lmax=1, mmax=1, nelem=5, nnodes=15, method="HF"), -128.54709811, 1e-7),
    ("He_LDA", dict(Z=2, lmax=0, mmax=0, nelem=5, nnodes=15, method="lda_x-lda_c_vwn"), -2.834836, 1e-6),
    ("Ne_LDA", dict(Z=10, lmax=1, mmax=1, nelem=5, nnodes=15, method="lda_x-lda_c_vwn"), -128.233481, 1e-6),
    ("He_PBE0", dict(Z=2, lmax=0, mmax=0, nelem=5, nnodes=15, method="hyb_gga_xc_pbeh"), -2.895178, 2e-6),
    ("He_TPSS", dict(Z=2, lmax=0, mmax=0, nelem=5, nnodes=15, method="mgga_x_tpss-mgga_c_tpss"), -2.9097, 1e-4),
    ("Be_TPSS", dict(Z=4, lmax=0, mmax=0, nelem=5, nnodes=15, method="mgga_x_tpss-mgga_c_tpss"), -14.6717, 2e-4),
    # B-LYP and B3LYP (libxc's definition: VWN RPA fit): basis-set-limit totals quoted to four decimals in the literature
    # [external]: He -2.9071 / -2.9152, Ne -128.9730 / -128.9810; the checker gives -2.907067, -2.915219, -128.973015, -128.980973
    ("He_BLYP", dict(Z=2, lmax=0, mmax=0, nelem=5, nnodes=12, method="gga_x_b88-gga_c_lyp"), -2.9071, 1e-4),
    ("He_B3LYP", dict(Z=2, lmax=0, mmax=0, nelem=5, nnodes=12, method="hyb_gga_xc_b3lyp"), -2.9152, 1e-4),
    ("Ne_BLYP", dict(Z=10, lmax=1, mmax=1, nelem=5, nnodes=12, method="gga_x_b88-gga_c_lyp"), -128.9730, 2e-4),
]


def test_becke88_exchange_energy_of_the_hydrogen_atom():
    """Becke, Phys. Rev. A 38, 3098 (1988), Table I: exchange energy of the exact hydrogen density, LDA -0.2680, B88 -0.3098
    (exact -0.3125); one-dimensional radial quadrature of the checker's spin-polarised functional (one spin channel)"""
    r = np.linspace(1e-6, 40.0, 200001)
    rho = np.exp(-2.0 * r) / np.pi
    g = 2.0 * rho  # |grad rho|
    pr = np.stack([rho, 0 * rho], 1)
    ps = np.stack([g * g, 0 * g, 0 * g], 1)
    out = {}
    for fid in (1, 106):
        e, _, _ = orc.xc_polarized(fid, pr, ps, 1e-300)
        f = 4 * np.pi * r * r * rho * e
        out[fid] = float(np.sum(0.5 * (f[1:] + f[:-1]) * np.diff(r)))
    assert abs(out[1] - (-0.2680)) < 1e-4 and abs(out[106] - (-0.3098)) < 1e-4, out


@pytest.mark.parametrize("name,kw,lit,tol", ATOMIC_LITERATURE, ids=[c[0] for c in ATOMIC_LITERATURE])
def test_atomic_oracle_literature_energies(name, kw, lit, tol):
    r = orc.scf_atomic(convthr=1e-9, maxit=60, **kw)
    assert r["converged"]
    assert abs(r["Etot"] - lit) < tol, (name, r["Etot"], lit)
    if kw["method"] == "HF":
        # virial theorem at the HF limit
        assert abs(-(r["Etot"] - r["Ekin"]) / r["Ekin"] - 2.0) < 1e-5
    if name == "He_LDA":
        # NIST atomic reference data, He LDA: Ekin = 2.767922, Ecoul = 1.996120, Eenuc = -6.625564, Exc = -0.973314
        for k, v in (("Ekin", 2.767922), ("Ecoul", 1.996120), ("Epot", -6.625564), ("Exc", -0.973314)):
            assert abs(r[k] - v) < 2e-6, (k, r[k], v)


def test_atomic_grid_electron_count_and_exchange_energy():
    """He 1s^2 with the exact hydrogenic orbital shape: Tr PS = 2 and E_x^{HF} = -E_J/2 for a two-electron singlet"""
    import common
    _, ob = common.make_atomic_bases(2, 0, 0, 5, 15, product=False)
    ob.compute_tei(True)
    import scipy.linalg
    S, T, V = ob.onebody("overlap"), ob.onebody("kinetic"), ob.onebody("nuclear")
    E, C = scipy.linalg.eigh(T + V, S)
    Pa = np.outer(C[:, 0], C[:, 0])
    J = ob.coulomb(2 * Pa)
    K = ob.exchange(Pa)
    EJ = 0.5 * np.sum(2 * Pa * J)
    EK = np.sum(Pa * K)
    assert abs(EJ - 2 * 5.0 / 8.0 * 2) < 1e-8          # J_1s1s = 5Z/8, E_J = 2 J  (Z=2)
    assert abs(EK + 0.5 * EJ) < 1e-10
    H, Exc, Nel, _ = ob.eval_Fxc(10, 5, 1, 0, 2 * Pa)
    assert abs(Nel - 2.0) < 1e-9


# ---------------------------------------------------------------------------------------------------
# spin-polarised functionals and unrestricted runs
# ---------------------------------------------------------------------------------------------------
def test_b88_lyp_b3lyp_known_limits():
    """gga_x_b88 reduces to lda_x at vanishing gradient and lowers the energy with it; gga_c_lyp (Miehlich form through
    the checker's differentiation type) equals the closed-shell reduction of the same formula written out independently
    here, has the Colle-Salvetti uniform-gas value at sigma = 0 and vanishes for a fully polarised density (no
    self-correlation); hyb_gga_xc_b3lyp is 0.08 lda_x + 0.72 gga_x_b88 + 0.19 lda_c_vwn_rpa + 0.81 gga_c_lyp"""
    import oracle_lib as orc
    rho = np.array([1e-4, 0.02, 0.3, 1.7, 25.0])
    sig = np.array([1e-9, 1e-4, 0.05, 2.0, 900.0])
    e0, v0, _ = orc.xc_unpolarized(1, rho, 0 * sig)
    eb, vb, vsb = orc.xc_unpolarized(106, rho, 1e-300 + 0 * sig)
    assert np.max(np.abs(eb - e0)) < 1e-14 and np.max(np.abs(vb - v0)) < 1e-13
    eb2, _, vs2 = orc.xc_unpolarized(106, rho, sig)
    assert np.all(eb2 < e0) and np.all(vs2 < 0)
    # small-gradient expansion: e = e_LDA - beta (rho/2)^{4/3} x^2 * 2/rho, x^2 = (sigma/4)/(rho/2)^{8/3}
    s_small = 1e-5 * rho ** (8.0 / 3.0)
    es, _, _ = orc.xc_unpolarized(106, rho, s_small)
    x2 = (0.25 * s_small) / (0.5 * rho) ** (8.0 / 3.0)
    assert np.max(np.abs((es - e0) - (-0.0042 * (0.5 * rho) ** (4.0 / 3.0) * x2 * 2.0 / rho)) / np.abs(es - e0)) < 1e-5
    # LYP, closed shell, written out: E/rho = -a/(1 + d r) - a b exp(-c r)/(1 + d r) [C_F - rho^{-8/3} sigma (1/24 + 7 delta/72)], r = rho^{-1/3}
    a, b, c, d = 0.04918, 0.132, 0.2533, 0.349
    CF = 0.3 * (3 * np.pi ** 2) ** (2.0 / 3.0)
    r = rho ** (-1.0 / 3.0)
    delta = c * r + d * r / (1 + d * r)
    closed = -a / (1 + d * r) - a * b * np.exp(-c * r) / (1 + d * r) * (CF - rho ** (-8.0 / 3.0) * sig * (1.0 / 24 + 7.0 * delta / 72))
    el, vl, vsl = orc.xc_unpolarized(131, rho, sig)
    assert np.max(np.abs(el - closed) / np.abs(closed)) < 1e-13
    # fully polarised: zero (threshold 0 so that the empty channel stays empty)
    pr = np.stack([rho, 0 * rho], axis=1)
    ps = np.stack([sig, 0 * sig, 0 * sig], axis=1)
    ep, vp, vsp = orc.xc_polarized(131, pr, ps, 0.0)
    assert np.max(np.abs(ep)) < 1e-16
    # composition of B3LYP
    ex, vx, _ = orc.xc_unpolarized(1, rho, sig)
    ev, vv, _ = orc.xc_unpolarized(8, rho, sig)
    e3, v3, vs3 = orc.xc_unpolarized(402, rho, sig)
    assert np.max(np.abs(e3 - (0.08 * ex + 0.72 * eb2 + 0.19 * ev + 0.81 * el))) < 1e-15
    assert np.max(np.abs(vs3 - (0.72 * vs2 + 0.81 * vsl))) < 1e-15 * np.max(np.abs(vs3)) + 1e-18
    # VWN: the RPA fit lies below the Ceperley-Alder fit (RPA overcorrelates) at every density
    e5, _, _ = orc.xc_unpolarized(7, rho, sig)
    assert np.all(ev < e5)


@pytest.mark.parametrize("fid", [1, 7, 8, 12, 101, 130, 106, 131, 402])
def test_polarized_functionals_reduce_to_unpolarized_and_match_finite_differences(fid):
    rng = np.random.RandomState(fid)
    n = 40
    rt = 10 ** rng.uniform(-4, 2, n)
    g = rng.uniform(0, 3, n) * rt ** (4.0 / 3.0)
    eu, vu, vsu = orc.xc_unpolarized(fid, rt, g * g)
    e, v, vs = orc.xc_polarized(fid, np.stack([rt / 2, rt / 2], 1), np.stack([g * g / 4] * 3, 1))
    assert np.max(np.abs(e - eu) / np.abs(eu)) < 1e-13
    assert np.max(np.abs(v[:, 0] - vu) / np.abs(vu)) < 1e-12 and np.max(np.abs(v[:, 1] - vu) / np.abs(vu)) < 1e-12
    if fid > 100:  # d/d sigma_total = (vs_aa + vs_ab + vs_bb)/4 at equal spin densities
        assert np.max(np.abs((vs.sum(axis=1)) / 4 - vsu) / (np.abs(vsu) + 1e-300)) < 1e-10
    # general polarisation: central differences of the energy density
    z = rng.uniform(-0.95, 0.95, n)
    ra, rb = rt * (1 + z) / 2, rt * (1 - z) / 2
    ga = rng.normal(size=(n, 3)) * ra[:, None] ** (4.0 / 3.0)
    gb = rng.normal(size=(n, 3)) * rb[:, None] ** (4.0 / 3.0)
    sig = np.stack([(ga * ga).sum(1), (ga * gb).sum(1), (gb * gb).sum(1)], 1)

    def energy(ra, rb, sig):
        ee, _, _ = orc.xc_polarized(fid, np.stack([ra, rb], 1), sig)
        return ee * (ra + rb)

    _, v, vs = orc.xc_polarized(fid, np.stack([ra, rb], 1), sig)
    h = 1e-6
    fa = (energy(ra * (1 + h), rb, sig) - energy(ra * (1 - h), rb, sig)) / (2 * h * ra)
    fb = (energy(ra, rb * (1 + h), sig) - energy(ra, rb * (1 - h), sig)) / (2 * h * rb)
    assert np.max(np.abs(fa - v[:, 0]) / np.abs(v[:, 0])) < 1e-6
    assert np.max(np.abs(fb - v[:, 1]) / np.abs(v[:, 1])) < 1e-6
    if fid > 100:
        for k in range(3):
            sp, sm = sig.copy(), sig.copy()
            d = h * np.maximum(np.abs(sig[:, k]), 1e-30)
            sp[:, k] += d
            sm[:, k] -= d
            fd = (energy(ra, rb, sp) - energy(ra, rb, sm)) / (2 * d)
            assert np.max(np.abs(fd - vs[:, k]) / (np.abs(vs[:, k]) + 1e-8 * np.abs(vs).max())) < 1e-4, (fid, k)


@pytest.mark.parametrize("fid", [1, 101, 546, 641, 178, 406, 202])
def test_exchange_channel_screening_at_the_density_threshold(fid):
    """libxc (>= 5) leaves a spin channel whose density is below dens_threshold out of the exchange sum, in the
    unpolarised evaluation (rho/2) as in the polarised one, so that both agree on a closed shell through the whole
    threshold window; the correlation part of a hybrid survives."""
    thr = 1e-12
    rt = np.array([0.5e-12, 1.0e-12, 1.5e-12, 1.99e-12, 2.0e-12, 2.5e-12, 1e-9, 1e-3])
    g = 0.3 * rt ** (4.0 / 3.0)
    t = 0.4 * rt ** (5.0 / 3.0) + g * g / (8 * rt)
    if fid == 202:
        eu, vu, vsu, vtu = orc.xc_unpolarized_mgga(fid, rt, g * g, t, thr)
        e, v, vs, vt = orc.xc_polarized_mgga(fid, np.stack([rt / 2, rt / 2], 1), np.stack([g * g / 4] * 3, 1),
                                             np.stack([t / 2, t / 2], 1), thr)
        assert np.max(np.abs(vt[:, 0] - vtu)) <= 1e-12 * np.max(np.abs(vtu))
    else:
        eu, vu, vsu = orc.xc_unpolarized(fid, rt, g * g, thr)
        e, v, vs = orc.xc_polarized(fid, np.stack([rt / 2, rt / 2], 1), np.stack([g * g / 4] * 3, 1), thr)
    dead = rt < 2 * thr
    pure_x = fid in (1, 101, 546, 641, 202)
    if pure_x:
        assert np.all(eu[dead] == 0.0) and np.all(vu[dead] == 0.0) and np.all(e[dead] == 0.0) and np.all(v[dead] == 0.0)
    else:  # the hybrids: below 2 thr only the correlation part is left (libxc id 13 / 130)
        cid = 13 if fid == 178 else 130
        ec, vc, _ = orc.xc_unpolarized(cid, rt, g * g, thr)
        assert np.all(eu[dead] == ec[dead]) and np.all(vu[dead] == vc[dead])
        assert np.all(eu[0:1] == 0.0)  # rho < thr: nothing at all
    live = ~dead
    assert np.all(eu[live] < 0.0)
    assert np.max(np.abs(e[live] - eu[live]) / np.abs(eu[live])) < 1e-12
    assert np.max(np.abs(v[live, 0] - vu[live]) / np.abs(vu[live])) < 1e-11
    if pure_x:  # dead channels agree too (both zero); for correlation the polarised call clamps rho_s to thr
        assert np.all(e[dead] == eu[dead])


def test_functionals_stay_finite_in_the_far_field():
    """With the density threshold lowered to zero the far field of the grid hands densities of 1e-30 and less to the
    functionals; log(1 + 1/q) of PW92 and exp(-ec/gamma) - 1 of PBE must not round to 0 there (A = inf, NaN Fock matrix)."""
    rt = 10.0 ** np.arange(-36.0, -8.0, 2.0)
    for sc in (0.0, 1e-3, 1.0, 30.0):
        g = sc * rt ** (4.0 / 3.0)
        t = 0.3 * rt ** (5.0 / 3.0) + g * g / (8 * rt)
        for fid in (1, 7, 12, 13, 101, 130, 406, 178, 546, 641):
            out = orc.xc_unpolarized(fid, rt, g * g, 0.0)
            assert all(np.all(np.isfinite(o)) for o in out), (fid, sc)
            out = orc.xc_polarized(fid, np.stack([0.7 * rt, 0.3 * rt], 1), np.stack([0.49 * g * g, 0.21 * g * g, 0.09 * g * g], 1), 0.0)
            assert all(np.all(np.isfinite(o)) for o in out), (fid, sc, "pol")
        for fid in (202, 231):
            out = orc.xc_unpolarized_mgga(fid, rt, g * g, t, 0.0)
            assert all(np.all(np.isfinite(o)) for o in out), (fid, sc)
            out = orc.xc_polarized_mgga(fid, np.stack([0.7 * rt, 0.3 * rt], 1), np.stack([0.49 * g * g, 0.21 * g * g, 0.09 * g * g], 1),
                                        np.stack([0.7 * t, 0.3 * t], 1), 0.0)
            assert all(np.all(np.isfinite(o)) for o in out), (fid, sc, "pol")
    # PW92 keeps its leading far-field behaviour ec -> -2a a1/b4 / rs ... i.e. ec rs -> const
    e, _, _ = orc.xc_unpolarized(12, rt, 0 * rt, 0.0)
    rs = (3.0 / (4 * np.pi * rt)) ** (1.0 / 3.0)
    lim = -0.031091 * 2 * 0.21370 / (2 * 0.031091 * 0.49294)
    far = rt < 1e-24
    assert np.max(np.abs(e[far] * rs[far] / lim - 1.0)) < 1e-3


def test_polarized_correlation_textbook_values():
    """uniform-gas correlation energies per particle at rs = 2 (Perdew-Wang 1992, Table; VWN fit of the same data)"""
    rs = 2.0
    n0 = 3.0 / (4.0 * np.pi * rs ** 3)
    z = np.zeros((1, 3))
    for fid, para, ferro in ((12, -0.04476, -0.02391), (7, -0.04478, -0.02386)):
        e0, _, _ = orc.xc_polarized(fid, np.array([[n0 / 2, n0 / 2]]), z)
        e1, _, _ = orc.xc_polarized(fid, np.array([[n0, 0.0]]), z)
        assert abs(e0[0] - para) < 2e-5 and abs(e1[0] - ferro) < 2e-5, (fid, e0, e1)


OPEN_SHELL_LITERATURE = [
    # NIST atomic reference data (LSD = Slater exchange + VWN), numerical UHF limits, PBE hydrogen atom
    ("H_LSD", dict(Z=1, lmax=0, mmax=0, nelem=5, nnodes=15, method="lda_x-lda_c_vwn", M=2), -0.478671, 1e-6),
    ("Li_LSD", dict(Z=3, lmax=0, mmax=0, nelem=5, nnodes=15, method="lda_x-lda_c_vwn", M=2), -7.343957, 1e-6),
    ("H_PBE", dict(Z=1, lmax=0, mmax=0, nelem=5, nnodes=15, method="gga_x_pbe-gga_c_pbe", M=2), -0.499990, 1e-6),
    ("H_UHF", dict(Z=1, lmax=0, mmax=0, nelem=5, nnodes=15, method="HF", M=2), -0.5, 1e-9),
    ("Li_UHF", dict(Z=3, lmax=0, mmax=0, nelem=5, nnodes=15, method="HF", M=2), -7.432751, 1e-6),
    ("N_UHF", dict(Z=7, lmax=1, mmax=1, nelem=5, nnodes=15, method="HF", M=4), -54.404548, 1e-6),
    # restricted open shell (M < 0): numerical ROHF limits
    ("Li_ROHF", dict(Z=3, lmax=0, mmax=0, nelem=5, nnodes=15, method="HF", M=-2), -7.4327269, 1e-6),
    ("N_ROHF", dict(Z=7, lmax=1, mmax=1, nelem=5, nnodes=15, method="HF", M=-4), -54.400934, 1e-6),
]


@pytest.mark.parametrize("name,kw,lit,tol", OPEN_SHELL_LITERATURE, ids=[c[0] for c in OPEN_SHELL_LITERATURE])
def test_unrestricted_oracle_literature_energies(name, kw, lit, tol):
    r = orc.scf_atomic(convthr=1e-8, maxit=80, **kw)
    assert r["converged"]
    assert abs(r["Etot"] - lit) < tol, (name, r["Etot"], lit)


# ---- spin-polarised meta-GGA (TPSS): known answers -------------------------------------------------------
def test_polarized_tpss_known_answers():
    """(1) zeta = 0 reduces to the spin-unpolarised functional (itself pinned by the He/Be/Ne literature energies);
    (2) all seven derivatives against central differences; (3) TPSS correlation vanishes for any fully spin-polarised
    one-orbital density (tau = tau_W): its self-correlation freedom; (4) on the exact hydrogen density the exchange
    energy is -5/16 Eh -- the constants c, e of TPSS were fitted to that -- and the correlation energy 0."""
    import oracle_lib as orc
    import common
    import scipy.linalg as sl
    rho = np.array([1e-3, 0.05, 0.3, 2.0, 40.0])
    sig = np.array([1e-6, 0.01, 0.2, 3.0, 500.0])
    tau = np.array([2e-4, 0.03, 0.3, 4.0, 300.0])
    for fid in (202, 231):
        e, v, vs, vt = orc.xc_unpolarized_mgga(fid, rho, sig, tau)
        rp, sp, tp = np.stack([rho / 2] * 2, 1), np.stack([sig / 4] * 3, 1), np.stack([tau / 2] * 2, 1)
        e2, v2, vs2, vt2 = orc.xc_polarized_mgga(fid, rp, sp, tp)
        assert np.max(np.abs(e2 - e) / np.abs(e)) < 1e-13
        assert np.max(np.abs(0.5 * v2.sum(1) - v) / np.abs(v)) < 1e-12
        assert np.max(np.abs(0.25 * vs2.sum(1) - vs) / np.abs(vs)) < 1e-12
        assert np.max(np.abs(0.5 * vt2.sum(1) - vt) / np.abs(vt)) < 1e-12
    rng = np.random.RandomState(3)
    N = 6
    ra, rb = rng.uniform(0.05, 2, N), rng.uniform(0.02, 1.5, N)
    ga, gb = rng.uniform(-1, 1, (N, 3)), rng.uniform(-1, 1, (N, 3))
    saa, sab, sbb = (ga * ga).sum(1), (ga * gb).sum(1), (gb * gb).sum(1)
    ta, tb = saa / (8 * ra) + rng.uniform(0.01, 1, N), sbb / (8 * rb) + rng.uniform(0.01, 1, N)
    X = np.stack([ra, rb, saa, sab, sbb, ta, tb], 1)

    def energy(fid, Y):
        return orc.xc_polarized_mgga(fid, Y[:, 0:2], Y[:, 2:5], Y[:, 5:7])[0] * (Y[:, 0] + Y[:, 1])

    for fid in (202, 231):
        _, v, vs, vt = orc.xc_polarized_mgga(fid, X[:, 0:2], X[:, 2:5], X[:, 5:7])
        an = np.concatenate([v, vs, vt], 1)
        for k in range(7):
            h = 1e-6 * np.maximum(np.abs(X[:, k]), 1e-2)
            Xp, Xm = X.copy(), X.copy()
            Xp[:, k] += h
            Xm[:, k] -= h
            fd = (energy(fid, Xp) - energy(fid, Xm)) / (2 * h)
            assert np.max(np.abs(fd - an[:, k]) / np.maximum(np.abs(an[:, k]), 1e-6)) < 1e-4, (fid, k)
    n = np.array([0.01, 0.3, 5.0])
    s = np.array([0.05, 0.4, 20.0]) ** 2
    z3 = np.zeros(3)
    e, _, _, _ = orc.xc_polarized_mgga(231, np.stack([n, z3], 1), np.stack([s, z3, z3], 1), np.stack([s / (8 * n), z3], 1))
    epbe, _, _ = orc.xc_polarized(130, np.stack([n, z3], 1), np.stack([s, z3, z3], 1))
    assert np.max(np.abs(e)) < 1e-10 * np.max(np.abs(epbe))
    _, ob = common.make_atomic_bases(Z=1, lmax=0, mmax=0, nelem=5, nnodes=12, product=False)
    S, T, V = ob.onebody("overlap"), ob.onebody("kinetic"), ob.onebody("nuclear")
    _, C = sl.eigh(T + V, S)
    Pa = np.asfortranarray(C[:, :1] @ C[:, :1].T)
    Pb = np.zeros_like(Pa, order="F")
    _, _, Ex, Nel, Ekin = ob.eval_Fxc_pol(10, 5, 202, 0, Pa, Pb)
    _, _, Ec, _, _ = ob.eval_Fxc_pol(10, 5, 0, 231, Pa, Pb)
    assert abs(Nel - 1.0) < 1e-12 and abs(Ekin - 0.5) < 1e-8  # integral of tau = <T> of the 1s orbital
    assert abs(Ex + 0.3125) < 2e-7, Ex
    assert abs(Ec) < 1e-10, Ec


def test_oracle_unrestricted_tpss_atoms():
    """TPSS total energies of open-shell atoms, Staroverov, Scuseria, Tao, Perdew, PRB 69, 075102 (4 decimals):
    H -0.5002, Li -7.4891; N is this oracle's own number (regression)."""
    import oracle_lib as orc
    for Z, M, lm, lit, tol in ((1, 2, 0, -0.5002, 1e-4), (3, 2, 0, -7.4891, 1e-4), (7, 4, 1, -54.616172, 2e-6)):
        r = orc.scf_atomic(Z, lm, lm, 5, 12, "mgga_x_tpss-mgga_c_tpss", M=M, convthr=1e-9, maxit=60)
        assert r["converged"]
        assert abs(r["Etot"] - lit) < tol, (Z, r["Etot"], lit)
