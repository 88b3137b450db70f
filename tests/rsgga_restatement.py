"""Independent restatement of the short-range GGA exchange functionals and the range-separated GGA hybrids, for
test_rsgga_cpu.py and test_gpu_rsgga.py.  Written from the published construction, not from the kernels' code:

  per spin channel, spin scaling E_x[ra, rb] = (E_x[2 ra] + E_x[2 rb]) / 2, and for an unpolarised density n
      k_F = (3 pi^2 n)^{1/3},  a = omega sqrt(F_x(s)) / (2 k_F),  eps_x^sr = eps_x^LDA(n) F_x(s) att(a)
  erfc kernel   (Iikura, Tsuneda, Yanai, Hirao, JCP 115, 3540 (2001); attenuation of Toulouse, Savin, Flad, IJQC 100, 1047 (2004)):
      att = 1 - (8/3) a [sqrt(pi) erf(1/(2a)) + (2a - 4a^3) exp(-1/(4a^2)) - 3a + 4a^3]
  Yukawa kernel (Savin, Flad, IJQC 56, 327 (1995); Akinaga, Ten-no, CPL 462, 348 (2008)):
      att = 1 - (8/3) a [atan(1/a) + a/4 - (a/4)(a^2 + 3) ln(1 + 1/a^2)]
  F_x of B88 (Becke, PRA 38, 3098 (1988)): 1 + (beta/C_x) x^2 / (1 + 6 beta x asinh x), x = |grad n_s| / n_s^{4/3}, beta = 0.0042,
      C_x = (3/2)(3/(4 pi))^{1/3};  F_x of PBE: 1 + kappa - kappa/(1 + mu s^2/kappa), kappa = 0.804, mu = 0.2195149727645171.

Both attenuation functions cancel like a^4 at large a.  They are evaluated here in their closed forms with mpmath at 120 digits
(no series), and the derivatives are complex steps of 1e-60 in the same arithmetic."""
import numpy as np
from mpmath import mp, mpf, mpc

DPS = 120  # set around every evaluation (mp.workdps): other test modules set mpmath's global precision for themselves

PRIMITIVES = {
    "gga_x_ityh": dict(F="b88", kernel="erfc", omega=0.2),
    "gga_x_sfat": dict(F="b88", kernel="yukawa", omega=0.44),
    "gga_x_ityh_pbe": dict(F="pbe", kernel="erfc", omega=0.2),
    "gga_x_sfat_pbe": dict(F="pbe", kernel="yukawa", omega=0.44),
}

# 1/r = [1 - alpha - beta s(r)]/r + [alpha + beta s(r)]/r: DFT exchange (1 - alpha - beta) X + beta X^sr(omega).
# parts: (weight, functional name, external parameters or None)
HYBRIDS = {
    "hyb_gga_xc_cam_b3lyp": dict(id=433, kernel="erfc", alpha=0.19, beta=0.46, omega=0.33,
                                 parts=[(0.35, "gga_x_b88", None), (0.46, "gga_x_ityh", [0.33]), (0.19, "lda_c_vwn", None),
                                        (0.81, "gga_c_lyp", None)]),
    "hyb_gga_xc_camy_b3lyp": dict(id=470, kernel="yukawa", alpha=0.19, beta=0.46, omega=0.34,
                                  parts=[(0.35, "gga_x_b88", None), (0.46, "gga_x_sfat", [0.34]), (0.19, "lda_c_vwn", None),
                                         (0.81, "gga_c_lyp", None)]),
    "hyb_gga_xc_camy_blyp": dict(id=455, kernel="yukawa", alpha=0.20, beta=0.80, omega=0.44,
                                 parts=[(0.80, "gga_x_sfat", [0.44]), (1.0, "gga_c_lyp", None)]),
    "hyb_gga_xc_lcy_blyp": dict(id=468, kernel="yukawa", alpha=0.0, beta=1.0, omega=0.75,
                                parts=[(1.0, "gga_x_sfat", [0.75]), (1.0, "gga_c_lyp", None)]),
    "hyb_gga_xc_lcy_pbe": dict(id=467, kernel="yukawa", alpha=0.0, beta=1.0, omega=0.75,
                               parts=[(1.0, "gga_x_sfat_pbe", [0.75]), (1.0, "gga_c_pbe", None)]),
}

PI = mp.pi  # a lazy constant: evaluated at the working precision of its use


def lda_x_eps_np(n):
    return -0.75 * (3 / np.pi) ** (1 / 3) * n ** (1 / 3)


def _att(kernel, a):
    if kernel == "erfc":
        return 1 - mpf(8) / 3 * a * (mp.sqrt(PI) * mp.erf(1 / (2 * a)) + (2 * a - 4 * a ** 3) * mp.exp(-1 / (4 * a * a)) - 3 * a + 4 * a ** 3)
    return 1 - mpf(8) / 3 * a * (mp.atan(1 / a) + a / 4 - a / 4 * (a * a + 3) * mp.log(1 + 1 / (a * a)))


def _fx(which, n, sig):
    if which == "b88":
        beta, cx = mpf("0.0042"), mpf(3) / 2 * (3 / (4 * PI)) ** (mpf(1) / 3)
        x2 = (sig / 4) / (n / 2) ** (mpf(8) / 3)
        x = mp.sqrt(x2)
        return 1 + beta / cx * x2 / (1 + 6 * beta * x * mp.asinh(x))
    kappa, mu = mpf("0.804"), mpf("0.06672455060314922") * PI ** 2 / 3
    s2 = sig / (4 * (3 * PI ** 2) ** (2 * (mpf(1) / 3)) * n ** (mpf(8) / 3))
    return 1 + kappa - kappa / (1 + mu * s2 / kappa)


def energy_density(name, omega, n, sig):
    """n eps_x^sr of an unpolarised density (mpmath numbers, real or complex)"""
    p = PRIMITIVES[name]
    F = _fx(p["F"], n, sig)
    kf = (3 * PI ** 2 * n) ** (mpf(1) / 3)
    a = mpf(omega) * mp.sqrt(F) / (2 * kf)
    return n * (-mpf(3) / 4 * (3 / PI) ** (mpf(1) / 3) * n ** (mpf(1) / 3)) * F * _att(p["kernel"], a)


def _point(name, omega, n, sig):
    """(n eps, d/dn, d/dsigma) at one point"""
    with mp.workdps(DPS):
        return _point_at_working_precision(name, omega, n, sig)


def _point_at_working_precision(name, omega, n, sig):
    H = mpf(10) ** -60
    n, sig = mpf(float(n)), mpf(float(sig))
    e = energy_density(name, omega, n, sig)
    dn = energy_density(name, omega, mpc(n, n * H), sig).imag / (n * H)
    hs = (sig if sig > 0 else n ** (mpf(8) / 3)) * H
    ds = energy_density(name, omega, n, mpc(sig, hs)).imag / hs
    return float(e), float(dn), float(ds)


def ref_unpol(name, omega, n, sig):
    out = np.array([_point(name, omega, a, b) for a, b in zip(n, sig)])
    return out[:, 0], out[:, 1], out[:, 2]


def ref_pol(name, omega, pts):
    """E = (E[2 ra, 4 saa] + E[2 rb, 4 sbb]) / 2 per volume and its derivatives by (ra, rb, saa, sab, sbb)"""
    ra, rb, saa, sab, sbb = pts
    ea, da_n, da_s = ref_unpol(name, omega, 2 * ra, 4 * saa)
    eb, db_n, db_s = ref_unpol(name, omega, 2 * rb, 4 * sbb)
    return 0.5 * (ea + eb), [da_n, db_n, 2 * da_s, np.zeros_like(ra), 2 * db_s]


S_VALUES = np.array([0.0, 1e-3, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0, 20.0, 50.0, 80.0])


def _sigma_of(n, s):
    """sigma of an unpolarised density with reduced gradient s = |grad n| / (2 k_F n)"""
    return s ** 2 * 4 * (3 * np.pi ** 2 * n) ** (2 / 3) * n ** 2


def grid_unpol():
    """n from the default density threshold of the programs (1e-12) to 1e3, s from 0 to 80"""
    n = np.repeat(10 ** np.linspace(-12, 3, 16), len(S_VALUES))
    s = np.tile(S_VALUES, 16)
    return n, _sigma_of(n, s)


def grid_pol():
    """each channel over the same ranges (as the unpolarised density 2 r_s), decorrelated; sigma_ab within the Schwarz bound"""
    rng = np.random.RandomState(11)
    m = 120
    ra, rb = 0.5 * 10 ** rng.uniform(-12, 3, m), 0.5 * 10 ** rng.uniform(-12, 3, m)
    sa, sb = S_VALUES[rng.randint(0, len(S_VALUES), m)], S_VALUES[rng.randint(0, len(S_VALUES), m)]
    saa, sbb = _sigma_of(2 * ra, sa) / 4, _sigma_of(2 * rb, sb) / 4
    sab = np.sqrt(saa * sbb) * rng.uniform(-1, 1, m)
    return [ra, rb, saa, sab, sbb]


# ---------------------------------------------------------------------------------------------------------------------
# The same construction in double precision NumPy, fast enough for every point of a DFT grid (test_gpu_rsgga.py drives the
# dense grid worker of tests/lapl_dense.py with it); test_rsgga_cpu.py pins it against the 120-digit closed forms above.
# Where the closed forms cancel, the attenuation functions are summed from their expansions in 1/a^2,
#   erfc:   att = sum_{k>=1} (-1)^{k+1} 2 / (4^k k! (2k+1)(k+1)(k+2)) a^{-2k}   (a >= 0.5; entire in 1/a^2)
#   Yukawa: att = sum_{k>=1} (-1)^{k+1} 2 / ((2k+1)(k+1)(k+2)) a^{-2k}          (a >= 1.5; converges for a > 1)
# (term-by-term integration of the kernels' momentum-space forms).  All operations are analytic, so a complex step
# differentiates them; erf takes its first-order expansion in the imaginary part, which is exact for a step of 1e-30.
# ---------------------------------------------------------------------------------------------------------------------
import math  # noqa: E402

_verf = np.vectorize(math.erf, otypes=[float])


def _erf_cs(z):
    x = np.real(z)
    return _verf(x) + 1j * np.imag(z) * 2 / np.sqrt(np.pi) * np.exp(-x * x)


A_SWITCH = {"erfc": 0.5, "yukawa": 1.5}


def att_closed_np(kernel, a):
    if kernel == "erfc":
        return 1 - 8 / 3 * a * (np.sqrt(np.pi) * _erf_cs(1 / (2 * a)) + (2 * a - 4 * a ** 3) * np.exp(-1 / (4 * a * a)) - 3 * a + 4 * a ** 3)
    return 1 - 8 / 3 * a * (np.arctan(1 / a) + a / 4 - a / 4 * (a * a + 3) * np.log(1 + 1 / (a * a)))


def att_over_u_np(kernel, u):
    """att(a) / u, u = 1/a^2, from the expansion"""
    g = np.zeros_like(u)
    for k in range(40 if kernel == "erfc" else 90, 0, -1):  # small terms first
        c = 2.0 / ((2 * k + 1) * (k + 1) * (k + 2))
        if kernel == "erfc":
            c /= 4.0 ** k * math.factorial(k)
        g = g + (-1) ** (k + 1) * c * u ** (k - 1)
    return g


def _fx_np(which, n, sig):
    if which == "b88":
        beta, cx = 0.0042, 1.5 * (3 / (4 * np.pi)) ** (1 / 3)
        x2 = (sig / 4) / (n / 2) ** (8 / 3)
        x = np.sqrt(x2)
        return 1 + beta / cx * x2 / (1 + 6 * beta * x * np.arcsinh(x))
    kappa, mu = 0.804, 0.06672455060314922 * np.pi ** 2 / 3
    s2 = sig / (4 * (3 * np.pi ** 2) ** (2 / 3) * n ** (8 / 3))
    return 1 + kappa - kappa / (1 + mu * s2 / kappa)


def energy_density_np(name, omega, n, sig):
    """n eps_x^sr of an unpolarised density, NumPy arrays (real or complex)"""
    p = PRIMITIVES[name]
    n, sig = np.atleast_1d(np.asarray(n, dtype=complex)), np.atleast_1d(np.asarray(sig, dtype=complex))
    n, sig = np.broadcast_arrays(n, sig)
    F = _fx_np(p["F"], n, sig)
    kf = (3 * np.pi ** 2 * n) ** (1 / 3)
    a = omega * np.sqrt(F) / (2 * kf)
    big = a.real >= A_SWITCH[p["kernel"]]
    Fatt = np.zeros_like(a)
    Fatt[~big] = F[~big] * att_closed_np(p["kernel"], a[~big])
    # att = u g(u) with u = 1/a^2 = 4 k_F^2 / (omega^2 F): F att = (4 k_F^2 / omega^2) g(u), whose leading term does not depend on
    # F -- as a product F * att the sigma derivative would cancel to 1/a^2 of its terms
    uF = 4 * kf[big] ** 2 / omega ** 2
    Fatt[big] = uF * att_over_u_np(p["kernel"], uF / F[big])
    return n * lda_x_eps_np(n) * Fatt


def eval_unpol_np(name, omega, n, sig):
    """(n eps, d/dn, d/dsigma), complex steps of relative size 1e-30"""
    n, sig = np.asarray(n, dtype=float), np.asarray(sig, dtype=float)
    e = energy_density_np(name, omega, n, sig).real
    hn = 1e-30 * n
    dn = energy_density_np(name, omega, n + 1j * hn, sig).imag / hn
    hs = 1e-30 * np.where(sig > 0, sig, n ** (8 / 3))
    ds = energy_density_np(name, omega, n, sig + 1j * hs).imag / hs
    return e, dn, ds


class Evaluator(object):
    """stands in for the helfem_amd module where tests/lapl_dense.py asks for point values (xc_eval): the short-range exchange
    of the new ids comes from the NumPy restatement, with the kernels' threshold rules (a point below the density threshold
    carries nothing; an exchange spin channel below it is left out); every other functional and the other parts of the hybrids
    from the module's own evaluator, which its own tests pin.  Everything else is forwarded."""

    def __init__(self, hf):
        self._hf = hf
        self.ids = {hf.xc_func_ids(k)[0]: k for k in PRIMITIVES}
        self.hyb = {h["id"]: h for h in HYBRIDS.values()}

    def __getattr__(self, k):
        return getattr(self._hf, k)

    def _primitive(self, name, omega, rho, sigma, nspin, thr):
        rho = np.asarray(rho, dtype=float)
        if nspin == 1:
            out = {"exc": np.zeros_like(rho), "vrho": np.zeros_like(rho), "vsigma": np.zeros_like(rho)}
            live = (rho >= thr) & (rho > 0) & (0.5 * rho >= thr)
            e, dn, ds = eval_unpol_np(name, omega, rho[live], sigma[live])
            out["exc"][live], out["vrho"][live], out["vsigma"][live] = e / rho[live], dn, ds
        else:
            npt = rho.shape[0]
            out = {"exc": np.zeros(npt), "vrho": np.zeros((npt, 2)), "vsigma": np.zeros((npt, 3))}
            tot_ok = (rho.sum(1) >= thr) & (rho.sum(1) > 0)
            rt = np.maximum(rho[:, 0], thr) + np.maximum(rho[:, 1], thr)
            for sp, col in ((0, 0), (1, 2)):
                live = tot_ok & (rho[:, sp] >= thr) & (rho[:, sp] > 0)
                e, dn, ds = eval_unpol_np(name, omega, 2 * rho[live, sp], 4 * sigma[live, col])
                out["exc"][live] += 0.5 * e / rt[live]
                out["vrho"][live, sp] = dn
                out["vsigma"][live, col] = 2 * ds
        out["vlapl"], out["vtau"] = np.zeros_like(out["vrho"]), np.zeros_like(out["vrho"])
        return out

    def xc_eval(self, fid, rho, sigma=None, lapl=None, tau=None, nspin=1, thr=0.0):
        if fid in self.ids:
            return self._primitive(self.ids[fid], PRIMITIVES[self.ids[fid]]["omega"], rho, sigma, nspin, thr)
        if fid in self.hyb:
            out = None
            for w, part, pars in self.hyb[fid]["parts"]:
                if part in PRIMITIVES:
                    o = self._primitive(part, pars[0], rho, sigma, nspin, thr)
                else:
                    o = self._hf.xc_eval(self._hf.xc_func_ids(part)[0], rho, sigma, lapl, tau, nspin=nspin, thr=thr)
                out = {k: w * o[k] for k in o} if out is None else {k: out[k] + w * o[k] for k in o}
            return out
        return self._hf.xc_eval(fid, rho, sigma, lapl, tau, nspin=nspin, thr=thr)
