"""Short-range GGA exchange (gga_x_ityh 529, gga_x_sfat 530, gga_x_ityh_pbe, gga_x_sfat_pbe) and the range-separated GGA hybrids
built on it (hyb_gga_xc_cam_b3lyp 433, hyb_gga_xc_camy_b3lyp 470, hyb_gga_xc_camy_blyp 455, hyb_gga_xc_lcy_blyp 468,
hyb_gga_xc_lcy_pbe 467), host side (no GPU): the grid kernels' point code through hfg_xc_eval / hfg_xc_eval_ext.

The CPU oracle does not know these functionals and there is no libxc to compare with, so nothing here (or in
test_gpu_rsgga.py) is oracle or libxc parity.  Correctness rests on
  - an independent restatement of the published construction (rsgga_restatement.py: mpmath at 120 digits, closed forms only,
    no series branch), with complex-step derivatives of the restatement for the potentials;
  - exact reductions to point code that is pinned elsewhere (lda_x_erf / lda_x_yukawa at sigma = 0, gga_x_b88 / gga_x_pbe for
    omega -> 0, the bound att <= 1/(9 a^2) for large omega);
  - the composition of the hybrids out of evaluators that are pinned elsewhere, spin scaling, and polarised = restricted;
  - the names, ids, exact-exchange triples and option handling of the drivers."""
import os
import subprocess

import numpy as np
import pytest

import rsgga_restatement as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "helfem_amd", "bin")


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    helfem_amd.lib()
    return helfem_amd


# ---------------------------------------------------------------------------------------------------------------------
# 1. names, ids, exact exchange, screened kernel
# ---------------------------------------------------------------------------------------------------------------------
def test_names_ids_exact_exchange_and_kernel(hf):
    for name in rs.PRIMITIVES:
        fid = hf.xc_func_ids(name)[0]
        assert fid > 0 and hf.xc_func_ids(name) == (fid, 0) and hf.xc_func_ids(name.upper()) == (fid, 0)
        assert hf.xc_func_name(fid) == name
        assert hf.xc_exact_exchange(fid) == (0.0, 0.0, 0.0) and hf.xc_rs_kind(fid) == 0
    assert hf.xc_func_ids("gga_x_ityh") == (529, 0) and hf.xc_func_ids("gga_x_sfat") == (530, 0)
    ids = [hf.xc_func_ids(n)[0] for n in list(rs.PRIMITIVES) + list(rs.HYBRIDS)]
    assert len(set(ids)) == len(ids)
    for name, h in rs.HYBRIDS.items():
        assert hf.xc_func_ids(name) == (h["id"], 0)
        assert hf.xc_func_name(h["id"]) == name
        om, kfrac, kshort = hf.xc_exact_exchange(h["id"])
        assert om == h["omega"]
        assert abs(kfrac - (h["alpha"] + h["beta"])) <= 1e-15 and kshort == -h["beta"]
        assert hf.xc_rs_kind(h["id"]) == (1 if h["kernel"] == "yukawa" else 2)
    om, kfrac, kshort = hf.xc_exact_exchange(433)
    assert (om, round(kfrac, 14), kshort) == (0.33, 0.65, -0.46)
    assert hf.xc_rs_kind(433) == 2 and hf.xc_rs_kind(178) == 2 and hf.xc_rs_kind(402) == 0 and hf.xc_rs_kind(-1) == 0
    assert hf.xc_func_ids("gga_x_ityh-gga_c_lyp") == (529, 131)
    assert hf.xc_func_ids("hyb_gga_xc_lcy_pbe") == (467, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the independent restatement: values and potentials
# ---------------------------------------------------------------------------------------------------------------------
def _eval(hf, name, omega, pts, nspin):
    fid = hf.xc_func_ids(name)[0]
    pars = None if omega is None else [omega]
    if nspin == 1:
        return hf.xc_eval(fid, pts[0], pts[1], pars=pars)
    return hf.xc_eval(fid, np.stack(pts[0:2], 1), np.stack(pts[2:5], 1), nspin=2, pars=pars)


def _relerr(a, b, floor):
    return np.abs(a - b) / (np.abs(b) + floor)


# the tolerances are those of tests/test_scan_cpu.py for the same comparison: 1e-12 relative for exc (line 227), 1e-9
# relative for the potentials over a floor of 1e-12 |n eps| / x (lines 284-285)
TOL_EXC, TOL_V, V_FLOOR = 1e-12, 1e-9, 1e-12


@pytest.mark.parametrize("name", list(rs.PRIMITIVES))
@pytest.mark.parametrize("omega", [None, 0.33, 0.75])
def test_unpolarised_against_restatement(hf, name, omega):
    n, sig = rs.grid_unpol()
    o = _eval(hf, name, omega, (n, sig), 1)
    for k in ("exc", "vrho", "vsigma"):
        assert np.all(np.isfinite(o[k])), k
    om = rs.PRIMITIVES[name]["omega"] if omega is None else omega
    en, d_n, d_s = rs.ref_unpol(name, om, n, sig)
    err = _relerr(o["exc"], en / n, 0.0)
    print(name, omega, "exc max rel err %.3e" % err.max())
    assert err.max() <= TOL_EXC, (err.max(), n[err.argmax()], sig[err.argmax()])
    e1 = _relerr(o["vrho"], d_n, V_FLOOR * np.abs(en) / n)
    pos = sig > 0
    e2 = _relerr(o["vsigma"][pos], d_s[pos], V_FLOOR * np.abs(en[pos]) / sig[pos])
    e3 = _relerr(o["vsigma"][~pos], d_s[~pos], 0.0)  # sigma = 0: the derivative is finite and non-zero
    print(name, omega, "vrho %.3e vsigma %.3e (sigma = 0: %.3e)" % (e1.max(), e2.max(), e3.max()))
    assert e1.max() <= TOL_V and e2.max() <= TOL_V and e3.max() <= TOL_V


@pytest.mark.parametrize("name", list(rs.PRIMITIVES))
def test_polarised_against_restatement(hf, name):
    pts = rs.grid_pol()
    o = _eval(hf, name, None, pts, 2)
    for k in ("exc", "vrho", "vsigma"):
        assert np.all(np.isfinite(o[k])), k
    en, d = rs.ref_pol(name, rs.PRIMITIVES[name]["omega"], pts)
    nt = pts[0] + pts[1]
    err = _relerr(o["exc"], en / nt, 0.0)
    print(name, "polarised exc max rel err %.3e" % err.max())
    assert err.max() <= TOL_EXC
    v = np.concatenate([o["vrho"], o["vsigma"]], 1)
    assert np.all(v[:, 3] == 0.0)  # exchange does not depend on sigma_ab
    for k in (0, 1, 2, 4):
        x = pts[k]
        pos = x > 0
        e = _relerr(v[pos, k], d[k][pos], V_FLOOR * np.abs(en[pos]) / x[pos])
        assert e.max() <= TOL_V, (k, e.max())
        if np.any(~pos):
            assert _relerr(v[~pos, k], d[k][~pos], 0.0).max() <= TOL_V, k


@pytest.mark.parametrize("name", list(rs.PRIMITIVES))
@pytest.mark.parametrize("omega", [0.2, 0.75])
def test_numpy_restatement_against_the_closed_forms(name, omega):
    """the double-precision restatement that drives the dense grid worker of the GPU tests, against the 120-digit one"""
    n, sig = rs.grid_unpol()
    e, dn, ds = rs.eval_unpol_np(name, omega, n, sig)
    en, d_n, d_s = rs.ref_unpol(name, omega, n, sig)
    assert _relerr(e, en, 0.0).max() <= TOL_EXC
    assert _relerr(dn, d_n, V_FLOOR * np.abs(en) / n).max() <= TOL_V
    assert _relerr(ds, d_s, V_FLOOR * np.abs(en) / np.where(sig > 0, sig, np.inf)).max() <= TOL_V


def test_evaluator_follows_the_threshold_rules_of_the_kernels(hf):
    """rsgga_restatement.Evaluator against hfg_xc_eval with a density threshold in the middle of the grid"""
    ev = rs.Evaluator(hf)
    n, sig = rs.grid_unpol()
    pts = rs.grid_pol()
    R, S = np.stack(pts[0:2], 1), np.stack(pts[2:5], 1)
    for fid in list(ev.ids) + list(ev.hyb):
        for thr in (1e-12, 1e-6):
            a, b = ev.xc_eval(fid, n, sig, thr=thr), hf.xc_eval(fid, n, sig, thr=thr)
            assert np.all((a["exc"] == 0) == (b["exc"] == 0)), fid
            assert _relerr(a["exc"], b["exc"], 1e-300).max() <= 1e-11, fid
            keep = np.minimum(R[:, 0], R[:, 1]) >= 1e-10 if fid in ev.hyb else np.ones(len(R), bool)
            a, b = ev.xc_eval(fid, R[keep], S[keep], nspin=2, thr=thr), hf.xc_eval(fid, R[keep], S[keep], nspin=2, thr=thr)
            assert _relerr(a["exc"], b["exc"], 1e-300).max() <= 1e-11, fid
            assert np.all((a["vrho"] == 0) == (b["vrho"] == 0)), fid


# ---------------------------------------------------------------------------------------------------------------------
# 3. exact reductions
# ---------------------------------------------------------------------------------------------------------------------
def test_uniform_gas_point_is_the_short_range_lda(hf):
    """F_x(0) = 1: at sigma = 0 gga_x_ityh(omega = 0.3) is lda_x_erf (546) and gga_x_sfat(omega = 0.3) lda_x_yukawa (641)"""
    n = 10 ** np.linspace(-12, 3, 61)
    for name, ref in (("gga_x_ityh", 546), ("gga_x_sfat", 641), ("gga_x_ityh_pbe", 546), ("gga_x_sfat_pbe", 641)):
        a, b = _eval(hf, name, 0.3, (n, 0 * n), 1), hf.xc_eval(ref, n)
        for k in ("exc", "vrho"):
            err = np.max(np.abs(a[k] - b[k]) / np.abs(b[k]))
            assert err <= 4e-16 * 8, (name, k, err)  # a few roundings: sqrt(F) and the product with F = 1 are exact
        assert np.all(np.isfinite(a["vsigma"]))
    R = np.stack([n, n[::-1]], 1)
    for name, ref in (("gga_x_ityh", 546), ("gga_x_sfat", 641)):
        fid = hf.xc_func_ids(name)[0]
        a, b = hf.xc_eval(fid, R, nspin=2, pars=[0.3]), hf.xc_eval(ref, R, nspin=2)
        for k in ("exc", "vrho"):
            assert np.max(np.abs(a[k] - b[k]) / np.abs(b[k])) <= 4e-15, (name, k)


def test_small_omega_is_the_full_range_gga(hf):
    """omega -> 0: att = 1 - (8/3) sqrt(pi) a + O(a^2) for erfc and 1 - (4 pi/3) a + O(a^2) for Yukawa, both within
    [1 - (8/3) sqrt(pi) a, 1] for a <= 0.01; so |eps_sr / eps_GGA - 1| <= (8/3) sqrt(pi) a with a = omega sqrt(F_x) / (2 k_F)"""
    n, sig = rs.grid_unpol()
    om = 1e-8
    for name, ref in (("gga_x_ityh", 106), ("gga_x_ityh_pbe", 101), ("gga_x_sfat", 106), ("gga_x_sfat_pbe", 101)):
        a, b = _eval(hf, name, om, (n, sig), 1), hf.xc_eval(ref, n, sig)
        F = b["exc"] / rs.lda_x_eps_np(n)
        aa = om * np.sqrt(F) / (2 * (3 * np.pi ** 2 * n) ** (1 / 3))
        assert aa.max() < 0.01
        bound = (8 / 3) * np.sqrt(np.pi) * aa + 1e-14
        dev = np.abs(a["exc"] / b["exc"] - 1)
        assert np.all(dev <= bound), (name, np.max(dev / bound))
        assert np.all(a["exc"] / b["exc"] <= 1 + 1e-14)


@pytest.mark.parametrize("omega", [1e2, 1e5, 1e9, 1e14])
def test_large_omega_goes_to_zero_through_the_series(hf, omega):
    """att(a) <= 1/(9 a^2) for both kernels (first term of either series, which alternate with decreasing terms for a >= 1), so
    |eps_sr| <= |eps_x^LDA| F 4 k_F^2 / (9 omega^2 F) = |eps_x^LDA| 4 k_F^2 / (9 omega^2); nothing is NaN or Inf"""
    n, sig = rs.grid_unpol()
    kf = (3 * np.pi ** 2 * n) ** (1 / 3)
    ok = omega / (2 * kf) >= 2.0  # in the series branch of both kernels whatever F_x >= 1 is
    for name in rs.PRIMITIVES:
        o = _eval(hf, name, omega, (n, sig), 1)
        for k in ("exc", "vrho", "vsigma"):
            assert np.all(np.isfinite(o[k])), (name, k)
        assert np.all(o["exc"] <= 0.0)
        bound = np.abs(rs.lda_x_eps_np(n)) * 4 * kf ** 2 / (9 * omega ** 2)
        assert np.all(np.abs(o["exc"][ok]) <= bound[ok] * (1 + 1e-12)), name
    pts = rs.grid_pol()
    for name in rs.PRIMITIVES:
        o = _eval(hf, name, omega, pts, 2)
        for k in ("exc", "vrho", "vsigma"):
            assert np.all(np.isfinite(o[k])), (name, k)


def test_omega_must_be_positive_and_single(hf):
    n = np.array([0.1, 1.0])
    with pytest.raises(RuntimeError, match="omega must be positive"):
        hf.xc_eval(529, n, n, pars=[0.0])
    with pytest.raises(RuntimeError, match="External parameters are not supported for exchange functional 529 with 2 values"):
        hf.xc_eval(529, n, n, pars=[0.2, 0.3])
    with pytest.raises(RuntimeError, match="External parameters are not supported for exchange functional 433"):
        hf.xc_eval(433, n, n, pars=[0.2])
    # the parameter is in force for its call only
    a, b, c = hf.xc_eval(529, n, n), hf.xc_eval(529, n, n, pars=[0.7]), hf.xc_eval(529, n, n)
    assert np.all(a["exc"] == c["exc"]) and np.all(a["exc"] != b["exc"])
    assert np.all(hf.xc_eval(529, n, n, pars=[0.2])["exc"] == a["exc"])
    assert np.all(hf.xc_eval(530, n, n, pars=[0.44])["exc"] == hf.xc_eval(530, n, n)["exc"])


# ---------------------------------------------------------------------------------------------------------------------
# 4. composition of the hybrids
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rs.HYBRIDS))
@pytest.mark.parametrize("nspin", [1, 2])
def test_hybrid_is_the_sum_of_its_parts(hf, name, nspin):
    h = rs.HYBRIDS[name]
    if nspin == 1:
        n, sig = rs.grid_unpol()
        keep = n >= 1e-10  # gga_c_lyp and gga_c_pbe as they are; their own tests cover them down to this density
        args = (n[keep], sig[keep])
        kw = {}
    else:
        pts = rs.grid_pol()
        pts = [p[np.minimum(pts[0], pts[1]) >= 1e-10] for p in pts]
        args = (np.stack(pts[0:2], 1), np.stack(pts[2:5], 1))
        kw = {"nspin": 2}
    o = hf.xc_eval(h["id"], *args, **kw)
    tot = {k: np.zeros_like(o[k]) for k in ("exc", "vrho", "vsigma")}
    mag = {k: np.zeros_like(o[k]) for k in ("exc", "vrho", "vsigma")}
    for w, part, pars in h["parts"]:
        fid = hf.xc_func_ids(part)[0]
        r = hf.xc_eval(fid, *args, pars=pars, **kw)
        for k in tot:
            tot[k] += w * r[k]
            mag[k] += abs(w) * np.abs(r[k])
    for k in tot:
        assert np.all(np.isfinite(o[k]))
        err = np.max(np.abs(o[k] - tot[k]) / (mag[k] + 1e-300))
        assert err <= 1e-13, (name, k, err)  # the same operations in another order of summation


# ---------------------------------------------------------------------------------------------------------------------
# 5. spin scaling; polarised = restricted for equal spins
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rs.PRIMITIVES))
def test_spin_scaling(hf, name):
    """E_x[ra, rb] = (E_x[2 ra] + E_x[2 rb]) / 2, the potentials with it"""
    fid = hf.xc_func_ids(name)[0]
    ra, rb, saa, sab, sbb = rs.grid_pol()
    p = hf.xc_eval(fid, np.stack([ra, rb], 1), np.stack([saa, sab, sbb], 1), nspin=2)
    ua, ub = hf.xc_eval(fid, 2 * ra, 4 * saa), hf.xc_eval(fid, 2 * rb, 4 * sbb)
    E = 0.5 * (2 * ra * ua["exc"] + 2 * rb * ub["exc"])

    def close(a, b):
        return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)) <= 1e-14

    assert close(p["exc"] * (ra + rb), E)
    assert close(p["vrho"][:, 0], ua["vrho"]) and close(p["vrho"][:, 1], ub["vrho"])
    assert close(p["vsigma"][:, 0], 2 * ua["vsigma"]) and close(p["vsigma"][:, 2], 2 * ub["vsigma"])
    assert np.all(p["vsigma"][:, 1] == 0.0)


@pytest.mark.parametrize("name", list(rs.PRIMITIVES) + list(rs.HYBRIDS))
def test_polarised_equal_spins_equals_restricted(hf, name):
    fid = hf.xc_func_ids(name)[0]
    n, s = rs.grid_unpol()
    keep = n >= 1e-10
    n, s = n[keep], s[keep]
    o = hf.xc_eval(fid, n, s)
    p = hf.xc_eval(fid, np.stack([n / 2, n / 2], 1), np.stack([s / 4] * 3, 1), nspin=2)
    tol = 1e-11  # tests/test_scan_cpu.py:367, the bound for GGAs that run other arithmetic in their two forms

    def close(a, b):
        return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)) <= tol

    assert close(p["exc"], o["exc"])
    assert close(p["vrho"][:, 0], o["vrho"]) and close(p["vrho"][:, 1], o["vrho"])
    assert close(p["vsigma"].sum(1) / 4, o["vsigma"])


# ---------------------------------------------------------------------------------------------------------------------
# 6. command lines
# ---------------------------------------------------------------------------------------------------------------------
def _run(exe, *args):
    p = subprocess.run([os.path.join(BIN, exe)] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.fixture(scope="module")
def cli(hf):
    from helfem_amd import build
    build.build_cli(verbose=False)


ATOM = ["--Z", "Ne", "--lmax", "0", "--mmax", "0", "--nelem", "3"]
DIATOM = ["--Z1", "H", "--Z2", "H", "--Rbond", "1.4", "--lmax", "4", "--nelem", "2"]
REFUSALS = ("not available in this build", "not supported", "not implemented", "Functional not found")


def test_atomic_accepts_the_new_functionals(cli):
    """the option check passes (on a machine without a GPU the run then stops at the device)"""
    import helfem_amd
    gpu = helfem_amd.device_count() > 0
    for method in list(rs.HYBRIDS) + ["gga_x_ityh-gga_c_lyp", "gga_x_sfat_pbe-gga_c_pbe"]:
        for extra in ([], ["--M", "3", "--Q", "0"]):
            rc, out, err = _run("atomic", *(ATOM + ["--method", method, "--maxit", "1"] + extra))
            assert not any(t in err for t in REFUSALS), (method, err)
            if not gpu:
                assert "HIP device" in err or "hip" in err.lower(), (method, err)
    rc, out, err = _run("atomic", *(ATOM + ["--method", "gga_x_ityh-gga_c_lyp", "--x_pars", "0.3", "--maxit", "1"]))
    assert not any(t in err for t in REFUSALS), err


def test_diatomic_refuses_the_hybrids_and_runs_the_primitives_as_lda_x_erf(cli):
    for method in rs.HYBRIDS:
        rc, out, err = _run("diatomic", *(DIATOM + ["--method", method]))
        assert rc == 1 and "Range separated functionals are not supported" in err, (method, err)
    # lda_x_erf is a pure functional there; so are the short-range GGA primitives
    for method in ("lda_x_erf", "gga_x_ityh-gga_c_lyp", "gga_x_sfat"):
        rc, out, err = _run("diatomic", *(DIATOM + ["--method", method]))
        assert not any(t in err for t in REFUSALS), (method, err)


def test_external_parameter_counts(cli):
    for exe, args in (("atomic", ATOM), ("diatomic", DIATOM)):
        rc, out, err = _run(exe, *(args + ["--method", "gga_x_ityh-gga_c_lyp", "--x_pars", "0.2 0.3"]))
        assert rc == 1 and "External parameters are not supported for exchange functional 529 with 2 values" in err, err
    for method, fid in (("hyb_gga_xc_cam_b3lyp", 433), ("hyb_gga_xc_lcy_pbe", 467)):
        rc, out, err = _run("atomic", *(ATOM + ["--method", method, "--x_pars", "0.3"]))
        assert rc == 1 and "External parameters are not supported for exchange functional %d" % fid in err, err
    rc, out, err = _run("atomic", *(ATOM + ["--method", "hyb_gga_xc_lcy_pbe", "--c_pars", "0.046 0.031 1.0"]))
    assert rc == 1 and "External parameters are not supported for correlation functional 0" in err, err
