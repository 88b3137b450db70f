"""The one list of functionals (csrc/host/xc_funcs.h) as hfg_xc_func_table shows it, host side (no GPU): a frozen copy of the
names, ids and exact-exchange answers, the name <-> id lookups, what each row declares about its inputs and external
parameters checked through the point code (hfg_xc_eval / hfg_xc_eval_ext), and the refusal of ids that are not in the list."""
import numpy as np
import pytest

# (name, id, kfrac, kshort, omega, rs_kind) as hfg_xc_func_ids / hfg_xc_exact_exchange / hfg_xc_rs_kind answered before the
# list existed: a row cannot drift or vanish unnoticed
FROZEN = [
    ("lda_x", 1, 0.0, 0.0, 0.0, 0),
    ("lda_c_vwn", 7, 0.0, 0.0, 0.0, 0),
    ("lda_c_vwn_rpa", 8, 0.0, 0.0, 0.0, 0),
    ("lda_c_pw", 12, 0.0, 0.0, 0.0, 0),
    ("lda_c_pw_mod", 13, 0.0, 0.0, 0.0, 0),
    ("gga_x_pbe", 101, 0.0, 0.0, 0.0, 0),
    ("gga_c_pbe", 130, 0.0, 0.0, 0.0, 0),
    ("gga_x_b88", 106, 0.0, 0.0, 0.0, 0),
    ("gga_c_lyp", 131, 0.0, 0.0, 0.0, 0),
    ("hyb_gga_xc_b3lyp", 402, 0.2, 0.0, 0.0, 0),
    ("hyb_gga_xc_pbeh", 406, 0.25, 0.0, 0.0, 0),
    ("mgga_x_tpss", 202, 0.0, 0.0, 0.0, 0),
    ("mgga_c_tpss", 231, 0.0, 0.0, 0.0, 0),
    ("lda_x_erf", 546, 0.0, 0.0, 0.0, 0),
    ("lda_x_yukawa", 641, 0.0, 0.0, 0.0, 0),
    ("hyb_lda_xc_cam_lda0", 178, 0.5, -0.25, 0.3333333333333333, 2),
    ("mgga_x_br89", 206, 0.0, 0.0, 0.0, 0),
    ("mgga_c_cs", 72, 0.0, 0.0, 0.0, 0),
    ("mgga_x_scan", 263, 0.0, 0.0, 0.0, 0),
    ("mgga_c_scan", 267, 0.0, 0.0, 0.0, 0),
    ("hyb_mgga_x_scan0", 264, 0.25, 0.0, 0.0, 0),
    ("gga_x_pbe_sol", 116, 0.0, 0.0, 0.0, 0),
    ("gga_c_pbe_sol", 133, 0.0, 0.0, 0.0, 0),
    ("gga_x_pbe_r", 102, 0.0, 0.0, 0.0, 0),
    ("gga_x_ityh", 529, 0.0, 0.0, 0.0, 0),
    ("gga_x_sfat", 530, 0.0, 0.0, 0.0, 0),
    ("gga_x_ityh_pbe", 623, 0.0, 0.0, 0.0, 0),
    ("gga_x_sfat_pbe", 601, 0.0, 0.0, 0.0, 0),
    ("hyb_gga_xc_cam_b3lyp", 433, 0.65, -0.46, 0.33, 2),
    ("hyb_gga_xc_camy_b3lyp", 470, 0.65, -0.46, 0.34, 1),
    ("hyb_gga_xc_camy_blyp", 455, 1.0, -0.8, 0.44, 1),
    ("hyb_gga_xc_lcy_blyp", 468, 1.0, -1.0, 0.75, 1),
    ("hyb_gga_xc_lcy_pbe", 467, 1.0, -1.0, 0.75, 1),
]
PARS = {1: [1.1], 2: [0.9, 0.2], 3: [0.07, 0.03, 1.0]}  # accepted values by count; {omega} below
NPT = 50


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    helfem_amd.lib()
    return helfem_amd


@pytest.fixture(scope="module")
def rows(hf):
    return hf.xc_func_table()


def _points(nspin):
    """NPT fixed points, rho from 1e-12 to 1e2, with gradients, kinetic energy densities (above the von Weizsaecker bound) and
    Laplacians of either sign that vary from point to point"""
    k = np.arange(NPT)
    rho = np.logspace(-12, 2, NPT)
    s = 0.05 + 0.45 * (k % 7)  # reduced gradient
    sigma = (s * 2.0 * (3.0 * np.pi ** 2) ** (1.0 / 3.0) * rho ** (4.0 / 3.0)) ** 2
    tau = (1.2 + 0.1 * (k % 5)) * sigma / (8.0 * rho) + 0.3 * (3.0 * np.pi ** 2) ** (2.0 / 3.0) * rho ** (5.0 / 3.0) * (0.5 + 0.25 * (k % 3))
    lapl = np.where(k % 2, -1.0, 0.6) * rho ** (5.0 / 3.0) * (1.0 + k % 4)
    if nspin == 1:
        return dict(rho=rho, sigma=sigma, tau=tau, lapl=lapl)
    two = lambda a: np.stack([0.6 * a, 0.4 * a], axis=1)
    return dict(rho=two(rho), sigma=np.stack([0.36 * sigma, 0.2 * sigma, 0.16 * sigma], axis=1), tau=two(tau), lapl=two(lapl))


def _same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("exc", "vrho", "vsigma", "vlapl", "vtau"))


def test_frozen_copy(rows):
    assert [(r["name"], r["id"], r["kfrac"], r["kshort"], r["omega"], r["rs_kind"]) for r in rows] == FROZEN


def test_names_and_ids(hf, rows):
    assert len({r["id"] for r in rows}) == len(rows) and len({r["name"] for r in rows}) == len(rows)
    for r in rows:
        assert r["id"] > 0 and r["role"] in ("x", "c", "xc") and r["npar"] == len(r["pars"])
        assert hf.xc_func_ids(r["name"]) == (r["id"], 0) and hf.xc_func_ids(r["name"].upper()) == (r["id"], 0)
        assert hf.xc_func_ids(str(r["id"])) == (r["id"], 0)
        assert hf.xc_func_name(r["id"]) == r["name"]
        assert hf.xc_exact_exchange(r["id"]) == (r["omega"], r["kfrac"], r["kshort"]) and hf.xc_rs_kind(r["id"]) == r["rs_kind"]
    assert hf.xc_func_ids("none") == (0, 0) and hf.xc_func_name(0) == "none"
    assert hf.xc_func_ids("HF") == (-1, 0) and hf.xc_func_ids("hyb_x_hf") == (-1, 0) and hf.xc_func_name(-1) == "HF"
    assert hf.xc_exact_exchange(-1) == (0.0, 1.0, 0.0) and hf.xc_exact_exchange(0) == (0.0, 0.0, 0.0)
    assert hf.xc_func_ids("gga_x_pbe-gga_c_pbe") == (101, 130) and hf.xc_func_ids("101-130") == (101, 130)
    assert hf.xc_func_ids("lda_x-7") == (1, 7) and hf.xc_func_ids("999") == (999, 0)
    assert hf.xc_func_name(999) == "unknown"
    with pytest.raises(RuntimeError, match="functional gga_x_nonesuch is not available in this build!"):
        hf.xc_func_ids("gga_x_nonesuch")


@pytest.mark.parametrize("nspin", [1, 2])
def test_declared_inputs(hf, rows, nspin):
    pts = _points(nspin)
    for r in rows:
        base = hf.xc_eval(r["id"], nspin=nspin, **pts)
        assert np.all(np.isfinite(base["exc"])) and np.any(base["exc"] != 0.0), r["name"]
        for col, inp, out in (("grad", "sigma", "vsigma"), ("tau", "tau", "vtau"), ("lapl", "lapl", "vlapl")):
            if r[col]:
                assert np.any(base[out] != 0.0), (r["name"], out)  # the input is used somewhere on the set
                continue
            # the input is ignored, not small: exact zeros, and nothing moves when it changes
            assert not np.any(base[out]), (r["name"], out)
            moved = dict(pts)
            moved[inp] = 1.37 * pts[inp] + 0.01
            assert _same(base, hf.xc_eval(r["id"], nspin=nspin, **moved)), (r["name"], inp)
            assert _same(base, hf.xc_eval(r["id"], nspin=nspin, **{k: v for k, v in pts.items() if k != inp})), (r["name"], inp)


def test_external_parameters(hf, rows):
    pts = _points(1)
    for r in rows:
        word = "correlation" if r["role"] == "c" and r["npar"] else "exchange"
        for n in (1, 2, 3, 4):
            omega = r["pars"] == ("x_omega",)
            pars = [0.3] if omega and n == 1 else PARS.get(n, [0.5] * n)
            if n == r["npar"]:
                out = hf.xc_eval_ext(r["id"], pars, **pts)
                assert np.all(np.isfinite(out["exc"])) and not _same(out, hf.xc_eval(r["id"], **pts)), (r["name"], n)
            else:
                with pytest.raises(RuntimeError, match=r"External parameters are not supported for %s functional %d with %d values \(supported: "
                                   % (word, r["id"], n)):
                    hf.xc_eval_ext(r["id"], pars, **pts)
        if r["pars"] == ("x_omega",):
            for bad in (0.0, -0.2):
                with pytest.raises(RuntimeError, match="The range-separation constant omega must be positive."):
                    hf.xc_eval_ext(r["id"], [bad], **pts)
        assert _same(hf.xc_eval(r["id"], **pts), hf.xc_eval(r["id"], **pts))  # the defaults are back after every call
    assert sorted(r["id"] for r in rows if r["pars"] == ("x_omega",)) == [529, 530, 601, 623]


def test_unknown_ids(hf, rows):
    known = {r["id"] for r in rows}
    pts = _points(1)
    for fid in (0, -1, -178, -402, 2, 100, 132, 265, 624, 999):
        assert fid not in known
        with pytest.raises(RuntimeError, match="Functional not found!"):
            hf.xc_eval(fid, **pts)
