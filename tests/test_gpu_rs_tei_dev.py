"""Range-separated exchange tables built on the GPU (hip/rs_tei_dev.hip, hip/special_dev.h) against the host build
(host/atomic_basis.cpp, host/special.cpp) and the independent fixtures.

Point functions: the device may differ from the host by at most what the host itself differs from the 40-digit values,
worst case over the same points (tests/golden/rs_special.json, and tests/golden/rs_special_dev.json with arguments on both
sides of every branch).  Tables: the bounds the host tables meet in tests/test_tei_golden_cpu.py (1e-11 relative for the
four Yukawa sets, 1e-9 for the two erfc sets), against the fixture and against the host tables.  Use: hfg_rs_exchange and the
SCF drivers with device-built tables against the same with host-built tables.

Measured on MI355X, worst relative difference (device vs host | host vs fixture):
  rs_special.json      i_L 0 | 9.0e-16, k_L 0 | 5.2e-16, Phi_L 3.6e-15 | 2.5e-10 (exact binomials), 4.6e-05 (the reference's)
  rs_special_dev.json  i_L 0 | 1.1e-15, k_L 2.0e-16 | 5.2e-16, Phi_L 3.4e-10 | 8.4e-07 (exact), 2.1e-04 (the reference's)
(the Phi_L figures are the closed form's cancellation at L = 8 next to the switching points: (1, 0.401), (0.51, 0.45))
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YUKAWA_BOUND, ERFC_BOUND = 1e-11, 1e-9  # tests/test_tei_golden_cpu.py: the host tables against atomic_tei.npz
YUKAWA_TABLES = (("disjoint_iL", "disjoint_iL"), ("disjoint_kL", "disjoint_kL"), ("rs_tei", "yukawa_tei"), ("rs_ktei", "yukawa_ktei"))
ERFC_TABLES = (("rs_tei", "erfc_tei"), ("rs_ktei", "erfc_ktei"))


@pytest.fixture(scope="module")
def hf():
    import helfem_amd
    if helfem_amd.device_count() < 1:
        pytest.fail("no HIP device visible")
    return helfem_amd


# ---- point functions ---------------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(b != 0.0)
    return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.0


def _by_order(points, key):
    out = {}
    for e in points:
        out.setdefault(e[key], []).append(e)
    return sorted(out.items())


@pytest.mark.parametrize("fixture", ["rs_special.json", "rs_special_dev.json"])
def test_bessel_functions_device_against_host_and_fixture(hf, fixture):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", fixture)))
    for which, name, host_fn in ((0, "il", hf.bessel_il), (1, "kl", hf.bessel_kl)):
        dev_host = host_fix = 0.0
        for L, pts in _by_order(gold["bessel"], "L"):
            x = np.array([e["x"] for e in pts])
            ref = np.array([float(e[name]) for e in pts])
            host = np.array([host_fn(v, L) for v in x])
            dev = hf.rs_special_dev(which, L, x)
            dev_host, host_fix = max(dev_host, _rel(dev, host)), max(host_fix, _rel(host, ref))
        print("%s %s: device vs host %.3e, host vs fixture %.3e" % (fixture, name, dev_host, host_fix))
        assert dev_host <= host_fix, (name, dev_host, host_fix)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("fixture", ["rs_special.json", "rs_special_dev.json"])
def test_phi_device_against_host_and_fixture(hf, fixture, mode):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", fixture)))
    hf.set_erfc_binomial_mode(mode)
    try:
        dev_host = host_fix = 0.0
        for n, pts in _by_order(gold["phi"], "n"):
            Xi, xi = np.array([e["Xi"] for e in pts]), np.array([e["xi"] for e in pts])
            ref = np.array([float(e["phi"]) for e in pts])
            host = np.array([hf.erfc_phi(n, a, b) for a, b in zip(Xi, xi)])
            dev = hf.rs_special_dev(2, n, Xi, xi)
            assert np.array_equal(dev, hf.rs_special_dev(2, n, xi, Xi))  # argument order is free
            dev_host, host_fix = max(dev_host, _rel(dev, host)), max(host_fix, _rel(host, ref))
        print("%s Phi mode %d: device vs host %.3e, host vs fixture %.3e" % (fixture, mode, dev_host, host_fix))
        assert dev_host <= host_fix, (dev_host, host_fix)
        # xi == 0: Phi_n = 0 for n > 0 (no fixture value to divide by), the k = 0 term alone for n = 0
        for n in range(9):
            Xi = np.array([1e-8, 0.3, 0.7, 3.0, 5.0])  # (erfc(Xi) underflows beyond 26)
            dev = hf.rs_special_dev(2, n, Xi, np.zeros_like(Xi))
            host = np.array([hf.erfc_phi(n, a, 0.0) for a in Xi])
            if n:
                assert np.all(dev == 0.0) and np.all(host == 0.0)
            else:
                assert _rel(dev, host) <= host_fix
    finally:
        hf.set_erfc_binomial_mode(0)


# ---- tables ------------------------------------------------------------------------------------------------------------------
def _small_basis(hf):
    g = np.load(os.path.join(ROOT, "tests", "golden", "atomic_tei.npz"))
    NL = int(g["case_NL"])
    lval = list(range((NL - 1) // 2 + 1))
    ab = hf.AtomicTwoDBasis(2, int(g["case_nnodes"]), int(g["case_nquad"]), g["bval"], lval, [0] * len(lval), ctx=hf.default_context())
    return g, ab, NL, len(g["bval"]) - 1


def _tables(ab, kind, NL, E):
    """every table of the kind, read back through hfg_basis_get_prim: {(name, L, e[, f]): table}"""
    out = {}
    for name, _ in (YUKAWA_TABLES if kind == "yukawa" else ERFC_TABLES):
        for L in range(NL):
            for e in range(E):
                if kind == "yukawa":
                    out[(name, L, e)] = ab.atomic_table(name, L, e)
                else:
                    for f in range(E):  # every ordered pair, (0,0), (0,k) and (k,0) among them
                        out[(name, L, e, f)] = ab.atomic_table(name, L, e, f)
    return out


def _worst(got, ref):
    worst = 0.0
    for key in ref:
        assert got[key].shape == ref[key].shape, (key, got[key].shape, ref[key].shape)
        worst = max(worst, float(np.max(np.abs(got[key] - ref[key])) / np.max(np.abs(ref[key]))))
    return worst


@pytest.fixture(scope="module")
def small(hf):
    """host-built and device-built tables of the basis of tests/golden/atomic_tei.npz, built once"""
    g, host, NL, E = _small_basis(hf)
    _, dev, _, _ = _small_basis(hf)
    out = {"g": g, "NL": NL, "E": E}
    for kind, omega in (("yukawa", float(g["case_lam"])), ("erfc", float(g["case_mu"]))):
        getattr(host, "compute_" + kind)(omega)
        out[kind + "_host"] = _tables(host, kind, NL, E)
        getattr(dev, "compute_" + kind)(omega, device=True)
        out[kind + "_dev"] = _tables(dev, kind, NL, E)
        getattr(dev, "compute_" + kind)(omega, device=True)
        out[kind + "_dev2"] = _tables(dev, kind, NL, E)
    return out


@pytest.mark.parametrize("kind", ["yukawa", "erfc"])
def test_device_tables_against_fixture_and_host(small, kind):
    g, bound = small["g"], YUKAWA_BOUND if kind == "yukawa" else ERFC_BOUND
    dev, host = small[kind + "_dev"], small[kind + "_host"]
    assert set(dev) == set(host)
    if kind == "erfc":
        E = small["E"]
        assert {k[2:] for k in dev} == {(e, f) for e in range(E) for f in range(E)}
    for name, fix in (YUKAWA_TABLES if kind == "yukawa" else ERFC_TABLES):
        ref = {k: g[fix + "_" + "_".join(str(q) for q in k[1:])] for k in dev if k[0] == name}
        vs_fix, vs_host = _worst(dev, ref), _worst(dev, {k: host[k] for k in ref})
        print("%s %s: device vs fixture %.3e, device vs host %.3e, host vs fixture %.3e" % (kind, name, vs_fix, vs_host, _worst(host, ref)))
        assert vs_fix < bound and vs_host < bound, (name, vs_fix, vs_host)


@pytest.mark.parametrize("kind", ["yukawa", "erfc"])
def test_two_device_builds_are_bitwise_equal(small, kind):
    a, b = small[kind + "_dev"], small[kind + "_dev2"]
    assert all(np.array_equal(a[k], b[k]) for k in a)


# 15 nodes: nq = 75, p^2 = 225 (196 in the first and last element) -- the products cross the 64 x 64 tiles with partial edge
# tiles, a row (L, e) has three blocks and the batches more than one diagonal pair; 6 nodes: p^2 = 36 (25), below one tile
@pytest.mark.parametrize("nnodes,lmax", [(15, 2), (6, 2)])
@pytest.mark.parametrize("kind", ["yukawa", "erfc"])
def test_edge_shapes_against_host_tables(hf, kind, nnodes, lmax):
    bases = [common.make_atomic_bases(Z=2, lmax=lmax, mmax=0, nelem=3, nnodes=nnodes, oracle=False)[0] for _ in range(2)]
    host, dev = bases
    dev.ctx = hf.default_context()
    NL, E = 2 * lmax + 1, 3
    getattr(host, "compute_" + kind)(0.45)
    getattr(dev, "compute_" + kind)(0.45, device=True)
    th, td = _tables(host, kind, NL, E), _tables(dev, kind, NL, E)
    assert td[("rs_tei", 0, 1) + ((1,) if kind == "erfc" else ())].shape == (nnodes * nnodes, nnodes * nnodes)
    for name, _ in (YUKAWA_TABLES if kind == "yukawa" else ERFC_TABLES):
        worst = _worst(td, {k: v for k, v in th.items() if k[0] == name})
        print("nnodes %d %s %s: device vs host %.3e" % (nnodes, kind, name, worst))
        assert worst < (YUKAWA_BOUND if kind == "yukawa" else ERFC_BOUND), (name, worst)


# ---- use ---------------------------------------------------------------------------------------------------------------------
def _worker(mode, path, env):
    e = {k: v for k, v in os.environ.items() if k not in ("HELFEM_RS_TEI", "HELFEM_EXL_PAIR", "HELFEM_SCF")}
    e.update(env)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rs_tei_dev_worker.py"), mode, path], env=e, cwd=ROOT, timeout=600,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    return np.load(path)


@pytest.mark.parametrize("pair", ["1", "0"], ids=["lowrank", "general"])
def test_exchange_with_device_tables_equals_exchange_with_host_tables(hf, tmp_path, pair):
    r = _worker("exchange", str(tmp_path / "k.npz"), {"HELFEM_EXL_PAIR": pair})
    for kind in ("yukawa", "erfc"):
        Kh, Kd = r["K_%s_host" % kind], r["K_%s_dev" % kind]
        assert np.max(np.abs(Kh)) > 1e-3
        err = common.relerr(Kd, Kh)
        print("rs_exchange %s HELFEM_EXL_PAIR=%s: device tables vs host tables %.3e" % (kind, pair, err))
        assert err <= 1e-11, (kind, err)


def test_scf_with_the_switch_reaches_the_host_table_energy(hf, tmp_path):
    host = _worker("scf", str(tmp_path / "h.npz"), {})
    dev = _worker("scf", str(tmp_path / "d.npz"), {"HELFEM_RS_TEI": "dev"})
    assert str(host["rs_tei"][0]) == "host" and str(dev["rs_tei"][0]) == "dev"
    keys = [k for k in host.files if k.startswith("E_")]
    assert len(keys) == 4
    for k in keys:
        print("%s: host tables %.10f device tables %.10f" % (k, host[k][0], dev[k][0]))
        assert abs(host[k][0] - dev[k][0]) < 1e-8, (k, host[k][0], dev[k][0])
