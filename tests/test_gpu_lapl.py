"""Laplacian-dependent meta-GGAs of the atomic program on the GPU (mgga_x_br89 = 206, mgga_c_cs = 72): the XC kernels'
Laplacian planes against the dense NumPy restatement of the reference's atomic grid worker (tests/lapl_dense.py), the Fock
matrix against central differences of Exc, spin and shard consistency, and the SCF drivers."""
import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

CASES = {
    # name: (Z, lmax, mmax, nelem, nnodes)
    "s_only": (2, 0, 0, 3, 6),
    "sp": (10, 1, 1, 3, 5),
    "spd_m1": (18, 2, 1, 2, 6),
}
PAIRS = [(206, 72), (206, 0), (0, 72), (202, 72), (106, 72)]


@pytest.fixture(scope="module")
def hf():
    import helfem_amd
    if helfem_amd.device_count() < 1:
        pytest.fail("no HIP device visible")
    return helfem_amd


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request, hf):
    import lapl_dense
    Z, lmax, mmax, nelem, nnodes = CASES[request.param]
    gb, _ = common.make_atomic_bases(Z, lmax, mmax, nelem, nnodes, oracle=False)
    gb.compute_tei(True)
    ldft, mdft = 4 * lmax + 10, 4 * mmax + 5
    gb.upload(ldft, mdft)
    dense = lapl_dense.DenseWorker(hf, gb, hf.get_grid(40.0, nelem, 4, 2.0), nnodes, ldft, mdft)
    blocks = gb.get_sym_idx(1)
    return request.param, gb, dense, ldft, mdft, blocks


def _pd(gb, blocks, seed):
    return common.random_density(gb.Nbf(), 2, seed=seed, blocks=blocks)


@pytest.mark.parametrize("pair", PAIRS, ids=["%d-%d" % p for p in PAIRS])
def test_restricted_parity_with_dense_restatement(hf, case, pair):
    name, gb, dense, ldft, mdft, blocks = case
    P = _pd(gb, blocks, 3)
    H, Exc, Nel, _ = hf.DFTGrid(gb, ldft, mdft).eval_Fxc(pair[0], pair[1], P)
    Hd, Excd, Neld = dense.eval_Fxc(pair[0], pair[1], P)
    assert abs(Exc - Excd) <= 1e-11 * abs(Excd), (name, Exc, Excd)
    assert abs(Nel - Neld) <= 1e-11 * abs(Neld)
    assert common.relerr(H, Hd) <= 1e-10, (name, common.relerr(H, Hd))


@pytest.mark.parametrize("pair", [(206, 72), (202, 72)], ids=["206-72", "202-72"])
def test_polarised_parity_with_dense_restatement(hf, case, pair):
    name, gb, dense, ldft, mdft, blocks = case
    Pa, Pb = _pd(gb, blocks, 4), 0.5 * _pd(gb, blocks, 5)
    Ha, Hb, Exc, Nel, _ = hf.DFTGrid(gb, ldft, mdft).eval_Fxc_pol(pair[0], pair[1], Pa, Pb)
    Had, Hbd, Excd, Neld = dense.eval_Fxc_pol(pair[0], pair[1], Pa, Pb)
    assert abs(Exc - Excd) <= 1e-11 * abs(Excd), (name, Exc, Excd)
    assert abs(Nel - Neld) <= 1e-11 * abs(Neld)
    assert common.relerr(Ha, Had) <= 1e-10 and common.relerr(Hb, Hbd) <= 1e-10, (common.relerr(Ha, Had), common.relerr(Hb, Hbd))


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
    """d/dt f(t) at 0 from central differences at h and h/2, extrapolated (the h^2 term removed: the low-density regions
    where CS and BR89 are steep make it about 1e-6 of the derivative at h = 1e-5).  What remains is of order 1e-7: points
    that cross the density threshold between the displaced densities, where Exc is not differentiable"""
    c = lambda s: (f(s) - f(-s)) / (2 * s)  # noqa: E731
    return (4 * c(h / 2) - c(h)) / 3


def test_fock_matrix_is_the_derivative_of_exc(hf, case):
    name, gb, dense, ldft, mdft, blocks = case
    g = hf.DFTGrid(gb, ldft, mdft)
    P = _pd(gb, blocks, 6)
    H, _, _, _ = g.eval_Fxc(206, 72, P)
    Pa, Pb = _pd(gb, blocks, 7), 0.5 * _pd(gb, blocks, 8)
    Ha, Hb, _, _, _ = g.eval_Fxc_pol(206, 72, Pa, Pb)
    h = 1e-4
    for D in _directions(gb, blocks):
        fd = _richardson(lambda t: g.eval_Fxc(206, 72, P + t * D)[1], h)
        an = np.sum(H * D)
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1e-3), (name, fd, an)
        fda = _richardson(lambda t: g.eval_Fxc_pol(206, 72, Pa + t * D, Pb)[2], h)
        fdb = _richardson(lambda t: g.eval_Fxc_pol(206, 72, Pa, Pb + t * D)[2], h)
        assert abs(fda - np.sum(Ha * D)) <= 1e-6 * max(abs(fda), 1e-3), (name, fda, np.sum(Ha * D))
        assert abs(fdb - np.sum(Hb * D)) <= 1e-6 * max(abs(fdb), 1e-3), (name, fdb, np.sum(Hb * D))


def test_polarised_equals_restricted_for_equal_spins(hf, case):
    name, gb, dense, ldft, mdft, blocks = case
    g = hf.DFTGrid(gb, ldft, mdft)
    P = _pd(gb, blocks, 9)
    H, Exc, Nel, Ekin = g.eval_Fxc(206, 72, P)
    Ha, Hb, Excp, Nelp, Ekinp = g.eval_Fxc_pol(206, 72, 0.5 * P, 0.5 * P)
    assert abs(Exc - Excp) <= 1e-12 * abs(Exc) and abs(Nel - Nelp) <= 1e-12 * Nel
    assert common.relerr(Ha, H) <= 1e-11 and common.relerr(Hb, H) <= 1e-11


def test_shards_sum_to_the_unsharded_result(hf, case):
    name, gb, dense, ldft, mdft, blocks = case
    g = hf.DFTGrid(gb, ldft, mdft)
    P = _pd(gb, blocks, 10)
    Pa, Pb = _pd(gb, blocks, 12), 0.5 * _pd(gb, blocks, 13)
    H, Exc, Nel, _ = g.eval_Fxc_dev(206, 72, P)
    Ha, Hb, Excp, _, _ = g.eval_Fxc_dev(206, 72, Pa, Pb)
    ctx = gb.ctx
    for n in (2, 3):
        acc, e, accA, accB, ep = np.zeros_like(H), 0.0, np.zeros_like(H), np.zeros_like(H), 0.0
        try:
            for rk in range(n):
                ctx.set_shard(rk, n)
                h, x, _, _ = g.eval_Fxc_dev(206, 72, P)
                acc += h
                e += x
                ha, hb, xp, _, _ = g.eval_Fxc_dev(206, 72, Pa, Pb)
                accA += ha
                accB += hb
                ep += xp
        finally:
            ctx.set_shard(0, 1)
        assert common.relerr(acc, H) <= 1e-12 and abs(e - Exc) <= 1e-12 * abs(Exc)
        assert common.relerr(accA, Ha) <= 1e-12 and common.relerr(accB, Hb) <= 1e-12 and abs(ep - Excp) <= 1e-12 * abs(Excp)


def test_restricted_is_reproducible_bitwise(hf, case):
    name, gb, dense, ldft, mdft, blocks = case
    g = hf.DFTGrid(gb, ldft, mdft)
    P = _pd(gb, blocks, 14)
    a, b = g.eval_Fxc(206, 72, P), g.eval_Fxc(206, 72, P)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def test_diatomic_basis_refuses_laplacian_functionals(hf):
    gb, _ = common.make_bases(1, 1, 1.4, (3, 2), 2, 5, oracle=False)
    gb.compute_tei(True)
    gb.upload(12, 9)
    P = common.random_density(gb.Nbf(), 1, seed=1)
    with pytest.raises(RuntimeError, match="Laplacian not implemented!"):
        hf.DFTGrid(gb, 12, 9).eval_Fxc(206, 72, P)


def test_hydrogen_br89_exchange_on_the_1s_density(hf):
    """BR89 is exact for the hydrogen 1s density: on the ground state of the one-electron problem in the product's own basis
    (core Hamiltonian: the one-electron SCF), Ex = -5/16 Eh within the basis error.  The bound is the observed deviation
    (5e-10 with this basis) with a margin; it is not derived."""
    gb, _ = common.make_atomic_bases(1, 0, 0, 5, 15, oracle=False)
    gb.compute_tei(True)
    S, H0 = gb.overlap(), gb.kinetic() + gb.nuclear()
    e, U = np.linalg.eigh(S)
    X = U @ np.diag(e ** -0.5) @ U.T
    E, C = np.linalg.eigh(X @ H0 @ X)
    c = X @ C[:, 0]
    assert abs(E[0] + 0.5) < 1e-8
    Pa = np.outer(c, c)
    _, _, Ex, Nel, _ = hf.DFTGrid(gb, 10, 5).eval_Fxc_pol(206, 0, Pa, np.zeros_like(Pa))
    print("H 1s: BR89 Ex = %.12f, Nel = %.12f" % (Ex, Nel))
    assert abs(Nel - 1.0) < 1e-8
    assert abs(Ex + 0.3125) < 1e-6, Ex


@pytest.mark.parametrize("kw", [dict(Z=10, lmax=1, mmax=1, nelem=4, nnodes=10, method="mgga_x_br89-mgga_c_cs"),
                                dict(Z=7, lmax=1, mmax=1, nelem=4, nnodes=10, method="mgga_x_br89-mgga_c_cs", M=4)],
                         ids=["Ne_restricted", "N_unrestricted"])
def test_scf_converges_and_device_driver_matches_host_driver(hf, kw, monkeypatch):
    """No literature totals are pinned for BR89-CS here: the SCF must converge, and the device-resident driver must equal the
    host-pointer driver"""
    dev = hf.scf_atomic(convthr=1e-8, maxit=80, **kw)
    monkeypatch.setenv("HELFEM_SCF", "host")
    host = hf.scf_atomic(convthr=1e-8, maxit=80, **kw)
    assert dev["converged"] and host["converged"], (dev, host)
    for k in ("Etot", "Exc"):
        assert abs(dev[k] - host[k]) < 1e-8 * max(1.0, abs(host[k])), (k, dev[k], host[k])
    print("SCF", kw["method"], kw["Z"], dev["Etot"], dev["Exc"], dev["iterations"])
