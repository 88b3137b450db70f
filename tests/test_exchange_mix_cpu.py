"""The mixed-kernel exchange tables of the range-separated hybrids (hfg_mix_exchange_tables, hip/exchange_mix.hip): what can
be checked without a GPU -- the algebra of the mixed table (tests/exchange_mix_restatement.py), the argument checks that
come before any device call, the switch, the keywords of the step objects and the adapter program."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import exchange_mix_restatement as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = xr.EPS
ENTRIES = ("hfg_mix_exchange_tables", "hfg_mix_exchange", "hfg_mix_exchange_devptr", "hfg_mix_exchange_occ_devptr",
           "hfg_mix_exchange_occ_batch_devptr")


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    return helfem_amd


# (elements, nodes, lmax, mmax): the He-like basis with a non-adjacent element pair and M != 0 couplings; one element
SHAPES = [(3, 4, 1, 1), (1, 4, 1, 1)]


@pytest.mark.parametrize("kind", [1, 2], ids=["yukawa", "erfc"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s[:2] for s in SHAPES])
@pytest.mark.parametrize("ab", [(0.19, 0.46), (0.25, -0.25), (0.0, 1.0)], ids=["cam-b3lyp", "cam-lda0", "screened-only"])
def test_mixed_table_gives_the_weighted_sum_of_the_two_exchange_matrices(hf, kind, shape, ab):
    """K from the pair-form contraction over the mixed blocks (Coulomb LM_fac, the ratio of the weights folded in) against
    alpha K_coul + beta K_rs from the separate tables in their own forms (factorised with the outer element taking Q, or
    erfc pair blocks) and their own LM_fac.

    Bound 8 N eps max|K|: both sides sum the same products term by term, an entry of K being a sum of at most
    A^2 N_L p^2 E <= N^2 terms of which, by the element and angular selection rules, fewer than N are non-zero per block
    pair; the sides differ in how each term is rounded -- the mixed side rounds the outer product, the two scalings and
    the sum of the two kernels (4 roundings), the separate side the two contractions and their weighted sum (4 more)."""
    E, p, lmax, mmax = shape
    alpha, beta = ab
    gb, t = xr.make(hf, 2, lmax, mmax, E, p, kind, 0.4)
    N = gb.Nbf()
    import common
    P = common.random_density(N, 2, seed=5)
    Kc, Ks = t.K_coulomb(P), t.K_screened(P)
    want = alpha * Kc + beta * Ks
    got = t.K_mixed(alpha, beta, P)
    scale = float(np.max(np.abs(want)))
    err = float(np.max(np.abs(got - want)))
    print("kind %d %dx%d alpha %.2f beta %.2f: max|K| %.3e, deviation %.3e, bound %.3e" % (kind, E, p, alpha, beta, scale, err, 8 * N * EPS * scale))
    assert scale > 1e-3 and float(np.max(np.abs(Ks))) > 1e-4, "a reference that vanishes would prove nothing"
    assert err <= 8 * N * EPS * scale
    # the orientation of the cross blocks matters: with P and Q swapped the Coulomb part is off by orders of magnitude
    if E > 1:
        swapped = t.dense_K_factorised(t.tei, t.Q0, t.P0, t.fac, P)
        assert float(np.max(np.abs(swapped - Kc))) > 1e-3 * float(np.max(np.abs(Kc)))


def test_restatement_agrees_with_the_oracle(hf):
    """the dense contraction itself: against the oracle's exchange and rs_exchange (1e-12 relative, the parity bound of
    tests/test_gpu_rs.py)"""
    import common
    _, ob = common.make_atomic_bases(Z=2, lmax=1, mmax=1, nelem=3, nnodes=4, product=False)
    ob.compute_tei(True)
    P = common.random_density(ob.Nbf, 2, seed=5)
    for kind in (1, 2):
        gb, t = xr.make(hf, 2, 1, 1, 3, 4, kind, 0.4)
        (ob.compute_yukawa if kind == 1 else ob.compute_erfc)(0.4)
        assert common.relerr(t.K_coulomb(P), ob.exchange(P)) < 1e-12
        assert common.relerr(t.K_screened(P), ob.rs_exchange(P)) < 1e-12


def test_padding_of_the_restated_blocks_is_zero(hf):
    gb, t = xr.make(hf, 2, 1, 1, 3, 4, 1, 0.4)
    p, E = t.p, t.E
    blocks = t.mixed_blocks(0.19, 0.46)
    for L in range(t.NL):
        for e in range(E):
            for f in range(E):
                b4 = blocks[L][e][f].reshape(p, p, p, p)
                if e == 0:
                    assert not np.any(b4[0]) and not np.any(b4[:, 0])
                if f == 0:
                    assert not np.any(b4[:, :, 0]) and not np.any(b4[:, :, :, 0])
                if e == E - 1:
                    assert not np.any(b4[p - 1]) and not np.any(b4[:, p - 1])
                if f == E - 1:
                    assert not np.any(b4[:, :, p - 1]) and not np.any(b4[:, :, :, p - 1])
                assert np.any(b4)


def test_symbols_exported_and_declared(hf):
    L = hf.lib()
    header = open(os.path.join(ROOT, "include", "helfem_gpu.h")).read()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert re.search(r"^int %s\(" % name, header, re.M), name


def test_argument_checks_come_before_any_device_call(hf):
    import common
    L = hf.lib()
    f = L.hfg_mix_exchange_tables
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double]
    fake = ctypes.c_void_p(8)  # never dereferenced
    gb, _ = common.make_atomic_bases(Z=2, lmax=1, mmax=1, nelem=3, nnodes=4, oracle=False)
    dia, _ = common.make_bases(oracle=False)
    assert f(None, gb.h, 0.2, 0.4) == 1 and b"null context" in L.hfg_last_error()
    assert f(fake, None, 0.2, 0.4) == 1 and b"null context or basis" in L.hfg_last_error()
    assert f(fake, dia.h, 0.2, 0.4) == 1 and L.hfg_last_error() == b"Range separated functionals are not supported.\n"
    assert f(fake, gb.h, 0.2, 0.4) == 1 and b"needs range-separated tables" in L.hfg_last_error()
    assert f(fake, gb.h, 0.2, 0.0) == 1 and b"have not been uploaded" in L.hfg_last_error()
    gb.compute_tei(True)
    gb.compute_erfc(0.4)
    assert f(fake, gb.h, 0.2, 0.4) == 1 and b"have not been uploaded" in L.hfg_last_error()
    # the exchange entries without a mixed set
    g = L.hfg_mix_exchange_devptr
    g.argtypes = [ctypes.c_void_p] * 4
    assert g(fake, gb.h, fake, fake) == 1 and b"mixed exchange tables have not been built" in L.hfg_last_error()
    assert g(None, gb.h, fake, fake) == 1 and g(fake, gb.h, None, fake) == 1 and b"null matrix pointer" in L.hfg_last_error()
    assert g(fake, dia.h, fake, fake) == 1 and L.hfg_last_error() == b"Range separated functionals are not supported.\n"
    o = L.hfg_mix_exchange_occ_devptr
    o.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_void_p]
    assert o(fake, gb.h, fake, None, 2, fake) == 1 and b"occupied orbitals missing" in L.hfg_last_error()
    assert o(fake, gb.h, fake, fake, 0, fake) == 1
    b = L.hfg_mix_exchange_occ_batch_devptr
    b.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                  ctypes.c_int64, ctypes.c_void_p]
    n = (ctypes.c_int64 * 2)(1, 9)
    assert b(fake, gb.h, 0, None, None, None, 4, None) == 0  # nothing to do
    assert b(fake, gb.h, -1, fake, fake, n, 4, fake) == 1
    assert b(fake, gb.h, 2, fake, fake, n, 4, fake) == 1 and b"outside 0 ... ldc_cols" in L.hfg_last_error()
    assert b(fake, gb.h, 2, fake, fake, None, 4, fake) == 1 and b"null pointer to the occupied orbitals" in L.hfg_last_error()
    with pytest.raises(RuntimeError, match="mixed exchange tables have not been built"):
        gb.mix_exchange(np.zeros((gb.Nbf(), gb.Nbf())))


def test_a_set_beyond_the_bound_of_the_pair_path_is_refused_with_its_own_status(hf):
    """3 slots x 170^2 element pairs x 15^4 doubles = 35.1e9 bytes > 32e9: status 4 before anything is looked at on a device"""
    lval, mval = hf.angular_basis(1, 1)
    gb = hf.AtomicTwoDBasis(18, 15, 75, hf.get_grid(40.0, 170, 4, 2.0), lval, mval)
    L = hf.lib()
    f = L.hfg_mix_exchange_tables
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double]
    assert 3 * 170 ** 2 * 15 ** 4 * 8 > 32e9 > 3 * 162 ** 2 * 15 ** 4 * 8
    assert f(ctypes.c_void_p(8), gb.h, 0.2, 0.0) == 4 and b"more than the" in L.hfg_last_error()


def test_switch_is_in_the_table(hf):
    rows = {r["name"]: r for r in hf.tuning_table()}
    r = rows["HELFEM_EXL_MIX"]
    assert (r["kind"], r["default"], r["read"]) == ("int", "-1", "live")
    assert set(hf.MIX_BY_DEFAULT) == {1, 2}


@pytest.mark.parametrize("cls", ["DeviceSCFStep", "DeviceUSCFStep", "DeviceROHFStep"])
def test_step_classes_accept_the_keywords(hf, cls):
    import common
    klass = getattr(hf, cls)
    if cls != "DeviceROHFStep":  # (takes *args, **kw and hands them on)
        pars = inspect.signature(klass.__init__).parameters
        assert list(pars)[-3:] == ["kshort", "omega", "rs_kind"]
        assert (pars["kshort"].default, pars["omega"].default, pars["rs_kind"].default) == (0.0, 0.0, None)
        assert list(pars)[:15] == ["self", "basis", "x_func", "c_func", "ldft", "mdft", "nocc", "symmetry", "device", "rank", "nranks",
                                   "dens_thr", "kfrac", "device_tei", "fock_shard"]
    dia, _ = common.make_bases(oracle=False)
    nocc = 1 if cls == "DeviceSCFStep" else (1, 1)
    with pytest.raises(RuntimeError, match="Range separated functionals are not supported."):
        klass(dia, 0, 0, 0, 0, nocc, kfrac=0.19, kshort=0.46, omega=0.33, rs_kind=2)
    gb, _ = common.make_atomic_bases(oracle=False)
    with pytest.raises(ValueError, match="screened kernel"):
        klass(gb, 0, 0, 0, 0, nocc, kfrac=0.19, kshort=0.46, omega=0.33)  # no functional to take the kernel from


def test_adapter_program_compiles_and_links(native_libs):
    from helfem_amd import build
    exe = build._build_adapter_program("mix_exchange_adapter_check", False)
    p = subprocess.run([exe, "compile-only"], stdout=subprocess.PIPE, timeout=60)
    assert p.returncode == 0 and b"adapter compiled" in p.stdout
    text = open(os.path.join(ROOT, "include", "helfem_gpu_arma.hpp")).read()
    assert re.search(r"Mat mix_exchange\(const Mat &P, double alpha, double beta\)", text)
