"""Finite nuclei, confinement potentials and off-centre nuclei of the atomic program, on the host: grids, one-electron
matrices against the NumPy restatement tests/atomic_potentials_dense.py (same elements, same rule), analytic one-electron
pins, the reference's refusals, and the command line as far as it gets without a device."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import atomic_potentials_dense as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "helfem_amd", "bin")
NN, NQ = 15, 75


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    helfem_amd.lib()
    from helfem_amd import build
    build.build_cli(verbose=False)
    return helfem_amd


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


TABLE_BAR = 1e-12  # same basis, same rule on both sides: the project's bar for tables


def dense(hf, g, l, m, **kw):
    return D.DenseAtom(g, hf.lobatto_nodes(NN), NQ, l, m, gaunt=hf.gaunt_coefficient, **kw)


# ---- grids ---------------------------------------------------------------------------------------------------------------
def test_plain_grid_is_the_radial_grid(hf):
    assert np.array_equal(hf.atomic_grid(7, Rmax=35.0, igrid=4, zexp=2.0), hf.get_grid(35.0, 7, 4, 2.0))
    assert np.array_equal(hf.atomic_grid(7, Rmax=35.0, add_conf=True, shift_conf=0.0), hf.get_grid(35.0, 7, 4, 2.0))


@pytest.mark.parametrize("model,rnuc", [(1, 3 * 1e-4), (2, math.sqrt(5.0 / 3.0) * 1e-4), (3, 1e-4)])
def test_finite_nucleus_grid(hf, model, rnuc):
    g = hf.atomic_grid(5, Rmax=40.0, finitenuc=model, Rrms=1e-4, nelem0=2, Z=80)
    assert len(g) == 5 + 2 * 2 + 1 and np.all(np.diff(g) > 0) and g[0] == 0.0
    # the nuclear grid is laid down twice (to rnuc and to 2 rnuc) before the electronic one of length Rmax - rnuc
    assert np.sum(g == rnuc) == 1 and np.sum(np.abs(g - 2 * rnuc) < 1e-18) == 1 and abs(g[-1] - (40.0 + rnuc)) < 1e-13
    assert np.array_equal(g, D.form_grid(5, 40.0, finitenuc=model, Rrms=1e-4, nelem0=2, Z=80))


@pytest.mark.parametrize("Z,Zl,Zr,Rmid", [(0, 1, 1, 1.0), (3, 0, 1, 1.5), (3, 2, 1, 1.5)])
def test_offcentre_grid(hf, Z, Zl, Zr, Rmid):
    g = hf.atomic_grid(4, Rmax=40.0, nelem0=2, Z=Z, Zl=Zl, Zr=Zr, Rmid=Rmid)
    assert np.all(np.diff(g) > 0) and np.sum(g == Rmid) == 1
    assert np.sum(g < Rmid) == (4 if Z else 2)  # nelem0 elements per segment inside Rmid
    assert np.array_equal(g, D.form_grid(4, 40.0, nelem0=2, Z=Z, Zl=Zl, Zr=Zr, Rmid=Rmid))
    # a shift on the nucleus' own boundary is not added twice
    g2 = hf.atomic_grid(4, Rmax=40.0, nelem0=2, Z=Z, Zl=Zl, Zr=Zr, Rmid=Rmid, add_conf=True, shift_conf=Rmid)
    assert np.array_equal(g, g2)


def test_confinement_boundary(hf):
    g0 = hf.get_grid(40.0, 5, 4, 2.0)
    g = hf.atomic_grid(5, Rmax=40.0, add_conf=True, shift_conf=6.0)
    assert np.sum(g == 6.0) == 1 and len(g) == len(g0) + 1 and np.array_equal(np.sort(np.append(g0, 6.0)), g)
    assert np.array_equal(hf.atomic_grid(5, Rmax=40.0, add_conf=False, shift_conf=6.0), g0)
    assert np.array_equal(hf.atomic_grid(5, Rmax=40.0, add_conf=True, shift_conf=g0[3]), g0)


# ---- matrices against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [1, 2, 3])
def test_finite_nucleus_matrix(hf, model):
    Z, Rrms = 80, 1e-4
    g = hf.atomic_grid(5, Rmax=40.0, finitenuc=model, Rrms=Rrms, nelem0=2, Z=Z)
    l, m = hf.angular_basis(1, 1)
    b = hf.AtomicTwoDBasis(Z, NN, NQ, g, l, m, finitenuc=model, Rrms=Rrms)
    d = dense(hf, g, l, m)
    V = b.nuclear()
    e = rel(V, d.nuclear_finite(model, Z, Rrms))
    print("finite nucleus model %d: rel. deviation %.2e" % (model, e))
    assert e <= TABLE_BAR
    assert rel(b.overlap(), d.overlap()) <= TABLE_BAR and rel(b.kinetic(), d.kinetic()) <= TABLE_BAR
    assert rel(V, d.nuclear_point(Z)) > 1e-6  # and it is not the point nucleus


@pytest.mark.parametrize("Z,a", [(1, 2.0), (10, 5.0)])
def test_regularized_nucleus(hf, Z, a):
    """--finitenuc 4: the matrix against the restatement, and the property that defines the model: its 1s level is -Z^2/2
    whatever a is.  The basis error of that level, measured with the restatement at this basis: 2e-13 (Z = 1, a = 2) and
    5.584e-6 (Z = 10, a = 5, whose core of width 1/(Z a) = 0.02 bohr sits inside the first element); bounds ten times those."""
    g = hf.atomic_grid(5, Rmax=40.0, finitenuc=4, Rrms=a, Z=Z)
    assert np.array_equal(g, hf.get_grid(40.0, 5, 4, 2.0))  # the normal grid
    l, m = hf.angular_basis(1, 0)
    b = hf.AtomicTwoDBasis(Z, NN, NQ, g, l, m, finitenuc=4, Rrms=a)
    d = dense(hf, g, l, m)
    V = b.nuclear()
    e = rel(V, d.nuclear_finite(4, Z, a))
    E = D.lowest(b.kinetic() + V, b.overlap())[0]
    Ed = D.lowest(d.kinetic() + d.nuclear_finite(4, Z, a), d.overlap())[0]
    print("regularized nucleus Z %d a %g: rel. deviation %.2e, 1s %.13f (restatement %.13f)" % (Z, a, e, E, Ed))
    assert e <= TABLE_BAR
    assert abs(E + 0.5 * Z * Z) < {1: 2e-12, 10: 5.584e-5}[Z] and abs(E - Ed) < 1e-10
    assert rel(V, d.nuclear_point(Z)) > 1e-3  # finite at the origin: not the point nucleus


CONF_CASES = [(1, 2, 3.0, 0.0, 0.0), (1, 2, -3.0, 0.0, 0.0), (1, 4, 2.0, 0.0, 6.0), (1, -1, 2.0, 0.0, 0.0), (2, 2, 5.0, 0.0, 6.0),
              (3, 0, 0.0, 1.0, 6.0), (4, 2, 0.0, 0.5, 6.0)]


@pytest.mark.parametrize("add_conf", [True, False])
@pytest.mark.parametrize("iconf,N,R,V,shift", CONF_CASES)
def test_confinement_matrix(hf, add_conf, iconf, N, R, V, shift):
    g = hf.atomic_grid(5, Rmax=40.0, add_conf=add_conf, shift_conf=shift)
    l, m = hf.angular_basis(1, 0)
    b = hf.AtomicTwoDBasis(1, NN, NQ, g, l, m)
    Vc = b.confinement(iconf, N, R, V, shift)
    e = rel(Vc, dense(hf, g, l, m).confinement(iconf, N, R, V, shift))
    print("iconf %d N %d shift %g add_conf %d: rel. deviation %.2e" % (iconf, N, shift, add_conf, e))
    assert e <= TABLE_BAR
    assert np.abs(Vc - Vc.T).max() == 0.0 or rel(Vc, Vc.T) < 1e-14
    if iconf == 1 and R < 0:
        assert np.all(np.diag(Vc) <= 0.0)  # attractive


@pytest.mark.parametrize("Z,Zl,Zr,Rmid", [(0, 1, 1, 1.0), (3, 0, 1, 1.5), (3, 2, 1, 1.5)])
def test_offcentre_nuclear_matrix(hf, Z, Zl, Zr, Rmid):
    g = hf.atomic_grid(4, Rmax=40.0, nelem0=2, Z=Z, Zl=Zl, Zr=Zr, Rmid=Rmid)
    l, m = hf.angular_basis(3, 1)
    b = hf.AtomicTwoDBasis(Z, NN, NQ, g, l, m, Zl=Zl, Zr=Zr, Rmid=Rmid)
    d = dense(hf, g, l, m)
    V = b.nuclear()
    e = rel(V, d.nuclear_point(Z) + d.nuclear_offcenter(Zl, Zr, Rmid))
    print("Z %d Zl %d Zr %d: rel. deviation %.2e" % (Z, Zl, Zr, e))
    assert e <= TABLE_BAR
    R = b.Nrad()
    odd = np.abs(V[0:R, R:2 * R]).max()  # <l=0|V|l=1>, m = 0
    assert (odd == 0.0) if Zl == Zr else (odd > 1e-3)  # a symmetric pair has no odd multipoles


# ---- zeroder --------------------------------------------------------------------------------------------------------------
def test_zeroder_keeps_the_last_function(hf):
    g = hf.get_grid(40.0, 5, 4, 2.0)
    l, m = hf.angular_basis(1, 1)
    b0 = hf.AtomicTwoDBasis(1, NN, NQ, g, l, m)
    b1 = hf.AtomicTwoDBasis(1, NN, NQ, g, l, m, zeroder=True)
    assert b1.Nbf() == b0.Nbf() + b0.Nang() and b1.Nang() == b0.Nang()
    d1 = dense(hf, g, l, m, zeroder=True)
    assert rel(b1.overlap(), d1.overlap()) <= TABLE_BAR and rel(b1.kinetic(), d1.kinetic()) <= TABLE_BAR
    assert rel(b1.nuclear(), d1.nuclear_point(1)) <= TABLE_BAR
    E0 = D.lowest(b0.kinetic() + b0.nuclear(), b0.overlap())[0]
    E1 = D.lowest(b1.kinetic() + b1.nuclear(), b1.overlap())[0]
    # the basis's own accuracy for the 1s level: 2.3e-13 either way (restatement), the generalised eigensolver's noise
    # included; ten times that
    assert abs(E0 + 0.5) < 2.4e-12 and abs(E1 + 0.5) < 2.4e-12 and abs(E1 - E0) < 2.4e-12


# ---- analytic pins: one electron, the library's matrices, NumPy's eigensolver ------------------------------------------
def test_oscillator_from_polynomial_confinement(hf):
    """V = (r/r0)^2 on a chargeless centre: E0 = 1.5 sqrt(2)/r0.  Truncation error of this basis (5 elements to 40 bohr,
    15 nodes), measured with the restatement: 3.2e-11 Eh; bound ten times that."""
    r0 = 2.0
    g = hf.get_grid(40.0, 5, 4, 2.0)
    b = hf.AtomicTwoDBasis(0, NN, NQ, g, [0], [0])
    assert np.abs(b.nuclear()).max() == 0.0
    E = D.lowest(b.kinetic() + b.confinement(1, 2, r0), b.overlap())[0]
    d = dense(hf, g, [0], [0])
    Ed = D.lowest(d.kinetic() + d.confinement(1, 2, r0), d.overlap())[0]
    print("oscillator: E %.14f exact %.14f restatement %.14f" % (E, 1.5 * math.sqrt(2) / r0, Ed))
    assert abs(E - 1.5 * math.sqrt(2) / r0) < 3.2e-10
    assert abs(E - Ed) < 1e-11


def test_uniform_sphere_shift_of_hydrogen_1s(hf):
    """1s level of a uniformly charged sphere against the point nucleus: first order (2/3) Z^4 Rrms^2.  Z = 1, Rrms = 0.01:
    the restatement gives 6.556069e-5 against 6.666667e-5 first order, i.e. 1.106e-6 of higher order in Z Rrms; bound ten
    times that."""
    Z, Rrms = 1, 1e-2
    g = hf.atomic_grid(5, Rmax=40.0, finitenuc=2, Rrms=Rrms, nelem0=2, Z=Z)
    bf = hf.AtomicTwoDBasis(Z, NN, NQ, g, [0], [0], finitenuc=2, Rrms=Rrms)
    bp = hf.AtomicTwoDBasis(Z, NN, NQ, g, [0], [0])
    S, T = bf.overlap(), bf.kinetic()
    shift = D.lowest(T + bf.nuclear(), S)[0] - D.lowest(T + bp.nuclear(), S)[0]
    print("uniform sphere: shift %.9e first order %.9e" % (shift, 2.0 / 3.0 * Z ** 4 * Rrms ** 2))
    assert shift > 0.0 and abs(shift - 2.0 / 3.0 * Z ** 4 * Rrms ** 2) < 1.106e-5
    assert abs(shift - 6.556069204e-05) < 1e-11  # the restatement's value for this basis


def test_h2plus_single_centre(hf):
    """H2+ at R = 2 as Z = 0, Zl = Zr = 1, Rmid = 1: electronic energy -1.1026342144949 Eh.  Partial waves to l = 16, m = 0:
    the truncation error measured at this basis is 2.331e-4 Eh (the l expansion of a cusp off the centre converges
    algebraically); bound ten times that, and from above (variational)."""
    g = hf.atomic_grid(5, Rmax=40.0, nelem0=3, Z=0, Zl=1, Zr=1, Rmid=1.0)
    l, m = hf.angular_basis(16, 0)
    b = hf.AtomicTwoDBasis(0, NN, NQ, g, l, m, Zl=1, Zr=1, Rmid=1.0)
    E = D.lowest(b.kinetic() + b.nuclear(), b.overlap())[0]
    print("H2+: E %.12f, above exact by %.3e" % (E, E + 1.1026342144949))
    assert 0.0 < E + 1.1026342144949 < 2.331e-3
    # the same through partial waves to l = 8 against the restatement: one number, both sides
    l, m = hf.angular_basis(8, 0)
    b = hf.AtomicTwoDBasis(0, NN, NQ, g, l, m, Zl=1, Zr=1, Rmid=1.0)
    d = dense(hf, g, l, m)
    E8 = D.lowest(b.kinetic() + b.nuclear(), b.overlap())[0]
    Ed = D.lowest(d.kinetic() + d.nuclear_offcenter(1, 1, 1.0), d.overlap())[0]
    assert abs(E8 - Ed) < 1e-11 and E8 > E


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_carry_the_reference_texts(hf):
    g = hf.get_grid(40.0, 5, 4, 2.0)
    with pytest.raises(RuntimeError, match="Off-center nuclei not supported in finite nucleus mode!"):
        hf.AtomicTwoDBasis(1, NN, NQ, g, [0], [0], finitenuc=2, Rrms=1e-4, Zl=1, Zr=1, Rmid=1.0)
    with pytest.raises(RuntimeError, match="Off-center nuclei not supported in finite nucleus mode!"):
        hf.atomic_grid(5, finitenuc=2, Rrms=1e-4, nelem0=2, Z=1, Zl=1, Rmid=1.0)
    with pytest.raises(RuntimeError, match="Nucleus placed within element!"):
        hf.AtomicTwoDBasis(0, NN, NQ, g, [0], [0], Zl=1, Zr=1, Rmid=1.0).nuclear()  # 1.0 is no boundary of this grid
    b = hf.AtomicTwoDBasis(1, NN, NQ, g, [0], [0])
    with pytest.raises(RuntimeError, match="Cannot have a divergent potential with a shift!"):
        b.confinement(1, -1, 2.0, 0.0, 3.0)
    with pytest.raises(RuntimeError, match="Exponential confinement potential requires N >= 1!"):
        b.confinement(2, 0, 2.0)
    with pytest.raises(RuntimeError, match="Exponential confinement potential does not make sense with negative N!"):
        b.confinement(2, -1, 2.0)
    with pytest.raises(RuntimeError, match="Cannot have attractive barrier!"):
        b.confinement(3, 0, 0.0, -1.0, 3.0)
    with pytest.raises(RuntimeError, match="Junquera confinement potential requires N >= 1!"):
        b.confinement(4, 0, 0.0, 1.0, 3.0)
    with pytest.raises(RuntimeError, match="No such nucleus!"):
        hf.AtomicTwoDBasis(1, NN, NQ, g, [0], [0], finitenuc=5, Rrms=1e-4)
    with pytest.raises(RuntimeError, match="Unrecognized model"):
        hf.AtomicTwoDBasis(1, NN, NQ, g, [0], [0], finitenuc=7, Rrms=1e-4)
    with pytest.raises(RuntimeError, match="Nuclear grid not handled!"):
        hf.atomic_grid(5, finitenuc=7, Rrms=1e-4, nelem0=2, Z=1)


def test_options_check_with_and_without_extras(hf):
    """hfg_scf_options_check / hfg_scf_run keep their refusals; the extras lift them for the atomic program and validate
    the combination on the host"""
    for kw, msg in ((dict(finitenuc=2), "Finite nuclear models are not supported"), (dict(iconf=3), "Confinement potentials"),
                    (dict(zeroder=1), "--zeroder is not supported")):
        with pytest.raises(RuntimeError, match=msg):
            hf.scf_run_atomic(2, 0, 0, 4, 10, check_only=True, **kw)
    ok = hf.scf_run_atomic
    ok(2, 0, 0, 4, 10, check_only=True, iconf=3, extras=dict(conf_barrier=1.0, shift_conf=6.0))
    ok(2, 0, 0, 4, 10, check_only=True, finitenuc=1, extras=dict(Rrms=1e-4, nelem0=2))
    ok(2, 0, 0, 4, 10, check_only=True, finitenuc=4, extras=dict(Rrms=3.0))
    with pytest.raises(RuntimeError, match="SCF runs with zero derivative at Rmax are not supported"):
        ok(2, 0, 0, 4, 10, check_only=True, zeroder=1, extras=dict())
    with pytest.raises(RuntimeError, match="Nuclear grid not handled!"):
        ok(2, 0, 0, 4, 10, check_only=True, finitenuc=5, extras=dict(Rrms=1e-4))
    ok(0, 4, 0, 4, 10, check_only=True, extras=dict(Zl=1, Zr=1, Rmid=0.7, nelem0=2))   # electrons from Z + Zl + Zr
    ok(3, 4, 0, 4, 10, check_only=True, symmetry=2, extras=dict(Zr=1, Rmid=1.5, nelem0=2))
    with pytest.raises(RuntimeError, match="Off-center nuclei not supported in finite nucleus mode!"):
        ok(2, 0, 0, 4, 10, check_only=True, finitenuc=2, extras=dict(Rrms=1e-4, nelem0=2, Zl=1, Zr=1, Rmid=1.0))
    with pytest.raises(RuntimeError, match="Cannot have attractive barrier!"):
        ok(2, 0, 0, 4, 10, check_only=True, iconf=3, extras=dict(conf_barrier=-1.0, shift_conf=6.0))
    with pytest.raises(RuntimeError, match="Cannot have a divergent potential with a shift!"):
        ok(2, 0, 0, 4, 10, check_only=True, iconf=1, extras=dict(conf_N=-1, conf_R=2.0, shift_conf=6.0))
    with pytest.raises(RuntimeError, match="Thomas-Fermi guess"):
        ok(0, 4, 0, 4, 10, check_only=True, iguess=3, extras=dict(Zl=1, Zr=1, Rmid=0.7, nelem0=2))
    with pytest.raises(RuntimeError, match="fields are not supported"):
        ok(2, 0, 0, 4, 10, check_only=True, Ez=0.01, extras=dict())


def test_options_structure_keeps_its_size(hf):
    """hfg_scf_options is what hfg_scf_options_default clears: 1504 bytes, the binding's declaration field by field"""
    buf = (ctypes.c_ubyte * 4096)(*([0xAA] * 4096))
    hf.lib().hfg_scf_options_default.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert hf.lib().hfg_scf_options_default(ctypes.addressof(buf), 1) == 0
    touched = max(i for i in range(4096) if buf[i] != 0xAA) + 1
    assert touched == ctypes.sizeof(hf.hfg_scf_options) == 1504


# ---- command lines ----------------------------------------------------------------------------------------------------------
def run(exe, *args):
    p = subprocess.run([os.path.join(BIN, exe)] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def gpu_present(hf):
    return hf.device_count() > 0


ATOM = ["--lmax", "0", "--mmax", "0", "--nelem", "4", "--nnodes", "10", "--save", "", "--maxit", "1"]


@pytest.mark.parametrize("args", [["--Z", "H", "--M", "2", "--iconf", "3", "--conf_barrier", "1", "--shift_conf", "6"],
                                  ["--Z", "Ne", "--finitenuc", "1", "--Rrms", "1e-4", "--nelem0", "2"],
                                  ["--Z", "", "--Zl", "H", "--Zr", "H", "--Rmid", "0.7", "--nelem0", "2"],
                                  ["--Z", "He", "--finitenuc", "4", "--Rrms", "3.0"]])
def test_atomic_command_line_gets_to_the_device(hf, args):
    rc, out, err = run("atomic", *(args + ATOM))
    assert "not supported by this build" not in err, err
    if gpu_present(hf):  # one iteration, then the energy table
        assert rc == 0 and "Total" in out, err
    else:
        assert rc == 1 and "no usable HIP device" in err, err


@pytest.mark.parametrize("args,msg", [
    (["--Z", "He", "--finitenuc", "2", "--Rrms", "1e-4", "--nelem0", "2", "--Zl", "H", "--Zr", "H", "--Rmid", "1"], "Off-center nuclei not supported in finite nucleus mode!"),
    (["--Z", "He", "--iconf", "3", "--conf_barrier", "-1", "--shift_conf", "6"], "Cannot have attractive barrier!"),
    (["--Z", "He", "--iconf", "2", "--conf_N", "0", "--conf_R", "2"], "requires N >= 1"),
    (["--Z", "He", "--zeroder", "1"], "SCF runs with zero derivative at Rmax are not supported"),
    (["--Z", "He", "--Ez", "0.01"], "fields are not supported")])
def test_atomic_command_line_refusals(hf, args, msg):
    rc, out, err = run("atomic", *(args + ATOM))
    assert rc == 1 and msg in err, err
    assert "no usable HIP device" not in err


def test_diatomic_command_line_is_untouched(hf):
    base = ["--Z1", "H", "--Z2", "H", "--Rbond", "1.4", "--lmax", "4", "--nelem", "2"]
    for extra, msg in ((["--finitenuc", "1"], "Finite nuclear models are not supported by this build."),
                       (["--Ez", "0.01"], "fields are not supported")):
        rc, out, err = run("diatomic", *(base + extra))
        assert rc == 1 and msg in err and "no usable HIP device" not in err, err
