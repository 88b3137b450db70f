"""P_L^M(xi), Q_L^M(xi) of the reference's own Fortran Legendre library (oracle/_ref/libref_legendre.so, built from the
reference sources by oracle/build_ref.sh; run where that library has been built) at every xi that the oracle's compute_tei asks for
in the SCF of tests/test_golden_cpu.py::test_reference_legendre_library_does_not_move_energies.  The calls are the ones
LegendreTable::compute makes (src/general/legendretable.cpp:74-75): calc_Plm_arr / calc_Qlm_arr(array, Lpad, Lpad, xi)
with Lpad = Lmax + lpad, of which the [M, L] corner M <= Mmax, L <= Lmax is kept as the library returned it.
Output: tests/golden/legendre_reference_scf.npz (inputs and outputs only)."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as orc  # noqa: E402

from test_golden_cpu import LEGENDRE_SCF_CASE  # noqa: E402

lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_legendre.so"))
dp = ctypes.POINTER(ctypes.c_double)
for f in (lib.calc_Plm_arr, lib.calc_Qlm_arr):
    f.argtypes = [dp, ctypes.c_int, ctypes.c_int, ctypes.c_double]
CB = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, dp, dp)

shape, rec = set(), {}


def provider(Lmax, Mmax, lpad, xi, P, Q):
    shape.add((Lmax, Mmax, lpad))
    Lp = Lmax + lpad
    a = np.zeros((Lp + 1, Lp + 1))
    b = np.zeros((Lp + 1, Lp + 1))
    if xi != 1.0:
        lib.calc_Plm_arr(a.ctypes.data_as(dp), Lp, Lp, xi)
        lib.calc_Qlm_arr(b.ctypes.data_as(dp), Lp, Lp, xi)
        rec[xi] = (a[:Mmax + 1, :Lmax + 1].copy(), b[:Mmax + 1, :Lmax + 1].copy())
    for M in range(Mmax + 1):
        for L in range(Lmax + 1):
            P[M * (Lmax + 1) + L] = a[M, L]
            Q[M * (Lmax + 1) + L] = b[M, L]


cb = CB(provider)
L = orc.lib()
L.orc_set_legendre_provider.argtypes = [CB]
L.orc_set_legendre_provider.restype = None
os.chdir("/tmp")  # the Fortran library writes fort.9 into the cwd
L.orc_set_legendre_provider(cb)
try:
    orc.scf_diatomic(**LEGENDRE_SCF_CASE)
finally:
    L.orc_set_legendre_provider(ctypes.cast(None, CB))
assert len(shape) == 1, shape
(Lmax, Mmax, lpad), = shape
xi = np.array(sorted(rec))
np.savez_compressed(os.path.join(HERE, "legendre_reference_scf.npz"), xi=xi, Lmax=Lmax, Mmax=Mmax, lpad=lpad,
                    P=np.array([rec[x][0] for x in xi]), Q=np.array([rec[x][1] for x in xi]),
                    source="src/legendre/*.f90 via Legendre_Wrapper.f90:135,173")
print("wrote", len(xi), "points, Lmax", Lmax, "Mmax", Mmax, "lpad", lpad)
