"""Known answers for the device special functions (hip/special_dev.h) at arguments on both sides of every branch of
i_L, k_L and Phi_L, L = 0 ... 8, computed with mpmath at 40 digits (Phi_L: 120) as tests/golden/make_rs_golden.py computes its own
(Bessel functions from mpmath's, Phi_L by numerical integration of its definition), written to
tests/golden/rs_special_dev.json.

  i_L, k_L: x at 1e-8 and 1e-3 (leading term of the series), around 4L and around 30 (the switch to the upward recurrence
            is x > 30 and x > 4L), and at 16, 40, 60 (outermost element, 40 bohr, times omega = 0.4, 1, 1.5)
  Phi_L:    xi around 0.4; Xi around 0.5 with xi below it; arguments given in either order (xi on both sides of Xi and
            of 2 Xi); xi = 0 for L = 0; arguments of 1e-8; 16 and 40 (outermost element times omega; erfc underflows in
            FP64 beyond 26, so the small partner of 40 is 39 and that of 16 is 0.2)

Run:  python tests/golden/make_rs_special_dev_golden.py
"""
import json
import os

import mpmath as mp

mp.mp.dps = 40
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rs_special_dev.json")


def s(x):
    return mp.nstr(x, 20)


bessel = []
for L in range(9):
    xs = ["1e-8", "1e-3", "0.5", "3.0", "16.0", "29.9", "30.1", "31.9", "32.1", "40.0", "60.0"]
    if L:
        xs += [repr(4.0 * L - 0.1), repr(4.0 * L + 0.1)]
    for x in xs:
        xv = mp.mpf(float(mp.mpf(x)))
        i_ref = mp.sqrt(mp.pi / (2 * xv)) * mp.besseli(L + mp.mpf(1) / 2, xv)
        k_ref = mp.sqrt(mp.pi / (2 * xv)) * mp.besselk(L + mp.mpf(1) / 2, xv) * 2 / mp.pi
        bessel.append({"L": L, "x": float(xv), "il": s(i_ref), "kl": s(k_ref)})


def phi_num(n, Xi, xi):
    def f(t):
        r = mp.sqrt(Xi ** 2 + xi ** 2 - 2 * Xi * xi * t)
        return mp.erfc(r) / r * mp.legendre(n, t)
    return (2 * n + 1) / mp.mpf(2) * mp.quad(f, [-1, 0, 1])


PAIRS = [("1.0", "0.399"), ("1.0", "0.401"), ("0.49", "0.45"), ("0.51", "0.45"), ("0.49", "0.3"), ("0.2", "0.45"), ("0.2", "0.39"),
         ("0.45", "0.49"), ("0.45", "0.51"), ("0.3", "0.7"), ("2e-8", "1e-8"), ("1e-8", "0.3"), ("2.0", "1e-8"), ("16.0", "15.5"),
         ("40.0", "39.0"), ("16.0", "0.2"), ("0.7", "0.6")]
mp.mp.dps = 120  # Phi_8(2, 1e-8) is 1e-67 of the integrand: the quadrature needs the digits
phi = []
for n in range(9):
    for Xi, xi in PAIRS + ([("0.7", "0.0"), ("0.0", "3.0")] if n == 0 else []):
        a, b = float(mp.mpf(Xi)), float(mp.mpf(xi))
        phi.append({"n": n, "Xi": a, "xi": b, "phi": s(phi_num(n, mp.mpf(a), mp.mpf(b)))})

json.dump({"bessel": bessel, "phi": phi}, open(OUT, "w"), indent=0)
print("wrote", OUT)
