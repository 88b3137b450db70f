"""Dense NumPy restatement of the atomic program's one-electron matrices beyond the point nucleus (reference:
src/atomic/TwoDBasis.cpp:304-506 overlap / kinetic / nuclear / confinement, libhelfem/src/RadialBasis.cpp:361-476,
src/general/model_potential.cpp get_nuclear_model, src/atomic/basis.cpp:34-172 form_grid) on the same LIP elements and the
same modified Gauss-Chebyshev rule as the library: radial functions u_i = B_i(r), basis (B_i / r) Y_lm.  The Lobatto nodes and
the Gaunt coefficients are taken from the library (both are pinned by their own known-answer tests).  Everything else is
restated here, element by element, with plain loops over the Lagrange products."""
import math

import numpy as np


def chebyshev(n):
    i = np.arange(1, n + 1)
    s, c = np.sin(i * math.pi / (n + 1)), np.cos(i * math.pi / (n + 1))
    w = 16.0 / 3.0 / (n + 1) * s ** 4
    x = 1.0 - 2.0 * i / (n + 1) + 2.0 / math.pi * (1.0 + 2.0 / 3.0 * s * s) * c * s
    return x[::-1].copy(), w[::-1].copy()


def get_grid(rmax, nel, igrid=4, zexp=2.0):
    i = np.arange(nel + 1, dtype=float)
    if igrid == 1:
        b = rmax * i / nel
    elif igrid == 2:
        b = i * i * rmax / (nel * nel)
    elif igrid == 3:
        b = rmax * (i / nel) ** zexp
    elif igrid == 4:
        b = np.exp((math.log(rmax + 1) ** (1.0 / zexp) * i / nel) ** zexp) - 1.0
    else:
        raise ValueError(igrid)
    b[0], b[-1] = 0.0, rmax
    return b


def _cat(left, right):
    return np.concatenate([left, right[1:] + left[-1]])


def form_grid(nelem, Rmax, igrid=4, zexp=2.0, finitenuc=0, Rrms=0.0, nelem0=0, igrid0=4, zexp0=2.0, Z=0, Zl=0, Zr=0, Rmid=0.0,
              add_conf=False, shift_conf=0.0):
    if finitenuc in (1, 2, 3):
        rnuc = {3: Rrms, 2: math.sqrt(5.0 / 3.0) * Rrms, 1: 3 * Rrms}[finitenuc]
        if nelem0:
            bn = get_grid(rnuc, nelem0, igrid0, zexp0)
            b = _cat(_cat(bn, bn), get_grid(Rmax - rnuc, nelem, igrid, zexp))
        else:
            b = get_grid(Rmax, nelem, igrid, zexp)
    elif Zl or Zr:
        b0 = Z * Rmid / (Z + max(Zl, Zr))
        parts = []
        if Z:
            parts.append(get_grid(b0, nelem0, igrid, zexp))
        g = get_grid(Rmid - b0, nelem0, igrid, zexp)
        g = (Rmid - b0) - g[::-1]
        g[0], g[-1] = 0.0, Rmid - b0
        parts.append(g)
        parts.append(get_grid(Rmax - Rmid, nelem, igrid, zexp))
        b = parts[0]
        for p in parts[1:]:
            b = _cat(b, p)
    else:
        b = get_grid(Rmax, nelem, igrid, zexp)
    if add_conf and not np.any(b == shift_conf):
        b = np.sort(np.append(b, shift_conf))
    return b


def nuclear_model(model, Z, Rrms):
    """V(r) of the finite nuclei: 1 Gaussian, 2 uniformly charged sphere, 3 hollow sphere (Visscher and Dyall 1997)"""
    if model == 1:
        mu = math.sqrt(1.5) / Rrms
        rcut = (42.0 * np.finfo(float).eps) ** (1.0 / 6.0) / mu

        def V(r):
            if r <= rcut:
                x2 = (mu * r) ** 2
                return -Z * 2.0 / math.sqrt(math.pi) * mu * (1.0 + (-1.0 / 3.0 + (0.1 - x2 / 42.0) * x2) * x2)
            return -Z * math.erf(mu * r) / r
    elif model == 2:
        R0 = math.sqrt(5.0 / 3.0) * Rrms

        def V(r):
            return -Z / r if r >= R0 else -Z / (2.0 * R0) * (3.0 - (r / R0) ** 2)
    elif model == 3:
        def V(r):
            return -Z / r if r >= Rrms else -Z / Rrms
    elif model == 4:
        return regularized_nucleus(Z, Rrms)
    else:
        raise ValueError(model)
    return V


def regularized_nucleus(Z, a):
    """Gygi's regularized nucleus: the potential whose exact 1s state for Z = 1 is phi = exp(h)/sqrt(pi) with
    h = -r erf(a r) - b exp(-a^2 r^2), b from the normalisation of phi; V_1 = -1/2 + (h'' + h'^2)/2 + h'/r, V_Z(r) = Z^2 V_1(Z r).
    SciPy's adaptive quadrature and root finder, derivatives of h written out term by term."""
    import scipy.integrate
    import scipy.optimize

    def defect(b):
        f = lambda r: r * r * math.exp(2.0 * (-r * math.erf(a * r) - b * math.exp(-(a * r) ** 2)))  # noqa: E731
        pts = [1.0 / a, 4.0 / a]
        v = scipy.integrate.quad(f, 0.0, 8.0 / a, points=pts, epsabs=1e-17, epsrel=1e-13, limit=400)[0]
        v += scipy.integrate.quad(f, 8.0 / a, 8.0 / a + 60.0, epsabs=1e-18, epsrel=1e-13, limit=400)[0]
        return 4.0 * v - 1.0
    b = scipy.optimize.brentq(defect, -40.0, 40.0, xtol=1e-15, rtol=4 * np.finfo(float).eps)

    def V1(r):
        g = math.exp(-(a * r) ** 2)
        erf_r = math.erf(a * r) / r if a * r > 1e-2 else \
            2 * a / math.sqrt(math.pi) * sum((-1) ** k * (a * r) ** (2 * k) / (math.factorial(k) * (2 * k + 1)) for k in range(6))
        d1_r = -erf_r - 2 * a / math.sqrt(math.pi) * g + 2 * a * a * b * g
        d1 = d1_r * r
        d2 = (-4 * a / math.sqrt(math.pi) + 4 * a ** 3 / math.sqrt(math.pi) * r * r + 2 * a * a * b - 4 * a ** 4 * b * r * r) * g
        return -0.5 + 0.5 * (d2 + d1 * d1) + d1_r
    V = lambda r: Z * Z * V1(Z * r)  # noqa: E731
    V.b = b
    return V


def confinement_function(iconf, N, R, V, shift, r_c):
    """the radial function f with Vconf = int B_i B_j f dr (the polynomial form integrates (B_i/r)(B_j/r)(r - shift)^(N+2),
    i.e. f = (r - shift)^(N+2) / r^2, as RadialBasis::polynomial_confinement does)"""
    sign, r0 = (-1.0 if R < 0 else 1.0), abs(R)
    if iconf == 1:
        return lambda r: 0.0 if r < shift else sign * r0 ** (-abs(N)) * (r - shift) ** (N + 2) / (r * r)
    if iconf == 2:
        def f(r):
            if r < shift:
                return 0.0
            x = (r - shift) / r0
            return math.factorial(N) * (math.exp(x) - sum(x ** k / math.factorial(k) for k in range(N)))
        return f
    if iconf == 3:
        return lambda r: 0.0 if r < shift else V
    if iconf == 4:
        return lambda r: 0.0 if r < shift else V * math.exp(-(r_c - shift) / (r - shift)) / (r_c - r) ** N
    raise ValueError(iconf)


class DenseAtom(object):
    """nodes: Gauss-Lobatto nodes on [-1, 1]; gaunt(li, mi, L, M, lj, mj): Gaunt coefficient"""

    def __init__(self, bval, nodes, nquad, lval, mval, gaunt=None, zeroder=False):
        self.bval = np.asarray(bval, dtype=float)
        self.x0 = np.asarray(nodes, dtype=float)
        self.xq, self.wq = chebyshev(nquad)
        self.lval, self.mval = list(lval), list(mval)
        self.gaunt = gaunt
        nel, n = len(self.bval) - 1, len(self.x0)
        self.elem = []
        first = 0
        for iel in range(nel):
            keep = list(range(n))
            if iel == 0:
                keep = keep[1:]
            if iel == nel - 1 and not zeroder:
                keep = keep[:-1]
            if iel > 0:
                first = self.elem[-1][1] + len(self.elem[-1][0]) - 1  # one shared function between neighbours
            self.elem.append((keep, first))
        self.Nrad = self.elem[-1][1] + len(self.elem[-1][0])
        self.Nbf = self.Nrad * len(self.lval)

    # Lagrange products -----------------------------------------------------------------------------------------------
    def _lip(self, fi, x, skip=()):
        v = np.ones_like(x)
        for p in range(len(self.x0)):
            if p != fi and p not in skip:
                v = v * (x - self.x0[p])
        return v

    def _den(self, fi):
        return np.prod([self.x0[fi] - self.x0[p] for p in range(len(self.x0)) if p != fi])

    def _tables(self, iel):
        """r, weights, B, dB/dr and B/r at the quadrature points of element iel"""
        a, b = self.bval[iel], self.bval[iel + 1]
        sc = 0.5 * (b - a)
        r = 0.5 * (a + b) + sc * self.xq
        keep, first = self.elem[iel]
        B = np.array([self._lip(fi, self.xq) / self._den(fi) for fi in keep]).T
        dB = np.array([sum(self._lip(fi, self.xq, skip=(d,)) for d in range(len(self.x0)) if d != fi) / self._den(fi)
                       for fi in keep]).T / sc
        if iel == 0:  # B_i / r without the division: the factor (x - x_0) = r / sc left out of the product
            Br = np.array([self._lip(fi, self.xq, skip=(0,)) / self._den(fi) for fi in keep]).T / sc
        else:
            Br = B / r[:, None]
        return r, self.wq * sc, B, dB, Br, first

    def _assemble(self, block):
        M = np.zeros((self.Nrad, self.Nrad))
        for iel in range(len(self.elem)):
            m, first = block(iel)
            M[first:first + m.shape[0], first:first + m.shape[1]] += m
        return M

    def radial(self, f):
        """int B_i B_j f(r) dr"""
        def block(iel):
            r, w, B, dB, Br, first = self._tables(iel)
            fw = w * np.array([f(x) for x in r])
            return B.T @ (fw[:, None] * B), first
        return self._assemble(block)

    def radial_power(self, k):
        """int (B_i/r)(B_j/r) r^(k+2) dr"""
        def block(iel):
            r, w, B, dB, Br, first = self._tables(iel)
            return Br.T @ ((w * r ** (k + 2.0))[:, None] * Br), first
        return self._assemble(block)

    def _diag(self, rads):
        R = self.Nrad
        M = np.zeros((self.Nbf, self.Nbf))
        for a, m in enumerate(rads):
            M[a * R:(a + 1) * R, a * R:(a + 1) * R] = m
        return M

    # matrices ----------------------------------------------------------------------------------------------------------
    def overlap(self):
        return self._diag([self.radial_power(0)] * len(self.lval))

    def kinetic(self):
        def block(iel):
            r, w, B, dB, Br, first = self._tables(iel)
            return 0.5 * dB.T @ (w[:, None] * dB), first
        T0 = self._assemble(block)
        Tl = 0.5 * self.radial_power(-2)
        return self._diag([T0 + l * (l + 1) * Tl for l in self.lval])

    def nuclear_point(self, Z):
        return self._diag([-Z * self.radial_power(-1)] * len(self.lval))

    def nuclear_finite(self, model, Z, Rrms):
        return self._diag([self.radial(nuclear_model(model, Z, Rrms))] * len(self.lval))

    def confinement(self, iconf, N=0, R=0.0, V=0.0, shift=0.0):
        if iconf == 1:  # on B/r, as the reference integrates it
            sign, r0 = (-1.0 if R < 0 else 1.0), abs(R)

            def block(iel):
                r, w, B, dB, Br, first = self._tables(iel)
                f = np.where(r < shift, 0.0, np.abs(r - shift) ** (N + 2.0))
                return sign * r0 ** (-abs(N)) * Br.T @ ((w * f)[:, None] * Br), first
            return self._diag([self._assemble(block)] * len(self.lval))
        return self._diag([self.radial(confinement_function(iconf, N, R, V, shift, self.bval.max()))] * len(self.lval))

    def nuclear_offcenter(self, Zl, Zr, Rmid):
        """charges Zl at z = -Rmid and Zr at z = +Rmid: -Z_c sum_L r_<^L / r_>^(L+1) P_L(+-cos theta)"""
        Lmax = 2 * max(self.lval)
        Vaux = []
        for L in range(Lmax + 1):
            def block(iel, L=L):
                r, w, B, dB, Br, first = self._tables(iel)
                a, b = self.bval[iel], self.bval[iel + 1]
                if b <= Rmid:
                    f = r ** L / Rmid ** (L + 1)
                elif a >= Rmid:
                    f = Rmid ** L / r ** (L + 1)
                else:
                    raise ValueError("nucleus inside an element")
                return -math.sqrt(4 * math.pi / (2 * L + 1)) * B.T @ ((w * f)[:, None] * B), first
            Vaux.append(self._assemble(block))
        R = self.Nrad
        V = np.zeros((self.Nbf, self.Nbf))
        for ia, (li, mi) in enumerate(zip(self.lval, self.mval)):
            for ja, (lj, mj) in enumerate(zip(self.lval, self.mval)):
                if mi != mj:
                    continue
                for L in range(abs(li - lj), li + lj + 1):
                    c = self.gaunt(li, mi, L, 0, lj, mj)
                    if c != 0.0:
                        V[ia * R:(ia + 1) * R, ja * R:(ja + 1) * R] += c * ((-1) ** L * Zl + Zr) * Vaux[L]
        return V


def lowest(H, S, k=1):
    import scipy.linalg
    return scipy.linalg.eigh(H, S, eigvals_only=True)[:k]
