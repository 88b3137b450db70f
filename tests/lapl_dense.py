"""Dense NumPy restatement of the atomic program's DFT grid worker on the Laplacian path (reference:
src/atomic/dftgrid.cpp compute_bf :700-793 with TwoDBasis::eval_lf, update_density :51-120 / :122-229 with lapl,
eval_Fxc :499-571 / :573-667 with increment_mgga_lapl, dftgrid.h:257-281).  Point values come from the host evaluator
hfg_xc_eval.  Complex basis functions g_n(r) Theta_lm(theta) e^{i m phi} on the full (r, theta, phi) product grid, one
radial element at a time, as the reference loops; the theta derivatives of Theta_lm from numpy.polynomial.legendre (|m| <= 1).
Slow by design: small bases only."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import diatomic_tei as dt  # noqa: E402  (chebyshev rule)


def _theta_tables(hf, lval, mval, cth):
    """Theta_lm(cos theta) and d/dtheta Theta_lm at the points cth (values cross-checked against the product's theta_lm)"""
    from numpy.polynomial import legendre as L
    s = np.sqrt(1.0 - cth * cth)
    T, dT = [], []
    for l, m in zip(lval, mval):
        c = np.zeros(l + 1)
        c[l] = 1.0
        p0, p1, p2 = L.legval(cth, c), L.legval(cth, L.legder(c)), L.legval(cth, L.legder(c, 2))
        am = abs(m)
        if am == 0:
            t, dtdx = p0, p1
        elif am == 1:
            t, dtdx = -s * p1, (cth / s) * p1 - s * p2
        else:
            raise ValueError("the dense restatement covers |m| <= 1")
        N = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - am) / math.factorial(l + am))
        ref = np.array([hf.theta_lm(l, m, x) for x in cth])
        sign = 1.0 if np.dot(ref, N * t) >= 0 else -1.0
        t, dtdx = sign * N * t, sign * N * dtdx
        assert np.max(np.abs(t - ref)) < 1e-12 * max(1.0, np.max(np.abs(ref))), (l, m)
        T.append(t)
        dT.append(-s * dtdx)  # d/dtheta = -sin(theta) d/dcos(theta)
    return np.array(T), np.array(dT)


class DenseWorker(object):
    def __init__(self, hf, basis, bval, nnodes, ldft, mdft):
        self.hf = hf
        self.b = basis
        self.lval, self.mval = np.array(basis.lval), np.array(basis.mval)
        self.nel = len(bval) - 1
        self.nnodes = nnodes
        self.Nrad = basis.Nrad()
        cth, wth = dt.chebyshev(ldft)
        self.T, self.dT = _theta_tables(hf, self.lval, self.mval, cth)
        self.sth = np.sqrt(1.0 - cth * cth)
        self.wth = wth
        self.phi = 2 * math.pi * np.arange(mdft) / mdft
        self.wphi = 2 * math.pi / mdft
        self.elem = []
        for iel in range(self.nel):
            r = basis.radial_table("r", iel)
            nq = len(r)
            _, wq = dt.chebyshev(nq)
            wr = wq * 0.5 * (bval[iel + 1] - bval[iel])
            g, dg, lg = basis.radial_table("bf", iel), basis.radial_table("df", iel), basis.radial_table("lf", iel)
            first = iel * (nnodes - 1) - 1 + (1 if iel == 0 else 0)
            self.elem.append((r, wr, g, dg, lg, first))

    def _bf(self, iel):
        """basis functions of element iel on its grid points: value, gradient (r, theta, phi components), Laplacian; the
        global indices of the functions; the volume weights"""
        r, wr, g, dg, lg, first = self.elem[iel]
        nq, nf = g.shape
        A = len(self.lval)
        rr = r[:, None, None]
        st = self.sth[None, :, None]
        ph = np.exp(1j * np.outer(self.mval, self.phi))  # [a][j]
        shp = (nq, len(self.sth), len(self.phi))
        w = (wr[:, None, None] * r[:, None, None] ** 2 * self.wth[None, :, None] * self.wphi) * np.ones(shp)
        F, Fr, Ft, Fp, FL, idx = [], [], [], [], [], []
        for a in range(A):
            l, m = self.lval[a], self.mval[a]
            Ta, dTa = self.T[a][None, :, None], self.dT[a][None, :, None]
            e = ph[a][None, None, :]
            for n in range(nf):
                gn, dgn, lgn = g[:, n][:, None, None], dg[:, n][:, None, None], lg[:, n][:, None, None]
                F.append(gn * Ta * e)
                Fr.append(dgn * Ta * e)
                Ft.append(gn * dTa * e / rr)
                Fp.append(1j * m * gn * Ta * e / (rr * st))
                FL.append((lgn + 2 * dgn / rr - l * (l + 1) * gn / rr ** 2) * Ta * e)  # eval_lf
                idx.append(a * self.Nrad + first + n)
        f = lambda X: np.array([x.ravel() for x in X])  # noqa: E731  [function][point]
        return f(F), (f(Fr), f(Ft), f(Fp)), f(FL), np.array(idx), w.ravel()

    @staticmethod
    def _dens(P, F, G, FL):
        """rho, grad rho (3 components), tau (libxc), lapl of one density matrix block"""
        PF = P @ F  # P conj? P is real symmetric: sum_nu P_mu,nu phi_nu
        rho = np.real(np.sum(np.conj(F) * PF, 0))
        grad = [2 * np.real(np.sum(np.conj(F) * (P @ Gc), 0)) for Gc in G]
        kin = sum(np.real(np.sum(np.conj(Gc) * (P @ Gc), 0)) for Gc in G)
        lap = np.real(np.sum(np.conj(F) * (P @ FL), 0))
        return rho, grad, 0.5 * kin, 2.0 * (kin + lap)

    def _xc(self, funcs, nspin, rho, sigma, lapl, tau, thr):
        out = None
        for fid in funcs:
            if fid <= 0:
                continue
            o = self.hf.xc_eval(fid, rho, sigma, lapl, tau, nspin=nspin, thr=thr)
            out = o if out is None else {k: out[k] + o[k] for k in o}
        return out

    @staticmethod
    def _fock(F, G, FL, w, vrho, gvec, vtl, vl):
        """H_mu,nu = sum_p w Re[vrho phi_mu* phi_nu + gvec.(grad phi_mu* phi_nu + phi_mu* grad phi_nu)
        + vtl grad phi_mu*.grad phi_nu + vl (phi_mu* lapl phi_nu + lapl phi_mu* phi_nu)]"""
        Fc = np.conj(F)
        H = (Fc * (w * vrho)) @ F.T
        for c in range(3):
            H += (np.conj(G[c]) * (w * gvec[c])) @ F.T + (Fc * (w * gvec[c])) @ G[c].T
            H += (np.conj(G[c]) * (w * vtl)) @ G[c].T
        H += (Fc * (w * vl)) @ FL.T + (np.conj(FL) * (w * vl)) @ F.T
        return np.real(H)

    def eval_Fxc(self, x_func, c_func, P, thr=1e-12):
        N = P.shape[0]
        H = np.zeros((N, N))
        Exc = Nel = 0.0
        for iel in range(self.nel):
            F, G, FL, idx, w = self._bf(iel)
            Pe = P[np.ix_(idx, idx)]
            rho, grad, tau, lapl = self._dens(Pe, F, G, FL)
            sigma = sum(gc * gc for gc in grad)
            o = self._xc((x_func, c_func), 1, rho, sigma, lapl, tau, thr)
            Exc += np.sum(w * o["exc"] * rho)
            Nel += np.sum(w * rho)
            gvec = [2 * o["vsigma"] * gc for gc in grad]
            He = self._fock(F, G, FL, w, o["vrho"], gvec, 0.5 * o["vtau"] + 2 * o["vlapl"], o["vlapl"])
            H[np.ix_(idx, idx)] += He
        return H, Exc, Nel

    def eval_Fxc_pol(self, x_func, c_func, Pa, Pb, thr=1e-12):
        N = Pa.shape[0]
        Ha, Hb = np.zeros((N, N)), np.zeros((N, N))
        Exc = Nel = 0.0
        for iel in range(self.nel):
            F, G, FL, idx, w = self._bf(iel)
            ra, ga, ta, la = self._dens(Pa[np.ix_(idx, idx)], F, G, FL)
            rb, gb, tb, lb = self._dens(Pb[np.ix_(idx, idx)], F, G, FL)
            saa = sum(x * x for x in ga)
            sab = sum(x * y for x, y in zip(ga, gb))
            sbb = sum(y * y for y in gb)
            o = self._xc((x_func, c_func), 2, np.stack([ra, rb], 1), np.stack([saa, sab, sbb], 1), np.stack([la, lb], 1),
                         np.stack([ta, tb], 1), thr)
            rt = ra + rb
            Exc += np.sum(w * o["exc"] * rt)
            Nel += np.sum(w * rt)
            vs = o["vsigma"]
            gva = [2 * vs[:, 0] * x + vs[:, 1] * y for x, y in zip(ga, gb)]
            gvb = [2 * vs[:, 2] * y + vs[:, 1] * x for x, y in zip(ga, gb)]
            Ha[np.ix_(idx, idx)] += self._fock(F, G, FL, w, o["vrho"][:, 0], gva, 0.5 * o["vtau"][:, 0] + 2 * o["vlapl"][:, 0],
                                               o["vlapl"][:, 0])
            Hb[np.ix_(idx, idx)] += self._fock(F, G, FL, w, o["vrho"][:, 1], gvb, 0.5 * o["vtau"][:, 1] + 2 * o["vlapl"][:, 1],
                                               o["vlapl"][:, 1])
        return Ha, Hb, Exc, Nel
