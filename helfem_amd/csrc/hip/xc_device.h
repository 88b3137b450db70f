// Exchange-correlation functionals (spin-unpolarised and spin-polarised) evaluated on the GPU grid (reference: the
// libxc calls of DFTGridWorker::compute_xc, src/diatomic/dftgrid.cpp:343-458).  libxc is a
// third-party dependency of the reference that is not vendored and not present here; the energy
// densities below are the published closed forms and the derivatives vrho = d(rho exc)/d rho,
// vsigma = d(rho exc)/d sigma come from forward-mode automatic differentiation (two-component
// dual numbers), deliberately a different route from the oracle's hand-derived formulas.
#pragma once
#include <hip/hip_runtime.h>
#include "../host/xc_funcs.h"

namespace hfg {
namespace xc {

struct Dual {
  double v, dr, ds;  // value, d/d rho, d/d sigma
};

__host__ __device__ inline Dual mk(double v, double dr = 0.0, double ds = 0.0) {
  Dual d;
  d.v = v;
  d.dr = dr;
  d.ds = ds;
  return d;
}
__host__ __device__ inline Dual operator+(Dual a, Dual b) { return mk(a.v + b.v, a.dr + b.dr, a.ds + b.ds); }
__host__ __device__ inline Dual operator-(Dual a, Dual b) { return mk(a.v - b.v, a.dr - b.dr, a.ds - b.ds); }
__host__ __device__ inline Dual operator-(Dual a) { return mk(-a.v, -a.dr, -a.ds); }
__host__ __device__ inline Dual operator*(Dual a, Dual b) {
  return mk(a.v * b.v, a.dr * b.v + a.v * b.dr, a.ds * b.v + a.v * b.ds);
}
__host__ __device__ inline Dual operator/(Dual a, Dual b) {
  double inv = 1.0 / b.v;
  double q = a.v * inv;
  return mk(q, (a.dr - q * b.dr) * inv, (a.ds - q * b.ds) * inv);
}
__host__ __device__ inline Dual operator+(Dual a, double c) { return mk(a.v + c, a.dr, a.ds); }
__host__ __device__ inline Dual operator+(double c, Dual a) { return mk(a.v + c, a.dr, a.ds); }
__host__ __device__ inline Dual operator-(Dual a, double c) { return mk(a.v - c, a.dr, a.ds); }
__host__ __device__ inline Dual operator-(double c, Dual a) { return mk(c - a.v, -a.dr, -a.ds); }
__host__ __device__ inline Dual operator*(Dual a, double c) { return mk(a.v * c, a.dr * c, a.ds * c); }
__host__ __device__ inline Dual operator*(double c, Dual a) { return mk(a.v * c, a.dr * c, a.ds * c); }
__host__ __device__ inline Dual operator/(Dual a, double c) { return a * (1.0 / c); }
__host__ __device__ inline Dual operator/(double c, Dual a) { return mk(c) / a; }
__host__ __device__ inline Dual dsqrt(Dual a) {
  double s = sqrt(a.v);
  double f = 0.5 / s;
  return mk(s, a.dr * f, a.ds * f);
}
__host__ __device__ inline Dual dcbrt(Dual a) {
  double c = cbrt(a.v);
  double f = c / (3.0 * a.v);
  return mk(c, a.dr * f, a.ds * f);
}
__host__ __device__ inline Dual dlog(Dual a) { return mk(log(a.v), a.dr / a.v, a.ds / a.v); }
// log(1 + a) and exp(a) - 1 without the cancellation: at densities below ~1e-28 (reached in the far field when the
// density threshold is lowered to zero) log(1 + 1/den) of PW92 rounds to 0, exp(-ec/gamma) - 1 with it, and PBE's A = inf
__host__ __device__ inline Dual dlog1p(Dual a) { return mk(log1p(a.v), a.dr / (1.0 + a.v), a.ds / (1.0 + a.v)); }
__host__ __device__ inline Dual dexpm1(Dual a) {
  double e = exp(a.v);
  return mk(expm1(a.v), a.dr * e, a.ds * e);
}
__host__ __device__ inline Dual dexp(Dual a) {
  double e = exp(a.v);
  return mk(e, a.dr * e, a.ds * e);
}
__host__ __device__ inline Dual datan(Dual a) {
  double f = 1.0 / (1.0 + a.v * a.v);
  return mk(atan(a.v), a.dr * f, a.ds * f);
}

__host__ __device__ inline Dual derf(Dual a) {
  double f = 1.1283791670955126 * exp(-a.v * a.v);  // 2/sqrt(pi)
  return mk(erf(a.v), a.dr * f, a.ds * f);
}

#define HFG_PI 3.14159265358979323846

// energy per particle of each functional as a Dual in (rho, sigma)
// External functional parameters (libxc's xc_func_set_ext_params as the reference calls it for --x_pars / --c_pars,
// dftgrid.cpp:405-410), in libxc's order: lda_x {alpha = 1}, gga_x_pbe {kappa = 0.8040, mu = beta pi^2/3},
// gga_c_pbe {beta = 0.06672455060314922, gamma = (1 - ln 2)/pi^2, BB = 1}.  One constant-memory copy per translation
// unit (this header is included by fock.hip only); set_xc_params() there fills it before the grid kernels are launched.
// x_omega: the range-separation constant of the short-range GGA exchange primitives (gga_x_ityh, gga_x_sfat and their PBE
// forms, libxc's {_omega}); negative: the functional's own default.
struct XCPar {
  double x_alpha, x_kappa, x_mu, c_beta, c_gamma, c_BB, x_omega;
};
#define HFG_XCPAR_DEFAULTS \
  { 1.0, 0.8040, 0.06672455060314922 * HFG_PI * HFG_PI / 3.0, 0.06672455060314922, (1.0 - 0.6931471805599453) / (HFG_PI * HFG_PI), 1.0, -1.0 }
static __constant__ XCPar c_xcpar = HFG_XCPAR_DEFAULTS;
// the parameters as the point code reads them: the constant-memory copy on the device; in a host build of the same code
// (hfg_xc_eval, hfg_xc_eval_ext) a per-thread copy that holds the defaults unless hfg_xc_eval_ext has set it for its call
inline XCPar &host_xcpar() {
  static thread_local XCPar h = HFG_XCPAR_DEFAULTS;
  return h;
}
__host__ __device__ inline const XCPar &xcpar() {
#if defined(__HIP_DEVICE_COMPILE__)
  return c_xcpar;
#else
  return host_xcpar();
#endif
}

__host__ __device__ inline Dual eps_lda_x(Dual rho) { return (-0.75 * cbrt(3.0 / HFG_PI)) * dcbrt(rho); }

// Short-range LDA exchange of the range-separated hybrids: eps_x^sr = eps_x^LDA(rho) F(a), a = omega/(2 k_F).
// erfc(omega r)/r (libxc lda_x_erf; Toulouse, Savin, Flad, Int. J. Quantum Chem. 100, 1047 (2004), eq 18-19):
//   F = 1 - (8/3) a [sqrt(pi) erf(1/(2a)) + (2a - 4a^3) exp(-1/(4a^2)) - 3a + 4a^3]
// exp(-omega r)/r (libxc lda_x_yukawa; Savin, Flad, Int. J. Quantum Chem. 56, 327 (1995)):
//   F = 1 - (8/3) a [atan(1/a) + a/4 - (a/4)(a^2 + 3) ln(1 + 1/a^2)]
// Both closed forms cancel like a^4 for large a (low density); there the expansions in 1/a^2 are summed:
//   erf: sum_k (-1)^{k+1} 2/(4^k k! (2k+1)(k+1)(k+2)) a^{-2k},  Yukawa: sum_k (-1)^{k+1} 2/((2k+1)(k+1)(k+2)) a^{-2k}.
__host__ __device__ inline Dual att_erf(Dual a) {
  if (a.v > 0.75) {
    Dual u = 1.0 / (a * a), t = mk(1.0), sum = mk(0.0);
    for (int k = 1; k <= 24; k++) {
      t = t * u * (-0.25 / k);
      sum = sum - t * (2.0 / ((2.0 * k + 1.0) * (k + 1.0) * (k + 2.0)));
    }
    return sum;
  }
  Dual a2 = a * a;
  Dual e = dexp(-0.25 / a2);
  return 1.0 - (8.0 / 3.0) * a * (1.7724538509055159 * derf(0.5 / a) + (2.0 * a - 4.0 * a2 * a) * e - 3.0 * a + 4.0 * a2 * a);
}
__host__ __device__ inline Dual att_yukawa(Dual a) {
  if (a.v > 2.0) {
    Dual u = 1.0 / (a * a), t = mk(-1.0), sum = mk(0.0);
    for (int k = 1; k <= 40; k++) {
      t = -1.0 * t * u;
      sum = sum + t * (2.0 / ((2.0 * k + 1.0) * (k + 1.0) * (k + 2.0)));
    }
    return sum;
  }
  Dual a2 = a * a;
  return 1.0 - (8.0 / 3.0) * a * (datan(1.0 / a) + 0.25 * a - 0.25 * a * (a2 + 3.0) * dlog(1.0 + 1.0 / a2));
}
/// kind 1: Yukawa, 2: erfc
__host__ __device__ inline Dual eps_lda_x_sr(Dual rho, double omega, int kind) {
  Dual kf = dcbrt((3.0 * HFG_PI * HFG_PI) * rho);
  Dual a = (0.5 * omega) / kf;
  return eps_lda_x(rho) * (kind == 1 ? att_yukawa(a) : att_erf(a));
}
// hyb_lda_xc_cam_lda0 (libxc id 178; Mosquera, Borca, Ratner, Schatz, J. Phys. Chem. A 120, 1605 (2016)): omega = 1/3,
// exact exchange alpha = 1/2 over the full range plus beta = -1/4 of the short range (1/4 at short, 1/2 at long range);
// DFT part (1 - alpha) lda_x - beta lda_x_erf + lda_c_pw_mod
#define HFG_CAM_LDA0_OMEGA (1.0 / 3.0)
__host__ __device__ inline Dual eps_cam_lda0_x(Dual rho) {
  return 0.5 * eps_lda_x(rho) + 0.25 * eps_lda_x_sr(rho, HFG_CAM_LDA0_OMEGA, 2);
}

__host__ __device__ inline Dual eps_vwn_fit(Dual rho, double A, double b, double c, double x0) {
  Dual rs = dcbrt(3.0 / (4.0 * HFG_PI) / rho);
  Dual x = dsqrt(rs);
  Dual X = x * x + b * x + c;
  const double X0 = x0 * x0 + b * x0 + c;
  const double Q = sqrt(4.0 * c - b * b);
  Dual at = datan(Q / (2.0 * x + b));
  Dual xm = x - x0;
  return A * (dlog(x * x / X) + (2.0 * b / Q) * at -
              (b * x0 / X0) * (dlog(xm * xm / X) + (2.0 * (b + 2.0 * x0) / Q) * at));
}
// VWN5 (libxc lda_c_vwn = 7: fit to the Ceperley-Alder data) and the RPA fit of the same paper (lda_c_vwn_rpa = 8, the
// "VWN" inside B3LYP as libxc and Gaussian define it); Vosko, Wilk, Nusair, Can. J. Phys. 58, 1200 (1980), paramagnetic sets
__host__ __device__ inline Dual eps_lda_c_vwn(Dual rho) { return eps_vwn_fit(rho, 0.0310907, 3.72744, 12.9352, -0.10498); }
__host__ __device__ inline Dual eps_lda_c_vwn_rpa(Dual rho) { return eps_vwn_fit(rho, 0.0310907, 13.0720, 42.7198, -0.409286); }

// Becke 88 exchange (libxc gga_x_b88 = 106; Becke, Phys. Rev. A 38, 3098 (1988)), per spin channel s:
//   e_s = -Cx rho_s^{4/3} - beta rho_s^{4/3} x^2 / (1 + 6 beta x asinh x),  x = |grad rho_s| / rho_s^{4/3},  beta = 0.0042
// written in t = x^2: x asinh x is smooth in t (no square-root singularity where the gradient vanishes)
__host__ __device__ inline Dual d_x_asinh_x(Dual t) {
  const double sq = sqrt(t.v), as = asinh(sq);
  const double df = (sq > 1e-8 ? as / (2.0 * sq) : 0.5) + 0.5 / sqrt(1.0 + t.v);
  return mk(sq * as, t.dr * df, t.ds * df);
}
__host__ __device__ inline Dual eps_gga_x_b88(Dual rho, Dual sigma) {
  const double beta = 0.0042, Cx = 0.9305257363491000;  // (3/2) (3/(4 pi))^{1/3}
  Dual rs = 0.5 * rho;  // one spin channel of the unpolarised density, gradient invariant sigma/4
  Dual r43 = rs * dcbrt(rs);
  Dual t = (0.25 * sigma) / (r43 * r43);
  Dual es = (-1.0 * r43) * (Cx + beta * t / (1.0 + (6.0 * beta) * d_x_asinh_x(t)));
  return 2.0 * es / rho;
}

// Lee-Yang-Parr correlation (libxc gga_c_lyp = 131; Lee, Yang, Parr, Phys. Rev. B 37, 785 (1988)) in the gradient-only
// form of Miehlich, Savin, Stoll, Preuss, Chem. Phys. Lett. 157, 200 (1989).  Closed shell (their eq 2 at rho_a = rho_b):
//   E = -a rho/(1 + d rho^{-1/3}) - a b omega [C_F rho^{14/3} - rho^2 sigma (1/24 + 7 delta/72)],
//   omega = exp(-c rho^{-1/3}) rho^{-11/3} / (1 + d rho^{-1/3}),  delta = c rho^{-1/3} + d rho^{-1/3}/(1 + d rho^{-1/3})
#define HFG_LYP_A 0.04918
#define HFG_LYP_B 0.132
#define HFG_LYP_C 0.2533
#define HFG_LYP_D 0.349
__host__ __device__ inline Dual eps_gga_c_lyp(Dual rho, Dual sigma) {
  const double CF = 0.3 * 9.570780000627305;  // (3/10) (3 pi^2)^{2/3}
  Dual rm13 = 1.0 / dcbrt(rho);
  Dual den = 1.0 + HFG_LYP_D * rm13;
  Dual delta = HFG_LYP_C * rm13 + HFG_LYP_D * rm13 / den;
  Dual rm23 = rm13 * rm13;
  Dual rm83 = rm23 * rm23 * rm23 * rm23;
  return (-HFG_LYP_A) / den -
         (HFG_LYP_A * HFG_LYP_B) * dexp(-HFG_LYP_C * rm13) / den * (CF - rm83 * sigma * (1.0 / 24.0 + (7.0 / 72.0) * delta));
}
// hyb_gga_xc_b3lyp (libxc 402; Stephens, Devlin, Chabalowski, Frisch, J. Phys. Chem. 98, 11623 (1994)), DFT part:
// 0.08 lda_x + 0.72 gga_x_b88 + 0.19 lda_c_vwn_rpa + 0.81 gga_c_lyp; 0.20 exact exchange
__host__ __device__ inline Dual eps_b3lyp(Dual r, Dual s) {
  return 0.08 * eps_lda_x(r) + 0.72 * eps_gga_x_b88(r, s) + 0.19 * eps_lda_c_vwn_rpa(r) + 0.81 * eps_gga_c_lyp(r, s);
}

__host__ __device__ inline Dual eps_pw92(Dual rs, bool mod) {
  const double a = mod ? 0.0310907 : 0.031091;  // libxc lda_c_pw.c: par_pw / par_pw_mod
  const double a1 = 0.21370, b1 = 7.5957, b2 = 3.5876, b3 = 1.6382, b4 = 0.49294;
  Dual srs = dsqrt(rs);
  Dual den = (2.0 * a) * (b1 * srs + b2 * rs + b3 * rs * srs + b4 * rs * rs);
  return (-2.0 * a) * (1.0 + a1 * rs) * dlog1p(1.0 / den);
}

__host__ __device__ inline Dual eps_lda_c_pw(Dual rho) {
  return eps_pw92(dcbrt(3.0 / (4.0 * HFG_PI) / rho), false);
}

// PBE exchange with explicit (kappa, mu): gga_x_pbe (101) passes the external parameters of xcpar(), gga_x_pbe_r (revPBE,
// 102; Zhang, Yang, PRL 80, 890 (1998)) kappa = 1.245 with PBE's mu, gga_x_pbe_sol (116; Perdew et al., PRL 100, 136406
// (2008)) kappa = 0.804, mu = 10/81
#define HFG_PBE_MU (0.06672455060314922 * HFG_PI * HFG_PI / 3.0)
#define HFG_PBE_GAMMA ((1.0 - 0.6931471805599453) / (HFG_PI * HFG_PI))
__host__ __device__ inline Dual eps_gga_x_pbe(Dual rho, Dual sigma, double kappa, double mu) {
  Dual exu = eps_lda_x(rho);
  Dual kf = dcbrt((3.0 * HFG_PI * HFG_PI) * rho);
  Dual s2 = sigma / (4.0 * kf * kf * rho * rho);
  Dual Fx = 1.0 + kappa - kappa / (1.0 + (mu / kappa) * s2);
  return exu * Fx;
}

// PBE correlation with explicit (beta, gamma, BB): gga_c_pbe (130) passes xcpar(), gga_c_pbe_sol (133) beta = 0.046
__host__ __device__ inline Dual eps_gga_c_pbe(Dual rho, Dual sigma, double beta, double gamma, double BB) {
  const double B = beta / gamma;
  Dual rs = dcbrt(3.0 / (4.0 * HFG_PI) / rho);
  Dual ec = eps_pw92(rs, true);
  Dual kf = dcbrt((3.0 * HFG_PI * HFG_PI) * rho);
  Dual ks2 = (4.0 / HFG_PI) * kf;
  Dual t2 = sigma / (4.0 * ks2 * rho * rho);
  Dual Aa = B / dexpm1(-ec / gamma);
  Dual At2 = Aa * t2;
  // libxc: f1 = t^2 + BB A t^4, H = gamma log(1 + (beta/gamma) f1 / (1 + A f1)); BB = 1 is PBE
  Dual f1 = t2 * (1.0 + BB * At2);
  Dual H = gamma * dlog1p(B * f1 / (1.0 + Aa * f1));
  return ec + H;
}

// The id predicates of the point code and of the launch plan, generated from the rows of host/xc_funcs.h (the columns are
// explained there); an id that is not in the list answers false everywhere.
#define HFG_XC_PREDICATE(fn)                                                                                  \
  __host__ __device__ inline bool fn(int id) {                                                                \
    switch (id) {                                                                                             \
      HELFEM_XC_FUNCS(HFG_XC_CASE_##fn)                                                                       \
      default: return false;                                                                                  \
    }                                                                                                         \
  }
#define HFG_XC_CASE_is_supported(id_, ...) case id_: return true;
#define HFG_XC_CASE_is_gga(id_, name, role, grad, ...) case id_: return grad;
#define HFG_XC_CASE_is_mgga(id_, name, role, grad, tau, lapl, ...) case id_: return (tau) && !(lapl);
#define HFG_XC_CASE_is_mgga_lapl(id_, name, role, grad, tau, lapl, ...) case id_: return lapl;
#define HFG_XC_CASE_is_ext(id_, name, role, grad, tau, lapl, ext, ...) case id_: return (ext) != 0;
#define HFG_XC_CASE_is_rsgga_x(id_, name, role, grad, tau, lapl, ext, ...) case id_: return (ext) == 2;
#define HFG_XC_CASE_is_rsgga_hyb(id_, name, role, grad, tau, lapl, ext, ...) case id_: return (ext) == 3;
#define HFG_XC_CASE_is_exchange(id_, name, role, grad, tau, lapl, ext, skip_dead, ...) case id_: return skip_dead;
HFG_XC_PREDICATE(is_supported)
HFG_XC_PREDICATE(is_gga)        /// needs the gradient (the meta-GGAs included)
HFG_XC_PREDICATE(is_mgga)       /// tau-dependent without the Laplacian: eval_add_mgga, or eval_add_ext for SCAN's ids
HFG_XC_PREDICATE(is_mgga_lapl)  /// Laplacian-dependent (tau as well): eval_add_mgga_lapl
HFG_XC_PREDICATE(is_ext)        /// evaluated by eval_add_ext / eval_add_ext_pol alone
HFG_XC_PREDICATE(is_rsgga_x)    /// short-range GGA exchange primitive
HFG_XC_PREDICATE(is_rsgga_hyb)  /// range-separated GGA hybrid
HFG_XC_PREDICATE(is_exchange)   /// the skip_dead column: left out as a whole where a spin channel is below the threshold

/// adds functional id's exc (per particle), vrho, vsigma at one point; rho >= threshold assumed.
/// live: the density of one spin channel, rho/2, reaches the threshold.  Exchange is a sum over the spin channels and
/// libxc (>= 5) leaves a channel below the threshold out of it, in the unpolarised evaluation too — which is what makes
/// the restricted and the unrestricted build agree on a closed shell.
__host__ __device__ inline void eval_add(int id, double rho, double sigma, bool live, double &exc, double &vrho,
                                         double &vsigma) {
  Dual r = mk(rho, 1.0, 0.0), s = mk(sigma, 0.0, 1.0);
  Dual e;
  if (!live) {
    if (is_exchange(id)) return;
    if (id == 178) id = 13;   // the hybrids keep their correlation part
    if (id == 406) id = 130;
    if (id == 402) id = -402;  // 0.19 lda_c_vwn_rpa + 0.81 gga_c_lyp
  }
  switch (id) {
    case 1: e = xcpar().x_alpha * eps_lda_x(r); break;
    case 7: e = eps_lda_c_vwn(r); break;
    case 12: e = eps_lda_c_pw(r); break;
    case 13: e = eps_pw92(dcbrt(3.0 / (4.0 * HFG_PI) / r), true); break;  // lda_c_pw_mod
    case 546: e = eps_lda_x_sr(r, 0.3, 2); break;                          // lda_x_erf, libxc default omega
    case 641: e = eps_lda_x_sr(r, 0.3, 1); break;                          // lda_x_yukawa, libxc default omega
    case 178: e = eps_cam_lda0_x(r) + eps_pw92(dcbrt(3.0 / (4.0 * HFG_PI) / r), true); break;  // hyb_lda_xc_cam_lda0, DFT part
    case 101: e = eps_gga_x_pbe(r, s, xcpar().x_kappa, xcpar().x_mu); break;
    case 130: e = eps_gga_c_pbe(r, s, xcpar().c_beta, xcpar().c_gamma, xcpar().c_BB); break;
    case 406:  // hyb_gga_xc_pbeh (PBE0), DFT part
      e = 0.75 * eps_gga_x_pbe(r, s, xcpar().x_kappa, xcpar().x_mu) + eps_gga_c_pbe(r, s, xcpar().c_beta, xcpar().c_gamma, xcpar().c_BB);
      break;  // hyb_gga_xc_pbeh (PBE0), DFT part
    case 8: e = eps_lda_c_vwn_rpa(r); break;
    case 106: e = eps_gga_x_b88(r, s); break;
    case 131: e = eps_gga_c_lyp(r, s); break;
    case 402: e = eps_b3lyp(r, s); break;
    case -402: e = 0.19 * eps_lda_c_vwn_rpa(r) + 0.81 * eps_gga_c_lyp(r, s); break;
    default: return;
  }
  Dual en = r * e;  // energy per volume
  exc += e.v;
  vrho += en.dr;
  vsigma += en.ds;
}

// ---------------------------------------------------------------------------------------------------------
// Spin-polarised evaluation (xc_*_exc_vxc with XC_POLARIZED; dftgrid.cpp:343-458 with rho 2 x N, sigma 3 x N).
// Exchange: spin scaling E_x[ra,rb] = (E_x[2ra] + E_x[2rb])/2 through the two-component duals above.
// Correlation: three-component duals in (rho_a, rho_b, sigma_total).
// ---------------------------------------------------------------------------------------------------------
struct T3 {
  double v, a, b, s;
};
__host__ __device__ inline T3 t3(double v, double a = 0.0, double b = 0.0, double s = 0.0) {
  T3 r;
  r.v = v;
  r.a = a;
  r.b = b;
  r.s = s;
  return r;
}
__host__ __device__ inline T3 t3f(T3 x, double f, double df) { return t3(f, df * x.a, df * x.b, df * x.s); }
__host__ __device__ inline T3 operator+(T3 x, T3 y) { return t3(x.v + y.v, x.a + y.a, x.b + y.b, x.s + y.s); }
__host__ __device__ inline T3 operator-(T3 x, T3 y) { return t3(x.v - y.v, x.a - y.a, x.b - y.b, x.s - y.s); }
__host__ __device__ inline T3 operator-(T3 x) { return t3(-x.v, -x.a, -x.b, -x.s); }
__host__ __device__ inline T3 operator*(T3 x, T3 y) {
  return t3(x.v * y.v, x.a * y.v + x.v * y.a, x.b * y.v + x.v * y.b, x.s * y.v + x.v * y.s);
}
__host__ __device__ inline T3 operator/(T3 x, T3 y) {
  double inv = 1.0 / y.v, q = x.v * inv;
  return t3(q, (x.a - q * y.a) * inv, (x.b - q * y.b) * inv, (x.s - q * y.s) * inv);
}
__host__ __device__ inline T3 operator+(T3 x, double c) { return t3(x.v + c, x.a, x.b, x.s); }
__host__ __device__ inline T3 operator+(double c, T3 x) { return t3(x.v + c, x.a, x.b, x.s); }
__host__ __device__ inline T3 operator-(T3 x, double c) { return t3(x.v - c, x.a, x.b, x.s); }
__host__ __device__ inline T3 operator-(double c, T3 x) { return t3(c - x.v, -x.a, -x.b, -x.s); }
__host__ __device__ inline T3 operator*(T3 x, double c) { return t3(x.v * c, x.a * c, x.b * c, x.s * c); }
__host__ __device__ inline T3 operator*(double c, T3 x) { return t3(x.v * c, x.a * c, x.b * c, x.s * c); }
__host__ __device__ inline T3 operator/(T3 x, double c) { return x * (1.0 / c); }
__host__ __device__ inline T3 operator/(double c, T3 x) { return t3(c) / x; }
__host__ __device__ inline T3 tsqrt(T3 x) {
  double r = sqrt(x.v);
  return t3f(x, r, 0.5 / r);
}
__host__ __device__ inline T3 tcbrt(T3 x) {
  double c = cbrt(x.v);
  return t3f(x, c, c / (3.0 * x.v));
}
__host__ __device__ inline T3 tlog(T3 x) { return t3f(x, log(x.v), 1.0 / x.v); }
__host__ __device__ inline T3 tlog1p(T3 x) { return t3f(x, log1p(x.v), 1.0 / (1.0 + x.v)); }
__host__ __device__ inline T3 texpm1(T3 x) { return t3f(x, expm1(x.v), exp(x.v)); }
__host__ __device__ inline T3 texp(T3 x) {
  double e = exp(x.v);
  return t3f(x, e, e);
}
__host__ __device__ inline T3 tatan(T3 x) { return t3f(x, atan(x.v), 1.0 / (1.0 + x.v * x.v)); }
__host__ __device__ inline T3 tpow43(T3 x) {
  double c = cbrt(x.v);
  return t3f(x, x.v * c, (4.0 / 3.0) * c);
}
__host__ __device__ inline T3 tpow23(T3 x) {
  double c = cbrt(x.v);
  return t3f(x, c * c, 2.0 / (3.0 * c));
}

// ---- seven-slot duals: derivatives with respect to (rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb, tau_a, tau_b), for
// the spin-polarised meta-GGA correlation; the correlation building blocks below are templates over the dual type ----
struct T7 {
  double v, d[7];
};
__host__ __device__ inline T7 t7(double v) {
  T7 r;
  r.v = v;
#pragma unroll
  for (int k = 0; k < 7; k++) r.d[k] = 0.0;
  return r;
}
__host__ __device__ inline T7 t7var(double v, int k) {
  T7 r = t7(v);
  r.d[k] = 1.0;
  return r;
}
__host__ __device__ inline T7 t7f(T7 x, double f, double df) {
  T7 r;
  r.v = f;
#pragma unroll
  for (int k = 0; k < 7; k++) r.d[k] = df * x.d[k];
  return r;
}
__host__ __device__ inline T7 operator+(T7 x, T7 y) {
  T7 r;
  r.v = x.v + y.v;
#pragma unroll
  for (int k = 0; k < 7; k++) r.d[k] = x.d[k] + y.d[k];
  return r;
}
__host__ __device__ inline T7 operator-(T7 x, T7 y) {
  T7 r;
  r.v = x.v - y.v;
#pragma unroll
  for (int k = 0; k < 7; k++) r.d[k] = x.d[k] - y.d[k];
  return r;
}
__host__ __device__ inline T7 operator-(T7 x) { return t7f(x, -x.v, -1.0); }
__host__ __device__ inline T7 operator*(T7 x, T7 y) {
  T7 r;
  r.v = x.v * y.v;
#pragma unroll
  for (int k = 0; k < 7; k++) r.d[k] = x.d[k] * y.v + x.v * y.d[k];
  return r;
}
__host__ __device__ inline T7 operator/(T7 x, T7 y) {
  const double inv = 1.0 / y.v, q = x.v * inv;
  T7 r;
  r.v = q;
#pragma unroll
  for (int k = 0; k < 7; k++) r.d[k] = (x.d[k] - q * y.d[k]) * inv;
  return r;
}
__host__ __device__ inline T7 operator+(T7 x, double c) { x.v += c; return x; }
__host__ __device__ inline T7 operator+(double c, T7 x) { x.v += c; return x; }
__host__ __device__ inline T7 operator-(T7 x, double c) { x.v -= c; return x; }
__host__ __device__ inline T7 operator-(double c, T7 x) { return t7f(x, c - x.v, -1.0); }
__host__ __device__ inline T7 operator*(T7 x, double c) { return t7f(x, x.v * c, c); }
__host__ __device__ inline T7 operator*(double c, T7 x) { return t7f(x, x.v * c, c); }
__host__ __device__ inline T7 operator/(T7 x, double c) { return x * (1.0 / c); }
__host__ __device__ inline T7 operator/(double c, T7 x) { return t7f(x, c / x.v, -c / (x.v * x.v)); }
__host__ __device__ inline T7 tsqrt(T7 x) {
  double r = sqrt(x.v);
  return t7f(x, r, 0.5 / r);
}
__host__ __device__ inline T7 tcbrt(T7 x) {
  double c = cbrt(x.v);
  return t7f(x, c, c / (3.0 * x.v));
}
__host__ __device__ inline T7 tlog(T7 x) { return t7f(x, log(x.v), 1.0 / x.v); }
__host__ __device__ inline T7 tlog1p(T7 x) { return t7f(x, log1p(x.v), 1.0 / (1.0 + x.v)); }
__host__ __device__ inline T7 texpm1(T7 x) { return t7f(x, expm1(x.v), exp(x.v)); }
__host__ __device__ inline T7 texp(T7 x) {
  double e = exp(x.v);
  return t7f(x, e, e);
}
__host__ __device__ inline T7 tpow43(T7 x) {
  double c = cbrt(x.v);
  return t7f(x, x.v * c, (4.0 / 3.0) * c);
}
__host__ __device__ inline T7 tpow23(T7 x) {
  double c = cbrt(x.v);
  return t7f(x, c * c, 2.0 / (3.0 * c));
}
__host__ __device__ inline T7 tmaxv(T7 x, T7 y) { return (x.v >= y.v) ? x : y; }

template <class T>
__host__ __device__ inline T pol_fzeta(T z) {
  return (tpow43(1.0 + z) + tpow43(1.0 - z) - 2.0) / (2.0 * 1.2599210498948732 - 2.0);
}
__host__ __device__ inline T3 pol_vwn_fit(T3 x, double A, double b, double c, double x0) {
  T3 X = x * x + b * x + c;
  const double X0 = x0 * x0 + b * x0 + c, Q = sqrt(4.0 * c - b * b);
  T3 at = tatan(Q / (2.0 * x + b));
  T3 xm = x - x0;
  return A * (tlog(x * x / X) + (2.0 * b / Q) * at - (b * x0 / X0) * (tlog(xm * xm / X) + (2.0 * (b + 2.0 * x0) / Q) * at));
}
__host__ __device__ inline T3 pol_eps_vwn(T3 rs, T3 z) {
  T3 x = tsqrt(rs);
  T3 eP = pol_vwn_fit(x, 0.0310907, 3.72744, 12.9352, -0.10498);
  T3 eF = pol_vwn_fit(x, 0.01554535, 7.06042, 18.0578, -0.32500);
  T3 al = pol_vwn_fit(x, -1.0 / (6.0 * HFG_PI * HFG_PI), 1.13107, 13.0045, -0.0047584);
  const double fpp = 4.0 / (9.0 * (1.2599210498948732 - 1.0));
  T3 f = pol_fzeta(z), z2 = z * z;
  T3 z4 = z2 * z2;
  return eP + al * f * (1.0 - z4) / fpp + (eF - eP) * f * z4;
}
template <class T>
__host__ __device__ inline T pol_pw_G(T rs, double A, double a1, double b1, double b2, double b3, double b4) {
  T s = tsqrt(rs);
  T den = (2.0 * A) * (b1 * s + b2 * rs + b3 * rs * s + b4 * rs * rs);
  return (-2.0 * A) * (1.0 + a1 * rs) * tlog1p(1.0 / den);
}
template <class T>
__host__ __device__ inline T pol_eps_pw(T rs, T z, bool mod) {
  T e0 = pol_pw_G(rs, mod ? 0.0310907 : 0.031091, 0.21370, 7.5957, 3.5876, 1.6382, 0.49294);
  T e1 = pol_pw_G(rs, mod ? 0.01554535 : 0.015545, 0.20548, 14.1189, 6.1977, 3.3662, 0.62517);
  T mac = pol_pw_G(rs, mod ? 0.0168869 : 0.016887, 0.11125, 10.357, 3.6231, 0.88026, 0.49671);
  const double fz20 = mod ? 1.709920934161365617563962776245 : 1.709921;
  T f = pol_fzeta(z), z2 = z * z;
  T z4 = z2 * z2;
  return e0 - mac * f * (1.0 - z4) / fz20 + (e1 - e0) * f * z4;
}
template <class T>
__host__ __device__ inline T pol_eps_pbe_c(T n, T rs, T z, T sig, double beta, double gamma, double BB) {
  // the stand-alone gga_c_pbe passes the external parameters, gga_c_pbe_sol beta = 0.046; TPSS's inner PBE the published
  // constants
  const double B = beta / gamma;
  T ec = pol_eps_pw(rs, z, true);
  T phi = 0.5 * (tpow23(1.0 + z) + tpow23(1.0 - z));
  T phi3 = phi * phi * phi;
  T kf = tcbrt((3.0 * HFG_PI * HFG_PI) * n);
  T ks2 = (4.0 / HFG_PI) * kf;
  T t2 = sig / (4.0 * phi * phi * ks2 * n * n);
  T Aa = B / texpm1(-ec / (gamma * phi3));
  T At2 = Aa * t2;
  T f1 = t2 * (1.0 + BB * At2);
  return ec + gamma * phi3 * tlog1p(B * f1 / (1.0 + Aa * f1));
}

// lda_c_vwn_rpa, spin-polarised: libxc interpolates the paramagnetic and the ferromagnetic RPA fits with f(zeta) alone
__host__ __device__ inline T3 pol_eps_vwn_rpa(T3 rs, T3 z) {
  T3 x = tsqrt(rs);
  T3 eP = pol_vwn_fit(x, 0.0310907, 13.0720, 42.7198, -0.409286);
  T3 eF = pol_vwn_fit(x, 0.01554535, 20.1231, 101.578, -0.743294);
  return eP + (eF - eP) * pol_fzeta(z);
}
// gga_c_lyp for a spin-polarised density, Miehlich et al. eq 2 (energy per particle):
//   n e = -a 4 ra rb / (n (1 + d n^{-1/3}))
//         - a b omega { ra rb [2^{11/3} C_F (ra^{8/3} + rb^{8/3}) + (47/18 - 7 delta/18) s_t - (5/2 - delta/18)(s_aa + s_bb)
//                              - (delta - 11)/9 (ra s_aa + rb s_bb)/n] - (2/3) n^2 s_t + ((2/3) n^2 - ra^2) s_bb + ((2/3) n^2 - rb^2) s_aa }
// (vanishes identically for a fully polarised density: no self-correlation)
template <class T>
__host__ __device__ inline T pol_eps_lyp(T ra, T rb, T saa, T sab, T sbb) {
  const double CF = 0.3 * 9.570780000627305, c11 = 12.699208415745595;  // 2^{11/3}
  T n = ra + rb;
  T rm13 = 1.0 / tcbrt(n);
  T den = 1.0 + HFG_LYP_D * rm13;
  T delta = HFG_LYP_C * rm13 + HFG_LYP_D * rm13 / den;
  T rm23 = rm13 * rm13;
  T rm113 = rm23 * rm23 * rm23 * rm23 * rm23 * rm13;  // n^{-11/3}
  T omega = texp((-HFG_LYP_C) * rm13) / den * rm113;
  T st = saa + 2.0 * sab + sbb;
  T rab = ra * rb, n2 = n * n;
  T ra83 = ra * ra * tpow23(ra), rb83 = rb * rb * tpow23(rb);
  T t1 = (c11 * CF) * (ra83 + rb83) + (47.0 / 18.0 - (7.0 / 18.0) * delta) * st - (2.5 - delta / 18.0) * (saa + sbb) -
         ((delta - 11.0) / 9.0) * (ra * saa + rb * sbb) / n;
  // the last three terms of the published brace, -(2/3) n^2 s_t + ((2/3) n^2 - ra^2) s_bb + ((2/3) n^2 - rb^2) s_aa, collapse to
  // -(4/3) n^2 s_ab - ra^2 s_bb - rb^2 s_aa: summed as published they cancel to 1e-8 of their size in strongly polarised
  // regions (the checker keeps the published arrangement)
  T E = (-4.0 * HFG_LYP_A) * rab / (n * den) -
        (HFG_LYP_A * HFG_LYP_B) * omega * (rab * t1 - (4.0 / 3.0) * n2 * sab - ra * ra * sbb - rb * rb * saa);
  (void)st;
  return E / n;
}

/// adds functional id's exc (per particle of ra+rb), vrho[2], vsigma[3] (aa, ab, bb); ra + rb >= threshold assumed,
/// ra, rb already raised to the threshold; live_a, live_b: the channel's own density reached the threshold (a channel
/// below it is left out of the exchange sum, as libxc >= 5 does)
__host__ __device__ inline void eval_add_pol_basic(int id, double ra, double rb, double saa, double sab, double sbb, bool live_a,
                                             bool live_b, double &exc, double &va, double &vb, double &vsaa, double &vsab,
                                             double &vsbb) {
  const double rt = ra + rb;
  if (id == 131) {  // gga_c_lyp: depends on the three gradient invariants separately
    T7 A = t7var(ra, 0), B = t7var(rb, 1), Saa = t7var(saa, 2), Sab = t7var(sab, 3), Sbb = t7var(sbb, 4);
    T7 e = pol_eps_lyp(A, B, Saa, Sab, Sbb);
    T7 en = (A + B) * e;
    exc += e.v;
    va += en.d[0];
    vb += en.d[1];
    vsaa += en.d[2];
    vsab += en.d[3];
    vsbb += en.d[4];
    return;
  }
  if (id == 1 || id == 101 || id == 546 || id == 641 || id == -178 || id == 106) {
    Dual a = mk(2.0 * ra, 1.0, 0.0), b = mk(2.0 * rb, 1.0, 0.0);
    Dual sa = mk(4.0 * saa, 0.0, 1.0), sb = mk(4.0 * sbb, 0.0, 1.0);
    Dual ea, eb;
    switch (id) {
      case 1: ea = xcpar().x_alpha * eps_lda_x(a); eb = xcpar().x_alpha * eps_lda_x(b); break;
      case 546: ea = eps_lda_x_sr(a, 0.3, 2); eb = eps_lda_x_sr(b, 0.3, 2); break;
      case 641: ea = eps_lda_x_sr(a, 0.3, 1); eb = eps_lda_x_sr(b, 0.3, 1); break;
      case -178: ea = eps_cam_lda0_x(a); eb = eps_cam_lda0_x(b); break;
      case 106: ea = eps_gga_x_b88(a, sa); eb = eps_gga_x_b88(b, sb); break;
      default: ea = eps_gga_x_pbe(a, sa, xcpar().x_kappa, xcpar().x_mu); eb = eps_gga_x_pbe(b, sb, xcpar().x_kappa, xcpar().x_mu); break;
    }
    Dual na = a * ea, nb = b * eb;  // energy per volume of the doubled densities
    if (!live_a) na = mk(0.0, 0.0, 0.0);
    if (!live_b) nb = mk(0.0, 0.0, 0.0);
    exc += 0.5 * (na.v + nb.v) / rt;
    va += na.dr;          // d/d ra [ (1/2) n(2 ra) ] = n'(2 ra)
    vb += nb.dr;
    vsaa += 2.0 * na.ds;  // d/d saa [ (1/2) n(.., 4 saa) ]
    vsbb += 2.0 * nb.ds;
    return;
  }
  T3 a = t3(ra, 1.0, 0.0, 0.0), b = t3(rb, 0.0, 1.0, 0.0), st = t3(saa + 2.0 * sab + sbb, 0.0, 0.0, 1.0);
  T3 n = a + b;
  T3 rs = tcbrt((3.0 / (4.0 * HFG_PI)) / n);
  T3 z = (a - b) / n;
  T3 e;
  switch (id) {
    case 7: e = pol_eps_vwn(rs, z); break;
    case 8: e = pol_eps_vwn_rpa(rs, z); break;
    case 12: e = pol_eps_pw(rs, z, false); break;
    case 13: e = pol_eps_pw(rs, z, true); break;
    case 130: e = pol_eps_pbe_c(n, rs, z, st, xcpar().c_beta, xcpar().c_gamma, xcpar().c_BB); break;
    default: return;
  }
  T3 en = n * e;
  exc += e.v;
  va += en.a;
  vb += en.b;
  vsaa += en.s;
  vsab += 2.0 * en.s;
  vsbb += en.s;
}

/// eval_add_pol_basic plus the composite functionals (no recursion: a recursive device function needs a dynamic stack)
__host__ __device__ inline void eval_add_pol(int id, double ra, double rb, double saa, double sab, double sbb, bool live_a,
                                             bool live_b, double &exc, double &va, double &vb, double &vsaa, double &vsab,
                                             double &vsbb) {
#define HFG_ADD_SCALED(ID, W)                                                                          \
  {                                                                                                    \
    double e_ = 0.0, a_ = 0.0, b_ = 0.0, x_ = 0.0, y_ = 0.0, z_ = 0.0;                                 \
    eval_add_pol_basic(ID, ra, rb, saa, sab, sbb, live_a, live_b, e_, a_, b_, x_, y_, z_);             \
    exc += (W)*e_;                                                                                     \
    va += (W)*a_;                                                                                      \
    vb += (W)*b_;                                                                                      \
    vsaa += (W)*x_;                                                                                    \
    vsab += (W)*y_;                                                                                    \
    vsbb += (W)*z_;                                                                                    \
  }
  if (id == 406) {  // hyb_gga_xc_pbeh (PBE0), DFT part: 0.75 gga_x_pbe + gga_c_pbe
    HFG_ADD_SCALED(101, 0.75)
    HFG_ADD_SCALED(130, 1.0)
  } else if (id == 178) {  // hyb_lda_xc_cam_lda0, DFT part: spin-scaled exchange mixture + lda_c_pw_mod
    HFG_ADD_SCALED(-178, 1.0)
    HFG_ADD_SCALED(13, 1.0)
  } else if (id == 402) {  // hyb_gga_xc_b3lyp, DFT part
    HFG_ADD_SCALED(1, 0.08)
    HFG_ADD_SCALED(106, 0.72)
    HFG_ADD_SCALED(8, 0.19)
    HFG_ADD_SCALED(131, 0.81)
  } else
    eval_add_pol_basic(id, ra, rb, saa, sab, sbb, live_a, live_b, exc, va, vb, vsaa, vsab, vsbb);
#undef HFG_ADD_SCALED
}

// ---------------------------------------------------------------------------------------------------------
// meta-GGA (tau-dependent), spin-unpolarised: TPSS exchange (libxc id 202) and correlation (231).  The T3 slots
// (a, b, s) carry the derivatives with respect to (rho, sigma, tau) here.
// ---------------------------------------------------------------------------------------------------------
__host__ __device__ inline T3 tmaxv(T3 x, T3 y) { return (x.v >= y.v) ? x : y; }

__host__ __device__ inline T3 mg_eps_tpss_x(T3 rho, T3 sig, T3 tau) {
  const double b = 0.40, c = 1.59096, e = 1.537, kappa = 0.804, mu = 0.21951, muge = 10.0 / 81.0;
  const double c32 = 9.570780000627305;  // (3 pi^2)^{2/3}
  T3 exu = (-0.75 * cbrt(3.0 / HFG_PI)) * tcbrt(rho);
  T3 rho23 = tpow23(rho);
  T3 pp = sig / ((4.0 * c32) * rho * rho * rho23);
  T3 tauw = sig / (8.0 * rho);
  T3 tt = tmaxv(tau, tauw);
  T3 z = tauw / tt;
  T3 tunif = (0.3 * c32) * rho * rho23;
  T3 alpha = (tt - tauw) / tunif;
  T3 qb = (9.0 / 20.0) * (alpha - 1.0) / tsqrt(1.0 + b * alpha * (alpha - 1.0)) + (2.0 / 3.0) * pp;
  T3 z2 = z * z;
  T3 opz2 = 1.0 + z2;
  T3 num = (muge + c * z2 / (opz2 * opz2)) * pp + (146.0 / 2025.0) * qb * qb -
           (73.0 / 405.0) * qb * tsqrt(0.5 * (9.0 / 25.0) * z2 + 0.5 * pp * pp) + (muge * muge / kappa) * pp * pp +
           (2.0 * sqrt(e) * muge * 9.0 / 25.0) * z2 + (e * mu) * pp * pp * pp;
  T3 den = 1.0 + sqrt(e) * pp;
  T3 x = num / (den * den);
  T3 F = 1.0 + kappa - kappa * kappa / (kappa + x);
  return exu * F;
}

template <class T>
__host__ __device__ inline T mg_eps_pbe_c_fullpol(T n, T sig) {
  const double beta = 0.06672455060314922;
  const double gamma = (1.0 - 0.6931471805599453) / (HFG_PI * HFG_PI);
  const double B = beta / gamma;
  T rs = tcbrt((3.0 / (4.0 * HFG_PI)) / n);
  T ec = pol_pw_G(rs, 0.01554535, 0.20548, 14.1189, 6.1977, 3.3662, 0.62517);
  const double phi = 0.7937005259840998, phi3 = 0.5;  // 2^{-1/3}
  T kf = tcbrt((3.0 * HFG_PI * HFG_PI) * n);
  T ks2 = (4.0 / HFG_PI) * kf;
  T t2 = sig / ((4.0 * phi * phi) * ks2 * n * n);
  T Aa = B / texpm1(-ec / (gamma * phi3));
  T At2 = Aa * t2;
  return ec + (gamma * phi3) * tlog1p(B * t2 * (1.0 + At2) / (1.0 + At2 + At2 * At2));
}

// TPSS correlation for a spin-polarised density (Tao, Perdew, Staroverov, Scuseria, PRL 91, 146401 (2003), eqs 11-14):
//   rev = e_PBE [1 + C(zeta,xi) z^2] - [1 + C(zeta,xi)] z^2 sum_s (n_s/n) max(e_PBE(n_s,0,grad n_s,0), e_PBE)
//   C(zeta,xi) = C(zeta,0) / {1 + xi^2 [(1+zeta)^{-4/3} + (1-zeta)^{-4/3}]/2}^4,  C(zeta,0) = 0.53 + 0.87 z^2 + 0.50 z^4 + 2.26 z^6
//   xi = |grad zeta| / (2 (3 pi^2 n)^{1/3}),  z = tau_W/tau,  e_c = rev [1 + d rev z^3]
__host__ __device__ inline T7 mg_eps_tpss_c_pol(T7 ra, T7 rb, T7 saa, T7 sab, T7 sbb, T7 ta, T7 tb) {
  const double d = 2.8;
  T7 n = ra + rb;
  T7 rs = tcbrt((3.0 / (4.0 * HFG_PI)) / n);
  T7 zeta = (ra - rb) / n;
  T7 st = saa + 2.0 * sab + sbb;
  T7 epbe = pol_eps_pbe_c(n, rs, zeta, st, 0.06672455060314922, HFG_PBE_GAMMA, 1.0);
  T7 eta = tmaxv(mg_eps_pbe_c_fullpol(ra, saa), epbe);
  T7 etb = tmaxv(mg_eps_pbe_c_fullpol(rb, sbb), epbe);
  T7 tauw = st / (8.0 * n);
  T7 tt = tmaxv(ta + tb, tauw);
  T7 z = tauw / tt;
  T7 z2 = z * z;
  T7 omz = 1.0 - zeta, opz = 1.0 + zeta;
  T7 gz2 = (omz * omz * saa - 2.0 * omz * opz * sab + opz * opz * sbb) / (n * n);  // |grad zeta|^2
  T7 kf = tcbrt((3.0 * HFG_PI * HFG_PI) * n);
  T7 xi2 = gz2 / (4.0 * kf * kf);
  T7 zz = zeta * zeta;
  T7 C0 = 0.53 + 0.87 * zz + 0.50 * zz * zz + 2.26 * zz * zz * zz;
  T7 den = 1.0 + 0.5 * xi2 * (1.0 / tpow43(opz) + 1.0 / tpow43(omz));
  T7 den2 = den * den;
  T7 Cz = C0 / (den2 * den2);
  T7 rev = epbe * (1.0 + Cz * z2) - (1.0 + Cz) * z2 * (ra * eta + rb * etb) / n;
  return rev * (1.0 + d * rev * z2 * z);
}

__host__ __device__ inline T3 mg_eps_tpss_c(T3 rho, T3 sig, T3 tau) {
  const double d = 2.8, C0 = 0.53;
  T3 rs = tcbrt((3.0 / (4.0 * HFG_PI)) / rho);
  T3 epbe = pol_eps_pbe_c(rho, rs, t3(0.0), sig, 0.06672455060314922, HFG_PBE_GAMMA, 1.0);
  T3 esig = mg_eps_pbe_c_fullpol(0.5 * rho, 0.25 * sig);
  T3 etil = tmaxv(esig, epbe);
  T3 tauw = sig / (8.0 * rho);
  T3 tt = tmaxv(tau, tauw);
  T3 z = tauw / tt;
  T3 z2 = z * z;
  T3 rev = epbe * (1.0 + C0 * z2) - (1.0 + C0) * z2 * etil;
  return rev * (1.0 + d * rev * z2 * z);
}

/// adds a meta-GGA's exc, vrho, vsigma, vtau at one point (rho >= threshold assumed)
__host__ __device__ inline void eval_add_mgga(int id, double rho, double sigma, double tau, bool live, double &exc,
                                              double &vrho, double &vsigma, double &vtau) {
  if (id == 202 && !live) return;  // exchange channel rho/2 below the threshold, see eval_add
  T3 r = t3(rho, 1.0, 0.0, 0.0), s = t3(fmax(sigma, 1e-40), 0.0, 1.0, 0.0), t = t3(fmax(tau, 1e-40), 0.0, 0.0, 1.0);
  T3 e = (id == 202) ? mg_eps_tpss_x(r, s, t) : mg_eps_tpss_c(r, s, t);
  T3 en = r * e;
  exc += e.v;
  vrho += en.a;
  vsigma += en.b;
  vtau += en.s;
}

/// spin-polarised meta-GGA: adds exc (per particle of ra + rb), v_rho[2], v_sigma[3] (aa, ab, bb), v_tau[2]; ra, rb
/// already raised to the threshold.  Exchange by spin scaling, E_x[a,b] = (E_x[2a] + E_x[2b])/2.
/// live_a, live_b: the channel's own density reached the threshold.  A channel below it is left out of the exchange sum
/// (libxc screens it the same way): its v_tau = d(n e)/d tau would be of order 1/tau_unif(threshold) and enters the Fock
/// matrix unweighted, unlike v_rho and v_sigma which multiply the channel's density or gradient.
__host__ __device__ inline void eval_add_mgga_pol(int id, double ra, double rb, double saa, double sab, double sbb, double ta,
                                                  double tb, bool live_a, bool live_b, double &exc, double &va, double &vb,
                                                  double &vsaa, double &vsab, double &vsbb, double &vta, double &vtb) {
  const double rt = ra + rb;
  if (id == 202) {
    T3 na = t3(0.0), nb = t3(0.0);
    if (live_a) {
      T3 Ra = t3(2.0 * ra, 1.0, 0.0, 0.0), Sa = t3(fmax(4.0 * saa, 1e-40), 0.0, 1.0, 0.0), Ta = t3(fmax(2.0 * ta, 1e-40), 0.0, 0.0, 1.0);
      na = Ra * mg_eps_tpss_x(Ra, Sa, Ta);
    }
    if (live_b) {
      T3 Rb = t3(2.0 * rb, 1.0, 0.0, 0.0), Sb = t3(fmax(4.0 * sbb, 1e-40), 0.0, 1.0, 0.0), Tb = t3(fmax(2.0 * tb, 1e-40), 0.0, 0.0, 1.0);
      nb = Rb * mg_eps_tpss_x(Rb, Sb, Tb);
    }
    exc += 0.5 * (na.v + nb.v) / rt;
    va += na.a;  // d/d ra [ n(2 ra, 4 saa, 2 ta)/2 ]
    vb += nb.a;
    vsaa += 2.0 * na.b;
    vsbb += 2.0 * nb.b;
    vta += na.s;
    vtb += nb.s;
    return;
  }
  if (id != 231) return;
  T7 A = t7var(ra, 0), B = t7var(rb, 1);
  T7 Saa = t7var(fmax(saa, 1e-40), 2), Sab = t7var(sab, 3), Sbb = t7var(fmax(sbb, 1e-40), 4);
  T7 Ta = t7var(fmax(ta, 1e-40), 5), Tb = t7var(fmax(tb, 1e-40), 6);
  T7 e = mg_eps_tpss_c_pol(A, B, Saa, Sab, Sbb, Ta, Tb);
  T7 en = (A + B) * e;
  exc += e.v;
  va += en.d[0];
  vb += en.d[1];
  vsaa += en.d[2];
  vsab += en.d[3];
  vsbb += en.d[4];
  vta += en.d[5];
  vtb += en.d[6];
}

// ---------------------------------------------------------------------------------------------------------
// SCAN (Sun, Ruzsinszky, Perdew, PRL 115, 036402 (2015), and its supplement): mgga_x_scan (libxc 263), mgga_c_scan (267),
// hyb_mgga_x_scan0 (264: 0.75 SCAN exchange + 0.25 exact exchange over the full range); and the PBE variants with fixed
// constants, gga_x_pbe_r (102), gga_x_pbe_sol (116), gga_c_pbe_sol (133).  These six ids (is_ext) are evaluated by
// eval_add_ext / eval_add_ext_pol alone, which the grid kernels call only in a separate instantiation (fock.hip): the code
// that runs every other functional is what it was.
// Shared quantities (tau is libxc's, 1/2 sum |grad phi|^2):
//   p = s^2 = sigma / (4 (3 pi^2)^{2/3} n^{8/3}),  tau_W = sigma/(8n),  alpha = (tau - tau_W)/tau_unif,
//   tau_unif = (3/10)(3 pi^2)^{2/3} n^{5/3} d_s(zeta),  d_s = [(1+zeta)^{5/3} + (1-zeta)^{5/3}]/2
// Exchange (unpolarised; polarised by spin scaling, E_x[a,b] = (E_x[2a] + E_x[2b])/2, as TPSS):
//   F_x = {h1 + f_x(alpha) (h0 - h1)} g_x(s),  h0 = 1.174,  h1 = 1 + k1 - k1/(1 + x/k1),  k1 = 0.065,
//   x = mu p [1 + (b4 p/mu) exp(-|b4| p/mu)] + [b1 p + b2 (1 - alpha) exp(-b3 (1 - alpha)^2)]^2,
//   mu = 10/81, b2 = sqrt(5913/405000), b1 = (511/13500)/(2 b2), b3 = 1/2, b4 = mu^2/k1 - 1606/18225 - b1^2,
//   f(alpha) = exp(-c1 alpha/(1 - alpha)) for alpha < 1, -d exp(c2/(1 - alpha)) for alpha > 1; f_x: (c1, c2, d) = (0.667, 0.8, 1.24)
//   g_x = 1 - exp(-a1/sqrt(s)) = 1 - exp(-a1 p^{-1/4}),  a1 = 4.9479
// Correlation (n, zeta, p, alpha of the total density, tau = tau_a + tau_b):
//   e_c = e_c1 + f_c(alpha) (e_c0 - e_c1),  f_c: (c1, c2, d) = (0.64, 1.5, 0.7)
//   e_c1 = e_LSDA + H1, e_LSDA = PW92 as in PBE (pol_eps_pw, modified), H1 = gamma phi^3 ln[1 + w1 (1 - (1 + 4 A t^2)^{-1/4})],
//   w1 = exp(-e_LSDA/(gamma phi^3)) - 1, A = beta(rs)/(gamma w1), beta(rs) = 0.066725 (1 + 0.1 rs)/(1 + 0.1778 rs),
//   gamma = (1 - ln 2)/pi^2, phi = [(1+zeta)^{2/3} + (1-zeta)^{2/3}]/2, t^2 = (3 pi^2/16)^{2/3} p/(phi^2 rs)
//   e_c0 = (e_LDA0 + H0) G_c(zeta), e_LDA0 = -b1c/(1 + b2c sqrt(rs) + b3c rs), (b1c, b2c, b3c) = (0.0285764, 0.0889, 0.125541),
//   H0 = b1c ln[1 + w0 (1 - (1 + 4 chi p)^{-1/4})], w0 = exp(-e_LDA0/b1c) - 1, chi = 0.128026,
//   G_c = [1 - 2.3631 (d_x(zeta) - 1)] (1 - zeta^12), d_x = [(1+zeta)^{4/3} + (1-zeta)^{4/3}]/2
// Numerical rules:
//   - f(alpha) has an essential singularity at alpha = 1, where all its derivatives vanish.  Once its exponent is below
//     -700, value and derivative are exactly 0: the chain rule would give 0 * inf = NaN where 1 - alpha underflows.
//   - tau below tau_W (rounding in one-orbital regions) is raised to tau_W (tmaxv, as TPSS does), so alpha >= 0.
//   - g_x is differentiated in p: where exp(-a1 p^{-1/4}) underflows (p -> 0) it is 1 with a zero derivative, no sqrt(0).
//   - (1 -+ zeta)^{2/3} in phi has an infinite zeta derivative at |zeta| = 1, which a density whose minority spin is at the
//     threshold reaches in rounding: there (1 -+ zeta <= DBL_EPSILON) its derivative is taken as 0, as libxc's zeta
//     threshold does.
// ---------------------------------------------------------------------------------------------------------
__host__ __device__ inline T3 tchain(T3 x, double f, double df) { return t3f(x, f, df); }
__host__ __device__ inline T7 tchain(T7 x, double f, double df) { return t7f(x, f, df); }
/// x^a, x > 0
template <class T>
__host__ __device__ inline T tpowr(T x, double a) {
  const double v = pow(x.v, a);
  return tchain(x, v, a * v / x.v);
}
/// x^{5/3}, differentiable at 0
template <class T>
__host__ __device__ inline T tpow53(T x) {
  const double c = cbrt(x.v);
  return tchain(x, x.v * c * c, (5.0 / 3.0) * c * c);
}
/// (1 -+ zeta)^{2/3} of phi, derivative 0 within DBL_EPSILON of zeta = +-1
template <class T>
__host__ __device__ inline T scan_opz23(T x) {
  const double c = cbrt(x.v);
  return tchain(x, c * c, x.v > 2.220446049250313e-16 ? 2.0 / (3.0 * c) : 0.0);
}
/// f_x / f_c of alpha (see above), exactly 0 with a zero derivative at alpha = 1 and wherever the exponent is below -700
template <class T>
__host__ __device__ inline T scan_switch(T alpha, double c1, double c2, double d) {
  const double u = 1.0 - alpha.v;
  double f = 0.0, df = 0.0;
  if (u > 0.0) {
    const double ex = -c1 * alpha.v / u;
    if (ex > -700.0) {
      f = exp(ex);
      df = -c1 * f / (u * u);
    }
  } else if (u < 0.0) {
    const double ex = c2 / u;
    if (ex > -700.0) {
      f = -d * exp(ex);
      df = c2 * f / (u * u);
    }
  }
  return tchain(alpha, f, df);
}
/// g_x = 1 - exp(-a1 p^{-1/4}) as a function of p = s^2
template <class T>
__host__ __device__ inline T scan_gx(T p) {
  const double a1 = 4.9479;
  if (!(p.v > 0.0)) return tchain(p, 1.0, 0.0);
  const double q = 1.0 / sqrt(sqrt(p.v));  // 1/sqrt(s)
  if (a1 * q > 700.0) return tchain(p, 1.0, 0.0);
  const double e = exp(-a1 * q);
  return tchain(p, 1.0 - e, -0.25 * a1 * e * q / p.v);
}

/// SCAN exchange energy per particle of an unpolarised density
template <class T>
__host__ __device__ inline T scan_eps_x(T rho, T sig, T tau) {
  const double c32 = 9.570780000627305;  // (3 pi^2)^{2/3}
  const double k1 = 0.065, h0 = 1.174, mu = 10.0 / 81.0, b3 = 0.5;
  const double b2 = 0.12083045973594572, b1 = 0.15663207743548518, b4 = 0.12183151020599578;  // see above; b4 > 0
  T exu = (-0.75 * cbrt(3.0 / HFG_PI)) * tcbrt(rho);
  T rho23 = tpow23(rho);
  T p = sig / ((4.0 * c32) * rho * rho * rho23);
  T tauw = sig / (8.0 * rho);
  T alpha = (tmaxv(tau, tauw) - tauw) / ((0.3 * c32) * rho * rho23);
  T oma = 1.0 - alpha;
  T bx = b1 * p + b2 * oma * texp((-b3) * oma * oma);
  T x = mu * p * (1.0 + (b4 / mu) * p * texp((-b4 / mu) * p)) + bx * bx;
  T h1 = (1.0 + k1) - k1 / (1.0 + x / k1);
  T F = (h1 + scan_switch(alpha, 0.667, 0.8, 1.24) * (h0 - h1)) * scan_gx(p);
  return exu * F;
}

/// SCAN correlation energy per particle; z = zeta, sig = |grad n|^2, tau = tau_a + tau_b
template <class T>
__host__ __device__ inline T scan_eps_c(T n, T z, T sig, T tau) {
  const double c32 = 9.570780000627305, ct2 = 1.5073033983379012;  // (3 pi^2)^{2/3}, (3 pi^2/16)^{2/3}
  const double gamma = HFG_PBE_GAMMA;
  const double b1c = 0.0285764, b2c = 0.0889, b3c = 0.125541, chi = 0.128026;
  T rs = tcbrt((3.0 / (4.0 * HFG_PI)) / n);
  T opz = 1.0 + z, omz = 1.0 - z;
  T n23 = tpow23(n);
  T p = sig / ((4.0 * c32) * n * n * n23);
  T ds = 0.5 * (tpow53(opz) + tpow53(omz));
  T tauw = sig / (8.0 * n);
  T alpha = (tmaxv(tau, tauw) - tauw) / ((0.3 * c32) * n * n23 * ds);
  // e_c1: PW92 plus H1
  T elsda = pol_eps_pw(rs, z, true);
  T phi = 0.5 * (scan_opz23(opz) + scan_opz23(omz));
  T gphi3 = gamma * phi * phi * phi;
  T t2 = ct2 * p / (phi * phi * rs);
  T w1 = texpm1(-elsda / gphi3);
  T A = 0.066725 * (1.0 + 0.1 * rs) / ((1.0 + 0.1778 * rs) * (gamma * w1));
  T ec1 = elsda + gphi3 * tlog1p(w1 * (1.0 - tpowr(1.0 + 4.0 * A * t2, -0.25)));
  // e_c0: the alpha = 0 limit
  T elda0 = (-b1c) / (1.0 + b2c * tsqrt(rs) + b3c * rs);
  T w0 = texpm1(-elda0 / b1c);
  T H0 = b1c * tlog1p(w0 * (1.0 - tpowr(1.0 + (4.0 * chi) * p, -0.25)));
  T dx = 0.5 * (tpow43(opz) + tpow43(omz));
  T z2 = z * z;
  T z4 = z2 * z2;
  T Gc = (1.0 - 2.3631 * (dx - 1.0)) * (1.0 - z4 * z4 * z4);
  T ec0 = (elda0 + H0) * Gc;
  return ec1 + scan_switch(alpha, 0.64, 1.5, 0.7) * (ec0 - ec1);
}

// ---------------------------------------------------------------------------------------------------------
// Short-range GGA exchange of the range-separated GGA hybrids, in the construction of Iikura, Tsuneda, Yanai, Hirao (J. Chem.
// Phys. 115, 3540 (2001); erfc kernel) and of Savin, Flad / Akinaga, Ten-no (Chem. Phys. Lett. 462, 348 (2008); Yukawa kernel,
// used by Seth, Ziegler, J. Chem. Theory Comput. 8, 901 (2012)) for an enhancement factor F_x(s).  For an unpolarised density
// (polarised by spin scaling, E_x[a,b] = (E_x[2a] + E_x[2b])/2):
//   k_GGA = k_F / sqrt(F_x(s)),  k_F = (3 pi^2 rho)^{1/3},  a = omega / (2 k_GGA),  eps_x^sr = eps_x^LDA(rho) F_x(s) att(a)
// with att = att_erf / att_yukawa of eps_lda_x_sr, to which this reduces for F_x = 1.  B88's F_x grows without bound in the
// density tail (x / (6 asinh x)), so a is large there and the attenuation comes from its series branch.
// Primitives (omega: libxc's default, or the external parameter x_omega): gga_x_ityh (529; B88, erfc, 0.2), gga_x_sfat (530;
// B88, Yukawa, 0.44), gga_x_ityh_pbe (HFG_ID_ITYH_PBE; PBE, erfc, 0.2), gga_x_sfat_pbe (HFG_ID_SFAT_PBE; PBE, Yukawa, 0.44).
// Hybrids, 1/r = [1 - alpha - beta erf(omega r)]/r + [alpha + beta erf(omega r)]/r (erfc; the Yukawa ones with exp(-omega r)
// in place of erfc): DFT exchange (1 - alpha - beta) X + beta X^sr(omega); the drivers add (alpha + beta) K - beta K^sr.
//   hyb_gga_xc_cam_b3lyp  (433; Yanai, Tew, Handy, Chem. Phys. Lett. 393, 51 (2004)): erfc, (0.19, 0.46, 0.33),
//                          0.35 B88 + 0.46 ITYH-B88 + 0.19 lda_c_vwn + 0.81 gga_c_lyp
//   hyb_gga_xc_camy_b3lyp (470; Seth, Ziegler): Yukawa, (0.19, 0.46, 0.34), 0.35 B88 + 0.46 SFAT-B88 + 0.19 lda_c_vwn + 0.81 gga_c_lyp
//   hyb_gga_xc_camy_blyp  (455; Akinaga, Ten-no): Yukawa, (0.20, 0.80, 0.44), 0.80 SFAT-B88 + gga_c_lyp
//   hyb_gga_xc_lcy_blyp   (468): Yukawa, (0, 1, 0.75), SFAT-B88 + gga_c_lyp
//   hyb_gga_xc_lcy_pbe    (467): Yukawa, (0, 1, 0.75), SFAT-PBE + gga_c_pbe
// Like the is_ext functionals these ids are evaluated by eval_add_ext / eval_add_ext_pol alone.
// ---------------------------------------------------------------------------------------------------------
/// B88's enhancement factor over eps_lda_x, F = 1 + (beta/Cx) t / (1 + 6 beta x asinh x) with t = x^2 of one spin channel
__host__ __device__ inline Dual fx_b88(Dual rho, Dual sigma) {
  const double beta = 0.0042, Cx = 0.9305257363491000;
  Dual rs = 0.5 * rho;
  Dual r43 = rs * dcbrt(rs);
  Dual t = (0.25 * sigma) / (r43 * r43);
  return 1.0 + (beta / Cx) * t / (1.0 + (6.0 * beta) * d_x_asinh_x(t));
}
__host__ __device__ inline Dual fx_pbe(Dual rho, Dual sigma, double kappa, double mu) {
  Dual kf = dcbrt((3.0 * HFG_PI * HFG_PI) * rho);
  Dual s2 = sigma / (4.0 * kf * kf * rho * rho);
  return 1.0 + kappa - kappa / (1.0 + (mu / kappa) * s2);
}
/// exchange part of a short-range GGA primitive or hybrid: eps_x^LDA F_x [wx + wsr att(a)].  Always inlined: as a device function
/// of its own it would renumber the local labels of every kernel behind it in the module, and the kernels of the other
/// functionals are kept identical to what they were, text included.
__host__ __device__ __attribute__((always_inline)) inline Dual eps_rsgga_x(int id, Dual rho, Dual sigma) {
  double wx = 0.0, wsr = 1.0, omega;
  int kind = 1;
  bool pbe = false;
  switch (id) {
    case 529: kind = 2; omega = 0.2; break;
    case 530: omega = 0.44; break;
    case HFG_ID_ITYH_PBE: kind = 2; pbe = true; omega = 0.2; break;
    case HFG_ID_SFAT_PBE: pbe = true; omega = 0.44; break;
    case 433: kind = 2; wx = 0.35; wsr = 0.46; omega = 0.33; break;
    case 470: wx = 0.35; wsr = 0.46; omega = 0.34; break;
    case 455: wsr = 0.80; omega = 0.44; break;
    case 467: pbe = true; omega = 0.75; break;
    default: omega = 0.75; break;  // 468
  }
  if (is_rsgga_x(id) && xcpar().x_omega >= 0.0) omega = xcpar().x_omega;
  Dual F = pbe ? fx_pbe(rho, sigma, 0.8040, HFG_PBE_MU) : fx_b88(rho, sigma);
  Dual kf = dcbrt((3.0 * HFG_PI * HFG_PI) * rho);
  Dual a = (0.5 * omega) * dsqrt(F) / kf;
  Dual Fatt;  // F_x att(a)
  if (a.v > (kind == 1 ? 2.0 : 0.75)) {
    // The series branch of att_erf / att_yukawa, as att(a) = u g(u) with u = 1/a^2 = 4 k_F^2 / (omega^2 F_x): the leading term of
    // F_x att is 4 k_F^2 / (36 or 9 omega^2), free of F_x.  Taken as the product F_x * att(a), the sigma derivative would be the
    // difference of two terms that cancel to 1/a^2 of their size, which is 1e-5 and less in the density tail.
    Dual ua = (4.0 / (omega * omega)) * kf * kf;  // u F_x
    Dual u = ua / F, g = mk(0.0);
    if (kind == 1) {
      Dual r = mk(1.0);
      for (int k = 1; k <= 40; k++) {
        g = g + r * (2.0 / ((2.0 * k + 1.0) * (k + 1.0) * (k + 2.0)));
        r = -1.0 * r * u;
      }
    } else {
      Dual r = mk(-0.25);
      for (int k = 1; k <= 24; k++) {
        g = g - r * (2.0 / ((2.0 * k + 1.0) * (k + 1.0) * (k + 2.0)));
        r = r * u * (-0.25 / (k + 1.0));
      }
    }
    Fatt = ua * g;
  } else
    Fatt = F * (kind == 1 ? att_yukawa(a) : att_erf(a));
  return eps_lda_x(rho) * (wx * F + wsr * Fatt);
}

__host__ __device__ inline double ext_pbe_kappa(int id) { return id == 102 ? 1.245 : 0.804; }
__host__ __device__ inline double ext_pbe_mu(int id) { return id == 102 ? HFG_PBE_MU : 10.0 / 81.0; }

/// adds an is_ext functional's exc, vrho, vsigma, vtau at one point (rho >= threshold assumed; live as in eval_add).  The
/// meta-GGA floors of eval_add_mgga (1e-40 under sigma and tau) apply to SCAN.
__host__ __device__ inline void eval_add_ext(int id, double rho, double sigma, double tau, bool live, double &exc, double &vrho,
                                             double &vsigma, double &vtau) {
  if (!live && is_exchange(id)) return;
  if (is_rsgga_x(id) || is_rsgga_hyb(id)) {
    if (!live && is_rsgga_x(id)) return;
    Dual r = mk(rho, 1.0, 0.0), s = mk(sigma, 0.0, 1.0);
    Dual e = live ? eps_rsgga_x(id, r, s) : mk(0.0);  // the hybrids keep their correlation part
    if (id == 433 || id == 470) e = e + 0.19 * eps_lda_c_vwn(r) + 0.81 * eps_gga_c_lyp(r, s);
    else if (id == 455 || id == 468) e = e + eps_gga_c_lyp(r, s);
    else if (id == 467) e = e + eps_gga_c_pbe(r, s, 0.06672455060314922, HFG_PBE_GAMMA, 1.0);
    Dual en = r * e;
    exc += e.v;
    vrho += en.dr;
    vsigma += en.ds;
    return;
  }
  if (id == 102 || id == 116 || id == 133) {
    Dual r = mk(rho, 1.0, 0.0), s = mk(sigma, 0.0, 1.0);
    Dual e = id == 133 ? eps_gga_c_pbe(r, s, 0.046, HFG_PBE_GAMMA, 1.0) : eps_gga_x_pbe(r, s, ext_pbe_kappa(id), ext_pbe_mu(id));
    Dual en = r * e;
    exc += e.v;
    vrho += en.dr;
    vsigma += en.ds;
    return;
  }
  T3 r = t3(rho, 1.0, 0.0, 0.0), s = t3(fmax(sigma, 1e-40), 0.0, 1.0, 0.0), t = t3(fmax(tau, 1e-40), 0.0, 0.0, 1.0);
  T3 e = id == 267 ? scan_eps_c(r, t3(0.0), s, t) : scan_eps_x(r, s, t);
  if (id == 264) e = 0.75 * e;  // hyb_mgga_x_scan0, DFT part
  T3 en = r * e;
  exc += e.v;
  vrho += en.a;
  vsigma += en.b;
  vtau += en.s;
}

/// spin-polarised is_ext functional: adds exc (per particle of ra + rb), v_rho[2], v_sigma[3], v_tau[2]; ra, rb already raised
/// to the threshold, live_a / live_b as in eval_add_mgga_pol
__host__ __device__ inline void eval_add_ext_pol(int id, double ra, double rb, double saa, double sab, double sbb, double ta,
                                                 double tb, bool live_a, bool live_b, double &exc, double &va, double &vb,
                                                 double &vsaa, double &vsab, double &vsbb, double &vta, double &vtb) {
  const double rt = ra + rb;
  if (is_rsgga_x(id) || is_rsgga_hyb(id)) {  // exchange by spin scaling; the correlation of the hybrids from the basic evaluators
    Dual na = mk(0.0), nb = mk(0.0);
    if (live_a) {
      Dual a = mk(2.0 * ra, 1.0, 0.0);
      na = a * eps_rsgga_x(id, a, mk(4.0 * saa, 0.0, 1.0));
    }
    if (live_b) {
      Dual b = mk(2.0 * rb, 1.0, 0.0);
      nb = b * eps_rsgga_x(id, b, mk(4.0 * sbb, 0.0, 1.0));
    }
    exc += 0.5 * (na.v + nb.v) / rt;
    va += na.dr;
    vb += nb.dr;
    vsaa += 2.0 * na.ds;
    vsbb += 2.0 * nb.ds;
    if (id == 467) {
      T3 a = t3(ra, 1.0, 0.0, 0.0), b = t3(rb, 0.0, 1.0, 0.0), st = t3(saa + 2.0 * sab + sbb, 0.0, 0.0, 1.0);
      T3 n = a + b;
      T3 e = pol_eps_pbe_c(n, tcbrt((3.0 / (4.0 * HFG_PI)) / n), (a - b) / n, st, 0.06672455060314922, HFG_PBE_GAMMA, 1.0);
      T3 en = n * e;
      exc += e.v;
      va += en.a;
      vb += en.b;
      vsaa += en.s;
      vsab += 2.0 * en.s;
      vsbb += en.s;
    } else if (is_rsgga_hyb(id)) {
      const bool b3 = id == 433 || id == 470;
      double e_ = 0.0, a_ = 0.0, b_ = 0.0, x_ = 0.0, y_ = 0.0, z_ = 0.0;
      eval_add_pol_basic(131, ra, rb, saa, sab, sbb, live_a, live_b, e_, a_, b_, x_, y_, z_);
      const double wl = b3 ? 0.81 : 1.0;
      exc += wl * e_;
      va += wl * a_;
      vb += wl * b_;
      vsaa += wl * x_;
      vsab += wl * y_;
      vsbb += wl * z_;
      if (b3) {
        e_ = a_ = b_ = x_ = y_ = z_ = 0.0;
        eval_add_pol_basic(7, ra, rb, saa, sab, sbb, live_a, live_b, e_, a_, b_, x_, y_, z_);
        exc += 0.19 * e_;
        va += 0.19 * a_;
        vb += 0.19 * b_;
      }
    }
    return;
  }
  if (id == 102 || id == 116) {  // spin scaling, as gga_x_pbe in eval_add_pol_basic
    Dual na = mk(0.0), nb = mk(0.0);
    if (live_a) {
      Dual a = mk(2.0 * ra, 1.0, 0.0);
      na = a * eps_gga_x_pbe(a, mk(4.0 * saa, 0.0, 1.0), ext_pbe_kappa(id), ext_pbe_mu(id));
    }
    if (live_b) {
      Dual b = mk(2.0 * rb, 1.0, 0.0);
      nb = b * eps_gga_x_pbe(b, mk(4.0 * sbb, 0.0, 1.0), ext_pbe_kappa(id), ext_pbe_mu(id));
    }
    exc += 0.5 * (na.v + nb.v) / rt;
    va += na.dr;
    vb += nb.dr;
    vsaa += 2.0 * na.ds;
    vsbb += 2.0 * nb.ds;
    return;
  }
  if (id == 133) {
    T3 a = t3(ra, 1.0, 0.0, 0.0), b = t3(rb, 0.0, 1.0, 0.0), st = t3(saa + 2.0 * sab + sbb, 0.0, 0.0, 1.0);
    T3 n = a + b;
    T3 e = pol_eps_pbe_c(n, tcbrt((3.0 / (4.0 * HFG_PI)) / n), (a - b) / n, st, 0.046, HFG_PBE_GAMMA, 1.0);
    T3 en = n * e;
    exc += e.v;
    va += en.a;
    vb += en.b;
    vsaa += en.s;
    vsab += 2.0 * en.s;
    vsbb += en.s;
    return;
  }
  if (id == 263 || id == 264) {
    const double w = id == 264 ? 0.75 : 1.0;
    T3 na = t3(0.0), nb = t3(0.0);
    if (live_a) {
      T3 Ra = t3(2.0 * ra, 1.0, 0.0, 0.0), Sa = t3(fmax(4.0 * saa, 1e-40), 0.0, 1.0, 0.0), Ta = t3(fmax(2.0 * ta, 1e-40), 0.0, 0.0, 1.0);
      na = w * (Ra * scan_eps_x(Ra, Sa, Ta));
    }
    if (live_b) {
      T3 Rb = t3(2.0 * rb, 1.0, 0.0, 0.0), Sb = t3(fmax(4.0 * sbb, 1e-40), 0.0, 1.0, 0.0), Tb = t3(fmax(2.0 * tb, 1e-40), 0.0, 0.0, 1.0);
      nb = w * (Rb * scan_eps_x(Rb, Sb, Tb));
    }
    exc += 0.5 * (na.v + nb.v) / rt;
    va += na.a;  // d/d ra [ n(2 ra, 4 saa, 2 ta)/2 ]
    vb += nb.a;
    vsaa += 2.0 * na.b;
    vsbb += 2.0 * nb.b;
    vta += na.s;
    vtb += nb.s;
    return;
  }
  if (id != 267) return;
  T7 A = t7var(ra, 0), B = t7var(rb, 1);
  T7 Saa = t7var(fmax(saa, 1e-40), 2), Sab = t7var(sab, 3), Sbb = t7var(fmax(sbb, 1e-40), 4);
  T7 Ta = t7var(fmax(ta, 1e-40), 5), Tb = t7var(fmax(tb, 1e-40), 6);
  T7 n = A + B;
  T7 e = scan_eps_c(n, (A - B) / n, Saa + 2.0 * Sab + Sbb, Ta + Tb);
  T7 en = n * e;
  exc += e.v;
  va += en.d[0];
  vb += en.d[1];
  vsaa += en.d[2];
  vsab += en.d[3];
  vsbb += en.d[4];
  vta += en.d[5];
  vtb += en.d[6];
}

// ---------------------------------------------------------------------------------------------------------
// Laplacian-dependent meta-GGAs (the atomic program's do_lapl path, src/atomic/dftgrid.cpp:105-120, 206-229, 557-571).
// N-slot forward-mode duals: unpolarised slots (rho, sigma, tau, lapl); polarised slots (rho_a, rho_b, sigma_aa,
// sigma_ab, sigma_bb, tau_a, tau_b, lapl_a, lapl_b).  tau is libxc's, 1/2 sum |grad phi|^2.
// ---------------------------------------------------------------------------------------------------------
template <int N>
struct DN {
  double v, d[N];
};
template <int N>
__host__ __device__ inline DN<N> dn(double v) {
  DN<N> r;
  r.v = v;
  for (int k = 0; k < N; k++) r.d[k] = 0.0;
  return r;
}
template <int N>
__host__ __device__ inline DN<N> dnvar(double v, int k) {
  DN<N> r = dn<N>(v);
  r.d[k] = 1.0;
  return r;
}
/// f(x) with f'(x) = df
template <int N>
__host__ __device__ inline DN<N> dnf(const DN<N> &x, double f, double df) {
  DN<N> r;
  r.v = f;
  for (int k = 0; k < N; k++) r.d[k] = df * x.d[k];
  return r;
}
template <int N>
__host__ __device__ inline DN<N> operator+(const DN<N> &x, const DN<N> &y) {
  DN<N> r;
  r.v = x.v + y.v;
  for (int k = 0; k < N; k++) r.d[k] = x.d[k] + y.d[k];
  return r;
}
template <int N>
__host__ __device__ inline DN<N> operator-(const DN<N> &x, const DN<N> &y) {
  DN<N> r;
  r.v = x.v - y.v;
  for (int k = 0; k < N; k++) r.d[k] = x.d[k] - y.d[k];
  return r;
}
template <int N>
__host__ __device__ inline DN<N> operator*(const DN<N> &x, const DN<N> &y) {
  DN<N> r;
  r.v = x.v * y.v;
  for (int k = 0; k < N; k++) r.d[k] = x.d[k] * y.v + x.v * y.d[k];
  return r;
}
template <int N>
__host__ __device__ inline DN<N> operator/(const DN<N> &x, const DN<N> &y) {
  const double inv = 1.0 / y.v, q = x.v * inv;
  DN<N> r;
  r.v = q;
  for (int k = 0; k < N; k++) r.d[k] = (x.d[k] - q * y.d[k]) * inv;
  return r;
}
template <int N>
__host__ __device__ inline DN<N> operator+(const DN<N> &x, double c) { return dnf(x, x.v + c, 1.0); }
template <int N>
__host__ __device__ inline DN<N> operator+(double c, const DN<N> &x) { return dnf(x, x.v + c, 1.0); }
template <int N>
__host__ __device__ inline DN<N> operator-(const DN<N> &x, double c) { return dnf(x, x.v - c, 1.0); }
template <int N>
__host__ __device__ inline DN<N> operator-(double c, const DN<N> &x) { return dnf(x, c - x.v, -1.0); }
template <int N>
__host__ __device__ inline DN<N> operator*(const DN<N> &x, double c) { return dnf(x, x.v * c, c); }
template <int N>
__host__ __device__ inline DN<N> operator*(double c, const DN<N> &x) { return dnf(x, x.v * c, c); }
template <int N>
__host__ __device__ inline DN<N> operator/(const DN<N> &x, double c) { return x * (1.0 / c); }
template <int N>
__host__ __device__ inline DN<N> operator/(double c, const DN<N> &x) { return dnf(x, c / x.v, -c / (x.v * x.v)); }
template <int N>
__host__ __device__ inline DN<N> dncbrt(const DN<N> &x) {
  const double c = cbrt(x.v);
  return dnf(x, c, c / (3.0 * x.v));
}
template <int N>
__host__ __device__ inline DN<N> dnexp(const DN<N> &x) {
  const double e = exp(x.v);
  return dnf(x, e, e);
}
template <int N>
__host__ __device__ inline DN<N> dnexpm1(const DN<N> &x) { return dnf(x, expm1(x.v), exp(x.v)); }

/// the root x of (x - 2) e^{2x/3} / x = u (Becke, Roussel, PRA 39, 3761 (1989), eq 21 with u = Q / ((2/3) pi^{2/3} rho^{5/3})).
/// The left side increases from -inf (x -> 0) through 0 (x = 2) to +inf, so the root is unique: x in (0, 2) for u < 0, x > 2
/// for u > 0.  Newton on F(x) = ln|x - 2| + 2x/3 - ln x - ln|u| (monotone on either branch), kept inside the bracket by
/// bisection, to full precision.
__host__ __device__ inline double br89_root(double u) {
  if (u == 0.0) return 2.0;
  const double lu = log(fabs(u));
  const double sgn = u > 0.0 ? 1.0 : -1.0;  // sgn * F increases with x on the branch
  double lo, hi, x;
  if (u > 0.0) {
    lo = 2.0;
    hi = fmax(4.0, 1.5 * (lu + 0.6931471805599453) + 1.0);
    x = fmin(2.0 + 2.0 * u * 0.26359713811572677, 0.5 * (lo + hi));  // 2 + 2 e^{-4/3} u near x = 2
  } else {
    lo = 0.0;
    hi = 2.0;
    x = 2.0 / (1.0 - u);
  }
  for (int it = 0; it < 200; it++) {
    const double F = log(fabs(x - 2.0)) + x * (2.0 / 3.0) - log(x) - lu;
    if (sgn * F > 0.0) hi = x;
    else lo = x;
    const double dF = 1.0 / (x - 2.0) + 2.0 / 3.0 - 1.0 / x;
    double xn = x - F / dF;
    if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
    const bool done = fabs(xn - x) <= 2e-16 * xn || hi - lo <= 2e-16 * hi;
    x = xn;
    if (done) break;
  }
  return x;
}

/// Becke-Roussel 89 exchange of one spin channel as an energy per volume, (1/2) rho_s U_s with
///   U_s = -(1 - e^{-x} - x e^{-x}/2) / b,  b = x e^{-x/3} / (8 pi rho_s)^{1/3},
///   Q_s = (lapl_s - 2 gamma D_s)/6,  D_s = 2 tau_s - sigma_ss/(4 rho_s),  gamma = 0.8  (libxc mgga_x_br89 = 206).
/// x depends on the point through u alone: its derivatives come from dx/du = 1 / (d/dx [(x-2) e^{2x/3}/x]), not from the
/// iterations.
template <int N>
__host__ __device__ inline DN<N> br89_channel(const DN<N> &r, const DN<N> &s, const DN<N> &t, const DN<N> &l) {
  const double gam = 0.8, c23 = (2.0 / 3.0) * 2.1450293971110255;  // (2/3) pi^{2/3}
  DN<N> D = 2.0 * t - s / (4.0 * r);
  DN<N> Q = (l - (2.0 * gam) * D) / 6.0;
  DN<N> r13 = dncbrt(r);
  DN<N> u = Q / (c23 * r * r13 * r13);
  const double xv = br89_root(u.v);
  const double dk = exp(xv * (2.0 / 3.0)) * 2.0 * (xv * xv - 2.0 * xv + 3.0) / (3.0 * xv * xv);
  DN<N> x = dnf(u, xv, 1.0 / dk);
  // (1 - e^{-x} - x e^{-x}/2) e^{x/3} / x, with 1 - e^{-x} = -expm1(-x) (small x: the bracket is x/2 + O(x^3))
  DN<N> em = -1.0 * dnexpm1(-1.0 * x);
  DN<N> ex3 = dnexp(x / 3.0);
  DN<N> e23 = dnexp(x * (-2.0 / 3.0));
  DN<N> g = (ex3 * em - 0.5 * x * e23) / x;
  return (-0.5 * 2.9291837751230463) * r * r13 * g;  // (8 pi)^{1/3}
}

/// Colle-Salvetti correlation (Theor. Chim. Acta 37, 329 (1975)) in the form of Lee, Yang, Parr, PRB 37, 785 (1988), eq 1,
/// energy per volume, with t_HF = tau - lapl/8 and t_W = sigma/(8 rho) - lapl/8 (libxc mgga_c_cs = 72):
///   e = -a/(1 + d rho^{-1/3}) {rho + b rho^{-2/3} [t_HF - 2 t_W] e^{-c rho^{-1/3}}}.
/// Replacing t_HF by its second-order gradient expansion C_F rho^{5/3} + t_W/9 + lapl/18 gives the LYP integrand before the
/// integration by parts (their eq 3), which gga_c_lyp carries after it.
template <int N>
__host__ __device__ inline DN<N> cs_unpol(const DN<N> &r, const DN<N> &s, const DN<N> &t, const DN<N> &l) {
  DN<N> rm13 = 1.0 / dncbrt(r);
  DN<N> den = 1.0 + HFG_LYP_D * rm13;
  DN<N> thf = t - l / 8.0, tw = s / (8.0 * r) - l / 8.0;
  DN<N> br = HFG_LYP_B * rm13 * rm13 * (thf - 2.0 * tw) * dnexp((-HFG_LYP_C) * rm13);
  return (-HFG_LYP_A) * (r + br) / den;
}
/// spin-resolved form (LYP eq 11 before their gradient expansion), gamma = 2 [1 - (rho_a^2 + rho_b^2)/rho^2]:
///   e = -a gamma/(1 + d rho^{-1/3}) {rho + 2 b rho^{-5/3} [rho_a t_HF^a + rho_b t_HF^b - rho t_W] e^{-c rho^{-1/3}}},
///   t_HF^s = tau_s - lapl_s/8,  t_W = sigma/(8 rho) - lapl/8 of the total density
__host__ __device__ inline DN<9> cs_pol(const DN<9> &ra, const DN<9> &rb, const DN<9> &saa, const DN<9> &sab, const DN<9> &sbb,
                                        const DN<9> &ta, const DN<9> &tb, const DN<9> &la, const DN<9> &lb) {
  DN<9> n = ra + rb;
  DN<9> rm13 = 1.0 / dncbrt(n);
  DN<9> den = 1.0 + HFG_LYP_D * rm13;
  DN<9> gam = 4.0 * ra * rb / (n * n);
  DN<9> lt = la + lb;
  DN<9> tw = (saa + 2.0 * sab + sbb) / (8.0 * n) - lt / 8.0;
  DN<9> br = ra * (ta - la / 8.0) + rb * (tb - lb / 8.0) - n * tw;
  DN<9> rm53 = rm13 * rm13 * rm13 * rm13 * rm13;
  return (-HFG_LYP_A) * gam * (n + (2.0 * HFG_LYP_B) * rm53 * br * dnexp((-HFG_LYP_C) * rm13)) / den;
}

/// adds a Laplacian-dependent meta-GGA's exc, vrho, vsigma, vtau, vlapl at one point (rho >= threshold assumed); live as in
/// eval_add (the exchange channels carry rho/2 each)
__host__ __device__ inline void eval_add_mgga_lapl(int id, double rho, double sigma, double tau, double lapl, bool live, double &exc,
                                                   double &vrho, double &vsigma, double &vtau, double &vlapl) {
  if (id == 206 && !live) return;
  DN<4> r = dnvar<4>(rho, 0), s = dnvar<4>(sigma, 1), t = dnvar<4>(tau, 2), l = dnvar<4>(lapl, 3);
  DN<4> en;
  if (id == 206) en = 2.0 * br89_channel(0.5 * r, 0.25 * s, 0.5 * t, 0.5 * l);  // E_x[rho] = 2 e_x[rho/2]
  else if (id == 72) en = cs_unpol(r, s, t, l);
  else return;
  exc += en.v / rho;
  vrho += en.d[0];
  vsigma += en.d[1];
  vtau += en.d[2];
  vlapl += en.d[3];
}

/// spin-polarised: adds exc (per particle of ra + rb), v_rho[2], v_sigma[3], v_tau[2], v_lapl[2]; ra, rb already raised to
/// the threshold, live_a / live_b as in eval_add_mgga_pol.  BR89 is spin-resolved: E_x = sum_s e_x(channel s).
__host__ __device__ inline void eval_add_mgga_lapl_pol(int id, double ra, double rb, double saa, double sab, double sbb, double ta,
                                                       double tb, double la, double lb, bool live_a, bool live_b, double &exc,
                                                       double &va, double &vb, double &vsaa, double &vsab, double &vsbb,
                                                       double &vta, double &vtb, double &vla, double &vlb) {
  const double rt = ra + rb;
  if (id == 206) {
    DN<4> ea = dn<4>(0.0), eb = dn<4>(0.0);
    if (live_a) ea = br89_channel(dnvar<4>(ra, 0), dnvar<4>(saa, 1), dnvar<4>(ta, 2), dnvar<4>(la, 3));
    if (live_b) eb = br89_channel(dnvar<4>(rb, 0), dnvar<4>(sbb, 1), dnvar<4>(tb, 2), dnvar<4>(lb, 3));
    exc += (ea.v + eb.v) / rt;
    va += ea.d[0];
    vb += eb.d[0];
    vsaa += ea.d[1];
    vsbb += eb.d[1];
    vta += ea.d[2];
    vtb += eb.d[2];
    vla += ea.d[3];
    vlb += eb.d[3];
    return;
  }
  if (id != 72) return;
  DN<9> en = cs_pol(dnvar<9>(ra, 0), dnvar<9>(rb, 1), dnvar<9>(saa, 2), dnvar<9>(sab, 3), dnvar<9>(sbb, 4), dnvar<9>(ta, 5),
                    dnvar<9>(tb, 6), dnvar<9>(la, 7), dnvar<9>(lb, 8));
  exc += en.v / rt;
  va += en.d[0];
  vb += en.d[1];
  vsaa += en.d[2];
  vsab += en.d[3];
  vsbb += en.d[4];
  vta += en.d[5];
  vtb += en.d[6];
  vla += en.d[7];
  vlb += en.d[8];
}


}  // namespace xc
}  // namespace hfg

// One functional at one point through the evaluator its row names: the four-way chain, written once for the grid kernels and
// for xc_eval_host (fock.hip).  EXT_: whether eval_add_ext can be reached (the kernels' template argument; true on the host);
// without it an is_ext id falls through to evaluators that ignore it.  The arguments are those of the eval_add_* functions.
// Macros, not functions: through a function, always inlined or not, the compiler allocates the registers of k_xc_grid<false>
// and k_xc_grid_pol<false> differently (4 bytes more scratch), and these kernels are kept as they were, instruction by instruction.
#define HFG_XC_EVAL_POINT(EXT_, id, rho, sigma, tau, lapl, live, exc, vrho, vsig, vtau, vlap)                          \
  do {                                                                                                                 \
    if (EXT_ && xc::is_ext(id)) xc::eval_add_ext(id, rho, sigma, tau, live, exc, vrho, vsig, vtau);                    \
    else if (xc::is_mgga_lapl(id)) xc::eval_add_mgga_lapl(id, rho, sigma, tau, lapl, live, exc, vrho, vsig, vtau, vlap); \
    else if (xc::is_mgga(id)) xc::eval_add_mgga(id, rho, sigma, tau, live, exc, vrho, vsig, vtau);                     \
    else xc::eval_add(id, rho, sigma, live, exc, vrho, vsig);                                                          \
  } while (0)
#define HFG_XC_EVAL_POINT_POL(EXT_, id, ra, rb, saa, sab, sbb, ta, tb, la, lb, live_a, live_b, exc, va, vb, vsaa, vsab, vsbb, vta, vtb, \
                              vla, vlb)                                                                                \
  do {                                                                                                                 \
    if (EXT_ && xc::is_ext(id))                                                                                        \
      xc::eval_add_ext_pol(id, ra, rb, saa, sab, sbb, ta, tb, live_a, live_b, exc, va, vb, vsaa, vsab, vsbb, vta, vtb); \
    else if (xc::is_mgga_lapl(id))                                                                                     \
      xc::eval_add_mgga_lapl_pol(id, ra, rb, saa, sab, sbb, ta, tb, la, lb, live_a, live_b, exc, va, vb, vsaa, vsab, vsbb, vta, vtb, \
                                 vla, vlb);                                                                            \
    else if (xc::is_mgga(id))                                                                                          \
      xc::eval_add_mgga_pol(id, ra, rb, saa, sab, sbb, ta, tb, live_a, live_b, exc, va, vb, vsaa, vsab, vsbb, vta, vtb); \
    else xc::eval_add_pol(id, ra, rb, saa, sab, sbb, live_a, live_b, exc, va, vb, vsaa, vsab, vsbb);                   \
  } while (0)
