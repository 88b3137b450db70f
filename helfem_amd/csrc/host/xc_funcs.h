// The exchange-correlation functionals of this build: one list, from which the name <-> id lookups and the hybrid / range
// separation / parameter queries of dftfuncs.cpp, the id predicates of the point code (hip/xc_device.h), the launch plan and
// the parameter mapping of hip/fock.hip and the table that hfg_xc_func_table() prints are generated (the lists of README.md and
// INTEGRATION.md are written from that output).  Plain C++: included by host and device translation units alike.
// To add a functional: one row here, its point code in hip/xc_device.h, its tests.
#pragma once
#include <cstddef>

// gga_x_ityh_pbe / gga_x_sfat_pbe: the integer ids are libxc's as recalled, not confirmed against libxc itself; the names are
// the interface
#define HFG_ID_ITYH_PBE 623
#define HFG_ID_SFAT_PBE 601

// X(id, name, role, grad, tau, lapl, ext, skip_dead, kfrac, kshort, omega, rs_kind, npar, pars, remark)
//   id, name   libxc's
//   role       "x" exchange, "c" correlation, "xc" both in one id
//   grad, tau, lapl   the inputs the point code reads beside rho: sigma, tau, the Laplacian (the launch plan computes the planes
//              of exactly these; a functional returns zero derivatives for the others)
//   ext        evaluated by eval_add_ext / eval_add_ext_pol alone, which the grid kernels call only in their EXT instantiation:
//              0 no; 1 SCAN and the PBE variants; 2 a short-range GGA exchange primitive; 3 a range-separated GGA hybrid
//   skip_dead  skipped as a whole by the common early return of eval_add / eval_add_ext when a spin channel, rho/2, is below the
//              density threshold.  NOT "role is exchange": mgga_x_br89 and the short-range primitives leave the channel out in
//              their own code, and a hybrid keeps its correlation part there.
//   kfrac, kshort, omega, rs_kind   what the drivers add: kfrac K[1/r12] + kshort K[screened kernel of omega], the kernel being
//              0 none, 1 Yukawa exp(-omega r)/r, 2 erfc(omega r)/r.  A CAM hybrid 1/r = [1 - a - b s(r)]/r + [a + b s(r)]/r has
//              kfrac = a + b, kshort = -b.
//   npar, pars external parameters (libxc's xc_func_set_ext_params): how many, and the XCPar fields they fill, in order
//   remark     composition of a hybrid, restrictions, doubts
#define HELFEM_XC_FUNCS(X) \
  X(1, "lda_x", "x", false, false, false, 0, true, 0.0, 0.0, 0.0, 0, 1, "x_alpha", "") \
  X(7, "lda_c_vwn", "c", false, false, false, 0, false, 0.0, 0.0, 0.0, 0, 0, "", "") \
  X(8, "lda_c_vwn_rpa", "c", false, false, false, 0, false, 0.0, 0.0, 0.0, 0, 0, "", "") \
  X(12, "lda_c_pw", "c", false, false, false, 0, false, 0.0, 0.0, 0.0, 0, 0, "", "") \
  X(13, "lda_c_pw_mod", "c", false, false, false, 0, false, 0.0, 0.0, 0.0, 0, 0, "", "") \
  X(101, "gga_x_pbe", "x", true, false, false, 0, true, 0.0, 0.0, 0.0, 0, 2, "x_kappa,x_mu", "") \
  X(130, "gga_c_pbe", "c", true, false, false, 0, false, 0.0, 0.0, 0.0, 0, 3, "c_beta,c_gamma,c_BB", "") \
  X(106, "gga_x_b88", "x", true, false, false, 0, true, 0.0, 0.0, 0.0, 0, 0, "", "") \
  X(131, "gga_c_lyp", "c", true, false, false, 0, false, 0.0, 0.0, 0.0, 0, 0, "", "") \
  X(402, "hyb_gga_xc_b3lyp", "xc", true, false, false, 0, false, 0.20, 0.0, 0.0, 0, 0, "", "0.08 lda_x + 0.72 gga_x_b88 + 0.19 lda_c_vwn_rpa + 0.81 gga_c_lyp + 0.20 exact exchange") \
  X(406, "hyb_gga_xc_pbeh", "xc", true, false, false, 0, false, 0.25, 0.0, 0.0, 0, 0, "", "PBE0: 0.75 gga_x_pbe + gga_c_pbe + 0.25 exact exchange") \
  X(202, "mgga_x_tpss", "x", true, true, false, 0, true, 0.0, 0.0, 0.0, 0, 0, "", "") \
  X(231, "mgga_c_tpss", "c", true, true, false, 0, false, 0.0, 0.0, 0.0, 0, 0, "", "") \
  X(546, "lda_x_erf", "x", false, false, false, 0, true, 0.0, 0.0, 0.0, 0, 0, "", "short-range LDA exchange, erfc kernel, omega 0.3") \
  X(641, "lda_x_yukawa", "x", false, false, false, 0, true, 0.0, 0.0, 0.0, 0, 0, "", "short-range LDA exchange, Yukawa kernel, omega 0.3") \
  X(178, "hyb_lda_xc_cam_lda0", "xc", false, false, false, 0, false, 0.5, -0.25, 1.0 / 3.0, 2, 0, "", "atomic program only; CAM-LDA0: spin-scaled exchange mixture + lda_c_pw_mod") \
  X(206, "mgga_x_br89", "x", true, true, true, 0, false, 0.0, 0.0, 0.0, 0, 0, "", "Laplacian-dependent: atomic program only") \
  X(72, "mgga_c_cs", "c", true, true, true, 0, false, 0.0, 0.0, 0.0, 0, 0, "", "Laplacian-dependent: atomic program only") \
  X(263, "mgga_x_scan", "x", true, true, false, 1, true, 0.0, 0.0, 0.0, 0, 0, "", "") \
  X(267, "mgga_c_scan", "c", true, true, false, 1, false, 0.0, 0.0, 0.0, 0, 0, "", "") \
  X(264, "hyb_mgga_x_scan0", "x", true, true, false, 1, true, 0.25, 0.0, 0.0, 0, 0, "", "0.75 mgga_x_scan + 0.25 exact exchange") \
  X(116, "gga_x_pbe_sol", "x", true, false, false, 1, true, 0.0, 0.0, 0.0, 0, 0, "", "PBEsol exchange") \
  X(133, "gga_c_pbe_sol", "c", true, false, false, 1, false, 0.0, 0.0, 0.0, 0, 0, "", "PBEsol correlation") \
  X(102, "gga_x_pbe_r", "x", true, false, false, 1, true, 0.0, 0.0, 0.0, 0, 0, "", "revPBE exchange") \
  X(529, "gga_x_ityh", "x", true, false, false, 2, false, 0.0, 0.0, 0.0, 0, 1, "x_omega", "short-range B88 exchange, erfc kernel, omega 0.2") \
  X(530, "gga_x_sfat", "x", true, false, false, 2, false, 0.0, 0.0, 0.0, 0, 1, "x_omega", "short-range B88 exchange, Yukawa kernel, omega 0.44") \
  X(HFG_ID_ITYH_PBE, "gga_x_ityh_pbe", "x", true, false, false, 2, false, 0.0, 0.0, 0.0, 0, 1, "x_omega", "short-range PBE exchange, erfc kernel, omega 0.2; id unconfirmed against libxc") \
  X(HFG_ID_SFAT_PBE, "gga_x_sfat_pbe", "x", true, false, false, 2, false, 0.0, 0.0, 0.0, 0, 1, "x_omega", "short-range PBE exchange, Yukawa kernel, omega 0.44; id unconfirmed against libxc") \
  X(433, "hyb_gga_xc_cam_b3lyp", "xc", true, false, false, 3, false, 0.19 + 0.46, -0.46, 0.33, 2, 0, "", "atomic program only; 0.35 gga_x_b88 + 0.46 gga_x_ityh + 0.19 lda_c_vwn + 0.81 gga_c_lyp") \
  X(470, "hyb_gga_xc_camy_b3lyp", "xc", true, false, false, 3, false, 0.19 + 0.46, -0.46, 0.34, 1, 0, "", "atomic program only; 0.35 gga_x_b88 + 0.46 gga_x_sfat + 0.19 lda_c_vwn + 0.81 gga_c_lyp") \
  X(455, "hyb_gga_xc_camy_blyp", "xc", true, false, false, 3, false, 0.20 + 0.80, -0.80, 0.44, 1, 0, "", "atomic program only; 0.80 gga_x_sfat + gga_c_lyp") \
  X(468, "hyb_gga_xc_lcy_blyp", "xc", true, false, false, 3, false, 0.0 + 1.0, -1.0, 0.75, 1, 0, "", "atomic program only; gga_x_sfat + gga_c_lyp") \
  X(467, "hyb_gga_xc_lcy_pbe", "xc", true, false, false, 3, false, 0.0 + 1.0, -1.0, 0.75, 1, 0, "", "atomic program only; gga_x_sfat_pbe + gga_c_pbe")

namespace helfem {
struct XCFunc {
  int id;
  const char *name, *role;
  bool grad, tau, lapl;
  int ext;
  bool skip_dead;
  double kfrac, kshort, omega;
  int rs_kind, npar;
  const char *pars, *remark;
};
#define X(...) {__VA_ARGS__},
constexpr XCFunc xc_funcs[] = {HELFEM_XC_FUNCS(X)};
#undef X
/// the row of an id, NULL for an id that is not in the list (0 "none" and -1 "HF" are not functionals)
inline const XCFunc *find_xc_func(int id) {
  for (const XCFunc &f : xc_funcs)
    if (f.id == id) return &f;
  return nullptr;
}
}  // namespace helfem
