#include "dftfuncs.h"
#include <cctype>
#include <cstdlib>
#include <sstream>
#include <stdexcept>
#include <strings.h>

namespace helfem {

namespace {
struct Known {
  const char *name;
  int id;
};
const Known known[] = {{"lda_x", 1}, {"lda_c_vwn", 7}, {"lda_c_vwn_rpa", 8}, {"lda_c_pw", 12}, {"lda_c_pw_mod", 13},
                       {"gga_x_pbe", 101}, {"gga_c_pbe", 130}, {"gga_x_b88", 106}, {"gga_c_lyp", 131},
                       {"hyb_gga_xc_b3lyp", 402},  // 0.08 lda_x + 0.72 gga_x_b88 + 0.19 lda_c_vwn_rpa + 0.81 gga_c_lyp + 0.20 exact exchange
                       {"hyb_gga_xc_pbeh", 406},  // PBE0: 0.75 gga_x_pbe + gga_c_pbe + 0.25 exact exchange
                       {"mgga_x_tpss", 202}, {"mgga_c_tpss", 231}, {"lda_x_erf", 546}, {"lda_x_yukawa", 641},
                       {"hyb_lda_xc_cam_lda0", 178},  // CAM-LDA0: erfc range separation, omega = 1/3
                       {"mgga_x_br89", 206}, {"mgga_c_cs", 72},  // Laplacian-dependent: atomic program only
                       {"mgga_x_scan", 263}, {"mgga_c_scan", 267},
                       {"hyb_mgga_x_scan0", 264},  // 0.75 mgga_x_scan + 0.25 exact exchange
                       {"gga_x_pbe_sol", 116}, {"gga_c_pbe_sol", 133}, {"gga_x_pbe_r", 102},  // PBEsol, revPBE exchange
                       // short-range GGA exchange, omega an external parameter (B88 / PBE enhancement, erfc / Yukawa kernel)
                       {"gga_x_ityh", 529}, {"gga_x_sfat", 530},
                       {"gga_x_ityh_pbe", 623}, {"gga_x_sfat_pbe", 601},  // ids as recalled, not confirmed against libxc
                       {"hyb_gga_xc_cam_b3lyp", 433},   // erfc, omega 0.33: 0.35 B88 + 0.46 ITYH + 0.19 VWN5 + 0.81 LYP
                       {"hyb_gga_xc_camy_b3lyp", 470},  // Yukawa, omega 0.34: 0.35 B88 + 0.46 SFAT + 0.19 VWN5 + 0.81 LYP
                       {"hyb_gga_xc_camy_blyp", 455},   // Yukawa, omega 0.44: 0.80 SFAT + LYP
                       {"hyb_gga_xc_lcy_blyp", 468},    // Yukawa, omega 0.75: SFAT + LYP
                       {"hyb_gga_xc_lcy_pbe", 467}};    // Yukawa, omega 0.75: SFAT-PBE + PBE correlation

int find_func(const std::string &name) {
  if (name.empty()) throw std::runtime_error("empty functional name\n");
  if (isdigit(name[0])) return atoi(name.c_str());
  if (!strcasecmp(name.c_str(), "none")) return 0;
  if (!strcasecmp(name.c_str(), "hyb_x_hf") || !strcasecmp(name.c_str(), "HF")) return -1;
  for (const Known &k : known)
    if (!strcasecmp(name.c_str(), k.name)) return k.id;
  std::ostringstream oss;
  oss << "\nError: functional " << name << " is not available in this build!\n";
  throw std::runtime_error(oss.str());
}
}  // namespace

void parse_xc_func(int &x_func, int &c_func, const std::string &xc) {
  x_func = 0;
  c_func = 0;
  size_t dpos = xc.find('-', 0);
  if (dpos != std::string::npos) {
    x_func = find_func(xc.substr(0, dpos));
    c_func = find_func(xc.substr(dpos + 1));
  } else
    x_func = find_func(xc);
}

namespace {
// CAM split 1/r = [1 - alpha - beta s(r)]/r + [alpha + beta s(r)]/r, s = erf(omega r) or 1 - exp(-omega r)
struct Cam {
  int id;
  bool yukawa;
  double alpha, beta, omega;
};
const Cam cam[] = {{433, false, 0.19, 0.46, 0.33}, {470, true, 0.19, 0.46, 0.34}, {455, true, 0.20, 0.80, 0.44},
                   {468, true, 0.0, 1.0, 0.75}, {467, true, 0.0, 1.0, 0.75}};
const Cam *find_cam(int id) {
  for (const Cam &c : cam)
    if (c.id == id) return &c;
  return nullptr;
}
}  // namespace

// fraction of exact exchange (libxc xc_hyb_exx_coef; dftfuncs.cpp:134-160 of the reference); for the range-separated
// hybrids the full-range coefficient the drivers use, alpha + beta
double exact_exchange(int x_func) {
  if (const Cam *c = find_cam(x_func)) return c->alpha + c->beta;
  return x_func == -1 ? 1.0 : ((x_func == 406 || x_func == 264) ? 0.25 : (x_func == 402 ? 0.20 : (x_func == 178 ? 0.5 : 0.0)));
}

// libxc's xc_hyb_cam_coef / hyb_type of the range-separated hybrids available here (dftfuncs.cpp:464-570 of the
// reference): K = alpha K[1/r12] + beta K[screened kernel]
void range_separation(int x_func, double &omega, double &alpha, double &beta) {
  omega = 0.0;
  alpha = exact_exchange(x_func);
  beta = 0.0;
  if (x_func == 178) {  // hyb_lda_xc_cam_lda0
    omega = 1.0 / 3.0;
    alpha = 0.5;
    beta = -0.25;
  } else if (const Cam *c = find_cam(x_func)) {  // kfrac = alpha + beta over the full range, kshort = -beta of the screened kernel
    omega = c->omega;
    beta = -c->beta;
  }
}
void is_range_separated(int x_func, bool &erf, bool &yukawa) {
  const Cam *c = find_cam(x_func);
  erf = (x_func == 178) || (c && !c->yukawa);
  yukawa = c && c->yukawa;
}

bool needs_laplacian(int id) { return id == 206 || id == 72; }

void check_xc_params(int x_func, int nx, int c_func, int nc) {
  const bool sr_gga = x_func == 529 || x_func == 530 || x_func == 623 || x_func == 601;  // {omega}
  if (nx > 0 && !((x_func == 1 && nx == 1) || (x_func == 101 && nx == 2) || (sr_gga && nx == 1)))
    throw std::runtime_error("External parameters are not supported for exchange functional " + std::to_string(x_func) + " with " +
                             std::to_string(nx) + " values (supported: lda_x {alpha}, gga_x_pbe {kappa, mu}, gga_x_ityh / gga_x_sfat"
                             " / gga_x_ityh_pbe / gga_x_sfat_pbe {omega}).\n");
  if (nc > 0 && !(c_func == 130 && nc == 3))
    throw std::runtime_error("External parameters are not supported for correlation functional " + std::to_string(c_func) + " with " +
                             std::to_string(nc) + " values (supported: gga_c_pbe {beta, gamma, BB}).\n");
}

const char *xc_func_name(int id) {
  if (id == -1) return "HF";
  if (id == 0) return "none";
  for (const Known &k : known)
    if (k.id == id) return k.name;
  return "unknown";
}

}  // namespace helfem
