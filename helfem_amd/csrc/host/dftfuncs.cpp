#include "dftfuncs.h"
#include "xc_funcs.h"
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <stdexcept>
#include <strings.h>

namespace helfem {

namespace {
int find_func(const std::string &name) {
  if (name.empty()) throw std::runtime_error("empty functional name\n");
  if (isdigit(name[0])) return atoi(name.c_str());
  if (!strcasecmp(name.c_str(), "none")) return 0;
  if (!strcasecmp(name.c_str(), "hyb_x_hf") || !strcasecmp(name.c_str(), "HF")) return -1;
  for (const XCFunc &f : xc_funcs)
    if (!strcasecmp(name.c_str(), f.name)) return f.id;
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

// fraction of exact exchange (libxc xc_hyb_exx_coef; dftfuncs.cpp:134-160 of the reference); for the range-separated
// hybrids the full-range coefficient the drivers use, alpha + beta
double exact_exchange(int x_func) {
  if (const XCFunc *f = find_xc_func(x_func)) return f->kfrac;
  return x_func == -1 ? 1.0 : 0.0;
}

// libxc's xc_hyb_cam_coef / hyb_type of the range-separated hybrids available here (dftfuncs.cpp:464-570 of the
// reference): K = alpha K[1/r12] + beta K[screened kernel]
void range_separation(int x_func, double &omega, double &alpha, double &beta) {
  const XCFunc *f = find_xc_func(x_func);
  omega = f ? f->omega : 0.0;
  alpha = exact_exchange(x_func);
  beta = f ? f->kshort : 0.0;
}
int rs_kind(int x_func) {
  const XCFunc *f = find_xc_func(x_func);
  return f ? f->rs_kind : 0;
}
void is_range_separated(int x_func, bool &erf, bool &yukawa) {
  erf = rs_kind(x_func) == 2;
  yukawa = rs_kind(x_func) == 1;
}

bool needs_laplacian(int id) {
  const XCFunc *f = find_xc_func(id);
  return f && f->lapl;
}

void check_xc_params(int x_func, int nx, int c_func, int nc) {
  auto takes = [](int id, const char *role, int n) {
    const XCFunc *f = find_xc_func(id);
    return f && !strcmp(f->role, role) && f->npar == n;
  };
  if (nx > 0 && !takes(x_func, "x", nx))
    throw std::runtime_error("External parameters are not supported for exchange functional " + std::to_string(x_func) + " with " +
                             std::to_string(nx) + " values (supported: lda_x {alpha}, gga_x_pbe {kappa, mu}, gga_x_ityh / gga_x_sfat"
                             " / gga_x_ityh_pbe / gga_x_sfat_pbe {omega}).\n");
  if (nc > 0 && !takes(c_func, "c", nc))
    throw std::runtime_error("External parameters are not supported for correlation functional " + std::to_string(c_func) + " with " +
                             std::to_string(nc) + " values (supported: gga_c_pbe {beta, gamma, BB}).\n");
}

const char *xc_func_name(int id) {
  switch (id) {
    case -1: return "HF";
    case 0: return "none";
  }
  const XCFunc *f = find_xc_func(id);
  return f ? f->name : "unknown";
}

std::string xc_func_table() {
  std::string s;
  char num[96];
  for (const XCFunc &f : xc_funcs) {
    s += std::to_string(f.id) + "\t" + f.name + "\t" + f.role + "\t" + std::to_string(f.grad) + "\t" + std::to_string(f.tau) + "\t" +
         std::to_string(f.lapl) + "\t" + std::to_string(f.ext) + "\t" + std::to_string(f.skip_dead) + "\t";
    snprintf(num, sizeof num, "%.17g\t%.17g\t%.17g\t", f.kfrac, f.kshort, f.omega);
    s += num + std::to_string(f.rs_kind) + "\t" + std::to_string(f.npar) + "\t" + f.pars + "\t" + f.remark + "\n";
  }
  return s;
}

}  // namespace helfem
