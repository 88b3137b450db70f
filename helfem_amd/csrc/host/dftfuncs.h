// Functional name / id handling of the drivers (reference: src/general/dftfuncs.cpp:64-118 parse_xc_func,
// :388-428 exact_exchange, :464-520 is_range_separated).  libxc is absent; the ids are libxc's and only the
// functionals of xc_funcs.h, the one list every answer here is looked up in, are accepted.
#pragma once
#include <string>

namespace helfem {
/// "HF" -> (-1,0); "none" -> (0,0); "x-c" keyword pair or numeric ids
void parse_xc_func(int &x_func, int &c_func, const std::string &method);
/// fraction of exact exchange: 1 for HF, the hybrids' fraction, 0 for the pure functionals available here
double exact_exchange(int x_func);
/// range separation of the exchange functional: omega, fraction alpha of full-range and beta of short-range exact
/// exchange (reference: range_separation, dftfuncs.cpp:505); omega = 0 for everything but the range-separated hybrids
void range_separation(int x_func, double &omega, double &alpha, double &beta);
/// which screened kernel the functional uses (reference: is_range_separated, dftfuncs.cpp:464)
void is_range_separated(int x_func, bool &erf, bool &yukawa);
/// the same as one number, as SCF options and hfg_compute_rs_tei take it: 0 none, 1 Yukawa, 2 erfc
int rs_kind(int x_func);
const char *xc_func_name(int func_id);
/// the functional depends on the density Laplacian (mgga_x_br89, mgga_c_cs): supported by the atomic program only
bool needs_laplacian(int func_id);
/// --x_pars / --c_pars: throws std::runtime_error unless the functional takes that many external parameters in that role (the
/// npar column of xc_funcs.h); n = 0 is always accepted
void check_xc_params(int x_func, int n_x_pars, int c_func, int n_c_pars);
/// one line per functional of xc_funcs.h, its columns in order (tab separated)
std::string xc_func_table();
}  // namespace helfem
