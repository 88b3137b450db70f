// `diatomic`: the command line of the reference's diatomic program (/root/reference/src/diatomic/main.cpp:87-1022) in front
// of the MI355X implementation of its SCF hot path.  Flags, defaults and the printed lines follow the reference; what the
// run itself prints (per-iteration energies, timings, the final energy table) comes from the driver behind hfg_scf_run.
// Options of features outside the hot-path scope are parsed and refused with a message when they are set.
#include "../../../include/helfem_gpu.h"
#include "options.h"
#include <cstring>
#include <sstream>


static void fail(const std::string &msg) {
  fprintf(stderr, "%s", msg.c_str());
  if (msg.empty() || msg.back() != '\n') fprintf(stderr, "\n");
  exit(1);
}

int main(int argc, char **argv) {
  cli::Parser parser;
  parser.add("Z1", "first nuclear charge", true);
  parser.add("Z2", "second nuclear charge", true);
  parser.add("Rbond", "internuclear distance", true);
  parser.add("angstrom", "input distances in angstrom", false, "0", true);
  parser.add("nela", "number of alpha electrons", false, "0");
  parser.add("nelb", "number of beta  electrons", false, "0");
  parser.add("Q", "charge state", false, "0");
  parser.add("M", "spin multiplicity", false, "0");
  parser.add("lmax", "maximum l quantum number", true);
  parser.add("mmax", "maximum m quantum number", false, "-1");
  parser.add("lpad", "padding for max l for more accurate Qlm recursion", false, "10");
  parser.add("Rmax", "practical infinity in au", false, "40.0");
  parser.add("grid", "type of grid: 1 for linear, 2 for quadratic, 3 for polynomial, 4 for exponential", false, "4");
  parser.add("zexp", "parameter in radial grid", false, "1.0");
  parser.add("nelem", "number of elements", true);
  parser.add("nnodes", "number of nodes per element", false, "15");
  parser.add("nquad", "number of quadrature points", false, "0");
  parser.add("maxit", "maximum number of iterations", false, "50");
  parser.add("convthr", "convergence threshold", false, "1e-7");
  parser.add("Ez", "electric dipole field", false, "0.0");
  parser.add("Qzz", "electric quadrupole field", false, "0.0");
  parser.add("Bz", "magnetic dipole field", false, "0.0");
  parser.add("diag", "exact diagonalization", false, "1", true);
  parser.add("finitenuc", "finite nuclear model", false, "0");
  parser.add("Rrms1", "nucleus 1 radius", false, "0.0");
  parser.add("Rrms2", "nucleus 2 radius", false, "0.0");
  parser.add("method", "method to use", false, "HF");
  parser.add("ldft", "theta rule for dft quadrature (0 for auto)", false, "0");
  parser.add("mdft", "phi rule for dft quadrature (0 for auto)", false, "0");
  parser.add("dftthr", "density threshold for dft", false, "1e-12");
  parser.add("restricted", "spin-restricted orbitals", false, "-1");
  parser.add("symmetry", "force orbital symmetry", false, "1");
  parser.add("primbas", "primitive radial basis", false, "4");
  parser.add("diiseps", "when to start mixing in diis", false, "1e-2");
  parser.add("diisthr", "when to switch over fully to diis", false, "1e-3");
  parser.add("diisorder", "length of diis history", false, "5");
  parser.add("readocc", "read occupations from file, use until nth build", false, "0");
  parser.add("perturb", "randomly perturb initial guess", false, "0.0");
  parser.add("seed", "seed for random perturbation", false, "0");
  // the reference's default guess is 2 (superposition of atomic potentials), a 30 000-line data table of its tree that is
  // outside this build's scope: the default here is the core guess, and --iguess 2 says why it is unavailable
  parser.add("iguess", "guess: 0 for core, 1 for GSZ, 2 for SAP, 3 for TF", false, "0");
  parser.add("load", "load guess from checkpoint", false, "");
  parser.add("save", "save calculation to checkpoint", false, "helfem.chk");
  parser.add("x_pars", "file for parameters for exchange functional", false, "");
  parser.add("c_pars", "file for parameters for correlation functional", false, "");
  parser.add("maverage", "average Fock matrix over m values", false, "0", true);
  parser.add("device", "HIP device to run on", false, "0");
  parser.parse_check(argc, argv);

  try {
    hfg_scf_options o;
    hfg_scf_options_default(&o, 0);
    o.Z1 = hfg_get_Z(parser.str("Z1").c_str());
    o.Z2 = hfg_get_Z(parser.str("Z2").c_str());
    if (o.Z1 < 0 || o.Z2 < 0) fail(hfg_last_error());
    o.Rbond = parser.real("Rbond");
    if (parser.boolean("angstrom")) o.Rbond *= ANGSTROMINBOHR;
    o.nela = parser.integer("nela");
    o.nelb = parser.integer("nelb");
    o.Q = parser.integer("Q");
    o.M = parser.integer("M");
    // --lmax: one value with --mmax, or a comma-separated list of l_max per |m| (main.cpp:253-268)
    const int mmax = parser.integer("mmax");
    const std::string lmax = parser.str("lmax");
    o.nlm = 0;
    if (mmax >= 0) {
      if (mmax + 1 > HFG_MAX_LMMAX) fail("--mmax is too large for this build\n");
      for (int m = 0; m <= mmax; m++) o.lmmax[o.nlm++] = cli::Parser::to_int("lmax", lmax);
    } else {
      std::stringstream ss(lmax);
      std::string item;
      while (std::getline(ss, item, ',')) {
        if (o.nlm == HFG_MAX_LMMAX) fail("too many entries in --lmax for this build\n");
        o.lmmax[o.nlm++] = cli::Parser::to_int("lmax", item);
      }
    }
    o.lpad = parser.integer("lpad");
    o.Rmax = parser.real("Rmax");
    o.grid = parser.integer("grid");
    o.zexp = parser.real("zexp");
    o.nelem = parser.integer("nelem");
    o.nnodes = parser.integer("nnodes");
    o.nquad = parser.integer("nquad");
    o.maxit = parser.integer("maxit");
    o.convthr = parser.real("convthr");
    o.Ez = parser.real("Ez");
    o.Qzz = parser.real("Qzz");
    o.Bz = parser.real("Bz");
    o.diag = parser.boolean("diag") ? 1 : 0;
    o.finitenuc = parser.integer("finitenuc");
    snprintf(o.method, sizeof(o.method), "%s", parser.str("method").c_str());
    o.ldft = parser.integer("ldft");
    o.mdft = parser.integer("mdft");
    o.dftthr = parser.real("dftthr");
    o.restricted = parser.integer("restricted");
    o.symmetry = parser.integer("symmetry");
    o.primbas = parser.integer("primbas");
    o.diiseps = parser.real("diiseps");
    o.diisthr = parser.real("diisthr");
    o.diisorder = parser.integer("diisorder");
    o.readocc = parser.integer("readocc");
    static std::vector<int> occ_table;  // occs.dat of the working directory (main.cpp: occs.load("occs.dat", arma::raw_ascii))
    if (o.readocc) {
      int rows = 0, cols = 0;
      if (!cli::read_int_table("occs.dat", occ_table, rows, cols)) fail("Could not read occupation data from occs.dat\n");
      o.occs = occ_table.data();
      o.occ_rows = rows;
      o.occ_cols = cols;
    }
    o.perturb = parser.real("perturb");
    o.iguess = parser.integer("iguess");
    snprintf(o.load, sizeof(o.load), "%s", parser.str("load").c_str());
    // With --load the reference switches on --iguess (main.cpp:552-648): its default 2 (and any value but 0) projects the
    // stored ORBITALS onto the new basis, which is what this build does; an explicit --iguess 0 projects the stored FOCK
    // matrices through the old S^-1/2 instead.  That branch is not built: refuse rather than run another guess silently.
    if (o.load[0] && parser.given("iguess") && o.iguess == 0)
      fail("--iguess 0 with --load (projection of the stored Fock matrix) is not available in this build; omit --iguess to project the stored orbitals\n");
    snprintf(o.save, sizeof(o.save), "%s", parser.str("save").c_str());
    o.maverage = parser.boolean("maverage") ? 1 : 0;
    double xp[64], cp[64];
    int nx = 64, nc = 64;
    if (hfg_parse_xc_params(parser.str("x_pars").c_str(), xp, &nx)) fail(hfg_last_error());
    if (hfg_parse_xc_params(parser.str("c_pars").c_str(), cp, &nc)) fail(hfg_last_error());
    o.x_pars = nx ? xp : nullptr;
    o.n_x_pars = nx;
    o.c_pars = nc ? cp : nullptr;
    o.n_c_pars = nc;
    o.verbose = 1;

    const int restr = (o.restricted == -1) ? -1 : o.restricted;
    printf("Running %s %s calculation with Rmax=%e and %i elements.\n", restr == 0 ? "unrestricted" : (restr == 1 ? "restricted" : "restricted/unrestricted (by occupations)"),
           o.method, o.Rmax, o.nelem);
    printf("Using %i point quadrature rule.\n", o.nquad ? o.nquad : 5 * o.nnodes);
    printf("Left- and right-hand nuclear charges are %i and %i at distance % .3f\n", o.Z1, o.Z2, o.Rbond);
    printf("Nuclear repulsion energy is %e\n", o.Z1 * o.Z2 / o.Rbond);
    fflush(stdout);

    if (hfg_scf_options_check(&o)) fail(hfg_last_error());
    hfg_ctx *ctx = nullptr;
    if (hfg_ctx_create(&ctx, parser.integer("device"), nullptr)) fail(hfg_last_error());
    hfg_scf_result r;
    int rc = hfg_scf_run(ctx, &o, &r, nullptr, nullptr);
    if (rc) {
      std::string msg = hfg_last_error();
      hfg_ctx_destroy(ctx);
      fail(msg);
    }
    printf("Number of electrons is %i %i\n", r.nela, r.nelb);
    printf("%s after %i iterations\n", r.converged ? "Converged" : "NOT converged", r.iterations);
    if (o.save[0]) printf("Checkpoint written to %s\n", o.save);
    hfg_ctx_destroy(ctx);
    return 0;  // like the reference, which prints its energy table and returns 0 whether or not the SCF converged (main.cpp:1096)
  } catch (const std::exception &e) {
    fail(e.what());
  }
  return 1;
}
