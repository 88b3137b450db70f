#include "atomic_basis.h"
#include "diatomic_basis.h"  // exchange_tei
#include "parallel.h"
#include <algorithm>
#include <cmath>

namespace helfem {
namespace atomic {

void angular_basis(int lmax, int mmax, IVec &lval, IVec &mval) {
  lval.clear();
  mval.clear();
  for (int mabs = 0; mabs <= mmax; mabs++)
    for (int l = mabs; l <= lmax; l++) {
      lval.push_back(l);
      mval.push_back(mabs);
      if (mabs > 0) {
        lval.push_back(l);
        mval.push_back(-mabs);
      }
    }
}

TwoDBasis::TwoDBasis(int Z_, int nnodes_, int n_quad, const Vec &bval, const IVec &lval_, const IVec &mval_)
    : Z(Z_), nnodes(nnodes_), lval(lval_), mval(mval_) {
  if (nnodes < 2) throw std::logic_error("Can't have finite element basis with less than two nodes per element.\n");
  if (bval.empty() || bval[0] != 0.0) throw std::logic_error("radial grid must start from zero\n");
  LIPBasis poly(lobatto_nodes(nnodes));
  // functions vanish at the nucleus (u = r R(r)) and at the practical infinity (TwoDBasis.cpp:48-52)
  fem = FEMBasis(poly, bval, true, true);
  chebyshev_rule(n_quad, xq, wq);
}

TwoDBasis::TwoDBasis(int Z_, int finitenuc_, double Rrms_, bool zeroder_, int nnodes_, int n_quad, const Vec &bval,
                     const IVec &lval_, const IVec &mval_, int Zl_, int Zr_, double Rhalf_)
    : TwoDBasis(Z_, nnodes_, n_quad, bval, lval_, mval_) {
  finitenuc = finitenuc_;
  Rrms = Rrms_;
  zeroder = zeroder_;
  Zl = Zl_;
  Zr = Zr_;
  Rhalf = Rhalf_;
  if (finitenuc != POINT_NUCLEUS && finitenuc != REGULARIZED_NUCLEUS) nuclear_model(finitenuc, Z, Rrms);  // refuses unknown models here
  if (zeroder) fem = FEMBasis(fem.poly, bval, true, false);
}

// Regularized nucleus (Gygi, J. Chem. Theory Comput. 19, 1300 (2023)): the potential whose exact 1s state of a unit charge is
// phi(r) = exp(h(r)) / sqrt(pi), h(r) = -r erf(a r) - b exp(-a^2 r^2); b makes phi normalised.  From (-1/2 Lap + V) phi =
// -phi/2:  V = -1/2 + (h'' + h'^2)/2 + h'/r, and for a charge Z, V_Z(r) = Z^2 V(Z r).
namespace {
struct Regularized {
  double a = 1.0, b = 0.0;
  // erf(a r)/r, by its series where the quotient would lose digits
  double erf_over_r(double r) const {
    const double x = a * r;
    if (x < 1e-2) {
      const double x2 = x * x;
      return a * M_2_SQRTPI * (1.0 + x2 * (-1.0 / 3.0 + x2 * (1.0 / 10.0 + x2 * (-1.0 / 42.0 + x2 / 216.0))));
    }
    return std::erf(x) / r;
  }
  double h(double r) const { return -r * std::erf(a * r) - b * std::exp(-a * a * r * r); }
  double V(double r) const {
    const double g = std::exp(-a * a * r * r), c = a * M_2_SQRTPI;
    const double h1_over_r = -erf_over_r(r) - c * g + 2.0 * a * a * b * g;
    const double h1 = h1_over_r * r;
    const double h2 = -2.0 * c * g + 2.0 * c * a * a * r * r * g + 2.0 * a * a * b * g - 4.0 * a * a * a * a * b * r * r * g;
    return -0.5 + 0.5 * (h2 + h1 * h1) + h1_over_r;
  }
  // 4 int r^2 exp(2 h) dr - 1 on panels that resolve both the Gaussian core (1/a) and the exponential tail
  double norm_defect(double bb, const Vec &x, const Vec &w) {
    b = bb;
    const double core = 8.0 / a;
    double sum = 0.0;
    for (int part = 0; part < 2; part++) {
      const int npanel = 64;
      const double lo = part ? core : 0.0, len = (part ? 60.0 : core) / npanel;
      for (int ip = 0; ip < npanel; ip++)
        for (size_t q = 0; q < x.size(); q++) {
          const double r = lo + (ip + 0.5 + 0.5 * x[q]) * len;
          sum += 0.5 * len * w[q] * r * r * std::exp(2.0 * h(r));
        }
    }
    return 4.0 * sum - 1.0;
  }
  explicit Regularized(double a_) : a(a_) {
    if (!(a > 0.0)) throw std::logic_error("The regularized nucleus needs a positive parameter a (--Rrms).\n");
    Vec x, w;
    chebyshev_rule(40, x, w);
    double lo = -40.0, hi = 40.0;  // the defect falls monotonically with b
    for (int it = 0; it < 200 && hi - lo > 1e-15 * std::max(1.0, std::fabs(lo)); it++) {
      const double mid = 0.5 * (lo + hi);
      (norm_defect(mid, x, w) > 0.0 ? lo : hi) = mid;
    }
    b = 0.5 * (lo + hi);
  }
};
}  // namespace

std::function<double(double)> nuclear_model(int model, int Z, double Rrms, bool verbose) {
  switch (model) {
    case POINT_NUCLEUS:
      if (verbose) printf("Getting point nucleus with Z=%i\n", Z);
      return [Z](double r) { return -Z / r; };
    case GAUSSIAN_NUCLEUS: {
      if (verbose) printf("Getting Gaussian nucleus with Z=%i Rrms=%e\n", Z, Rrms);
      // -Z erf(mu r)/r with mu = sqrt(3/2)/Rrms (Visscher and Dyall 1997, eq. 11); series below the radius where its
      // first neglected term reaches the rounding error
      const double mu = std::sqrt(1.5) / Rrms;
      const double Rcut = std::pow(42.0 * 2.220446049250313e-16, 1.0 / 6.0) / mu;
      return [Z, mu, Rcut](double r) {
        if (r <= Rcut) {
          const double x2 = (mu * r) * (mu * r);
          return -Z * M_2_SQRTPI * mu * (1.0 + (-1.0 / 3.0 + (1.0 / 10.0 - x2 / 42.0) * x2) * x2);
        }
        return -Z * std::erf(mu * r) / r;
      };
    }
    case SPHERICAL_NUCLEUS: {
      if (verbose) printf("Getting uniformly charged spherical nucleus with Z=%i Rrms=%e\n", Z, Rrms);
      const double R0 = std::sqrt(5.0 / 3.0) * Rrms;  // ibid. eqs. 4, 7
      return [Z, R0](double r) { return (r >= R0) ? -Z / r : -Z / (2.0 * R0) * (3.0 - (r / R0) * (r / R0)); };
    }
    case HOLLOW_NUCLEUS:
      if (verbose) printf("Getting hollow spherical nucleus with Z=%i Rrms=%e\n", Z, Rrms);
      return [Z, Rrms](double r) { return (r >= Rrms) ? -Z / r : -Z / Rrms; };
    case REGULARIZED_NUCLEUS: {
      if (verbose) printf("Getting regularized nucleus with Z=%i a=%e\n", Z, Rrms);
      Regularized unit(Rrms);
      if (verbose) printf("a = %.15e yields b = %.15e\n", unit.a, unit.b);
      return [Z, unit](double r) { return (double)Z * Z * unit.V(Z * r); };
    }
    case NOSUCH_NUCLEUS: throw std::logic_error("No such nucleus!\n");
  }
  throw std::logic_error("Unrecognized model\n");
}

// a segment that starts from zero, laid after the end of the grid so far
static void append_segment(Vec &grid, const Vec &segment) {
  if (segment.empty()) return;
  if (segment[0] != 0.0) throw std::logic_error("grid segment doesn't start from zero");
  if (grid.empty()) {
    grid = segment;
    return;
  }
  const double origin = grid.back();
  for (size_t i = 1; i < segment.size(); i++) grid.push_back(segment[i] + origin);
}

// arma::vec::print(header): one value per line in the cell layout arma_ostream picks from the magnitudes
static void print_vec(const char *header, const Vec &v) {
  printf("%s\n", header);
  bool sci = false, wide = false;
  for (double x : v) {
    if (!std::isfinite(x)) continue;
    const double a = std::fabs(x);
    if (a >= 100.0 || (a > 0.0 && a <= 1e-4)) sci = true;
    if (a >= 10.0) wide = true;
  }
  const int width = sci ? 13 : (wide ? 10 : 9);
  for (double x : v) {
    if (x == 0.0) printf("%*s\n", width, "0");
    else if (sci) printf("%*.4e\n", width, x);
    else printf("%*.4f\n", width, x);
  }
}

Vec form_grid(int model, double Rrms, int Nelem, double Rmax, int igrid, double zexp, int Nelem0, int igrid0, double zexp0,
              int Z, int Zl, int Zr, double Rhalf, bool add_el, double shift_conf, bool verbose) {
  Vec grid;
  if (model != POINT_NUCLEUS && model != REGULARIZED_NUCLEUS) {
    if (verbose) printf("Finite-nucleus grid\n");
    if (Zl != 0 || Zr != 0) throw std::logic_error("Off-center nuclei not supported in finite nucleus mode!\n");
    double rnuc;
    if (model == HOLLOW_NUCLEUS) rnuc = Rrms;
    else if (model == SPHERICAL_NUCLEUS) rnuc = std::sqrt(5.0 / 3.0) * Rrms;
    else if (model == GAUSSIAN_NUCLEUS) rnuc = 3 * Rrms;
    else throw std::logic_error("Nuclear grid not handled!\n");
    if (Nelem0) {
      // the nuclear segment twice (to rnuc and on to 2 rnuc), then an electronic segment of length Rmax - rnuc
      const Vec inside = get_grid(rnuc, Nelem0, igrid0, zexp0);
      append_segment(grid, inside);
      append_segment(grid, inside);
      append_segment(grid, get_grid(Rmax - rnuc, Nelem, igrid, zexp));
    } else
      grid = get_grid(Rmax, Nelem, igrid, zexp);
  } else if (Zl != 0 || Zr != 0) {
    if (verbose) printf("Off-center grid\n");
    // a boundary where the pull of the central charge and of the larger off-centre one balance (only with a central
    // charge), one on the off-centre nuclei, then out to Rmax; the segment that ends on the nuclei is mirrored so that its
    // small elements lie next to them
    const int Zoff = std::max(Zl, Zr);
    const bool central = (Z != 0), offcentre = (Zoff != 0);
    const double split = Z * Rhalf / (Z + Zoff);
    if (verbose) {
      printf("b0 = %e, b0used = %i\n", split, (int)central);
      printf("b1 = %e, b1used = %i\n", Rhalf, (int)offcentre);
      printf("b2 = %e\n", Rmax);
    }
    if (central) append_segment(grid, get_grid(split, Nelem0, igrid, zexp));
    if (offcentre) {
      const double len = Rhalf - split;
      const Vec g = get_grid(len, Nelem0, igrid, zexp);
      Vec mirrored(g.size());
      for (size_t i = 0; i < g.size(); i++) mirrored[i] = len - g[g.size() - 1 - i];
      mirrored.front() = 0.0;
      mirrored.back() = len;
      append_segment(grid, mirrored);
    }
    append_segment(grid, get_grid(Rmax - Rhalf, Nelem, igrid, zexp));
  } else {
    if (verbose) printf("Normal grid\n");
    grid = get_grid(Rmax, Nelem, igrid, zexp);
  }
  if (add_el && std::find(grid.begin(), grid.end(), shift_conf) == grid.end()) {
    grid.push_back(shift_conf);
    std::sort(grid.begin(), grid.end());
  }
  if (verbose) print_vec("Grid", grid);
  return grid;
}

int TwoDBasis::N_L() const { return 2 * *std::max_element(lval.begin(), lval.end()) + 1; }
int TwoDBasis::Mmax() const {
  return *std::max_element(mval.begin(), mval.end()) - *std::min_element(mval.begin(), mval.end());
}

std::vector<size_t> TwoDBasis::m_indices(int m) const {
  std::vector<size_t> idx;
  for (size_t i = 0; i < mval.size(); i++)
    if (mval[i] == m)
      for (size_t j = 0; j < Nrad(); j++) idx.push_back(i * Nrad() + j);
  return idx;
}

std::vector<size_t> TwoDBasis::lm_indices(int l, int m) const {
  std::vector<size_t> idx;
  for (size_t i = 0; i < mval.size(); i++)
    if (mval[i] == m && lval[i] == l)
      for (size_t j = 0; j < Nrad(); j++) idx.push_back(i * Nrad() + j);
  return idx;
}

std::vector<std::vector<size_t> > TwoDBasis::get_sym_idx(int symm) const {
  // TwoDBasis.cpp:202-224; symm 1: one block per m in order of first appearance (find_unique), symm 2: per (l,m)
  std::vector<std::vector<size_t> > idx;
  if (symm == 0) {
    idx.resize(1);
    for (size_t i = 0; i < Nbf(); i++) idx[0].push_back(i);
  } else if (symm == 1) {
    std::vector<int> seen;
    for (int m : mval)
      if (std::find(seen.begin(), seen.end(), m) == seen.end()) seen.push_back(m);
    for (int m : seen) idx.push_back(m_indices(m));
  } else if (symm == 2) {
    for (size_t i = 0; i < mval.size(); i++) idx.push_back(lm_indices(lval[i], mval[i]));
  } else
    throw std::logic_error("Unknown symmetry\n");
  return idx;
}

// g_i(x) = B_i(x)/(x-x_0) and its derivative for the enabled functions of the first element
static void reduced_lip(const LIPBasis &p, const Vec &x, Mat &g, Mat &dg) {
  const Vec &x0 = p.x0;
  const size_t np = x0.size();
  g.zeros(x.size(), p.enabled.size());
  dg.zeros(x.size(), p.enabled.size());
  for (size_t ix = 0; ix < x.size(); ix++)
    for (size_t c = 0; c < p.enabled.size(); c++) {
      size_t fi = p.enabled[c];
      if (fi == 0) throw std::logic_error("reduced LIP needs the first function dropped");
      double val = 1.0 / (x0[fi] - x0[0]);
      for (size_t ip = 1; ip < np; ip++)
        if (ip != fi) val *= (x[ix] - x0[ip]) / (x0[fi] - x0[ip]);
      double der = 0.0;
      for (size_t d1 = 1; d1 < np; d1++) {
        if (d1 == fi) continue;
        double t = 1.0 / (x0[fi] - x0[0]);
        for (size_t ip = 1; ip < np; ip++) {
          if (ip == fi || ip == d1) continue;
          t *= (x[ix] - x0[ip]) / (x0[fi] - x0[ip]);
        }
        der += t / (x0[fi] - x0[d1]);
      }
      g(ix, c) = val;
      dg(ix, c) = der;
    }
}

// second derivative of g_i(x) = B_i(x)/(x-x_0): the Lagrange product without its (x - x_0) factor, differentiated twice
static Mat reduced_lip_d2(const LIPBasis &p, const Vec &x) {
  const Vec &x0 = p.x0;
  const size_t np = x0.size();
  Mat d2(x.size(), p.enabled.size());
  for (size_t ix = 0; ix < x.size(); ix++)
    for (size_t c = 0; c < p.enabled.size(); c++) {
      size_t fi = p.enabled[c];
      if (fi == 0) throw std::logic_error("reduced LIP needs the first function dropped");
      double val = 0.0;
      for (size_t d1 = 1; d1 < np; d1++) {
        if (d1 == fi) continue;
        for (size_t e2 = 1; e2 < d1; e2++) {
          if (e2 == fi) continue;
          double t = 1.0 / (x0[fi] - x0[0]);
          for (size_t ip = 1; ip < np; ip++) {
            if (ip == fi || ip == d1 || ip == e2) continue;
            t *= (x[ix] - x0[ip]) / (x0[fi] - x0[ip]);
          }
          val += 2.0 * t / ((x0[fi] - x0[d1]) * (x0[fi] - x0[e2]));
        }
      }
      d2(ix, c) = val;
    }
  return d2;
}

Mat TwoDBasis::get_bf(size_t iel) const {
  double sc = fem.scaling_factor(iel);
  if (iel == 0) {
    Mat g, dg;
    reduced_lip(fem.get_basis(0), xq, g, dg);
    for (auto &v : g.d) v /= sc;  // r = sc (x - x_0)
    return g;
  }
  Mat f = fem.eval_dnf(xq, 0, iel);
  Vec r = get_r(iel);
  for (size_t j = 0; j < f.n_cols; j++)
    for (size_t i = 0; i < f.n_rows; i++) f(i, j) /= r[i];
  return f;
}

Mat TwoDBasis::get_df(size_t iel) const {
  double sc = fem.scaling_factor(iel);
  if (iel == 0) {
    Mat g, dg;
    reduced_lip(fem.get_basis(0), xq, g, dg);
    for (auto &v : dg.d) v /= sc * sc;
    return dg;
  }
  // RadialBasis.cpp:676-700: (-f/r + f')/r
  Mat f = fem.eval_dnf(xq, 0, iel), d = fem.eval_dnf(xq, 1, iel);
  Vec r = get_r(iel);
  for (size_t j = 0; j < f.n_cols; j++)
    for (size_t i = 0; i < f.n_rows; i++) {
      double invr = 1.0 / r[i];
      d(i, j) = (-f(i, j) * invr + d(i, j)) * invr;
    }
  return d;
}

Mat TwoDBasis::get_lf(size_t iel) const {
  double sc = fem.scaling_factor(iel);
  if (iel == 0) {
    // the exact counterpart of the reference's Taylor branch (RadialBasis.cpp:711-714): g is a polynomial in r here
    Mat d2 = reduced_lip_d2(fem.get_basis(0), xq);
    for (auto &v : d2.d) v /= sc * sc * sc;
    return d2;
  }
  // RadialBasis.cpp:716-726: ((2 f/r - 2 f')/r + f'')/r
  Mat f = fem.eval_dnf(xq, 0, iel), d = fem.eval_dnf(xq, 1, iel), l = fem.eval_dnf(xq, 2, iel);
  Vec r = get_r(iel);
  for (size_t j = 0; j < f.n_cols; j++)
    for (size_t i = 0; i < f.n_rows; i++) {
      double invr = 1.0 / r[i];
      l(i, j) = ((2.0 * f(i, j) * invr - 2.0 * d(i, j)) * invr + l(i, j)) * invr;
    }
  return l;
}

Vec TwoDBasis::get_wrad(size_t iel) const {
  Vec w(wq);
  for (auto &x : w) x *= fem.scaling_factor(iel);
  return w;
}

Mat TwoDBasis::radial_integral(int Rexp, size_t iel) const {
  Mat bf = get_bf(iel);
  Vec r = get_r(iel), w = get_wrad(iel);
  Mat wbf(bf);
  for (size_t q = 0; q < bf.n_rows; q++) {
    double wp = w[q] * std::pow(r[q], Rexp + 2);
    for (size_t j = 0; j < bf.n_cols; j++) wbf(q, j) *= wp;
  }
  return matmul(wbf, true, bf, false);
}

static Mat assemble_radial(const TwoDBasis &b, const std::function<Mat(size_t)> &el) {
  Mat M(b.Nrad(), b.Nrad());
  for (size_t iel = 0; iel < b.Nel(); iel++) {
    Mat m = el(iel);
    size_t i0 = b.fem.first[iel];
    for (size_t j = 0; j < m.n_cols; j++)
      for (size_t i = 0; i < m.n_rows; i++) M(i0 + i, i0 + j) += m(i, j);
  }
  return M;
}

static Mat place_diag(const TwoDBasis &b, const std::vector<Mat> &rad) {
  size_t R = b.Nrad();
  Mat O(b.Nbf(), b.Nbf());
  for (size_t a = 0; a < b.Nang(); a++)
    for (size_t j = 0; j < R; j++)
      for (size_t i = 0; i < R; i++) O(a * R + i, a * R + j) = rad[a](i, j);
  return O;
}

Mat TwoDBasis::overlap() const {
  Mat Orad = assemble_radial(*this, [this](size_t iel) { return radial_integral(0, iel); });
  return place_diag(*this, std::vector<Mat>(Nang(), Orad));
}

Mat TwoDBasis::overlap(const TwoDBasis &rh) const {
  // radial part: int (B_i / r)(B'_j / r) r^2 dr = int B_i B'_j dr over the intersections of the two element grids
  Vec xp, wp;
  chebyshev_rule((int)std::max(xq.size(), rh.xq.size()), xp, wp);
  Mat Srad(fem.nbf(), rh.fem.nbf());
  for (size_t iel = 0; iel < fem.nelem(); iel++)
    for (size_t jel = 0; jel < rh.fem.nelem(); jel++) {
      const double imin = fem.element_begin(iel), imax = fem.element_end(iel);
      const double jmin = rh.fem.element_begin(jel), jmax = rh.fem.element_end(jel);
      if (!((jmin >= imin && jmin < imax) || (imin >= jmin && imin < jmax))) continue;
      const double a = std::max(imin, jmin), b = std::min(imax, jmax);
      const double mid = 0.5 * (b + a), len = 0.5 * (b - a);
      Vec xi(xp.size()), xj(xp.size());
      for (size_t q = 0; q < xp.size(); q++) {
        const double r = mid + len * xp[q];
        xi[q] = (r - fem.element_midpoint(iel)) / fem.scaling_factor(iel);
        xj[q] = (r - rh.fem.element_midpoint(jel)) / rh.fem.scaling_factor(jel);
      }
      const Mat ibf = fem.eval_dnf(xi, 0, iel), jbf = rh.fem.eval_dnf(xj, 0, jel);
      const size_t i0 = fem.first[iel], j0 = rh.fem.first[jel];
      for (size_t fj = 0; fj < jbf.n_cols; fj++)
        for (size_t fi = 0; fi < ibf.n_cols; fi++) {
          double acc = 0.0;
          for (size_t q = 0; q < xp.size(); q++) acc += wp[q] * len * ibf(q, fi) * jbf(q, fj);
          Srad(i0 + fi, j0 + fj) += acc;
        }
    }
  // angular part: the same (l, m) only (atomic/TwoDBasis.cpp:338-341)
  const size_t R = Nrad(), R2 = rh.Nrad();
  Mat S(Nbf(), rh.Nbf());
  for (size_t ia = 0; ia < Nang(); ia++)
    for (size_t ja = 0; ja < rh.Nang(); ja++)
      if (lval[ia] == rh.lval[ja] && mval[ia] == rh.mval[ja])
        for (size_t j = 0; j < R2; j++)
          for (size_t i = 0; i < R; i++) S(ia * R + i, ja * R2 + j) = Srad(i, j);
  return S;
}

Mat TwoDBasis::kinetic() const {
  // TwoDBasis.cpp:349-380: 1/2 int B'B' + l(l+1) 1/2 int (B/r)(B/r)
  std::function<double(double)> none;
  Mat Trad = assemble_radial(*this, [&](size_t iel) { return 0.5 * fem.matrix_element(iel, 1, 1, xq, wq, none); });
  Mat Tl = assemble_radial(*this, [&](size_t iel) {
    Mat bf = get_bf(iel);
    Vec w = get_wrad(iel);
    Mat wbf(bf);
    for (size_t q = 0; q < bf.n_rows; q++)
      for (size_t j = 0; j < bf.n_cols; j++) wbf(q, j) *= w[q];
    return 0.5 * matmul(wbf, true, bf, false);
  });
  std::vector<Mat> rad;
  for (size_t a = 0; a < Nang(); a++) rad.push_back(Trad + (double)(lval[a] * (lval[a] + 1)) * Tl);
  return place_diag(*this, rad);
}

Mat TwoDBasis::nuclear_point() const {
  Mat Vrad = assemble_radial(*this, [this](size_t iel) { return radial_integral(-1, iel); });
  return place_diag(*this, std::vector<Mat>(Nang(), (-(double)Z) * Vrad));
}

Mat TwoDBasis::nuclear_offcenter(size_t iel, int L) const {
  // 1/|r - R| = sum_L 4 pi/(2L+1) r_<^L / r_>^(L+1) Y_L0(r) Y_L0(R), Y_L0 on the z axis = sqrt((2L+1)/(4 pi)): an element
  // beyond the nucleus sees Rhalf^L r^(-L-1), one inside it r^L Rhalf^(-L-1); the nucleus must sit on a boundary
  const double c = -std::sqrt(4.0 * M_PI / (2 * L + 1));
  if (fem.element_begin(iel) >= Rhalf) return (c * std::pow(Rhalf, (double)L)) * radial_integral(-L - 1, iel);
  if (fem.element_end(iel) <= Rhalf) return (c * std::pow(Rhalf, -(double)L - 1.0)) * radial_integral(L, iel);
  throw std::logic_error("Nucleus placed within element!\n");
}

Mat TwoDBasis::nuclear() const {
  if (finitenuc != POINT_NUCLEUS) {
    const std::function<double(double)> pot = nuclear_model(finitenuc, Z, Rrms);
    Mat Vrad = assemble_radial(*this, [&](size_t iel) { return fem.matrix_element(iel, 0, 0, xq, wq, pot); });
    return place_diag(*this, std::vector<Mat>(Nang(), Vrad));
  }
  Mat V = nuclear_point();
  if (Zl != 0 || Zr != 0) {
    const size_t R = Nrad();
    const int Lmax = 2 * *std::max_element(lval.begin(), lval.end());
    std::vector<Mat> Vaux((size_t)Lmax + 1);
    for (int L = 0; L <= Lmax; L++) Vaux[L] = assemble_radial(*this, [&](size_t iel) { return nuclear_offcenter(iel, L); });
    for (size_t ia = 0; ia < Nang(); ia++)
      for (size_t ja = 0; ja < Nang(); ja++) {
        if (mval[ia] != mval[ja]) continue;
        const int li = lval[ia], lj = lval[ja];
        for (int L = std::abs(li - lj); L <= li + lj; L++) {
          const double cpl = gaunt_coefficient(li, mval[ia], L, 0, lj, mval[ja]);
          if (cpl == 0.0) continue;
          const double f = cpl * ((L % 2 ? -1.0 : 1.0) * Zl + Zr);
          for (size_t j = 0; j < R; j++)
            for (size_t i = 0; i < R; i++) V(ia * R + i, ja * R + j) += f * Vaux[L](i, j);
        }
      }
  }
  return V;
}

Mat TwoDBasis::confinement(int N, double r_0, int iconf, double V, double shift, bool verbose) const {
  if (iconf == 0) return Mat(Nbf(), Nbf());
  const int sign = (r_0 < 0) ? -1 : 1;  // the sign of r_0 selects an attractive or a repulsive potential
  r_0 = std::fabs(r_0);
  const double r_c = *std::max_element(fem.bval.begin(), fem.bval.end());
  Mat Orad = assemble_radial(*this, [&](size_t iel) -> Mat {
    if (iconf == 1) {
      if (verbose) printf("Polynomial confinement, r_0 = %e N = %i shift = %e \n", r_0, N, shift);
      if (N < 0 && shift != 0.0) throw std::logic_error("Cannot have a divergent potential with a shift!\n");
      // int (B_i/r)(B_j/r) (r - shift)^(N+2) dr beyond the shift (RadialBasis.cpp:361-369)
      Mat bf = get_bf(iel);
      Vec r = get_r(iel), w = get_wrad(iel);
      Mat wbf(bf);
      for (size_t q = 0; q < bf.n_rows; q++) {
        const double wp = (r[q] < shift) ? 0.0 : w[q] * std::pow(r[q] - shift, N + 2);
        for (size_t j = 0; j < bf.n_cols; j++) wbf(q, j) *= wp;
      }
      return (sign * std::pow(r_0, -(double)std::abs(N))) * matmul(wbf, true, bf, false);
    } else if (iconf == 2) {
      if (verbose) printf("Exponential confinement, r_0 = %e N = %i shift = %e \n", r_0, N, shift);
      if (N < 0) throw std::logic_error("Exponential confinement potential does not make sense with negative N!\n");
      if (N == 0) throw std::logic_error("Exponential confinement potential requires N >= 1!");
      // N! [exp(x) - sum_{k<N} x^k/k!], x = (r - shift)/r_0: the exponential without its first N Taylor terms
      return fem.matrix_element(iel, 0, 0, xq, wq, [=](double r) {
        if (r < shift) return 0.0;
        const double x = (r - shift) / r_0;
        double term = 1.0, partial = 0.0, Nfactorial = 1.0;  // term = x^k / k!
        for (int k = 0; k < N; k++) {
          partial += term;
          term *= x / (k + 1);
          Nfactorial *= k + 1;
        }
        return Nfactorial * (std::exp(x) - partial);
      });
    } else if (iconf == 3) {
      if (V < 0) throw std::logic_error("Cannot have attractive barrier!\n");
      if (verbose) printf("Barrier confinement, V = %e shift = %e \n", V, shift);
      return fem.matrix_element(iel, 0, 0, xq, wq, [=](double r) { return (r < shift) ? 0.0 : V; });
    } else if (iconf == 4) {
      if (verbose) printf("Junquera-type confinement, r_0 = %e N = %i V = %e shift = %e \n", r_0, N, V, shift);
      if (N <= 0) throw std::logic_error("Junquera confinement potential requires N >= 1!");
      if (V <= 0) throw std::logic_error("Cannot have attractive Junquera potential!\n");
      // V0 exp(-(r_c - r_i)/(r - r_i)) / (r_c - r)^N with r_c the last grid point (Junquera et al. 2001)
      return fem.matrix_element(iel, 0, 0, xq, wq, [=](double r) {
        if (r < shift) return 0.0;
        return V * std::exp(-(r_c - shift) / (r - shift)) / std::pow(r_c - r, N);
      });
    }
    throw std::logic_error("Case not implemented!\n");
  });
  return place_diag(*this, std::vector<Mat>(Nang(), Orad));
}

// quadrature::twoe_inner_integral + twoe_integral / yukawa_integral (libhelfem/src/quadrature.cpp:22-169) for a kernel
// g(r<, r>) = fsmallbig(r<, r>) whose r> dependence is fbig(r>): the inner integral up to each outer quadrature point
// is built segment by segment (each segment with a fresh rule, scaled by the kernel at its upper end) and carried
// to the next point with the ratio fbig(r_ip)/fbig(r_ip-1).
static Mat twoe_integral_kernel(double rmin, double rmax, const Vec &xq, const Vec &wq, const LIPBasis &poly,
                                const std::function<double(double, double)> &fsmallbig,
                                const std::function<double(double)> &fbig) {
  const size_t nq = xq.size();
  const double rmid0 = 0.5 * (rmax + rmin), rlen0 = 0.5 * (rmax - rmin);
  const size_t Ni = poly.nbf(), Np = Ni * Ni;
  Vec r0(nq);
  for (size_t q = 0; q < nq; q++) r0[q] = rmid0 + rlen0 * xq[q];
  Mat inner(Np, nq);
  for (size_t ip = 0; ip < nq; ip++) {
    double a = (ip == 0) ? rmin : r0[ip - 1], bnd = r0[ip];
    double rmid = 0.5 * (bnd + a), rlen = 0.5 * (bnd - a);
    Vec xpoly(nq), wp(nq);
    for (size_t q = 0; q < nq; q++) {
      double r = rmid + rlen * xq[q];
      wp[q] = wq[q] * fsmallbig(r, bnd) * rlen;
      xpoly[q] = (r - rmid0) / rlen0;
    }
    Mat bf = poly.eval_dnf(xpoly, 0, rlen0);
    double *col = &inner.d[ip * Np];
    for (size_t q = 0; q < nq; q++)
      for (size_t l = 0; l < Ni; l++)
        for (size_t k = 0; k < Ni; k++) col[l * Ni + k] += wp[q] * bf(q, k) * bf(q, l);
    if (ip > 0) {
      double ratio = fbig(r0[ip]) / fbig(r0[ip - 1]);
      const double *prev = &inner.d[(ip - 1) * Np];
      for (size_t k = 0; k < Np; k++) col[k] += prev[k] * ratio;
    }
  }
  Mat bf0 = poly.eval_dnf(xq, 0, rlen0);
  Mat ints(Np, Np);
  for (size_t q = 0; q < nq; q++) {
    double w = wq[q] * rlen0;
    const double *in = &inner.d[q * Np];
    for (size_t c = 0; c < Np; c++) {
      double wi = w * in[c];
      double *colp = &ints.d[c * Np];
      for (size_t fj = 0; fj < Ni; fj++)
        for (size_t fi = 0; fi < Ni; fi++) colp[fi * Ni + fj] += bf0(q, fi) * bf0(q, fj) * wi;
    }
  }
  return ints + ints.t();
}

Mat twoe_integral(double rmin, double rmax, const Vec &xq, const Vec &wq, const LIPBasis &poly, int L) {
  // r_<^L / r_>^{L+1}: inner(q,(kl)) = r_q^{-L-1} int_{rmin}^{r_q} r^L B_k B_l dr
  return twoe_integral_kernel(
      rmin, rmax, xq, wq, poly, [L](double r, double R) { return std::pow(r / R, (double)L) / R; },
      [L](double r) { return std::pow(r, -(double)L - 1.0); });
}

Mat yukawa_integral(double rmin, double rmax, const Vec &xq, const Vec &wq, const LIPBasis &poly, int L, double lambda) {
  return twoe_integral_kernel(
      rmin, rmax, xq, wq, poly,
      [L, lambda](double r, double R) { return bessel_il(r * lambda, L) * bessel_kl(R * lambda, L); },
      [L, lambda](double r) { return bessel_kl(r * lambda, L); });
}

void TwoDBasis::compute_disjoint() {
  const size_t Ne = Nel(), NL = (size_t)N_L();
  disjoint_L.assign(Ne * NL, Mat());
  disjoint_m1L.assign(Ne * NL, Mat());
  for (size_t L = 0; L < NL; L++)
    for (size_t iel = 0; iel < Ne; iel++) {
      disjoint_L[L * Ne + iel] = radial_integral((int)L, iel);
      disjoint_m1L[L * Ne + iel] = radial_integral(-(int)L - 1, iel);
    }
  have_disjoint = true;
}

void TwoDBasis::tei_element_tables(size_t iel, diatomic::TwoDBasis::TeiElementTables &t) const {
  const size_t nq = xq.size(), NL = (size_t)N_L();
  const double rmin = fem.element_begin(iel), rmax = fem.element_end(iel);
  const double rmid0 = 0.5 * (rmax + rmin), rlen0 = 0.5 * (rmax - rmin);
  LIPBasis poly = fem.get_basis(iel);
  const size_t Ni = poly.nbf(), Np = Ni * Ni;
  t.Ni = Ni;
  t.Np = Np;
  t.nq = nq;
  t.Nlm = NL;
  t.bb0.zeros(Np, nq);
  t.bbs.zeros(Np, nq * nq);
  t.wQ.assign(NL * nq, 0.0);
  t.wP.assign(NL * nq * nq, 0.0);
  Vec r0(nq);
  for (size_t q = 0; q < nq; q++) r0[q] = rmid0 + rlen0 * xq[q];
  Mat bf0 = poly.eval_dnf(xq, 0, rlen0);
  for (size_t q = 0; q < nq; q++) {
    const double w = wq[q] * rlen0;
    for (size_t L = 0; L < NL; L++) t.wQ[L * nq + q] = w * std::pow(r0[q], -(double)L - 1.0);
    for (size_t j = 0; j < Ni; j++)
      for (size_t i = 0; i < Ni; i++) t.bb0(j * Ni + i, q) = bf0(q, i) * bf0(q, j);
  }
  for (size_t isub = 0; isub < nq; isub++) {
    const double a = (isub == 0) ? rmin : r0[isub - 1], bnd = r0[isub];
    const double rmid = 0.5 * (bnd + a), rlen = 0.5 * (bnd - a);
    Vec xpoly(nq);
    for (size_t q = 0; q < nq; q++) {
      const double r = rmid + rlen * xq[q];
      xpoly[q] = (r - rmid0) / rlen0;
      const double w = wq[q] * rlen;
      for (size_t L = 0; L < NL; L++) t.wP[L * nq * nq + isub * nq + q] = w * std::pow(r, (double)L);
    }
    Mat bf = poly.eval_dnf(xpoly, 0, rlen0);
    for (size_t q = 0; q < nq; q++)
      for (size_t j = 0; j < Ni; j++)
        for (size_t i = 0; i < Ni; i++) t.bbs(j * Ni + i, isub * nq + q) = bf(q, i) * bf(q, j);
  }
}

void TwoDBasis::compute_tei(bool exchange) {
  const size_t Ne = Nel(), NL = (size_t)N_L();
  compute_disjoint();
  prim_tei.assign(Ne * NL, Mat());
  parallel_for(Ne * NL, [&](size_t idx) {
    const size_t L = idx / Ne, iel = idx % Ne;
    prim_tei[L * Ne + iel] =
        twoe_integral(fem.element_begin(iel), fem.element_end(iel), xq, wq, fem.get_basis(iel), (int)L);
  });
  have_tei = true;
  if (exchange) {
    prim_ktei.assign(Ne * NL, Mat());
    for (size_t idx = 0; idx < Ne * NL; idx++) {
      size_t Ni = fem.nprim(idx % Ne);
      prim_ktei[idx] = diatomic::exchange_tei(prim_tei[idx], Ni, Ni, Ni, Ni);
    }
    have_ktei = true;
  }
}

Mat TwoDBasis::model_potential(const ModelPotential &pot) const {
  // RadialBasis::model_potential: (B_i/r)(B_j/r) V(r) r^2 = B_i B_j V(r)
  Mat Vrad = assemble_radial(*this, [&](size_t iel) {
    return fem.matrix_element(iel, 0, 0, xq, wq, [&pot](double r) { return pot.V(r); });
  });
  return place_diag(*this, std::vector<Mat>(Nang(), Vrad));
}

Mat TwoDBasis::bessel_il_integral(int L, double lambda, size_t iel) const {
  return fem.matrix_element(iel, 0, 0, xq, wq, [L, lambda](double r) { return bessel_il(r * lambda, L); });
}

Mat TwoDBasis::bessel_kl_integral(int L, double lambda, size_t iel) const {
  return fem.matrix_element(iel, 0, 0, xq, wq, [L, lambda](double r) { return bessel_kl(r * lambda, L); });
}

Mat TwoDBasis::erfc_integral(int L, double mu, size_t iel, size_t kel) const {
  // RadialBasis.cpp:502-558 + quadrature.cpp:171-222.  The kernel has a cusp at r = r', so the in-element integral
  // uses nq sub-intervals (each with its own nq-point rule) for the second coordinate; distinct elements use one.
  const size_t nq = xq.size();
  const size_t Nint = (iel == kel) ? nq : 1;
  Vec xk(nq * Nint), wk(nq * Nint);
  for (size_t ii = 0; ii < Nint; ii++) {
    double istart = ii * 2.0 / Nint - 1.0, iend = (ii + 1) * 2.0 / Nint - 1.0;
    double imid = 0.5 * (iend + istart), ilen = 0.5 * (iend - istart);
    for (size_t q = 0; q < nq; q++) {
      xk[ii * nq + q] = imid + xq[q] * ilen;
      wk[ii * nq + q] = wq[q] * ilen;
    }
  }
  Mat ibf = fem.eval_dnf(xq, 0, iel), kbf = fem.eval_dnf(xk, 0, kel);
  const double rleni = fem.scaling_factor(iel), rlenk = fem.scaling_factor(kel);
  Vec ri = fem.eval_coord(xq, iel), rk = fem.eval_coord(xk, kel);
  const size_t Ni = ibf.n_cols, Nk = kbf.n_cols, nqi = nq, nqk = nq * Nint;
  // Green's function and weighted product functions
  Mat Fn(nqi, nqk);
  for (size_t k = 0; k < nqk; k++)
    for (size_t i = 0; i < nqi; i++) Fn(i, k) = erfc_Phi(L, mu * ri[i], mu * rk[k]);
  Mat pij(nqi, Ni * Ni), pkl(nqk, Nk * Nk);
  for (size_t fi = 0; fi < Ni; fi++)
    for (size_t fj = 0; fj < Ni; fj++)
      for (size_t q = 0; q < nqi; q++) pij(q, fi * Ni + fj) = ibf(q, fi) * ibf(q, fj) * wq[q] * rleni;
  for (size_t fi = 0; fi < Nk; fi++)
    for (size_t fj = 0; fj < Nk; fj++)
      for (size_t q = 0; q < nqk; q++) pkl(q, fi * Nk + fj) = kbf(q, fi) * kbf(q, fj) * wk[q] * rlenk;
  Mat tei = matmul(pij, true, matmul(Fn, false, pkl, false), false);
  if (iel == kel) tei = 0.5 * (tei + tei.t());
  return tei;
}

void TwoDBasis::compute_yukawa(double lambda) {
  // TwoDBasis.cpp:741-778
  rs_kind = 1;
  rs_lambda = lambda;
  const size_t Ne = Nel(), NL = (size_t)N_L();
  disjoint_iL.assign(Ne * NL, Mat());
  disjoint_kL.assign(Ne * NL, Mat());
  rs_tei.assign(Ne * NL, Mat());
  rs_ktei.assign(Ne * NL, Mat());
  parallel_for(Ne * NL, [&](size_t idx) {
    const size_t L = idx / Ne, iel = idx % Ne;
    disjoint_iL[idx] = bessel_il_integral((int)L, lambda, iel);
    disjoint_kL[idx] = bessel_kl_integral((int)L, lambda, iel);
    rs_tei[idx] = yukawa_integral(fem.element_begin(iel), fem.element_end(iel), xq, wq, fem.get_basis(iel), (int)L, lambda);
    size_t Ni = fem.nprim(iel);
    rs_ktei[idx] = diatomic::exchange_tei(rs_tei[idx], Ni, Ni, Ni, Ni);
  });
}

void TwoDBasis::compute_erfc(double mu) {
  // TwoDBasis.cpp:780-815
  rs_kind = 2;
  rs_lambda = mu;
  const size_t Ne = Nel(), NL = (size_t)N_L();
  disjoint_iL.clear();
  disjoint_kL.clear();
  rs_tei.assign(Ne * Ne * NL, Mat());
  rs_ktei.assign(Ne * Ne * NL, Mat());
  parallel_for(Ne * Ne * NL, [&](size_t idx) {
    const size_t L = idx / (Ne * Ne), iel = (idx / Ne) % Ne, kel = idx % Ne;
    rs_tei[idx] = erfc_integral((int)L, mu, iel, kel);
    rs_ktei[idx] = diatomic::exchange_tei(rs_tei[idx], fem.nprim(iel), fem.nprim(iel), fem.nprim(kel), fem.nprim(kel));
  });
}

}  // namespace atomic
}  // namespace helfem

