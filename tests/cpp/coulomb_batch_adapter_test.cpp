// helfem::gpu BasisBase::coulomb(const std::vector<Mat> &) of include/helfem_gpu_arma.hpp on both basis classes, against
// the single-density overload on the same object.  Prints figures that tests/test_gpu_coulomb_batch.py checks.
//   coulomb_batch_adapter_test compile-only | run
#include "../../include/helfem_gpu_arma.hpp"
#include "../../helfem_amd/csrc/host/linalg.h"
#include <cmath>
#include <cstdio>
#include <cstring>

using helfem::Mat;
typedef std::vector<double> Vec;
typedef std::vector<int> IVec;
namespace hg = helfem::gpu;

static unsigned long long g_state = 2024;
static double rnd() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

// worst |J_batch[b] - coulomb(P[b])| / max |coulomb(P[b])| over nP random symmetric densities
template <class Basis>
static double worst(const Basis &basis, size_t nP) {
  const size_t N = basis.Nbf();
  std::vector<Mat> P;
  for (size_t b = 0; b < nP; b++) {
    P.push_back(Mat(N, N));
    for (size_t j = 0; j < N; j++)
      for (size_t i = j; i < N; i++) P[b](i, j) = P[b](j, i) = rnd();
  }
  std::vector<Mat> J = basis.coulomb(P);
  if (J.size() != nP) throw std::runtime_error("wrong number of matrices returned");
  double w = 0.0;
  for (size_t b = 0; b < nP; b++) {
    Mat Js = basis.coulomb(P[b]);
    double big = 0.0, d = 0.0;
    for (size_t k = 0; k < N * N; k++) {
      big = std::max(big, std::fabs(Js.d[k]));
      d = std::max(d, std::fabs(Js.d[k] - J[b].d[k]));
    }
    w = std::max(w, d / big);
  }
  return w;
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "compile-only")) {
    printf("adapter compiled\n");
    return 0;
  }
  try {
    auto ctx = std::make_shared<hg::Context>(0);
    {
      const double Rhalf = 0.7, Rmax = 40.0;
      const int nelem = 3, nnodes = 6;
      Vec bval(nelem + 1);
      if (hfg_radial_grid(std::acosh(Rmax / Rhalf), nelem, 4, 1.0, bval.data())) throw std::runtime_error(hfg_last_error());
      int lmmax[2] = {2, 1};
      IVec lval(64), mval(64);
      int nang = 64;
      if (hfg_lm_list(lmmax, 2, lval.data(), mval.data(), &nang)) throw std::runtime_error(hfg_last_error());
      lval.resize(nang);
      mval.resize(nang);
      hg::diatomic::TwoDBasis<Mat> basis(ctx, 1, 1, Rhalf, nnodes, 5 * nnodes, bval, lval, mval, 10);
      bool logic = false;
      try {
        basis.coulomb(std::vector<Mat>(2, Mat(basis.Nbf(), basis.Nbf())));
      } catch (const std::logic_error &e) {
        logic = std::string(e.what()).find("Primitive teis have not been computed") != std::string::npos;
      }
      printf("logic_error_before_compute_tei %d\n", logic ? 1 : 0);
      basis.compute_tei(false);
      printf("diatomic Nbf %zu worst %.3e\n", basis.Nbf(), worst(basis, 9));
      printf("empty_batch %zu\n", basis.coulomb(std::vector<Mat>()).size());
    }
    {
      const int nelem = 4, nnodes = 6;
      Vec bval(nelem + 1);
      if (hfg_radial_grid(40.0, nelem, 4, 2.0, bval.data())) throw std::runtime_error(hfg_last_error());
      IVec lval(64), mval(64);
      int nang = 64;
      if (hfg_angular_basis(2, 1, lval.data(), mval.data(), &nang)) throw std::runtime_error(hfg_last_error());
      lval.resize(nang);
      mval.resize(nang);
      hg::atomic::TwoDBasis<Mat> basis(ctx, 2, nnodes, 5 * nnodes, bval, lval, mval);
      basis.compute_tei(false);
      printf("atomic Nbf %zu worst %.3e\n", basis.Nbf(), worst(basis, 3));
    }
    printf("adapter ok\n");
  } catch (const std::exception &e) {
    printf("FAILED: %s\n", e.what());
    return 1;
  }
  return 0;
}
