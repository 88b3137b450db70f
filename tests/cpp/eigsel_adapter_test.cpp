// helfem::gpu::scf::eig_gsym_sub_sel through include/helfem_gpu_arma.hpp on a two-block problem (orders 40 and 25, rows
// interleaved, S = 1), against the full adapter call eig_gsym_sub: the first pairs of every block must be the same levels.
// Prints figures that tests/test_gpu_eigsel_adapter.py checks.
//   eigsel_adapter_test compile-only | run
#include "../../include/helfem_gpu_arma.hpp"
#include "../../helfem_amd/csrc/host/linalg.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

using helfem::Mat;
typedef std::vector<double> Vec;
namespace hg = helfem::gpu;

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "compile-only")) {
    printf("adapter compiled\n");
    return 0;
  }
  try {
    auto ctx = std::make_shared<hg::Context>(0);
    const size_t n1 = 40, n2 = 25, N = n1 + n2, nev = 6;
    std::vector<std::vector<size_t> > sym(2);
    for (size_t i = 0; i < N; i++) sym[(i % 3 == 1 && sym[1].size() < n2) ? 1 : 0].push_back(i);
    std::vector<int> blk(N);
    for (int b = 0; b < 2; b++)
      for (size_t i : sym[b]) blk[i] = b;
    Mat F(N, N), X(N, N);
    unsigned long long st = 12345;
    auto rnd = [&]() {
      st = st * 6364136223846793005ull + 1442695040888963407ull;
      return (double)(st >> 11) / 9007199254740992.0 * 2.0 - 1.0;
    };
    for (size_t j = 0; j < N; j++) {
      X(j, j) = 1.0;
      for (size_t i = j; i < N; i++)
        if (blk[i] == blk[j]) F(i, j) = F(j, i) = rnd() + (i == j ? 0.1 * (double)i : 0.0);
    }
    Vec E, Es;
    Mat C, Cs;
    hg::scf::eig_gsym_sub(*ctx, E, C, F, X, sym);
    hg::scf::eig_gsym_sub_sel(*ctx, Es, Cs, F, X, sym, nev);
    printf("K %zu cols %zu rows %zu\n", Es.size(), (size_t)Cs.n_cols, (size_t)Cs.n_rows);
    // the full call's levels block by block: a column belongs to the block where it is non-zero
    Vec want;
    size_t taken[2] = {0, 0};
    for (size_t j = 0; j < N; j++) {
      int b = 0;
      double big = 0.0;
      for (size_t i = 0; i < N; i++)
        if (std::fabs(C(i, j)) > big) big = std::fabs(C(i, j)), b = blk[i];
      if (taken[b]++ < nev) want.push_back(E[j]);
    }
    std::sort(want.begin(), want.end());
    double dE = 0.0, res = 0.0, orth = 0.0, leak = 0.0, aufbau = 0.0;
    for (size_t j = 0; j < Es.size() && j < want.size(); j++) dE = std::max(dE, std::fabs(Es[j] - want[j]));
    for (size_t j = 0; j < nev && j < Es.size(); j++) aufbau = std::max(aufbau, std::fabs(Es[j] - E[j]));
    for (size_t j = 0; j < Cs.n_cols; j++) {
      int b = 0;
      double big = 0.0;
      for (size_t i = 0; i < N; i++)
        if (std::fabs(Cs(i, j)) > big) big = std::fabs(Cs(i, j)), b = blk[i];
      for (size_t i = 0; i < N; i++) {
        if (blk[i] != b) leak = std::max(leak, std::fabs(Cs(i, j)));
        double r = -Es[j] * Cs(i, j);
        for (size_t k = 0; k < N; k++) r += F(i, k) * Cs(k, j);
        res = std::max(res, std::fabs(r));
      }
      for (size_t k = 0; k < Cs.n_cols; k++) {
        double s = k == j ? -1.0 : 0.0;
        for (size_t i = 0; i < N; i++) s += Cs(i, j) * Cs(i, k);
        orth = std::max(orth, std::fabs(s));
      }
    }
    printf("dE %.3e aufbau %.3e res %.3e orth %.3e leak %.3e\n", dE, aufbau, res, orth, leak);
    bool logic = false;
    try {
      hg::scf::eig_gsym_sub_sel(*ctx, Es, Cs, F, X, sym, 0);
    } catch (const std::logic_error &) {
      logic = true;
    }
    printf("logic_error_on_nev_0 %d\n", logic ? 1 : 0);
    printf("adapter ok\n");
  } catch (const std::exception &e) {
    printf("FAILED: %s\n", e.what());
    return 1;
  }
  return 0;
}
