// helfem::gpu::atomic::TwoDBasis<Mat>::mix_exchange through include/helfem_gpu_arma.hpp: alpha exchange(P) + beta rs_exchange(P)
// from one build on the mixed-kernel table set, against the two builds of the same adapter, for both screened kernels.
// Prints the deviations, which tests/test_gpu_exchange_mix.py checks.
//   mix_exchange_adapter_check compile-only | run
#include "../../include/helfem_gpu_arma.hpp"
#include "../../helfem_amd/csrc/host/linalg.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

using helfem::Mat;
namespace hg = helfem::gpu;

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "compile-only")) {
    printf("adapter compiled\n");
    return 0;
  }
  try {
    auto ctx = std::make_shared<hg::Context>(0);
    const int nelem = 3, nnodes = 5;
    std::vector<double> bval(nelem + 1);
    hg::check(hfg_radial_grid(40.0, nelem, 4, 2.0, bval.data()));
    std::vector<int> lval(16), mval(16);
    int nang = 16;
    hg::check(hfg_angular_basis(1, 1, lval.data(), mval.data(), &nang));
    lval.resize(nang);
    mval.resize(nang);
    hg::atomic::TwoDBasis<Mat> basis(ctx, 2, nnodes, 5 * nnodes, bval, lval, mval);
    basis.compute_tei(true);
    const size_t N = basis.Nbf();
    Mat C(N, 2), P(N, N);
    unsigned long long st = 2025;
    auto rnd = [&]() {
      st = st * 6364136223846793005ull + 1442695040888963407ull;
      return (double)(st >> 11) / 9007199254740992.0 * 2.0 - 1.0;
    };
    for (size_t j = 0; j < 2; j++)
      for (size_t i = 0; i < N; i++) C(i, j) = rnd();
    for (size_t j = 0; j < N; j++)
      for (size_t i = 0; i < N; i++) P(i, j) = C(i, 0) * C(j, 0) + C(i, 1) * C(j, 1);
    const double alpha = 0.19, beta = 0.46;
    for (int kind = 1; kind <= 2; kind++) {
      if (kind == 1) basis.compute_yukawa(0.33);
      else basis.compute_erfc(0.33);
      const Mat K = basis.exchange(P), Krs = basis.rs_exchange(P), Kmix = basis.mix_exchange(P, alpha, beta);
      double dev = 0.0, scale = 0.0;
      for (size_t i = 0; i < N * N; i++) {
        const double want = alpha * K.d[i] + beta * Krs.d[i];
        dev = std::max(dev, std::fabs(Kmix.d[i] - want));
        scale = std::max(scale, std::fabs(want));
      }
      printf("kind %d N %zu deviation %.3e scale %.3e\n", kind, N, dev, scale);
    }
    bool logic = false;
    try {
      Mat bad(N, N - 1);
      basis.mix_exchange(bad, alpha, beta);
    } catch (const std::logic_error &) {
      logic = true;
    }
    printf("logic_error_on_shape %d\n", logic ? 1 : 0);
    printf("adapter ok\n");
  } catch (const std::exception &e) {
    printf("FAILED: %s\n", e.what());
    return 1;
  }
  return 0;
}
