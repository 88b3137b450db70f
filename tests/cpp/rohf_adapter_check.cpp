// helfem::gpu::scf::ROHF_update through include/helfem_gpu_arma.hpp with the reference's argument list, on a problem whose
// answer is known in closed form: S = 1 (Sh = Sinvh = 1), Ca_o = (e0, e1), Cb_o = (e0), so P = diag(2, 1, 0, ...), the core
// orbital is e0, the active one e1 and lambda couples e0 with e2 ... e(N-1): lambda(0, v) = lambda(v, 0) = -Delta(0, v).
// Prints the largest deviation, which tests/test_gpu_rohf_run.py checks.
//   rohf_adapter_check compile-only | run
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
    const size_t N = 37;
    Mat Fa(N, N), Fb(N, N), P(N, N), Sh(N, N), Sinvh(N, N);
    unsigned long long st = 2024;
    auto rnd = [&]() {
      st = st * 6364136223846793005ull + 1442695040888963407ull;
      return (double)(st >> 11) / 9007199254740992.0 * 2.0 - 1.0;
    };
    for (size_t j = 0; j < N; j++) {
      Sh(j, j) = Sinvh(j, j) = 1.0;
      for (size_t i = j; i < N; i++) {
        Fa(i, j) = Fa(j, i) = rnd();
        Fb(i, j) = Fb(j, i) = rnd();
      }
    }
    P(0, 0) = 2.0;
    P(1, 1) = 1.0;
    const Mat Fa0 = Fa, Fb0 = Fb;
    hg::scf::ROHF_update(*ctx, Fa, Fb, P, Sh, Sinvh, 2, 1);
    double dev = 0.0, anti = 0.0;
    for (size_t j = 0; j < N; j++)
      for (size_t i = 0; i < N; i++) {
        const bool cv = (i == 0 && j >= 2) || (j == 0 && i >= 2);
        const double want = cv ? -0.5 * (Fa0(i, j) - Fb0(i, j)) : 0.0;
        dev = std::max(dev, std::fabs(Fa(i, j) - Fa0(i, j) - want));
        anti = std::max(anti, std::fabs((Fa(i, j) - Fa0(i, j)) + (Fb(i, j) - Fb0(i, j))));
      }
    printf("deviation %.3e opposite %.3e\n", dev, anti);
    // equal occupations: nothing to constrain, the matrices come back bit for bit
    Mat Fa1 = Fa0, Fb1 = Fb0;
    hg::scf::ROHF_update(*ctx, Fa1, Fb1, P, Sh, Sinvh, 1, 1);
    printf("untouched %d\n", (Fa1.d == Fa0.d && Fb1.d == Fb0.d) ? 1 : 0);
    bool logic = false;
    try {
      Mat bad(N, N - 1);
      hg::scf::ROHF_update(*ctx, Fa1, Fb1, bad, Sh, Sinvh, 2, 1);
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
