// The launch rules of the occupation stage (helfem_amd/csrc/host/occ_plan.h) against their limits: a workgroup of whole
// waves within the device's 1024 threads, grids that cover every column and every slot exactly once and fit a grid
// dimension, the wave-per-column rule on both sides of its threshold, and every refusal.  Stand-alone and host only:
// tests/test_frac_occ_cpu.py builds it with the address and undefined-behaviour sanitizers.
#include "../../helfem_amd/csrc/host/occ_plan.h"

#include <cstdio>
#include <cstring>
#include <initializer_list>

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);              \
      failures++;                                                        \
    }                                                                    \
  } while (0)

static void accepted(int64_t N, int64_t ncols, int64_t nslots) {
  const helfem::OccPlan p = helfem::occ_plan(N, ncols, nslots);
  CHECK(p.refused == nullptr);
  if (p.refused) return;
  CHECK(p.threads == 256 && p.threads % 64 == 0 && p.threads <= 1024);
  // k_occ_argmax: a wave per column up to 512 rows (eight loads per lane), the workgroup per column beyond
  CHECK(p.argmax_cols == (N <= 512 ? 4 : 1));
  CHECK(p.argmax_cols * 64 <= p.threads);
  CHECK(p.argmax_wgs * p.argmax_cols >= ncols && (p.argmax_wgs - 1) * p.argmax_cols < ncols);
  // k_occ_rank: one column per lane of a wave
  CHECK(p.rank_cols == 64);
  CHECK(p.rank_wgs * p.rank_cols >= ncols && (p.rank_wgs - 1) * p.rank_cols < ncols);
  CHECK(p.gather_wgs == nslots);
  CHECK(p.argmax_wgs < (int64_t(1) << 31) && p.rank_wgs < (int64_t(1) << 31) && p.gather_wgs < (int64_t(1) << 31));
  // the kernels index C with a size_t product of two ints and rows, columns and ranks with ints
  CHECK(N <= 46340 && ncols <= (int64_t(1) << 22));
}

static void refused(int64_t N, int64_t ncols, int64_t nslots, const char *word) {
  const helfem::OccPlan p = helfem::occ_plan(N, ncols, nslots);
  CHECK(p.refused != nullptr && std::strstr(p.refused, word) != nullptr);
  CHECK(p.argmax_wgs == 0 && p.rank_wgs == 0 && p.gather_wgs == 0);  // nothing to launch from a refused plan
}

int main() {
  long cases = 0;
  const int64_t sizes[] = {1, 64, 65, 4230, 6102, 512, 513, 46340};
  for (int64_t N : sizes)
    for (int64_t extra : {int64_t(0), int64_t(1), int64_t(63), int64_t(64)})
      for (int64_t nslots : {int64_t(0), int64_t(1), int64_t(7), int64_t(64), int64_t(65), N}) {
        if (nslots > N) continue;
        accepted(N, N + extra, nslots);
        cases++;
      }
  for (int64_t N = 1; N <= 1100; N++) {
    accepted(N, N, N);
    cases++;
  }
  refused(0, 0, 0, "1 <= N");
  refused(46341, 46341, 1, "1 <= N");
  refused(65, 64, 1, "ncols < N");
  refused(4230, 0, 1, "ncols < N");
  refused(64, (int64_t(1) << 22) + 1, 1, "columns");
  refused(64, 64, 65, "slots");
  refused(64, 64, -1, "slots");
  std::printf("%ld cases in the sweep\n", cases);
  if (failures) return 1;
  std::printf("occ plan check ok\n");
  return 0;
}
