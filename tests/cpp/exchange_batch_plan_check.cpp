// The chunk planner of the batched exchange build on hand-made rank lists, as a stand-alone program (host only: it
// includes the planner's header and nothing else of the library).  tests/test_exchange_batch_cpu.py compiles it with
// -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../helfem_amd/csrc/host/exchange_batch_plan.h"

static int failures = 0;

static void expect(const char *what, const std::vector<int> &ranks, int max_members, const std::vector<int> &want, int want_chunks) {
  std::vector<int> got(ranks.size(), -7);  // exactly nP entries: a write beyond them is the sanitizer's to find
  const int n = helfem::exchange_batch_plan((long)ranks.size(), ranks.data(), max_members, got.data());
  const bool ok = n == want_chunks && got == want;
  std::printf("%s: %s\n", what, ok ? "ok" : "FAILED");
  if (!ok) failures++;
  // no chunk exceeds the column limit, whatever the list
  std::vector<int> cols(n > 0 ? n : 0, 0);
  for (size_t b = 0; b < ranks.size(); b++)
    if (got[b] >= 0 && ranks[b] > 0 && ranks[b] <= helfem::EXCHANGE_BATCH_RMAX) cols[got[b]] += ranks[b];
  for (int c : cols)
    if (c > helfem::EXCHANGE_BATCH_RMAX) {
      std::printf("%s: a chunk of %d columns\n", what, c);
      failures++;
    }
}

int main() {
  expect("(21, 21, 30) splits after the second", {21, 21, 30}, 0, {0, 0, 1}, 2);
  expect("a rank of 0 takes no columns", {32, 0, 32, 1}, 0, {0, -1, 0, 1}, 2);
  expect("a rank above 64 is routed alone", {5, 70, 5, 5}, 0, {0, 1, 2, 2}, 3);
  expect("a density that is not reproduced is routed alone", {5, -1, 5}, 0, {0, 1, 2}, 3);
  expect("chunks of one", {2, 5, 1}, 1, {0, 1, 2}, 3);
  expect("chunks of two", {2, 5, 1}, 2, {0, 0, 1}, 2);
  expect("64 columns exactly", {64, 1, 63, 1}, 0, {0, 1, 1, 2}, 3);
  expect("empty batch", {}, 0, {}, 0);
  std::vector<int> many(1000), want(1000);
  for (int b = 0; b < 1000; b++) {
    many[b] = 1 + (b * 7) % 23;
    want[b] = 0;
  }
  {  // long list: only the column limit is checked (expect() recomputes it), the chunk numbers against a plain restatement
    int c = 0, cols = 0;
    for (int b = 0; b < 1000; b++) {
      if (b && cols + many[b] > 64) {
        c++;
        cols = 0;
      }
      cols += many[b];
      want[b] = c;
    }
    expect("1000 densities", many, 0, want, c + 1);
  }
  std::printf(failures ? "plan check FAILED\n" : "plan check ok\n");
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
