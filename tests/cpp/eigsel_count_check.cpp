// helfem::eig_sel_count on heap-allocated block lists, for a build with -fsanitize=address,undefined
// (tests/test_eigsel_cpu.py): clamping, the sum, the empty and the refused inputs.
#include "../../helfem_amd/csrc/host/eigsel_count.h"
#include <cstdio>
#include <vector>

static int64_t count(const std::vector<int64_t> &sizes, int64_t nev) {
  std::vector<int64_t> ptr(1, 0);
  for (int64_t s : sizes) ptr.push_back(ptr.back() + s);
  ptr.shrink_to_fit();
  return helfem::eig_sel_count((int)sizes.size(), ptr.data(), nev);
}

int main() {
  bool ok = count({1380, 1470, 1380}, 32) == 96 && count({1, 2, 3, 5, 31, 33}, 2) == 11 && count({7}, 100) == 7 && count({}, 3) == 0 &&
            count({4, 4}, 0) == 0 && count({4, 4}, -1) == 0 && count({3, 0, 2}, 5) == 5 && helfem::eig_sel_count(2, nullptr, 3) == 0 &&
            count({5}, INT64_MAX) == 5;
  printf(ok ? "count ok\n" : "count WRONG\n");
  return ok ? 0 : 1;
}
