// Number of eigenpairs a selected solve returns: from every block the lowest min(nev, n_b).  Host only (hfg_eig_sel_count
// needs no device; tests/cpp/eigsel_count_check.cpp runs it under the address and undefined-behaviour sanitizers).
#pragma once
#include <algorithm>
#include <cstdint>

namespace helfem {
inline int64_t eig_sel_count(int nblk, const int64_t *blk_ptr, int64_t nev) {
  if (nblk < 0 || !blk_ptr || nev < 1) return 0;
  int64_t K = 0;
  for (int ib = 0; ib < nblk; ib++) K += std::min<int64_t>(nev, std::max<int64_t>(0, blk_ptr[ib + 1] - blk_ptr[ib]));
  return K;
}
}  // namespace helfem
