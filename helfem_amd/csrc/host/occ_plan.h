// The host-side choices of the occupation stage (hip/occupy.hip, hfg_occupy_blocks_devptr): workgroup size, columns per
// workgroup and grid of its three kernels, and what the launcher refuses, from plain integers alone.  The launcher asks
// occ_plan() and keeps no copy of a rule.  A refusal comes back as the text of the std::logic_error that occupy.hip
// throws (null: accepted).  Host only: tests/cpp/occ_plan_check.cpp includes nothing else.
#pragma once
#include <cstdint>

namespace helfem {
constexpr int OCC_THREADS = 256;       // every kernel of the stage: four waves
constexpr int OCC_WAVE = 64;
constexpr int OCC_WAVE_ROWS = 512;     // columns of up to this many rows are searched by one wave each, longer ones by a workgroup
constexpr int OCC_RANK_COLS = 64;      // columns ranked per workgroup: one per lane, each wave counting a quarter of the others
constexpr int64_t OCC_MAX_N = 46340;   // N^2 fits an int, as everywhere the step objects index an N x N matrix
constexpr int64_t OCC_MAX_COLS = 1 << 22;  // columns of C (and so workgroups of a grid) at most

struct OccPlan {
  int threads;          // per workgroup, all three kernels
  int argmax_cols;      // columns per workgroup of k_occ_argmax: 1 (the workgroup strides over the column) or 4 (a wave each)
  int64_t argmax_wgs;   // ceil(ncols / argmax_cols)
  int rank_cols;        // columns per workgroup of k_occ_rank
  int64_t rank_wgs;     // ceil(ncols / rank_cols)
  int64_t gather_wgs;   // one workgroup per slot (0: no launch at all)
  const char *refused;
};

inline OccPlan occ_plan(int64_t N, int64_t ncols, int64_t nslots) {
  OccPlan p = {OCC_THREADS, 1, 0, OCC_RANK_COLS, 0, 0, nullptr};
  if (N < 1 || N > OCC_MAX_N) {
    p.refused = "hfg_occupy_blocks_devptr: 1 <= N <= 46340\n";
    return p;
  }
  if (ncols < N) {
    p.refused = "hfg_occupy_blocks_devptr: ncols < N (every block needs its columns: C has at least N)\n";
    return p;
  }
  if (ncols > OCC_MAX_COLS) {
    p.refused = "hfg_occupy_blocks_devptr: more than 4194304 columns\n";
    return p;
  }
  if (nslots < 0 || nslots > N) {
    p.refused = "hfg_occupy_blocks_devptr: 0 <= number of slots <= N\n";
    return p;
  }
  p.argmax_cols = N <= OCC_WAVE_ROWS ? OCC_THREADS / OCC_WAVE : 1;
  p.argmax_wgs = (ncols + p.argmax_cols - 1) / p.argmax_cols;
  p.rank_wgs = (ncols + p.rank_cols - 1) / p.rank_cols;
  p.gather_wgs = nslots;
  return p;
}
}  // namespace helfem
