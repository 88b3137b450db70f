// Plan of the banded product F X of the blocked eigensolve (hip/eig.hip, eig_blocks_multi_dev).  For every non-hybrid
// functional F = H0 + J + XC is local in the radial finite-element index: F(row, col) can be non-zero only when the radial
// functions of the two basis functions lie in a common element.  The ROWS of a symmetry block are taken radial-major (node
// first, then position in the caller's list), so that a 64-row tile holds three or four radial nodes; its non-zero COLUMNS,
// left in the caller's order, are then one short run per shell.  The tile becomes one GEMM task whose k loop takes only
// the steps of 16 columns that meet such a run.  The columns stay in the caller's order and every step starts at a multiple
// of 4, so each column keeps its place in the summation of the dense product and the skipped terms are exact zeros: the
// result is bit for bit the dense one.  Host only: tests/cpp/eig_band_plan_check.cpp includes nothing else.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

namespace helfem {
constexpr int EIG_BAND_TILE = 64;    // rows of a task: the 64 x 64 tiles of k_dgemm_tasklist
constexpr int EIG_BAND_K0_ALIGN = 4; // first column of a step: the group of four columns of one matrix instruction (and the
                                     // 16-byte staging loads of both operands) start there
constexpr int EIG_BAND_KSTEP = 16;   // columns of a step: the tile engine's k step
// A block keeps the dense product when it has a single row tile or when its tiles together take more than this fraction
// of the dense product's k steps.  A row task costs what its share of the dense task costs (same tiles, same prologue and
// epilogue, a shorter k loop), so any fraction below 1 gains; 0.9 keeps blocks out whose gain would be lost in the noise.
constexpr double EIG_BAND_MAX_FRACTION = 0.9;

// (the two functions below also run inside the kernel that checks H0 against the pattern)
#if defined(__HIPCC__)
#define HELFEM_BAND_HD __host__ __device__
#else
#define HELFEM_BAND_HD
#endif
/// nodes [lo, hi] that share an element with radial node n: n lies in element n / pm and, when it is a shared node, in the
/// one before (pm = p - 1 nodes per element not counting the shared one, E elements)
HELFEM_BAND_HD inline void eig_band_node_range(int n, int pm, int E, int &lo, int &hi) {
  const int e1 = n / pm;
  const int ehi = e1 < E - 1 ? e1 : E - 1;
  const int el = (n % pm == 0 && e1 >= 1) ? e1 - 1 : e1;
  const int elo = el < E - 1 ? el : E - 1;
  lo = elo * pm;
  hi = ehi * pm + pm;
}
HELFEM_BAND_HD inline bool eig_band_share(int n, int m, int pm, int E) {
  int lo, hi;
  eig_band_node_range(n, pm, E, lo, hi);
  return m >= lo && m <= hi;
}

/// perm: the positions 0 .. n-1 of a block's index list ordered by (node, position)
inline void eig_band_order(int64_t n, const int *node, int64_t *perm) {
  std::iota(perm, perm + n, (int64_t)0);
  std::stable_sort(perm, perm + n, [&](int64_t a, int64_t b) { return node[a] < node[b]; });
}

/// node: the nodes of a block in the caller's order; perm: eig_band_order's.  For row tile t (rows perm[64 t ...]) the k
/// steps kstart[toff[t] ... toff[t + 1]): ascending multiples of EIG_BAND_K0_ALIGN, at least EIG_BAND_KSTEP apart, below n;
/// every column (in the caller's order) that shares an element with a row of the tile lies in [start, start + 16) of one
/// of them.  Returns true when the block is worth the row tasks; otherwise every tile gets the steps 0, 16, 32, ...: the
/// dense product.
inline bool eig_band_plan(int64_t n, const int *node, const int64_t *perm, int pm, int E, std::vector<int> &kstart, std::vector<int> &toff) {
  const int nt = (int)((n + EIG_BAND_TILE - 1) / EIG_BAND_TILE);
  kstart.clear();
  toff.assign(1, 0);
  for (int t = 0; t < nt; t++) {
    const int64_t i0 = (int64_t)t * EIG_BAND_TILE, i1 = std::min<int64_t>(n, i0 + EIG_BAND_TILE);
    int lo = 0, hi = 0;
    for (int64_t i = i0; i < i1; i++) {
      int l, h;
      eig_band_node_range(node[perm[i]], pm, E, l, h);
      lo = (i == i0) ? l : std::min(lo, l);
      hi = (i == i0) ? h : std::max(hi, h);
    }
    int64_t next = 0;  // first column no step covers yet
    for (int64_t k = 0; k < n; k++) {
      if (k < next || node[k] < lo || node[k] > hi) continue;
      const int64_t st = k - k % EIG_BAND_K0_ALIGN;  // (>= next: next is a multiple of the alignment)
      kstart.push_back((int)st);
      next = st + EIG_BAND_KSTEP;
    }
    toff.push_back((int)kstart.size());
  }
  const double dense_steps = (double)nt * (double)((n + EIG_BAND_KSTEP - 1) / EIG_BAND_KSTEP);
  const bool banded = nt >= 2 && (double)kstart.size() <= EIG_BAND_MAX_FRACTION * dense_steps;
  if (!banded) {
    kstart.clear();
    toff.assign(1, 0);
    for (int t = 0; t < nt; t++) {
      for (int64_t k = 0; k < n; k += EIG_BAND_KSTEP) kstart.push_back((int)k);
      toff.push_back((int)kstart.size());
    }
  }
  return banded;
}
}  // namespace helfem
