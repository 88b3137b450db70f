// What the blocked eigensolve (hip/eig.hip, eig_blocks_multi_dev) and the tile engine (hip/gemm.hip) decide from numbers
// alone: which tiles and which split of K the three N^3 products take, whether F X runs as the banded row tasks, which
// outputs have to be zero first, and where a block's eigenvalues sit among all of them.  Host only, no HIP types:
// tests/cpp/eig_plan_check.cpp includes nothing else.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace hfg {
// how a GEMM task list is launched (gemm_tasklist_dev, hip/internal.h: the kernel behind every combination)
enum class GemmTile { Auto, T64, T128, T128x64 };  // Auto: gemm_prefers_128() picks T64 or T128 (T64 only up to 65535 tasks)
struct GemmHow {
  GemmTile tile = GemmTile::Auto;
  bool acc = false, split2 = false, map = false, scatter = false, klist = false;
};
}  // namespace hfg

namespace helfem {
using hfg::GemmHow;
using hfg::GemmTile;

/// 128 x 128 tiles (two workgroups per CU, 59-63 TFLOP/s when they fill the chip) or 64 x 64 tiles (three per CU, 52-56)?
/// The large tiles only when their count fills whole rounds of the slots (2 x CUs) to 85 %: 484 tiles (n = 2816) 59.1
/// against 56.1 TFLOP/s, 2304 (n = 6102) 55.8 against 54.1, 4096 (n = 8192) 63.5 against 58.5 -- but 1156 (n = 4230, 2.26
/// rounds) 47.7 against 52.1, and the 386 tiles of the eigensolve's three blocks 34 against 37 (profiles/r03_gemm_bench.txt).
/// gemm_tile (HELFEM_GEMM_TILE) = 64 / 128 forces one.
inline bool gemm_prefers_128(long tiles128, int slots, int gemm_tile) {
  if (gemm_tile) return gemm_tile == 128;
  const long rounds = (tiles128 + slots - 1) / slots;
  return tiles128 >= slots / 2 && (double)tiles128 >= 0.85 * (double)(rounds * slots);
}

/// the switches the rules below read (tuning.h: HELFEM_GEMM_TILE, _GEMM_SPLITK, _GEMM_RECT, HELFEM_MFMA)
struct EigSwitches {
  int gemm_tile = 0, gemm_splitk = -1;
  bool gemm_rect = false, mfma_4x4x4 = false;
};

struct EigProductPlan {
  GemmHow full;          // the full products F X and X Z
  GemmHow low;           // X^T (F X), of which only the lower tiles are formed (GemmTask::sym)
  bool band_fx = false;  // F X runs as the banded row tasks, not as the dense tasks
  bool zero_fx = false, zero_low = false;  // two half-K workgroups add into F X / X^T (F X): the caller zeroes them first
};
/// ns: the orders of the nb blocks of one batch; have_row_tasks: the declared pattern of F gave this batch row tasks.
/// Two workgroups per tile (split K) when the batch's large tiles would not fill the chip evenly: fewer than all of the
/// slots, in blocks of order 256 at least; gemm_splitk = 0 / 1 forces it off / on.  64 x 64 tiles unless the batch's 128 x
/// 128 tiles would fill whole rounds of the chip (gemm_prefers_128): 386 large tiles on 512 slots ran at 34 TFLOP/s as two
/// half-K workgroups each, 1452 small ones at 37 and without zeroing C.  HELFEM_GEMM_SPLITK=1 / HELFEM_GEMM_TILE=128 bring
/// the large tiles back (checkers).  The row tasks of the banded F X are 64 x 64 work with the 16x16x4 instruction: forced
/// large tiles, split K or HELFEM_MFMA keep the dense tasks.
inline EigProductPlan eig_product_plan(int nb, const int *ns, int slots, bool have_row_tasks, const EigSwitches &sw) {
  const int force_split = sw.gemm_splitk;
  long full_tiles = 0, low_tiles = 0;
  int nm = 0;
  for (int k = 0; k < nb; k++) {
    const long t1 = (ns[k] + 127) / 128;
    full_tiles += t1 * t1;
    low_tiles += t1 * (t1 + 1) / 2;
    nm = std::max(nm, ns[k]);
  }
  const bool large = gemm_prefers_128(full_tiles, slots, sw.gemm_tile);
  const bool split_full = force_split >= 0 ? force_split != 0 : (full_tiles < slots && nm >= 256);
  const bool split_low = force_split >= 0 ? force_split != 0 : (low_tiles < slots && nm >= 256);
  const bool tile64 = force_split < 0 && !large;
  EigProductPlan p;
  p.band_fx = have_row_tasks && force_split < 0 && !large && !sw.mfma_4x4x4;
  if (tile64) p.full.tile = p.low.tile = GemmTile::T64;
  else {
    if (split_full) p.full.tile = GemmTile::T128, p.full.split2 = true;
    else if (sw.gemm_rect) p.full.tile = GemmTile::T128x64;
    if (split_low) p.low.tile = GemmTile::T128, p.low.split2 = true;
  }
  p.zero_fx = p.full.split2;
  p.zero_low = p.low.split2;
  return p;
}

struct EigLastProduct {
  GemmHow how;
  bool zero_out = false;  // the block slots, or all of C on the direct path, have to be zero ahead of the product
};
/// The last product X Z (or Y^T Z).  full: the batch's EigProductPlan::full; selected: n x nev products, which take small
/// tiles and no split; direct: stored through the row and column maps straight into C, of which the product writes the
/// blocks' entries only.  The slots need zeroing where two half-K workgroups add into them.
inline EigLastProduct eig_last_product(const GemmHow &full, bool selected, bool direct) {
  EigLastProduct l;
  l.how = selected ? GemmHow{GemmTile::T64} : full;
  l.how.scatter = direct;
  l.zero_out = direct || l.how.split2;
  return l;
}

/// koff (nblk + 1 values, or null): first of block ib's eigenvalues among the wanted ones of all blocks, the lowest min(nev,
/// n_b) of every block (nev <= 0: all of them, koff = blk_ptr).  Returns their number K = koff[nblk].
inline int64_t eig_value_offsets(int nblk, const int64_t *blk_ptr, int64_t nev, int64_t *koff) {
  int64_t K = 0;
  if (koff) koff[0] = 0;
  for (int ib = 0; ib < nblk; ib++) {
    const int64_t n = blk_ptr[ib + 1] - blk_ptr[ib];
    K += nev > 0 ? std::min<int64_t>(nev, n) : n;
    if (koff) koff[ib + 1] = K;
  }
  return K;
}
/// order of the largest block; a block slot is nmax * nmax + nmax doubles (eig_block_buf_size)
inline size_t eig_block_nmax(int nblk, const int64_t *blk_ptr) {
  size_t nmax = 0;
  for (int ib = 0; ib < nblk; ib++) nmax = std::max<size_t>(nmax, blk_ptr[ib + 1] - blk_ptr[ib]);
  return nmax;
}
}  // namespace helfem
