// Chunks of the batched exchange build (hip/exchange_lr.hip, exchange_batch_dev): which densities of a batch share one pass
// over the exchange-ordered element tables.  The stages that are linear in the factors run once per chunk on the
// concatenated factor columns of its members, EXCHANGE_BATCH_RMAX columns at most.  Host only (hfg_exchange_batch_plan
// needs no device; tests/cpp/exchange_batch_plan_check.cpp includes nothing else).
#pragma once

namespace helfem {
constexpr int EXCHANGE_BATCH_RMAX = 64;  // factor columns of one pass (EXL_RMAX of exchange_lr.hip)

/// ranks[b]: factors of density b.  0: the zero matrix, which takes no columns and belongs to no chunk (chunk_of = -1);
/// negative or above EXCHANGE_BATCH_RMAX: not reproduced by one group of factors, routed alone (the single build's residual
/// groups or general kernels).  Every other density joins the chunk of the one before it while the chunk's ranks sum to at
/// most EXCHANGE_BATCH_RMAX and, with max_members > 0, it has fewer than max_members members; a density routed alone ends
/// the chunk before it.  chunk_of[b]: the chunk of density b, numbered from 0 in the order of the batch; chunks are runs of
/// consecutive densities (zero matrices aside).  Returns the number of chunks.
inline int exchange_batch_plan(long nP, const int *ranks, int max_members, int *chunk_of) {
  int nchunks = 0, cols = 0, members = 0;
  bool open = false;
  for (long b = 0; b < nP; b++) {
    const int r = ranks[b];
    if (r == 0) {
      chunk_of[b] = -1;
      continue;
    }
    if (r < 0 || r > EXCHANGE_BATCH_RMAX) {
      chunk_of[b] = nchunks++;
      open = false;
      continue;
    }
    if (!open || cols + r > EXCHANGE_BATCH_RMAX || (max_members > 0 && members >= max_members)) {
      nchunks++;
      cols = 0;
      members = 0;
      open = true;
    }
    chunk_of[b] = nchunks - 1;
    cols += r;
    members++;
  }
  return nchunks;
}
}  // namespace helfem
