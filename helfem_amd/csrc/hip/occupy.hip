// Fractional occupations by symmetry block on the device (hfg_occupy_blocks_devptr, include/helfem_gpu.h): from (E, C) as
// the blocked eigensolve leaves them -- ascending E, the blocks' columns interleaved -- the k-th lowest level of block b,
// scaled by sqrt(f[b][k]), into the fixed slot occ_ptr[b] + k of an N x nslots panel.  With C~_i = sqrt(f_i) C_i the
// density is P = C~ C~^T, so the density build, the low-rank exchange and the rank-nocc DIIS error take the panel as they
// take the occupied orbitals.  What scf::enforce_occupations (hip/scf_device.hip) does with an N^3 product S C, a
// read-back of all weights and a host sort, here in three launches and no trip to the host:
//
//   k_occ_argmax   one pass over C: the row of largest magnitude of every column, and that row's block
//   k_occ_rank     the rank of every column among the columns of its block, by (E, column index)
//   k_occ_gather   one workgroup per slot: the column of that block and rank, scaled, with its energy and occupation
//
// Every output element has one writer at a fixed place: no atomics, bitwise repeatable.  Launch shapes: host/occ_plan.h.
#include "internal.h"
#include "wave.h"
#include "../host/occ_plan.h"
#include <climits>
#include <cmath>

namespace hfg {
using helfem::OCC_RANK_COLS, helfem::OCC_THREADS, helfem::OCC_WAVE;

// one slot, as the host lays them out: sq = sqrt(f) from the host's correctly rounded sqrt
struct OccSlot {
  int blk, k;
  double f, sq;
};
static_assert(sizeof(OccSlot) == 24, "OccSlot is compared bytewise: keep it free of padding");

// the smallest v of the wave in every lane, for 0 <= v <= INT_MAX (exact in a double); all 64 lanes active
__device__ __forceinline__ int wave_min_index(int v) { return (int)(-wave_max(-(double)v)); }

// colblk[j] = block of the row of largest |C(i, j)| (the lowest such row), -1 for a block id outside 0 .. nblk - 1.
// cpw == 1: the workgroup strides over column blockIdx.x; cpw == 4: wave w takes column 4 blockIdx.x + w.
__global__ __launch_bounds__(OCC_THREADS) void k_occ_argmax(const double *__restrict__ C, int N, int ncols, const int *__restrict__ blockid,
                                                            int nblk, int cpw, int *__restrict__ colblk) {
  __shared__ double sbest[OCC_THREADS / OCC_WAVE];
  __shared__ int srow[OCC_THREADS / OCC_WAVE];
  const int t = threadIdx.x, lane = t & (OCC_WAVE - 1), w = t / OCC_WAVE;
  const int col = cpw == 1 ? (int)blockIdx.x : (int)blockIdx.x * cpw + w;
  const int start = cpw == 1 ? t : lane, stride = cpw == 1 ? OCC_THREADS : OCC_WAVE;
  double best = -1.0;
  int row = INT_MAX;
  if (col < ncols) {  // (uniform over the wave)
    const double *c = C + (size_t)col * N;
#pragma unroll 8
    for (int i = start; i < N; i += stride) {
      const double a = fabs(c[i]);
      if (a > best) {  // ascending i: the lowest row of a thread's maximum stays
        best = a;
        row = i;
      }
    }
  }
  const double m = wave_max(best);
  row = wave_min_index(best == m ? row : INT_MAX);
  if (cpw == 1) {
    if (lane == 0) {
      sbest[w] = m;
      srow[w] = row;
    }
    __syncthreads();
    if (t != 0) return;
    best = sbest[0];
    row = srow[0];
    for (int q = 1; q < OCC_THREADS / OCC_WAVE; q++)
      if (sbest[q] > best || (sbest[q] == best && srow[q] < row)) {
        best = sbest[q];
        row = srow[q];
      }
  } else if (lane != 0)
    return;
  if (col >= ncols) return;
  if (row < 0 || row >= N) row = 0;  // a column without one ordered magnitude (all NaN)
  const int b = blockid[row];
  colblk[col] = (b >= 0 && b < nblk) ? b : -1;
}

// rank[j] = number of columns j' of the same block with (E[j'], j') < (E[j], j).  A workgroup ranks OCC_RANK_COLS columns,
// one per lane; the others pass through LDS in tiles of OCC_THREADS (the next one loaded while this one is counted), of which
// each wave counts its quarter.
__global__ __launch_bounds__(OCC_THREADS) void k_occ_rank(const double *__restrict__ E, const int *__restrict__ colblk, int ncols,
                                                          int *__restrict__ rank) {
  __shared__ double sE[OCC_THREADS];
  __shared__ int sB[OCC_THREADS];
  __shared__ int part[OCC_THREADS / OCC_WAVE][OCC_RANK_COLS];
  const int t = threadIdx.x, lane = t & (OCC_WAVE - 1), w = t / OCC_WAVE;
  const int j = (int)blockIdx.x * OCC_RANK_COLS + lane;
  const bool live = j < ncols;
  const double myE = live ? E[j] : 0.0;
  const int myB = live ? colblk[j] : -3;
  int cnt = 0;
  // the next tile is on its way from memory while the waves count the one in LDS
  double nE = t < ncols ? E[t] : 0.0;
  int nB = t < ncols ? colblk[t] : -2;
  for (int base = 0; base < ncols; base += OCC_THREADS) {
    sE[t] = nE;
    sB[t] = nB;
    __syncthreads();
    const int jn = base + OCC_THREADS + t;
    nE = jn < ncols ? E[jn] : 0.0;
    nB = jn < ncols ? colblk[jn] : -2;
#pragma unroll 8
    for (int q = 0; q < OCC_WAVE; q++) {
      const int idx = w * OCC_WAVE + q, jp = base + idx;
      const double e = sE[idx];
      cnt += (sB[idx] == myB) & ((e < myE) | ((e == myE) & (jp < j)));
    }
    __syncthreads();
  }
  part[w][lane] = cnt;
  __syncthreads();
  if (w == 0 && live) {
    int r = 0;
    for (int q = 0; q < OCC_THREADS / OCC_WAVE; q++) r += part[q][lane];
    rank[j] = r;
  }
}

// slot s = blockIdx.x: the column of block slots[s].blk and rank slots[s].k (the lowest index, should two columns share a
// rank: energies that do not order, NaN), times sq, into Cocc[:, s]; its energy and occupation into Eocc[s], Focc[s].  An
// occupation of zero, or a slot whose column does not exist, gives a zero column (and, without a column, a zero energy).
__global__ __launch_bounds__(OCC_THREADS) void k_occ_gather(const double *__restrict__ C, const double *__restrict__ E, int N, int ncols,
                                                            const int *__restrict__ colblk, const int *__restrict__ rank,
                                                            const OccSlot *__restrict__ slots, double *__restrict__ Cocc,
                                                            double *__restrict__ Eocc, double *__restrict__ Focc) {
  __shared__ int scol[OCC_THREADS / OCC_WAVE];
  const int t = threadIdx.x, lane = t & (OCC_WAVE - 1), w = t / OCC_WAVE;
  const size_t s = blockIdx.x;
  const OccSlot sl = slots[s];
  int cand = INT_MAX;
  for (int j = t; j < ncols; j += OCC_THREADS)
    if (colblk[j] == sl.blk && rank[j] == sl.k && j < cand) cand = j;
  cand = wave_min_index(cand);
  if (lane == 0) scol[w] = cand;
  __syncthreads();
  int col = scol[0];
  for (int q = 1; q < OCC_THREADS / OCC_WAVE; q++) col = scol[q] < col ? scol[q] : col;
  const bool have = col < ncols;
  double *out = Cocc + s * N;
  if (have && sl.f != 0.0) {
    const double *c = C + (size_t)col * N;
    for (int i = t; i < N; i += OCC_THREADS) out[i] = sl.sq * c[i];
  } else
    for (int i = t; i < N; i += OCC_THREADS) out[i] = 0.0;
  if (t == 0) {
    Eocc[s] = have ? E[col] : 0.0;
    Focc[s] = sl.f;
  }
}

namespace {
// the context's workspace of the stage (workspace_owner.h, WS_OCC); DevBuf::resize only ever grows
struct OccWork : Workspace {
  DevBuf<int> colblk, rank;
  DevBuf<OccSlot> slots;
  std::vector<OccSlot> slots_host;  // what slots holds (upload_cached): an SCF run hands over the same lists every iteration
  // rows per block of the block-id array last seen, read back once per (address, N, nblk); occupy_forget_blocks drops them
  const int *bid = nullptr;
  int64_t bid_N = 0;
  int bid_nblk = 0;
  std::vector<int64_t> rows;
};

const std::vector<int64_t> &block_rows(hfg_ctx *ctx, OccWork &w, int64_t N, const int *dBlockId, int nblk) {
  if (w.bid == dBlockId && w.bid_N == N && w.bid_nblk == nblk) return w.rows;
  std::vector<int> id((size_t)N);
  HFG_HIP_CHECK(hipMemcpyAsync(id.data(), dBlockId, sizeof(int) * (size_t)N, hipMemcpyDeviceToHost, ctx->stream));
  HFG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  w.bid = nullptr;
  w.rows.assign((size_t)nblk, 0);
  for (int v : id)
    if (v >= 0 && v < nblk) w.rows[(size_t)v]++;
  w.bid = dBlockId;
  w.bid_N = N;
  w.bid_nblk = nblk;
  return w.rows;
}
}  // namespace

// the refusals that need no device (nblk, ncols, the occupations' range)
static void occupy_blocks_check(int64_t N, int64_t ncols, int nblk, const int64_t *occ_ptr, const double *occ) {
  if (nblk < 1) throw std::logic_error("hfg_occupy_blocks_devptr: nblk < 1\n");
  if (N < 1) throw std::logic_error("hfg_occupy_blocks_devptr: N < 1\n");
  if (ncols < N) throw std::logic_error("hfg_occupy_blocks_devptr: ncols < N (every block needs its columns: C has at least N)\n");
  if (!occ_ptr) throw std::logic_error("hfg_occupy_blocks_devptr: null occ_ptr\n");
  if (occ_ptr[0] != 0) throw std::logic_error("hfg_occupy_blocks_devptr: occ_ptr[0] must be 0\n");
  for (int b = 0; b < nblk; b++)
    if (occ_ptr[b + 1] < occ_ptr[b]) throw std::logic_error("hfg_occupy_blocks_devptr: occ_ptr must not decrease\n");
  if (occ_ptr[nblk] && !occ) throw std::logic_error("hfg_occupy_blocks_devptr: null occ\n");
  for (int64_t s = 0; s < occ_ptr[nblk]; s++)
    if (!(occ[s] >= 0.0 && occ[s] <= 1.0))
      throw std::logic_error("hfg_occupy_blocks_devptr: occupation " + std::to_string(s) + " outside [0, 1]\n");
}

void occupy_forget_blocks(hfg_ctx *ctx) {
  if (OccWork *w = ctx->work.find<OccWork>(WS_OCC)) w->bid = nullptr;
}

void occupy_blocks_dev(hfg_ctx *ctx, int64_t N, int64_t ncols, const double *dE, const double *dC, const int *dBlockId, int nblk,
                       const int64_t *occ_ptr, const double *occ, double *dCocc, double *dEocc, double *dFocc) {
  occupy_blocks_check(N, ncols, nblk, occ_ptr, occ);  // what needs no device comes first
  if (!ctx) throw std::logic_error("hfg_occupy_blocks_devptr: null context\n");
  const int64_t nslots = occ_ptr[nblk];
  if (!dE || !dC || !dBlockId || (nslots && (!dCocc || !dEocc || !dFocc)))
    throw std::logic_error("hfg_occupy_blocks_devptr: null device pointer\n");
  HFG_HIP_CHECK(hipSetDevice(ctx->device));
  OccWork &w = ctx->work.get<OccWork>(WS_OCC);
  const std::vector<int64_t> &rows = block_rows(ctx, w, N, dBlockId, nblk);
  for (int b = 0; b < nblk; b++)
    if (occ_ptr[b + 1] - occ_ptr[b] > rows[(size_t)b])
      throw std::logic_error("hfg_occupy_blocks_devptr: block " + std::to_string(b) + " has " + std::to_string(rows[(size_t)b]) +
                             " rows and " + std::to_string(occ_ptr[b + 1] - occ_ptr[b]) + " occupations\n");
  const helfem::OccPlan plan = helfem::occ_plan(N, ncols, nslots);
  if (plan.refused) throw std::logic_error(plan.refused);
  if (plan.gather_wgs == 0) return;
  std::vector<OccSlot> slots((size_t)nslots);
  for (int b = 0; b < nblk; b++)
    for (int64_t s = occ_ptr[b]; s < occ_ptr[b + 1]; s++) slots[(size_t)s] = {b, (int)(s - occ_ptr[b]), occ[s], std::sqrt(occ[s])};
  hipStream_t st = ctx->stream;
  upload_cached(w.slots, w.slots_host, slots, st);
  w.colblk.resize((size_t)ncols);
  w.rank.resize((size_t)ncols);
  ProfScope ps(ctx, "occupy");
  hipLaunchKernelGGL(k_occ_argmax, dim3((unsigned)plan.argmax_wgs), dim3(plan.threads), 0, st, dC, (int)N, (int)ncols, dBlockId, nblk,
                     plan.argmax_cols, w.colblk.p);
  hipLaunchKernelGGL(k_occ_rank, dim3((unsigned)plan.rank_wgs), dim3(plan.threads), 0, st, dE, w.colblk.p, (int)ncols, w.rank.p);
  hipLaunchKernelGGL(k_occ_gather, dim3((unsigned)plan.gather_wgs), dim3(plan.threads), 0, st, dC, dE, (int)N, (int)ncols, w.colblk.p,
                     w.rank.p, w.slots.p, dCocc, dEocc, dFocc);
  HFG_HIP_CHECK(hipGetLastError());
}

}  // namespace hfg
