// Device-resident DIIS accelerator on the caller's device pointers (hfg_diis_*, include/helfem_gpu.h): the reference's
// uDIIS::update / solve_F (src/general/diis.cpp:129-168, 392-412) with the history of Fock, density and error matrices in
// a ring in HBM that the object owns.  The small problem (ADIIS + CDIIS weights, dropping of entries) is helfem::DiisMixer
// (host/diis.h), the same arithmetic the device SCF driver (scf_device.hip) uses; that driver keeps its own private ring
// and is not touched by this file.
//
// Device code of this file:
//   k_diis_lowrank_err   err = A B^T - B A^T for A = X^T F C_o, B = X^T S C_o (n x nocc each, nocc <= DIIS_LR_MAXCOLS):
//                        one 32 x 32 tile of the lower triangle per workgroup, the mirrored tile written with the opposite
//                        sign, max |err| per workgroup in the same launch
//   k_diis_history       one pass over the ring: err_new . err_j, P_j . F_new, P_new . F_j for every stored j
//   k_diis_extrapolate   F_out = sum_j w_j F_j for both spins in one pass
// Every reduction is per-workgroup partials in a fixed grid plus a finishing launch that adds them in index order: no
// floating-point atomics, so two objects fed the same matrices produce the same bits.
#include "internal.h"
#include "../host/diis.h"
#include <algorithm>
#include <cmath>
#include <deque>
#include <memory>

namespace hfg {

namespace {

constexpr int RED_BLOCKS = 1024;  // grid of the history pass: four workgroups per CU
constexpr int HIST_ROWS = 3 * DIIS_HIST_CHUNK + 1;  // partial sums per workgroup: B, T(j, new), T(new, j) rows and max |err|

__global__ __launch_bounds__(256) void k_diis_lowrank_err(const DiisErrTask *__restrict__ tasks, double *__restrict__ partialmax) {
  const DiisErrTask t = tasks[blockIdx.z];
  const int bi = blockIdx.x, bj = blockIdx.y;
  const size_t pidx = ((size_t)blockIdx.z * gridDim.y + bj) * gridDim.x + bi;
  const int i0 = bi * 32, j0 = bj * 32;
  if (bj > bi || i0 >= t.n) {  // the upper triangle is written by the mirrored tiles
    if (threadIdx.x == 0) partialmax[pidx] = 0.0;
    return;
  }
  __shared__ double sAi[32][32], sBi[32][32], sAj[32][32], sBj[32][32];  // [k][row]
  __shared__ double sT[32][33];
  __shared__ double smax[4];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < t.k; k0 += 32) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int kk = ty + 8 * c, k = k0 + kk;
      const bool oki = k < t.k && i0 + tx < t.n, okj = k < t.k && j0 + tx < t.n;
      const size_t oi = (size_t)k * t.ld + i0 + tx, oj = (size_t)k * t.ld + j0 + tx;
      sAi[kk][tx] = oki ? t.A[oi] : 0.0;
      sBi[kk][tx] = oki ? t.B[oi] : 0.0;
      sAj[kk][tx] = okj ? t.A[oj] : 0.0;
      sBj[kk][tx] = okj ? t.B[oj] : 0.0;
    }
    __syncthreads();
    const int kc = min(32, t.k - k0);
    for (int kk = 0; kk < kc; kk++) {
      const double a = sAi[kk][tx], b = sBi[kk][tx];
#pragma unroll
      for (int c = 0; c < 4; c++) acc[c] += a * sBj[kk][ty + 8 * c] - b * sAj[kk][ty + 8 * c];
    }
    __syncthreads();
  }
  // a diagonal tile keeps its lower triangle only: the diagonal is zero and the upper triangle is the mirror, bit for bit
  double m = 0.0;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const int j = ty + 8 * c;
    if (bi == bj && j >= tx) acc[c] = 0.0;
    m = fmax(m, fabs(acc[c]));
    if (i0 + tx < t.n && j0 + j < t.n && (bi != bj || j <= tx)) t.out[(size_t)(j0 + j) * t.ldo + i0 + tx] = acc[c];
    sT[tx][j] = -acc[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const int il = ty + 8 * c;  // err(j0 + tx, i0 + il) = -err(i0 + il, j0 + tx)
    if (i0 + il < t.n && j0 + tx < t.n && (bi != bj || tx < il)) t.out[(size_t)(i0 + il) * t.ldo + j0 + tx] = sT[il][tx];
  }
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_down(m, o, 64));
  if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) partialmax[pidx] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
}

// out = max of count non-negative values (the maximum does not depend on the order it is taken in)
__global__ __launch_bounds__(64) void k_diis_finish_max(const double *__restrict__ partial, size_t count, double *__restrict__ out) {
  double m = 0.0;
  for (size_t i = threadIdx.x; i < count; i += 64) m = fmax(m, partial[i]);
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_down(m, o, 64));
  if (threadIdx.x == 0) *out = m;
}

// partial[q * gridDim.x + block]: q = k, CHUNK + k, 2 CHUNK + k for entry k of the chunk, 3 CHUNK for max |err_new|
template <bool WANT_MAX>
__global__ __launch_bounds__(256) void k_diis_history(DiisHistory h, const double *__restrict__ Enew, size_t elen, const double *__restrict__ Pnew,
                                                      const double *__restrict__ Fnew, size_t flen, double *__restrict__ partial) {
  constexpr int CH = DIIS_HIST_CHUNK;
  __shared__ double sh[HIST_ROWS][4];
  double s[HIST_ROWS];
#pragma unroll
  for (int q = 0; q < HIST_ROWS; q++) s[q] = 0.0;
  const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  for (size_t i = first; i < elen; i += stride) {
    const double e = Enew[i];
    if (WANT_MAX) s[3 * CH] = fmax(s[3 * CH], fabs(e));
#pragma unroll
    for (int k = 0; k < CH; k++)
      if (k < h.n) s[k] += h.E[k][i] * e;
  }
  for (size_t i = first; i < flen; i += stride) {
    const double p = Pnew[i], f = Fnew[i];
#pragma unroll
    for (int k = 0; k < CH; k++)
      if (k < h.n) {
        s[CH + k] += h.P[k][i] * f;
        s[2 * CH + k] += p * h.F[k][i];
      }
  }
#pragma unroll
  for (int q = 0; q < HIST_ROWS; q++) {
    double v = s[q];
    if (q == 3 * CH) {
      for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    } else {
      for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    }
    if ((threadIdx.x & 63) == 0) sh[q][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  const int q = threadIdx.x;
  if (q < 3 * CH) partial[(size_t)q * gridDim.x + blockIdx.x] = (sh[q][0] + sh[q][1]) + (sh[q][2] + sh[q][3]);
  else if (q == 3 * CH) partial[(size_t)q * gridDim.x + blockIdx.x] = fmax(fmax(sh[q][0], sh[q][1]), fmax(sh[q][2], sh[q][3]));
}

// res[1 + kind * nhtot + j0 + k] = the nb partials of row (kind, k) added in index order, one thread per row
__global__ __launch_bounds__(64) void k_diis_finish_history(const double *__restrict__ partial, int nb, int nchunk, int j0, int nhtot, double *__restrict__ res) {
  const int q = threadIdx.x, kind = q / DIIS_HIST_CHUNK, k = q % DIIS_HIST_CHUNK;
  if (q >= 3 * DIIS_HIST_CHUNK || k >= nchunk) return;
  double s = 0.0;
  for (int i = 0; i < nb; i++) s += partial[(size_t)q * nb + i];
  res[1 + kind * nhtot + j0 + k] = s;
}

__global__ __launch_bounds__(256) void k_diis_extrapolate(DiisComb c, size_t NN, int nspin, double *__restrict__ Fa, double *__restrict__ Fb) {
  const size_t len = NN * nspin, stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < len; i += stride) {
    double acc = c.w[0] * c.F[0][i];
#pragma unroll
    for (int k = 1; k < 16; k++)
      if (k < c.n) acc += c.w[k] * c.F[k][i];
    if (i < NN) Fa[i] = acc;
    else Fb[i - NN] = acc;
  }
}

// E = X - X^T for a matrix of order n
__global__ void k_diis_antisym(const double *__restrict__ X, int n, double *__restrict__ E) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i < n) E[(size_t)j * n + i] = X[(size_t)j * n + i] - X[(size_t)i * n + j];
}
// out (nr x ncol, column-major, ld nr) = M(rows, cols) of a matrix with N rows; cols null: the leading ncol columns
__global__ void k_diis_gather(const double *__restrict__ M, int N, const int64_t *__restrict__ rows, const int64_t *__restrict__ cols, int nr,
                              double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i < nr) out[(size_t)j * nr + i] = M[(size_t)(cols ? cols[j] : j) * N + rows[i]];
}

}  // namespace

size_t diis_lowrank_partials(int ntasks, int nmax) {
  const size_t t = (size_t)(nmax + 31) / 32;
  return t * t * (size_t)std::max(ntasks, 0);
}

void diis_lowrank_error_dev(hfg_ctx *ctx, const DiisErrTask *dtasks, int ntasks, int nmax, double *dPartialMax, double *dMax) {
  if (ntasks <= 0 || nmax <= 0) {
    HFG_HIP_CHECK(hipMemsetAsync(dMax, 0, sizeof(double), ctx->stream));
    return;
  }
  if (ntasks > 65535) throw std::logic_error("diis_lowrank_error_dev: more than 65535 tasks\n");
  const unsigned t = (unsigned)(nmax + 31) / 32;
  hipLaunchKernelGGL(k_diis_lowrank_err, dim3(t, t, ntasks), dim3(256), 0, ctx->stream, dtasks, dPartialMax);
  hipLaunchKernelGGL(k_diis_finish_max, dim3(1), dim3(64), 0, ctx->stream, dPartialMax, diis_lowrank_partials(ntasks, nmax), dMax);
  HFG_HIP_CHECK(hipGetLastError());
}

void diis_history_dev(hfg_ctx *ctx, const DiisHistory &h, int j0, int nhtot, const double *dEnew, size_t elen, const double *dPnew,
                      const double *dFnew, size_t flen, bool want_max, double *dPartial, double *dRes) {
  if (h.n < 1 || h.n > DIIS_HIST_CHUNK) throw std::logic_error("diis_history_dev: 1 to DIIS_HIST_CHUNK entries per pass\n");
  if (want_max) {
    hipLaunchKernelGGL(k_diis_history<true>, dim3(RED_BLOCKS), dim3(256), 0, ctx->stream, h, dEnew, elen, dPnew, dFnew, flen, dPartial);
    hipLaunchKernelGGL(k_diis_finish_max, dim3(1), dim3(64), 0, ctx->stream, dPartial + (size_t)3 * DIIS_HIST_CHUNK * RED_BLOCKS,
                       (size_t)RED_BLOCKS, dRes);
  } else
    hipLaunchKernelGGL(k_diis_history<false>, dim3(RED_BLOCKS), dim3(256), 0, ctx->stream, h, dEnew, elen, dPnew, dFnew, flen, dPartial);
  hipLaunchKernelGGL(k_diis_finish_history, dim3(1), dim3(64), 0, ctx->stream, dPartial, RED_BLOCKS, h.n, j0, nhtot, dRes);
  HFG_HIP_CHECK(hipGetLastError());
}

void diis_extrapolate_dev(hfg_ctx *ctx, const DiisComb &c, size_t NN, int nspin, double *dFa, double *dFb) {
  if (c.n < 1 || c.n > 16) throw std::logic_error("diis_extrapolate_dev: 1 to 16 terms\n");
  hipLaunchKernelGGL(k_diis_extrapolate, dim3(2048), dim3(256), 0, ctx->stream, c, NN, nspin, dFa, dFb);
  HFG_HIP_CHECK(hipGetLastError());
}

}  // namespace hfg

using hfg::DevBuf;
using hfg::DiisErrTask;
using hfg::GemmTask;

struct hfg_diis {
  hfg_ctx *ctx;
  size_t N, NN;
  int nspin, order;
  helfem::DiisMixer mixer;
  std::deque<int> slots;          // ring slots in age order
  std::vector<double> Bh, Th, Eh;  // the mixer's B and T (order x order, entries [0, size) in use) and energies, for the read-backs
  std::vector<double> wlast;
  // metric
  size_t n = 0;  // columns of Sinvh
  DevBuf<double> S, X;
  // symmetry blocks: unit u = spin * nblk + block.  Without blocks one unit per spin on the matrices themselves.
  int nblk = 0;
  std::vector<int64_t> ptr;
  std::vector<int64_t> hcols;
  std::vector<int> nb;
  std::vector<size_t> eoff;
  size_t elen = 0;  // stored error elements per spin
  int nrmax = 0, ncmax = 0;
  DevBuf<int64_t> rows, cols;
  DevBuf<double> Sg, Xg, Fg, Pg, Cg;
  size_t ccs = 0;  // doubles per unit in Cg: nrmax x the largest nocc of this update
  // ring and workspaces
  std::unique_ptr<DevBuf<double>[]> histF, histP, histE;
  DevBuf<double> Cown, T1, T2, lrT, lrG, partial, lrmax, res;
  double *hres = nullptr;  // pinned
  struct SlotTasks {
    DevBuf<GemmTask> g;
    std::vector<GemmTask> gc;
    DevBuf<DiisErrTask> e;
    std::vector<DiisErrTask> ec;
  };
  std::unique_ptr<SlotTasks[]> tasks;
  int newest = -1;

  hfg_diis(hfg_ctx *c, size_t N_, int nspin_, int order_, double eps, double thr, int mode)
      : ctx(c), N(N_), NN(N_ * N_), nspin(nspin_), order(order_), mixer(mode != 2, eps, thr, mode != 1, false, (size_t)order_) {
    Bh.assign((size_t)order * order, 0.0);
    Th.assign((size_t)order * order, 0.0);
    histF.reset(new DevBuf<double>[order]);
    histP.reset(new DevBuf<double>[order]);
    histE.reset(new DevBuf<double>[order]);
    tasks.reset(new SlotTasks[order]);
    res.resize(1 + 3 * (size_t)order);
    partial.resize((size_t)hfg::HIST_ROWS * hfg::RED_BLOCKS);
    HFG_HIP_CHECK(hipHostMalloc((void **)&hres, sizeof(double) * (1 + 3 * (size_t)order)));
  }
  ~hfg_diis() {
    if (hres) (void)hipHostFree(hres);
  }

  void clear_history() {
    while (mixer.size()) mixer.pop_oldest();
    slots.clear();
    Eh.clear();
    wlast.clear();
    newest = -1;
  }
  void pop_oldest_host() {
    const size_t sz = Eh.size();
    for (size_t i = 1; i < sz; i++)
      for (size_t j = 1; j < sz; j++) {
        Bh[(i - 1) * order + (j - 1)] = Bh[i * order + j];
        Th[(i - 1) * order + (j - 1)] = Th[i * order + j];
      }
    Eh.erase(Eh.begin());
    slots.pop_front();
  }
  void layout_single_block() {
    nblk = 0;
    elen = n * n;
    nrmax = (int)N;
    ncmax = (int)n;
  }
  void alloc_ring() {
    for (int k = 0; k < order; k++) {
      histF[k].resize(nspin * NN);
      histP[k].resize(nspin * NN);
      histE[k].resize(nspin * std::max<size_t>(elen, 1));
      tasks[k].gc.clear();
      tasks[k].ec.clear();
    }
  }

  void set_metric(const double *dS, const double *dX, int64_t ncol) {
    if (!dS || !dX) throw std::logic_error("hfg_diis_set_metric_devptr: null matrix pointer\n");
    if (ncol < 1 || (size_t)ncol > N) throw std::logic_error("hfg_diis_set_metric_devptr: Sinvh has 1 to N columns\n");
    hipStream_t s = ctx->stream;
    HFG_HIP_CHECK(hipStreamSynchronize(s));  // task lists in flight may still name the old layout
    clear_history();
    n = (size_t)ncol;
    S.resize(NN);
    X.resize(N * n);
    HFG_HIP_CHECK(hipMemcpyAsync(S.p, dS, sizeof(double) * NN, hipMemcpyDeviceToDevice, s));
    HFG_HIP_CHECK(hipMemcpyAsync(X.p, dX, sizeof(double) * N * n, hipMemcpyDeviceToDevice, s));
    layout_single_block();
    alloc_ring();
  }

  void set_blocks(int nblk_, const int64_t *blk_ptr, const int64_t *blk_idx) {
    if (!n) throw std::logic_error("hfg_diis_set_blocks: set the metric first\n");
    if (mixer.size()) throw std::logic_error("hfg_diis_set_blocks: the history is not empty\n");
    hipStream_t s = ctx->stream;
    HFG_HIP_CHECK(hipStreamSynchronize(s));
    if (nblk_ <= 0) {
      layout_single_block();
      alloc_ring();
      return;
    }
    if (!blk_ptr || !blk_idx) throw std::logic_error("hfg_diis_set_blocks: null block arrays\n");
    if (n != N) throw std::logic_error("hfg_diis_set_blocks: symmetry blocks need a square Sinvh\n");
    if (blk_ptr[0] != 0 || blk_ptr[nblk_] != (int64_t)N) throw std::logic_error("hfg_diis_set_blocks: the blocks must cover every basis function\n");
    std::vector<char> seen(N, 0);
    for (int64_t k = 0; k < (int64_t)N; k++) {
      if (blk_idx[k] < 0 || blk_idx[k] >= (int64_t)N || seen[blk_idx[k]]) throw std::logic_error("hfg_diis_set_blocks: the blocks must be a permutation of the basis functions\n");
      seen[blk_idx[k]] = 1;
    }
    std::vector<int64_t> c;
    hfg::eig_block_supports(ctx, (int)N, X.p, nblk_, blk_ptr, blk_idx, c);
    nblk = nblk_;
    ptr.assign(blk_ptr, blk_ptr + nblk + 1);
    hcols = c;
    nb.resize(nblk);
    eoff.resize(nblk);
    nrmax = 0;
    elen = 0;
    for (int b = 0; b < nblk; b++) {
      if (ptr[b + 1] < ptr[b]) throw std::logic_error("hfg_diis_set_blocks: block pointers must ascend\n");
      nb[b] = (int)(ptr[b + 1] - ptr[b]);
      nrmax = std::max(nrmax, nb[b]);
      eoff[b] = elen;
      elen += (size_t)nb[b] * nb[b];
    }
    ncmax = nrmax;
    std::vector<int64_t> r(blk_idx, blk_idx + N);
    rows.upload(r, s);
    cols.upload(c, s);
    const size_t sl = (size_t)nrmax * nrmax;
    Sg.resize(sl * nblk);
    Xg.resize(sl * nblk);
    Fg.resize(sl * nblk * nspin);
    for (int b = 0; b < nblk; b++) {
      if (!nb[b]) continue;
      dim3 g((nb[b] + 255) / 256, nb[b]);
      hipLaunchKernelGGL(hfg::k_diis_gather, g, dim3(256), 0, s, S.p, (int)N, rows.p + ptr[b], rows.p + ptr[b], nb[b], Sg.p + sl * b);
      hipLaunchKernelGGL(hfg::k_diis_gather, g, dim3(256), 0, s, X.p, (int)N, rows.p + ptr[b], cols.p + ptr[b], nb[b], Xg.p + sl * b);
    }
    HFG_HIP_CHECK(hipStreamSynchronize(s));  // r and c are locals
    alloc_ring();
  }

  // operands of unit (sp, b) for the entry in ring slot `slot`
  struct Unit {
    const double *F, *P, *C, *Sb, *Xb;
    int nr, nc, ldF, ldS, ldX, ldC;
    double *out;
  };
  Unit unit(int slot, int sp, int b) const {
    Unit u;
    if (nblk == 0) {
      u.F = histF[slot].p + sp * NN;
      u.P = histP[slot].p + sp * NN;
      u.C = Cown.p ? Cown.p + sp * NN : nullptr;
      u.Sb = S.p;
      u.Xb = X.p;
      u.nr = (int)N;
      u.nc = (int)n;
      u.ldF = u.ldS = u.ldX = u.ldC = (int)N;
      u.out = histE[slot].p + sp * elen;
    } else {
      const size_t sl = (size_t)nrmax * nrmax, k = (size_t)sp * nblk + b;
      u.F = Fg.p + sl * k;
      u.P = Pg.p ? Pg.p + sl * k : nullptr;
      u.C = Cg.p ? Cg.p + ccs * k : nullptr;
      u.Sb = Sg.p + sl * b;
      u.Xb = Xg.p + sl * b;
      u.nr = u.nc = nb[b];
      u.ldF = u.ldS = u.ldX = u.ldC = nb[b];
      u.out = histE[slot].p + sp * elen + eoff[b];
    }
    return u;
  }

  // A failure between the first change of the ring and the last (a HIP error, an allocation) would leave the slot list, the
  // energies and the mixer with different lengths and a ring slot half written: the history is emptied and the cached
  // task lists forgotten before the error goes on to the caller, whose next update starts a new history.
  double update(double E, const double *const *F, const double *const *P, const double *const *C, const int64_t *nocc) {
    try {
      return update_entry(E, F, P, C, nocc);
    } catch (...) {
      clear_history();
      for (int k = 0; k < order; k++) {
        tasks[k].gc.clear();
        tasks[k].ec.clear();
      }
      throw;
    }
  }
  double update_entry(double E, const double *const *F, const double *const *P, const double *const *C, const int64_t *nocc) {
    if (!n) throw std::logic_error("hfg_diis_update_devptr: set the metric first\n");
    for (int sp = 0; sp < nspin; sp++) {
      if (!F[sp] || !P[sp]) throw std::logic_error("hfg_diis_update_devptr: null Fock or density matrix\n");
      if (nocc[sp] < 0 || nocc[sp] > (int64_t)N) throw std::logic_error("hfg_diis_update_devptr: 0 <= nocc <= N\n");
    }
    hipStream_t s = ctx->stream;
    hfg::ProfScope ps(ctx, "diis_update");
    // the low-rank route needs the occupied orbitals of every spin that has any, at most DIIS_LR_MAXCOLS of them; anything
    // else takes the four dense products (a routing, not an error)
    bool lowrank = C[0] && nocc[0] > 0;
    if (nspin == 2 && nocc[1] > 0 && !C[1]) lowrank = false;
    const int kmax = (int)std::max(nocc[0], nspin == 2 ? nocc[1] : (int64_t)0);
    if (kmax > hfg::DIIS_LR_MAXCOLS) lowrank = false;

    int slot;
    if (mixer.full()) {
      mixer.pop_oldest();
      slot = slots.front();
      pop_oldest_host();
    } else {
      slot = -1;
      for (int q = 0; q < order && slot < 0; q++)
        if (std::find(slots.begin(), slots.end(), q) == slots.end()) slot = q;
    }
    slots.push_back(slot);
    newest = slot;
    const int nu = nblk ? nblk : 1;
    const size_t sl = (size_t)nrmax * nrmax;
    if (lowrank) {
      Cown.resize(nspin * NN);
      ccs = (size_t)nrmax * kmax;  // (a block may have fewer rows than there are orbitals)
      if (nblk) Cg.resize(ccs * nblk * nspin);
    } else if (nblk)
      Pg.resize(sl * nblk * nspin);
    for (int sp = 0; sp < nspin; sp++) {
      HFG_HIP_CHECK(hipMemcpyAsync(histF[slot].p + sp * NN, F[sp], sizeof(double) * NN, hipMemcpyDeviceToDevice, s));
      HFG_HIP_CHECK(hipMemcpyAsync(histP[slot].p + sp * NN, P[sp], sizeof(double) * NN, hipMemcpyDeviceToDevice, s));
      if (lowrank && nocc[sp])
        HFG_HIP_CHECK(hipMemcpyAsync(Cown.p + sp * NN, C[sp], sizeof(double) * N * (size_t)nocc[sp], hipMemcpyDeviceToDevice, s));
      for (int b = 0; b < nblk; b++) {
        if (!nb[b]) continue;
        const Unit u = unit(slot, sp, b);
        dim3 g((nb[b] + 255) / 256, nb[b]);
        hipLaunchKernelGGL(hfg::k_diis_gather, g, dim3(256), 0, s, histF[slot].p + sp * NN, (int)N, rows.p + ptr[b], rows.p + ptr[b], nb[b],
                           const_cast<double *>(u.F));
        if (!lowrank)
          hipLaunchKernelGGL(hfg::k_diis_gather, g, dim3(256), 0, s, histP[slot].p + sp * NN, (int)N, rows.p + ptr[b], rows.p + ptr[b], nb[b],
                             const_cast<double *>(u.P));
        else if (nocc[sp])
          hipLaunchKernelGGL(hfg::k_diis_gather, dim3((nb[b] + 255) / 256, (unsigned)nocc[sp]), dim3(256), 0, s, Cown.p + sp * NN, (int)N,
                             rows.p + ptr[b], (const int64_t *)nullptr, nb[b], const_cast<double *>(u.C));
      }
    }
    SlotTasks &st = tasks[slot];
    if (lowrank) {
      // A = X^T (F C_o), B = X^T (S C_o), err = A B^T - B A^T
      const size_t cs = (size_t)nrmax * std::max(kmax, 1);
      lrT.resize(2 * cs * nu * nspin);
      lrG.resize(2 * cs * nu * nspin);
      std::vector<GemmTask> t1, t2;
      std::vector<DiisErrTask> t3;
      for (int sp = 0; sp < nspin; sp++) {
        const int no = (int)nocc[sp];
        if (no == 0) {
          HFG_HIP_CHECK(hipMemsetAsync(histE[slot].p + sp * elen, 0, sizeof(double) * elen, s));
          continue;
        }
        for (int b = 0; b < nu; b++) {
          const Unit u = unit(slot, sp, b);
          if (!u.nr) continue;
          const size_t k = (size_t)sp * nu + b;
          double *FC = lrT.p + 2 * cs * k, *SC = FC + cs, *A = lrG.p + 2 * cs * k, *Bm = A + cs;
          GemmTask q;
          q.M = u.nr;
          q.N = no;
          q.K = u.nr;
          q.B = u.C;
          q.ldb = u.ldC;
          q.ldc = u.nr;
          q.A = u.F;
          q.lda = u.ldF;
          q.C = FC;
          t1.push_back(q);
          q.A = u.Sb;
          q.lda = u.ldS;
          q.C = SC;
          t1.push_back(q);
          q.M = u.nc;
          q.A = u.Xb;
          q.lda = u.ldX;
          q.tA = 1;
          q.ldb = u.nr;
          q.ldc = u.nc;
          q.B = FC;
          q.C = A;
          t2.push_back(q);
          q.B = SC;
          q.C = Bm;
          t2.push_back(q);
          DiisErrTask e;
          e.A = A;
          e.B = Bm;
          e.out = u.out;
          e.n = u.nc;
          e.k = no;
          e.ld = u.nc;
          e.ldo = u.nc;
          t3.push_back(e);
        }
      }
      std::vector<GemmTask> t(t1);
      t.insert(t.end(), t2.begin(), t2.end());
      hfg::upload_cached(st.g, st.gc, t, s);
      hfg::upload_cached(st.e, st.ec, t3, s);
      lrmax.resize(std::max<size_t>(1, hfg::diis_lowrank_partials((int)t3.size(), ncmax)));
      hfg::gemm_tasklist_dev(ctx, st.g.p, (int)t1.size(), nrmax, kmax, {hfg::GemmTile::T64});
      hfg::gemm_tasklist_dev(ctx, st.g.p + t1.size(), (int)t2.size(), ncmax, kmax, {hfg::GemmTile::T64});
      hfg::diis_lowrank_error_dev(ctx, st.e.p, (int)t3.size(), ncmax, lrmax.p, res.p);
    } else {
      // err = X^T (F P S - S P F) X, the four products of the reference's definition
      T1.resize(sl * nu * nspin);
      T2.resize(sl * nu * nspin);
      std::vector<GemmTask> t[4];
      std::vector<std::pair<size_t, int> > anti;
      for (int sp = 0; sp < nspin; sp++)
        for (int b = 0; b < nu; b++) {
          const Unit u = unit(slot, sp, b);
          if (!u.nr) continue;
          const size_t k = (size_t)sp * nu + b;
          double *W1 = T1.p + sl * k, *W2 = T2.p + sl * k;
          GemmTask q;
          q.M = q.N = q.K = u.nr;
          q.A = u.F;
          q.lda = u.ldF;
          q.B = u.P;
          q.ldb = u.ldF;
          q.C = W1;
          q.ldc = u.nr;
          t[0].push_back(q);  // W1 = F P
          q.A = W1;
          q.lda = u.nr;
          q.B = u.Sb;
          q.ldb = u.ldS;
          q.C = W2;
          t[1].push_back(q);  // W2 = F P S; then W1 = W2 - W2^T
          anti.push_back(std::make_pair(k, u.nr));
          q.M = u.nc;
          q.A = u.Xb;
          q.lda = u.ldX;
          q.tA = 1;
          q.B = W1;
          q.ldb = u.nr;
          q.C = W2;
          q.ldc = u.nc;
          t[2].push_back(q);  // W2 = X^T W1  (nc x nr)
          q.tA = 0;
          q.N = u.nc;
          q.A = W2;
          q.lda = u.nc;
          q.B = u.Xb;
          q.ldb = u.ldX;
          q.C = u.out;
          t[3].push_back(q);  // err = W2 X
        }
      std::vector<GemmTask> all;
      for (int q = 0; q < 4; q++) all.insert(all.end(), t[q].begin(), t[q].end());
      hfg::upload_cached(st.g, st.gc, all, s);
      const int nt = (int)t[0].size();
      hfg::gemm_tasklist_dev(ctx, st.g.p, nt, nrmax, nrmax);
      hfg::gemm_tasklist_dev(ctx, st.g.p + nt, nt, nrmax, nrmax);
      for (const auto &a : anti)
        hipLaunchKernelGGL(hfg::k_diis_antisym, dim3((a.second + 255) / 256, a.second), dim3(256), 0, s, T2.p + sl * a.first, a.second,
                           T1.p + sl * a.first);
      hfg::gemm_tasklist_dev(ctx, st.g.p + 2 * nt, nt, ncmax, nrmax);
      hfg::gemm_tasklist_dev(ctx, st.g.p + 3 * nt, nt, ncmax, ncmax);
    }
    // the new row of B, the new row and column of T
    const int nh = (int)slots.size();
    for (int j0 = 0; j0 < nh; j0 += hfg::DIIS_HIST_CHUNK) {
      hfg::DiisHistory h;
      h.n = std::min(hfg::DIIS_HIST_CHUNK, nh - j0);
      for (int k = 0; k < hfg::DIIS_HIST_CHUNK; k++) {
        const int sk = slots[std::min(j0 + k, nh - 1)];
        h.E[k] = histE[sk].p;
        h.P[k] = histP[sk].p;
        h.F[k] = histF[sk].p;
      }
      hfg::diis_history_dev(ctx, h, j0, nh, histE[slot].p, nspin * elen, histP[slot].p, histF[slot].p, nspin * NN, !lowrank && j0 == 0, partial.p,
                            res.p);
    }
    HFG_HIP_CHECK(hipMemcpyAsync(hres, res.p, sizeof(double) * (1 + 3 * (size_t)nh), hipMemcpyDeviceToHost, s));
    HFG_HIP_CHECK(hipStreamSynchronize(s));  // the one synchronisation of an update
    const double maxerr = hres[0], spinfac = nspin == 1 ? 2.0 : 1.0;
    mixer.push(E, maxerr);
    Eh.push_back(E);
    for (int k = 0; k < nh; k++) {
      const double b = spinfac * hres[1 + k], tkn = spinfac * hres[1 + nh + k], tnk = spinfac * hres[1 + 2 * nh + k];
      mixer.set_B((size_t)k, (size_t)nh - 1, b);
      mixer.set_T((size_t)k, (size_t)nh - 1, tkn);
      mixer.set_T((size_t)nh - 1, (size_t)k, tnk);
      Bh[(size_t)k * order + nh - 1] = Bh[(size_t)(nh - 1) * order + k] = b;
      Th[(size_t)k * order + nh - 1] = tkn;
      Th[(size_t)(nh - 1) * order + k] = tnk;
    }
    return maxerr;
  }

  void solve(double *dFa, double *dFb, int *dropped) {
    if (!mixer.size()) throw std::logic_error("hfg_diis_solve_devptr: empty history\n");
    if (!dFa || (nspin == 2 && !dFb)) throw std::logic_error("hfg_diis_solve_devptr: null output matrix\n");
    hfg::ProfScope ps(ctx, "diis_solve");
    size_t dr = 0;
    wlast = mixer.solve(dr);
    for (size_t k = 0; k < dr; k++) pop_oldest_host();
    if (dropped) *dropped = (int)dr;
    hfg::DiisComb c;
    c.n = (int)slots.size();
    for (int k = 0; k < 16; k++) {
      c.F[k] = histF[slots[std::min(k, c.n - 1)]].p;
      c.w[k] = k < c.n ? wlast[k] : 0.0;
    }
    hfg::diis_extrapolate_dev(ctx, c, NN, nspin, dFa, dFb);
  }

  void get(int which, double *out, int64_t cap) {
    if (!out) throw std::logic_error("hfg_diis_get: null output\n");
    const size_t sz = Eh.size();
    auto need = [&](size_t cnt) {
      if (cap < (int64_t)cnt) throw std::logic_error("hfg_diis_get: output too small\n");
    };
    if (which == 0 || which == 1) {
      need(sz * sz);
      const std::vector<double> &M = which ? Th : Bh;
      for (size_t i = 0; i < sz; i++)
        for (size_t j = 0; j < sz; j++) out[i * sz + j] = M[i * order + j];
    } else if (which == 2) {
      need(wlast.size());
      std::copy(wlast.begin(), wlast.end(), out);
    } else if (which == 3) {
      if (newest < 0) throw std::logic_error("hfg_diis_get: empty history\n");
      need(nspin * n * n);
      std::vector<double> e(nspin * elen);
      HFG_HIP_CHECK(hipMemcpyAsync(e.data(), histE[newest].p, sizeof(double) * e.size(), hipMemcpyDeviceToHost, ctx->stream));
      HFG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
      if (!nblk) std::copy(e.begin(), e.end(), out);
      else {
        std::fill(out, out + nspin * n * n, 0.0);
        for (int sp = 0; sp < nspin; sp++)
          for (int b = 0; b < nblk; b++)
            for (int j = 0; j < nb[b]; j++)
              for (int i = 0; i < nb[b]; i++)
                out[sp * n * n + (size_t)hcols[ptr[b] + j] * n + hcols[ptr[b] + i]] = e[sp * elen + eoff[b] + (size_t)j * nb[b] + i];
      }
    } else
      throw std::logic_error("hfg_diis_get: which = 0 B, 1 T, 2 weights, 3 error\n");
  }
};

namespace {
template <class Fn>
int guarded(Fn &&fn) {
  try {
    fn();
  } catch (const std::logic_error &e) {
    hfg::set_error(e.what());
    return 1;
  } catch (const std::runtime_error &e) {
    hfg::set_error(e.what());
    return 2;
  } catch (const std::exception &e) {
    hfg::set_error(e.what());
    return 3;
  }
  return 0;
}
}  // namespace

extern "C" {

int hfg_diis_create(hfg_ctx *ctx, int64_t N, int nspin, int order, double diiseps, double diisthr, int mode, hfg_diis **d) {
  return guarded([&] {
    if (!ctx || !d) throw std::logic_error("hfg_diis_create: null context or output pointer\n");
    *d = nullptr;
    if (N < 1 || N > 46340) throw std::logic_error("hfg_diis_create: 1 <= N <= 46340\n");
    if (nspin != 1 && nspin != 2) throw std::logic_error("hfg_diis_create: nspin is 1 or 2\n");
    if (order < 1 || order > 16) throw std::logic_error("hfg_diis_create: 1 <= order <= 16\n");
    if (mode < 0 || mode > 2) throw std::logic_error("hfg_diis_create: mode 0 mixed, 1 CDIIS, 2 ADIIS\n");
    HFG_HIP_CHECK(hipSetDevice(ctx->device));
    *d = new hfg_diis(ctx, (size_t)N, nspin, order, diiseps, diisthr, mode);
  });
}

int hfg_diis_destroy(hfg_diis *d) {
  return guarded([&] {
    if (!d) return;
    (void)hipSetDevice(d->ctx->device);
    (void)hipStreamSynchronize(d->ctx->stream);
    delete d;
  });
}

int hfg_diis_set_metric_devptr(hfg_diis *d, const double *dS, const double *dSinvh, int64_t n) {
  return guarded([&] {
    if (!d) throw std::logic_error("hfg_diis_set_metric_devptr: null object\n");
    HFG_HIP_CHECK(hipSetDevice(d->ctx->device));
    d->set_metric(dS, dSinvh, n);
  });
}

int hfg_diis_set_blocks(hfg_diis *d, int nblk, const int64_t *blk_ptr, const int64_t *blk_idx) {
  return guarded([&] {
    if (!d) throw std::logic_error("hfg_diis_set_blocks: null object\n");
    HFG_HIP_CHECK(hipSetDevice(d->ctx->device));
    d->set_blocks(nblk, blk_ptr, blk_idx);
  });
}

int hfg_diis_update_devptr(hfg_diis *d, double E, const double *dFa, const double *dPa, const double *dCa, int64_t nocca,
                           const double *dFb, const double *dPb, const double *dCb, int64_t noccb, double *maxerr) {
  return guarded([&] {
    if (!d) throw std::logic_error("hfg_diis_update_devptr: null object\n");
    HFG_HIP_CHECK(hipSetDevice(d->ctx->device));
    const double *F[2] = {dFa, dFb}, *P[2] = {dPa, dPb}, *C[2] = {dCa, dCb};
    const int64_t nocc[2] = {nocca, noccb};
    const double e = d->update(E, F, P, C, nocc);
    if (maxerr) *maxerr = e;
  });
}

int hfg_diis_solve_devptr(hfg_diis *d, double *dFa, double *dFb, int *dropped) {
  return guarded([&] {
    if (!d) throw std::logic_error("hfg_diis_solve_devptr: null object\n");
    HFG_HIP_CHECK(hipSetDevice(d->ctx->device));
    d->solve(dFa, dFb, dropped);
  });
}

int hfg_diis_size(const hfg_diis *d) { return d ? (int)d->Eh.size() : 0; }

int hfg_diis_get(hfg_diis *d, int which, double *out, int64_t cap) {
  return guarded([&] {
    if (!d) throw std::logic_error("hfg_diis_get: null object\n");
    HFG_HIP_CHECK(hipSetDevice(d->ctx->device));
    d->get(which, out, cap);
  });
}

}  // extern "C"
