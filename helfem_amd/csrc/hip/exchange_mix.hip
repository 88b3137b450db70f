// Mixed-kernel exchange tables of the atomic program (gfx950): the range-separated hybrids add
//     K = alpha K[1/r12] + beta K[screened kernel]          (src/atomic/main.cpp:763-780)
// and the exchange kernels are linear in the radial table, so K = K[alpha T_coul + beta T_screened] is ONE build on a table
// set that holds the sum.  The sum is stored in the pair layout of the erfc set (tables.h: pair_tei = 1,
// tei[tab][e][f][c][r], one p^2 x p^2 block per ordered element pair, rows = primitives of e, columns = primitives of f),
// which every kernel can be written into: a kernel that factorises over elements (Coulomb, Yukawa) has the blocks
//     e == f   tei00[tab][e]
//     e <  f   P0[tab][e][r] Q0[tab][f][c]        (the inner element gets P, the outer one Q: exchange.hip k_ex_radial)
//     e >  f   Q0[tab][e][r] P0[tab][f][c]
// and the erfc set is in that layout already.  The mixed set keeps the Coulomb weights LM_fac = 4 pi/(2L+1); the ratio of the
// screened set's weights to them, lambda (2L+1) for Yukawa (LM_fac = 4 pi lambda) and mu for erfc (4 pi mu/(2L+1)), is folded
// into the blocks per table slot (slot = L in the atomic tables):
//     block = alpha coulomb + beta ratio(L) screened.
// Every source is zero in its padding (the dropped first primitive of element 0, the missing last primitive of the last
// element), so the products and the sum are exactly zero there.  One pass, every element written once by one thread: two
// builds are bitwise equal.
#include "internal.h"
#include <cmath>
#include <memory>

namespace hfg {

// one workgroup per (element pair, table slot, slice of the block).  Entries go out two per 16-byte store, starting at the
// first entry of the slice whose ADDRESS is 16-byte aligned: a block of odd length (odd p: 15 nodes give 50625 entries) puts
// every second block at an odd multiple of 8 bytes.  The one entry in front of the first pair and the one behind the last
// pair, where there is one, are stored alone.
__global__ void k_exl_mix_tables(const double *__restrict__ ctei, const double *__restrict__ cdisj, const double *__restrict__ stei,
                                 const double *__restrict__ sdisj, int s_pair, const double *__restrict__ bfac, double alpha, int Ntab,
                                 int E, int p, unsigned chunk, double *__restrict__ out) {
  const int e = blockIdx.x / E, f = blockIdx.x % E, tab = blockIdx.y;
  const unsigned pp = (unsigned)(p * p), blk = pp * pp;
  const unsigned i0 = blockIdx.z * chunk, i1 = min(blk, i0 + chunk);
  if (i0 >= i1) return;
  const bool diag = e == f;
  // rows take P0 (type 0) when e is the inner element, else Q0 (type 1); the columns the other one
  const int tr = e < f ? 0 : 1, tc = 1 - tr;
  const double *cT = ctei + ((size_t)tab * E + e) * blk;
  const double *cR = cdisj + (((size_t)tr * Ntab + tab) * E + e) * pp;
  const double *cC = cdisj + (((size_t)tc * Ntab + tab) * E + f) * pp;
  const double *sT = nullptr, *sR = nullptr, *sC = nullptr;
  if (stei) {
    sT = s_pair ? stei + (((size_t)tab * E + e) * E + f) * blk : stei + ((size_t)tab * E + e) * blk;
    if (!s_pair) {
      sR = sdisj + (((size_t)tr * Ntab + tab) * E + e) * pp;
      sC = sdisj + (((size_t)tc * Ntab + tab) * E + f) * pp;
    }
  }
  const bool s_whole = s_pair || diag;  // the screened block is stored as a whole
  const double b = stei ? bfac[tab] : 0.0;
  double *o = out + (((size_t)tab * E + e) * E + f) * blk;
  auto value = [&](unsigned idx) {
    const unsigned c = idx / pp, r = idx - c * pp;
    double v = alpha * (diag ? cT[idx] : cR[r] * cC[c]);
    if (stei) v += b * (s_whole ? sT[idx] : sR[r] * sC[c]);
    return v;
  };
  const unsigned odd = (unsigned)((reinterpret_cast<uintptr_t>(o) >> 3) & 1u);  // o + idx is 16-byte aligned when idx + odd is even
  const unsigned first = i0 + ((i0 + odd) & 1u);                                // <= i1, since i0 < i1
  const unsigned last = first + ((i1 - first) & ~1u);                           // end of the pairs
  if (threadIdx.x == 0 && first > i0) o[i0] = value(i0);
  for (unsigned idx = first + 2 * threadIdx.x; idx < last; idx += 2 * blockDim.x) {  // idx + 1 < last <= i1
    double2 v;
    v.x = value(idx);
    v.y = value(idx + 1);
    *reinterpret_cast<double2 *>(o + idx) = v;
  }
  if (threadIdx.x == blockDim.x - 1 && last < i1) o[last] = value(last);
}

int mix_exchange_tables_dev(hfg_ctx *ctx, hfg_basis *basis, double alpha, double beta) {
  if (!ctx || !basis) throw std::logic_error("hfg_mix_exchange_tables: null context or basis\n");
  if (basis->kind == 0) throw std::logic_error("Range separated functionals are not supported.\n");  // diatomic/main.cpp:393
  const helfem::atomic::TwoDBasis &ab = basis->ab;
  if (beta != 0.0 && ab.rs_kind == 0)
    throw std::logic_error("hfg_mix_exchange_tables: beta != 0 needs range-separated tables (hfg_compute_rs_tei or "
                           "hfg_compute_rs_tei_dev, then hfg_basis_upload)\n");
  // the bound of the pair path (exchange_lowrank_dev): a set beyond it is never allocated, the caller builds K from the two sets
  const double bytes = (double)ab.N_L() * (double)ab.Nel() * (double)ab.Nel() * std::pow((double)ab.max_Nprim(), 4) * sizeof(double);
  if (bytes > EXL_PAIR_MAX_BYTES) {
    drop_mix_tables(basis);
    set_error("hfg_mix_exchange_tables: the mixed table set would take " + std::to_string(bytes) + " bytes, more than the " +
              std::to_string(EXL_PAIR_MAX_BYTES) + " of the pair path; build K from the two table sets\n");
    return 4;
  }
  const hfg_dev_tables *tc = basis->dev, *ts = basis->dev_rs;
  if (!tc || !tc->have_tei)
    throw std::logic_error("hfg_mix_exchange_tables: the exchange tables have not been uploaded (hfg_compute_tei, then hfg_basis_upload)\n");
  if (beta != 0.0 && (!ts || !ts->have_tei || ts->rs_kind != ab.rs_kind || ts->rs_omega != ab.rs_lambda))
    throw std::logic_error("hfg_mix_exchange_tables: the range-separated tables have not been uploaded (hfg_basis_upload after "
                           "hfg_compute_rs_tei)\n");
  if (basis->dev_device != ctx->device) throw std::logic_error("basis tables live on a different device\n");
  const int kind = beta != 0.0 ? ab.rs_kind : 0;
  const double omega = beta != 0.0 ? ab.rs_lambda : 0.0;
  if (basis->dev_mix && basis->mix_alpha == alpha && basis->mix_beta == beta && basis->mix_kind == kind && basis->mix_omega == omega)
    return 0;  // already there
  drop_mix_tables(basis);

  const int Ntab = tc->Ntab, E = tc->E, p = tc->p;
  const size_t pp = (size_t)p * p, blk = pp * pp;
  if (tc->geom != 1 || tc->ntt != 1 || tc->ndt != 2 || tc->pair_tei || tc->tei.n < (size_t)Ntab * E * blk || tc->disj.n < (size_t)2 * Ntab * E * pp)
    throw std::logic_error("hfg_mix_exchange_tables: unexpected layout of the Coulomb table set\n");
  if (blk > 0x7fffffffu || Ntab > 65535) throw std::logic_error("hfg_mix_exchange_tables: element blocks of more than 2^31 entries or more than 65535 table slots\n");
  bool s_pair = false;
  if (kind) {
    s_pair = ts->pair_tei != 0;
    const bool ok = ts->Ntab == Ntab && ts->E == E && ts->p == p && ts->ntt == 1 &&
                    (s_pair ? ts->tei.n >= (size_t)Ntab * E * E * blk
                            : (ts->ndt == 2 && ts->tei.n >= (size_t)Ntab * E * blk && ts->disj.n >= (size_t)2 * Ntab * E * pp));
    if (!ok || s_pair != (kind == 2)) throw std::logic_error("hfg_mix_exchange_tables: unexpected layout of the range-separated table set\n");
  }
  ProfScope ps(ctx, "exchange_mix_tables");
  std::unique_ptr<hfg_dev_tables> t(new_mix_tables(ctx, basis));
  if (t->tei.n < (size_t)Ntab * E * E * blk) throw std::logic_error("hfg_mix_exchange_tables: mixed table buffer has the wrong size\n");
  hipStream_t s = ctx->stream;
  // beta times the ratio of the screened set's LM_fac to the Coulomb one, per table slot (= L)
  std::vector<double> bfac(Ntab);
  for (int L = 0; L < Ntab; L++) bfac[L] = beta * (kind == 1 ? omega * (2 * L + 1) : omega);
  DevBuf<double> dbfac;
  dbfac.upload(bfac, s);
  // slices: at least ~2048 workgroups on the chip, at least 2048 entries each
  const size_t nblocks = (size_t)Ntab * E * E;
  size_t nslice = std::max<size_t>(1, std::min<size_t>((2048 + nblocks - 1) / nblocks, std::max<size_t>(1, blk / 2048)));
  nslice = std::min<size_t>(nslice, 65535);
  unsigned chunk = (unsigned)((blk + nslice - 1) / nslice);
  chunk += chunk & 1u;
  nslice = (blk + chunk - 1) / chunk;
  {
    ProfScope pk(ctx, "exchange_mix_kernel");  // the kernel alone; "exchange_mix_tables" also covers the set's shells and couplings
    hipLaunchKernelGGL(k_exl_mix_tables, dim3((unsigned)(E * E), (unsigned)Ntab, (unsigned)nslice), dim3(256), 0, s, tc->tei.p, tc->disj.p,
                       kind ? ts->tei.p : nullptr, (kind && !s_pair) ? ts->disj.p : nullptr, s_pair ? 1 : 0, dbfac.p, alpha, Ntab, E, p,
                       chunk, t->tei.p);
  }
  HFG_HIP_CHECK(hipGetLastError());
  HFG_HIP_CHECK(hipStreamSynchronize(s));  // once per run; bfac and dbfac live on this stack frame
  basis->dev_mix = t.release();
  basis->mix_alpha = alpha;
  basis->mix_beta = beta;
  basis->mix_kind = kind;
  basis->mix_omega = omega;
  return 0;
}

}  // namespace hfg
