// Range-separated exchange tables of the atomic program built on the GPU: TwoDBasis::compute_yukawa and compute_erfc
// (src/atomic/TwoDBasis.cpp:741-815, host/atomic_basis.cpp) with the special functions of hip/special_dev.h.
//
// The host keeps what is cheap and polynomial (quadrature points and weights, LIP products: tei_element_tables, eval_dnf);
// the Bessel / Phi_L weights and the O(p^4) sums run here and land in the padded layout of hip/tables.h
// (hfg_basis::dev_rs_tei, dev_rs_disj; upload_rs_tables copies them into dev_rs device to device).
//
// Yukawa (rs_kind 1), per radial element, the prefix form of tei_dev.hip with the carry of twoe_integral_kernel:
//   wP[L][isub][q] = w_s i_L(lambda r_s) k_L(lambda r_isub),  ratio[L][isub] = k_L(lambda r_isub) / k_L(lambda r_isub-1)
//   inner[L][isub] = sum_q wP[L][isub][q] bbs[., isub, q] + ratio[L][isub] inner[L][isub-1]
//   W[L] = (bb0 diag(w)) inner[L]^T  (FP64 MFMA task list),  tei = W + W^T;  disjoint_iL/kL = bb0 (w i_L), bb0 (w k_L)
// erfc (rs_kind 2), per (L, e, f): Fn[i,k] = Phi_L(mu r_i, mu r'_k) (nq x nq, or nq x nq^2 over the nq uniform
//   sub-intervals for e = f), T1 = Fn (pkl),  tei = pij^T T1  (two task lists), e = f symmetrised, one block per ordered pair.
//   Rows (L, e) are processed in batches whose Fn, T1, product and sub-interval operand buffers stay within RS_BATCH_BYTES.
//
// Exchange-ordered copies (rs_ktei) are not stored: the exchange kernels form theirs from dev_rs->tei (exchange_lr.hip),
// hfg_basis_get_prim permutes on read-back.
#include "internal.h"
#include "special_dev.h"
#include <algorithm>
#include <vector>

namespace hfg {

namespace {
constexpr size_t RS_BATCH_BYTES = (size_t)256 << 20;  // working set of one erfc batch (Fn + T1 + products + sub-interval operands)

struct RsBlock {  // one (L, e, f) block of an erfc batch
  int L, e, f, nk;          // nk: points of the second coordinate (nq, or nq^2 for e = f)
  const double *rk;         // their radii
  double *Fn, *C;           // nq x nk kernel values; Np_e x Np_f product
  int Ni, Nf, lo, lof;      // primitives held by e and f and their shifts in the padded layout
};
}  // namespace

__global__ void k_rs_special(int which, int L, const double *__restrict__ a, const double *__restrict__ b, size_t n, int mode,
                             double *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = which == 0 ? sf::bessel_il(a[i], L) : which == 1 ? sf::bessel_kl(a[i], L) : sf::erfc_phi(L, a[i], b[i], mode);
}

// per element: wP[L][isub*nq+q], ratio[L][isub], wI[L][q], wK[L][q]; one workgroup per L
__global__ void k_rs_yuk_weights(const double *__restrict__ r0, const double *__restrict__ w0, const double *__restrict__ rs,
                                 const double *__restrict__ ws, int nq, double lambda, double *__restrict__ wP,
                                 double *__restrict__ ratio, double *__restrict__ wI, double *__restrict__ wK) {
  const int L = blockIdx.x;
  for (int t = threadIdx.x; t < nq * nq; t += blockDim.x)
    wP[(size_t)L * nq * nq + t] = ws[t] * (sf::bessel_il(rs[t] * lambda, L) * sf::bessel_kl(r0[t / nq] * lambda, L));
  for (int q = threadIdx.x; q < nq; q += blockDim.x) {
    const double k = sf::bessel_kl(r0[q] * lambda, L);
    ratio[(size_t)L * nq + q] = q ? k / sf::bessel_kl(r0[q - 1] * lambda, L) : 0.0;
    wI[(size_t)L * nq + q] = w0[q] * sf::bessel_il(r0[q] * lambda, L);
    wK[(size_t)L * nq + q] = w0[q] * k;
  }
}

// inner[L][isub][(ij)]: one workgroup per L; thread = (ij)
__global__ __launch_bounds__(256) void k_rs_yuk_inner(const double *__restrict__ bbs, const double *__restrict__ wP,
                                                      const double *__restrict__ ratio, int Np, int nq, double *__restrict__ inner) {
  const int L = blockIdx.x;
  const double *w = wP + (size_t)L * nq * nq;
  double *out = inner + (size_t)L * nq * Np;
  for (int k = threadIdx.x; k < Np; k += blockDim.x) {
    double acc = 0.0;
    for (int isub = 0; isub < nq; isub++) {
      const double *b = bbs + (size_t)isub * nq * Np + k;
      double s = 0.0;
      for (int q = 0; q < nq; q++) s += w[isub * nq + q] * b[(size_t)q * Np];
      acc = s + acc * ratio[(size_t)L * nq + isub];
      out[(size_t)isub * Np + k] = acc;
    }
  }
}

// disj[t][L][e][j+lo][i+lo] = sum_q bb0[(j Ni + i), q] w_t[L][q], t = 0 (i_L), 1 (k_L); grid (NL, 2)
__global__ void k_rs_yuk_disj(const double *__restrict__ bb0, const double *__restrict__ wI, const double *__restrict__ wK, int Ni,
                              int nq, int p, int lo, int NL, int E, int e, double *__restrict__ disj) {
  const int L = blockIdx.x, t = blockIdx.y, Np = Ni * Ni;
  const double *w = (t ? wK : wI) + (size_t)L * nq;
  double *D = disj + (((size_t)t * NL + L) * E + e) * (size_t)p * p;
  for (int k = threadIdx.x; k < Np; k += blockDim.x) {
    double s = 0.0;
    for (int q = 0; q < nq; q++) s += bb0[(size_t)q * Np + k] * w[q];
    D[(size_t)(k / Ni + lo) * p + (k % Ni + lo)] = s;
  }
}

// tei[L][e][(c)][(r)] (p^2 x p^2 padded, primitives shifted by lo) = W[L] + W[L]^T; one workgroup per L
__global__ void k_rs_yuk_store(const double *__restrict__ W, int Ni, int p, int lo, int E, int e, double *__restrict__ tei) {
  const int L = blockIdx.x, Np = Ni * Ni, pp = p * p;
  const double *Wl = W + (size_t)L * Np * Np;
  double *T = tei + ((size_t)L * E + e) * (size_t)pp * pp;
  for (int t = threadIdx.x; t < pp * pp; t += blockDim.x) {
    const int r = t % pp, c = t / pp;
    const int ri = r % p - lo, rj = r / p - lo, ci = c % p - lo, cj = c / p - lo;
    double v = 0.0;
    if (ri >= 0 && ri < Ni && rj >= 0 && rj < Ni && ci >= 0 && ci < Ni && cj >= 0 && cj < Ni) {
      const int rr = rj * Ni + ri, cc = cj * Ni + ci;
      v = Wl[(size_t)cc * Np + rr] + Wl[(size_t)rr * Np + cc];
    }
    T[t] = v;
  }
}

// Fn[i + nq k] = Phi_L(mu r_i, mu r'_k) of every block of the batch; grid (chunks of the largest block, blocks)
__global__ void k_rs_erfc_fn(const RsBlock *__restrict__ blocks, const double *__restrict__ r0, int nq, double mu, int mode) {
  const RsBlock b = blocks[blockIdx.y];
  const double *ri = r0 + (size_t)b.e * nq;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < (size_t)nq * b.nk; t += (size_t)gridDim.x * blockDim.x)
    b.Fn[t] = sf::erfc_phi(b.L, mu * ri[t % nq], mu * b.rk[t / nq], mode);
}

// tei[L][e][f][(c)][(r)] (rows: primitives of e, columns: primitives of f) = C, or (C + C^T)/2 for e = f; one workgroup row per block
__global__ void k_rs_erfc_store(const RsBlock *__restrict__ blocks, int p, int E, double *__restrict__ tei) {
  const RsBlock b = blocks[blockIdx.y];
  const int pp = p * p, Npe = b.Ni * b.Ni;
  double *T = tei + (((size_t)b.L * E + b.e) * E + b.f) * (size_t)pp * pp;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < pp * pp; t += gridDim.x * blockDim.x) {
    const int r = t % pp, c = t / pp;
    const int ri = r % p - b.lo, rj = r / p - b.lo, ci = c % p - b.lof, cj = c / p - b.lof;
    double v = 0.0;
    if (ri >= 0 && ri < b.Ni && rj >= 0 && rj < b.Ni && ci >= 0 && ci < b.Nf && cj >= 0 && cj < b.Nf) {
      const int rr = rj * b.Ni + ri, cc = cj * b.Nf + ci;
      v = b.C[(size_t)cc * Npe + rr];
      if (b.e == b.f) v = 0.5 * (v + b.C[(size_t)rr * Npe + cc]);
    }
    T[t] = v;
  }
}

/// hfg_rs_special_dev: out[i] = i_L(a[i]) (which 0), k_L(a[i]) (1) or Phi_L(a[i], b[i]) (2) from the device functions, one launch
void rs_special_dev(hfg_ctx *ctx, int which, int L, const double *a, const double *b, size_t n, double *out) {
  if (which < 0 || which > 2 || L < 0) throw std::logic_error("hfg_rs_special_dev: which is 0 (i_L), 1 (k_L) or 2 (Phi_L), L >= 0\n");
  if (!n) return;
  HFG_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf<double> da, db, dout;
  da.upload(std::vector<double>(a, a + n), s);
  if (which == 2) db.upload(std::vector<double>(b, b + n), s);
  dout.resize(n);
  HFG_HIP_CHECK(hipStreamSynchronize(s));  // the staging vectors above are temporaries
  hipLaunchKernelGGL(k_rs_special, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, which, L, da.p, db.p, n,
                     helfem::get_erfc_binomial_mode(), dout.p);
  HFG_HIP_CHECK(hipGetLastError());
  HFG_HIP_CHECK(hipMemcpyAsync(out, dout.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
  HFG_HIP_CHECK(hipStreamSynchronize(s));
}

static void yukawa_dev(hfg_ctx *ctx, hfg_basis *basis, double lambda) {
  const helfem::atomic::TwoDBasis &b = basis->ab;
  hipStream_t s = ctx->stream;
  const int E = (int)b.Nel(), p = (int)b.max_Nprim(), NL = b.N_L(), nq = b.nquad();
  const size_t pp = (size_t)p * p;
  basis->dev_rs_tei.resize((size_t)NL * E * pp * pp);
  basis->dev_rs_disj.resize((size_t)2 * NL * E * pp);
  HFG_HIP_CHECK(hipMemsetAsync(basis->dev_rs_disj.p, 0, sizeof(double) * 2 * NL * E * pp, s));
  DevBuf<double> d_bb0, d_bbs, d_r0, d_w0, d_rs, d_ws, d_wP, d_ratio, d_wI, d_wK, d_inner, d_bq, d_W;
  DevBuf<GemmTask> d_tasks;
  d_wP.resize((size_t)NL * nq * nq);
  d_ratio.resize((size_t)NL * nq);
  d_wI.resize((size_t)NL * nq);
  d_wK.resize((size_t)NL * nq);
  for (int e = 0; e < E; e++) {
    helfem::diatomic::TwoDBasis::TeiElementTables t;
    b.tei_element_tables(e, t);
    const int Ni = (int)t.Ni, Np = (int)t.Np;
    // points and weights of the main rule and of the nq segments between its points (twoe_integral_kernel)
    const double rmin = b.fem.element_begin(e), rmax = b.fem.element_end(e);
    const double rmid0 = 0.5 * (rmax + rmin), rlen0 = 0.5 * (rmax - rmin);
    std::vector<double> r0(nq), w0(nq), rs((size_t)nq * nq), ws((size_t)nq * nq), bq(t.bb0.d);
    for (int q = 0; q < nq; q++) {
      r0[q] = rmid0 + rlen0 * b.xq[q];
      w0[q] = b.wq[q] * rlen0;
      for (int k = 0; k < Np; k++) bq[(size_t)q * Np + k] *= w0[q];
    }
    for (int isub = 0; isub < nq; isub++) {
      const double a = isub ? r0[isub - 1] : rmin, bnd = r0[isub];
      const double rmid = 0.5 * (bnd + a), rlen = 0.5 * (bnd - a);
      for (int q = 0; q < nq; q++) {
        rs[(size_t)isub * nq + q] = rmid + rlen * b.xq[q];
        ws[(size_t)isub * nq + q] = b.wq[q] * rlen;
      }
    }
    d_bb0.upload(t.bb0.d, s);
    d_bbs.upload(t.bbs.d, s);
    d_bq.upload(bq, s);
    d_r0.upload(r0, s);
    d_w0.upload(w0, s);
    d_rs.upload(rs, s);
    d_ws.upload(ws, s);
    d_inner.resize((size_t)NL * nq * Np);
    d_W.resize((size_t)NL * Np * Np);
    hipLaunchKernelGGL(k_rs_yuk_weights, dim3(NL), dim3(256), 0, s, d_r0.p, d_w0.p, d_rs.p, d_ws.p, nq, lambda, d_wP.p, d_ratio.p,
                       d_wI.p, d_wK.p);
    hipLaunchKernelGGL(k_rs_yuk_inner, dim3(NL), dim3(256), 0, s, d_bbs.p, d_wP.p, d_ratio.p, Np, nq, d_inner.p);
    const int lo = (e == 0) ? 1 : 0;  // the first element has lost its first primitive (hip/tables.cpp: lo)
    hipLaunchKernelGGL(k_rs_yuk_disj, dim3(NL, 2), dim3(256), 0, s, d_bb0.p, d_wI.p, d_wK.p, Ni, nq, p, lo, NL, E, e,
                       basis->dev_rs_disj.p);
    // W[L] (Np x Np) = bq (Np x nq) * inner[L]^T (nq x Np)
    std::vector<GemmTask> tasks((size_t)NL);
    for (int L = 0; L < NL; L++) {
      GemmTask g;
      g.A = d_bq.p;
      g.B = d_inner.p + (size_t)L * nq * Np;
      g.C = d_W.p + (size_t)L * Np * Np;
      g.M = g.N = Np;
      g.K = nq;
      g.lda = g.ldb = g.ldc = Np;
      g.tB = 1;
      tasks[L] = g;
    }
    d_tasks.upload(tasks, s);
    HFG_HIP_CHECK(hipStreamSynchronize(s));  // host vectors of this element live on this stack frame
    gemm_tasklist_dev(ctx, d_tasks.p, NL, Np, Np, {GemmTile::T64});
    hipLaunchKernelGGL(k_rs_yuk_store, dim3(NL), dim3(256), 0, s, d_W.p, Ni, p, lo, E, e, basis->dev_rs_tei.p);
    HFG_HIP_CHECK(hipGetLastError());
    HFG_HIP_CHECK(hipStreamSynchronize(s));
  }
}

static void erfc_dev(hfg_ctx *ctx, hfg_basis *basis, double mu) {
  const helfem::atomic::TwoDBasis &b = basis->ab;
  hipStream_t s = ctx->stream;
  const int E = (int)b.Nel(), p = (int)b.max_Nprim(), NL = b.N_L(), nq = b.nquad();
  const size_t pp = (size_t)p * p, nqq = (size_t)nq * nq;
  const int mode = helfem::get_erfc_binomial_mode();
  basis->dev_rs_tei.resize((size_t)NL * E * E * pp * pp);
  basis->dev_rs_disj.resize(1);

  // per element: radii of the main rule, pij^T = bb0 diag(w) (Np x nq, stride pp nq); radii of the nq uniform sub-intervals
  // of the second coordinate of a diagonal pair (erfc_integral)
  std::vector<int> Nprim(E);
  std::vector<double> r0((size_t)E * nq), bq((size_t)E * pp * nq, 0.0), ru((size_t)E * nqq), xk(nqq), wk(nqq);
  for (int ii = 0; ii < nq; ii++) {
    const double istart = ii * 2.0 / nq - 1.0, iend = (ii + 1) * 2.0 / nq - 1.0;
    const double imid = 0.5 * (iend + istart), ilen = 0.5 * (iend - istart);
    for (int q = 0; q < nq; q++) {
      xk[(size_t)ii * nq + q] = imid + b.xq[q] * ilen;
      wk[(size_t)ii * nq + q] = b.wq[q] * ilen;
    }
  }
  for (int e = 0; e < E; e++) {
    const helfem::Mat bf = b.fem.eval_dnf(b.xq, 0, e);
    const helfem::Vec r = b.fem.eval_coord(b.xq, e), rk = b.fem.eval_coord(xk, e);
    const int Ni = Nprim[e] = (int)bf.n_cols;
    const double rlen = b.fem.scaling_factor(e);
    std::copy(r.begin(), r.end(), r0.begin() + (size_t)e * nq);
    std::copy(rk.begin(), rk.end(), ru.begin() + (size_t)e * nqq);
    double *dst = &bq[(size_t)e * pp * nq];
    for (int q = 0; q < nq; q++)
      for (int j = 0; j < Ni; j++)
        for (int i = 0; i < Ni; i++) dst[(size_t)q * Ni * Ni + j * Ni + i] = bf(q, i) * bf(q, j) * b.wq[q] * rlen;
  }
  DevBuf<double> d_r0, d_bq, d_ru, d_bqu, d_Fn, d_T1, d_C;
  DevBuf<RsBlock> d_blocks;
  DevBuf<GemmTask> d_tasks1, d_tasks2;
  d_r0.upload(r0, s);
  d_bq.upload(bq, s);
  d_ru.upload(ru, s);
  HFG_HIP_CHECK(hipStreamSynchronize(s));

  // rows (e, L), e outermost so that a batch holds few distinct diagonal operands; bytes of one row: E - 1 off-diagonal
  // blocks, one diagonal block and (counted for every row) the diagonal pair's sub-interval operand
  const size_t row_doubles = (size_t)(E - 1) * (nqq + nq * pp + pp * pp) + (nq * nqq + nq * pp + pp * pp) + pp * nqq;
  const int rows_per_batch = (int)std::max<size_t>(1, RS_BATCH_BYTES / (row_doubles * sizeof(double)));
  const int nrows = E * NL;
  for (int row0 = 0; row0 < nrows; row0 += rows_per_batch) {
    const int row1 = std::min(nrows, row0 + rows_per_batch);
    const int e0 = row0 / NL, e1 = (row1 - 1) / NL;  // elements of this batch: e0 ... e1
    // sub-interval operands pkl^T (Np x nq^2) of the batch's diagonal pairs
    std::vector<double> bqu((size_t)(e1 - e0 + 1) * pp * nqq, 0.0);
    for (int e = e0; e <= e1; e++) {
      const helfem::Mat kbf = b.fem.eval_dnf(xk, 0, e);
      const int Ni = Nprim[e];
      const double rlen = b.fem.scaling_factor(e);
      double *dst = &bqu[(size_t)(e - e0) * pp * nqq];
      for (size_t q = 0; q < nqq; q++)
        for (int j = 0; j < Ni; j++)
          for (int i = 0; i < Ni; i++) dst[q * Ni * Ni + j * Ni + i] = kbf(q, i) * kbf(q, j) * wk[q] * rlen;
    }
    d_bqu.upload(bqu, s);
    const size_t nblk = (size_t)(row1 - row0) * E;
    d_Fn.resize((size_t)(row1 - row0) * ((size_t)(E - 1) * nqq + nq * nqq));
    d_T1.resize(nblk * nq * pp);
    d_C.resize(nblk * pp * pp);
    std::vector<RsBlock> blocks;
    std::vector<GemmTask> tasks1, tasks2;
    size_t offFn = 0;
    int maxNp = 0;
    for (int row = row0; row < row1; row++) {
      const int e = row / NL, L = row % NL;
      for (int f = 0; f < E; f++) {
        RsBlock k;
        k.L = L;
        k.e = e;
        k.f = f;
        k.nk = (e == f) ? (int)nqq : nq;
        k.rk = (e == f) ? d_ru.p + (size_t)e * nqq : d_r0.p + (size_t)f * nq;
        k.Fn = d_Fn.p + offFn;
        offFn += (size_t)nq * k.nk;
        k.C = d_C.p + blocks.size() * pp * pp;
        k.Ni = Nprim[e];
        k.Nf = Nprim[f];
        k.lo = (e == 0) ? 1 : 0;
        k.lof = (f == 0) ? 1 : 0;
        const int Npe = k.Ni * k.Ni, Npf = k.Nf * k.Nf;
        maxNp = std::max(maxNp, std::max(Npe, Npf));
        GemmTask g1, g2;  // T1 (nq x Npf) = Fn (nq x nk) pkl (nk x Npf);  C (Npe x Npf) = pij^T (Npe x nq) T1
        g1.A = k.Fn;
        g1.B = (e == f) ? d_bqu.p + (size_t)(e - e0) * pp * nqq : d_bq.p + (size_t)f * pp * nq;
        g1.C = d_T1.p + blocks.size() * nq * pp;
        g1.M = nq;
        g1.N = Npf;
        g1.K = k.nk;
        g1.lda = nq;
        g1.ldb = Npf;
        g1.ldc = nq;
        g1.tB = 1;
        g2.A = d_bq.p + (size_t)e * pp * nq;
        g2.B = g1.C;
        g2.C = k.C;
        g2.M = Npe;
        g2.N = Npf;
        g2.K = nq;
        g2.lda = Npe;
        g2.ldb = nq;
        g2.ldc = Npe;
        blocks.push_back(k);
        tasks1.push_back(g1);
        tasks2.push_back(g2);
      }
    }
    d_blocks.upload(blocks, s);
    d_tasks1.upload(tasks1, s);
    d_tasks2.upload(tasks2, s);
    HFG_HIP_CHECK(hipStreamSynchronize(s));  // host vectors of this batch live on this stack frame
    for (size_t b0 = 0; b0 < nblk; b0 += 65535) {  // (the grid's second dimension ends at 65535)
      const unsigned nb = (unsigned)std::min<size_t>(65535, nblk - b0);
      hipLaunchKernelGGL(k_rs_erfc_fn, dim3((unsigned)((nqq + 255) / 256), nb), dim3(256), 0, s, d_blocks.p + b0, d_r0.p, nq, mu, mode);
    }
    gemm_tasklist_dev(ctx, d_tasks1.p, (int)nblk, nq, maxNp, {GemmTile::T64});
    gemm_tasklist_dev(ctx, d_tasks2.p, (int)nblk, maxNp, maxNp, {GemmTile::T64});
    for (size_t b0 = 0; b0 < nblk; b0 += 65535) {
      const unsigned nb = (unsigned)std::min<size_t>(65535, nblk - b0);
      hipLaunchKernelGGL(k_rs_erfc_store, dim3((unsigned)std::min<size_t>(64, (pp * pp + 255) / 256), nb), dim3(256), 0, s,
                         d_blocks.p + b0, p, E, basis->dev_rs_tei.p);
    }
    HFG_HIP_CHECK(hipGetLastError());
    HFG_HIP_CHECK(hipStreamSynchronize(s));
  }
}

/// builds basis->dev_rs_tei (and, Yukawa, dev_rs_disj) on the device; the host keeps rs_kind and omega only
void compute_rs_tei_dev(hfg_ctx *ctx, hfg_basis *basis, int rs_kind, double omega) {
  if (basis->kind == 0) throw std::logic_error("Range separated functionals are not supported.\n");  // diatomic/main.cpp:393
  if (rs_kind != 1 && rs_kind != 2) throw std::logic_error("unknown range-separation kernel (1 = Yukawa, 2 = erfc)\n");
  if (!ctx) throw std::logic_error("hfg_compute_rs_tei_dev: a context is needed\n");
  if (basis->ab.zeroder)
    throw std::logic_error("A basis with zero derivative at Rmax (zeroder) keeps a radial function the device tables have no slot for: "
                           "its host matrices are available, the device path is not supported by this build.\n");
  HFG_HIP_CHECK(hipSetDevice(ctx->device));
  helfem::atomic::TwoDBasis &b = basis->ab;
  basis->rs_on_device = false;
  drop_mix_tables(basis);  // mixed from the tables this call replaces
  if (rs_kind == 1) yukawa_dev(ctx, basis, omega);
  else erfc_dev(ctx, basis, omega);
  b.rs_kind = rs_kind;
  b.rs_lambda = omega;
  for (std::vector<helfem::Mat> *t : {&b.disjoint_iL, &b.disjoint_kL, &b.rs_tei, &b.rs_ktei}) std::vector<helfem::Mat>().swap(*t);
  basis->rs_on_device = true;
}

}  // namespace hfg
