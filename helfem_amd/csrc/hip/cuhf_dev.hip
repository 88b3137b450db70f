// The constrained-UHF form of ROHF on the caller's device pointers (hfg_cuhf_update_devptr, include/helfem_gpu.h): the
// reference's scf::ROHF_update (src/general/scf_helpers.cpp:470-523), Fa += lambda, Fb -= lambda with lambda the
// core-virtual coupling of Delta = (Fa - Fb) / 2 between the natural orbitals of P = Pa + Pb.  The device SCF driver
// (scf_device.hip) keeps its own dense sequence and is not touched by this file.
//
// Low-rank route.  C = [Ca_o | Cb_o] (N x r, r = na + nb) holds the occupied orbitals.  G = C^T S C = R L R^T has the
// non-zero natural occupations as its eigenvalues; y_k = C r_k / sqrt(L_k) are the natural orbitals in the AO basis and
// t_k = S y_k the rows of the reference's NO_to_AO.  With the top Nc = min(na, nb) pairs as core (Y_c, T_c), the top
// Nw = max(na, nb) as core plus active (Y_w, T_w) and the completeness relation sum_k y_k t_k^T = 1 for the virtual space,
//   lambda = -(B + B^T),  B = T_c [A - (A Y_w) T_w^T],  A = Y_c^T Delta.
// Device code of this file:
//   k_cuhf_gram     G = C^T (S C), one workgroup per element of the lower triangle, the mirror written with it
//   k_cuhf_q        Q = R_w L_w^{-1/2}, the top Nw pairs in descending occupation
//   k_cuhf_a        A^T = Delta^T Y_c: reads Fa and Fb once, Delta is never stored
//   k_cuhf_apply    Fa -= W, Fb += W with W_ij = sum_c (T_c[i,c] A'[c,j] + A'[c,i] T_c[j,c]): one writer per element, the
//                   panels of T_c and A' staged in LDS per tile.  Each c term is the sum of the two rounded products, added
//                   to the accumulator in c order: W is symmetric bit for bit
//   k_cuhf_delta, k_cuhf_no_lambda, k_cuhf_add   the element-wise passes of the dense route
// The products S C, C Q, (S C) Q, A Y_w and A - M T_w^T go through the FP64 tile engine (gemm_dev).  Every sum runs in a
// fixed order and nothing is accumulated with atomics, so two contexts fed the same matrices produce the same bits.
#include "internal.h"
#include <algorithm>

namespace hfg {

namespace {

// the context's workspace of both routes (workspace_owner.h, WS_CUHF); DevBuf::resize only ever grows
struct CuhfWork : Workspace {
  DevBuf<double> C, SC, G, lam, R, Q, Y, T, AT, Mt;   // low-rank route
  DevBuf<double> Sinvh, Sh, P, T1, T2, Pvec, A2N, ShPv, occ;  // dense route
};

__global__ __launch_bounds__(256) void k_cuhf_gram(const double *__restrict__ C, const double *__restrict__ SC, int N, int r,
                                                   double *__restrict__ G) {
  const int a = blockIdx.x, b = blockIdx.y;
  if (b > a) return;  // (uniform per workgroup)
  __shared__ double sh[4];
  const double *ca = C + (size_t)a * N, *sb = SC + (size_t)b * N;
  double s = 0.0;
  for (int i = threadIdx.x; i < N; i += 256) s += ca[i] * sb[i];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double v = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    G[(size_t)b * r + a] = v;
    G[(size_t)a * r + b] = v;
  }
}

// eigenpairs ascending in (lam, R): column k of Q is eigenvector r - 1 - k over the square root of its eigenvalue
__global__ void k_cuhf_q(const double *__restrict__ R, const double *__restrict__ lam, int r, double *__restrict__ Q) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y, src = r - 1 - k;
  if (i < r) Q[(size_t)k * r + i] = R[(size_t)src * r + i] / sqrt(lam[src]);
}

// AT (N x Nc): AT[j, c] = sum_i (Fa[i, j] - Fb[i, j]) / 2 * Y[i, c], 16 columns j per workgroup, i in ascending order
__global__ __launch_bounds__(256) void k_cuhf_a(const double *__restrict__ Fa, const double *__restrict__ Fb, const double *__restrict__ Y,
                                                int N, int Nc, double *__restrict__ AT) {
  __shared__ double sD[16][65], sY[64][65];
  const int t = threadIdx.x, j0 = blockIdx.x * 16;
  const int li = t & 63, lq = t >> 6;  // loads: row i of the chunk, column / orbital lq + 4 q
  const int j = t & 15, cg = t >> 4;   // sums: column j, orbitals cg + 16 m
  const int mmax = (Nc + 15) / 16;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i0 = 0; i0 < N; i0 += 64) {
    const int gi = i0 + li;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int jj = lq + 4 * q, gj = j0 + jj;
      const bool ok = gi < N && gj < N;
      const size_t o = (size_t)gj * N + gi;
      sD[jj][li] = ok ? 0.5 * (Fa[o] - Fb[o]) : 0.0;
    }
    for (int q = 0; q < 4 * mmax; q++) {
      const int c = lq + 4 * q;
      sY[c][li] = (c < Nc && gi < N) ? Y[(size_t)c * N + gi] : 0.0;
    }
    __syncthreads();
    for (int ii = 0; ii < 64; ii++) {
      const double d = sD[j][ii];
#pragma unroll
      for (int m = 0; m < 4; m++)
        if (m < mmax) acc[m] += d * sY[cg + 16 * m][ii];
    }
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < 4; m++) {
    const int c = cg + 16 * m;
    if (c < Nc && j0 + j < N) AT[(size_t)c * N + j0 + j] = acc[m];
  }
}

// one 64 x 32 tile of Fa and Fb per workgroup; T (N x >= Nc): the columns t_c, AT (N x Nc): A'^T
__global__ __launch_bounds__(256) void k_cuhf_apply(const double *__restrict__ T, const double *__restrict__ AT, int N, int Nc,
                                                    double *__restrict__ Fa, double *__restrict__ Fb) {
  __shared__ double sTi[16][64], sAi[16][64], sTj[16][32], sAj[16][32];  // [c][row]
  const int t = threadIdx.x, tx = t & 63, ty = t >> 6;
  const int i0 = blockIdx.x * 64, j0 = blockIdx.y * 32;
  double acc[8];
#pragma unroll
  for (int q = 0; q < 8; q++) acc[q] = 0.0;
  for (int c0 = 0; c0 < Nc; c0 += 16) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int kk = ty + 4 * q, c = c0 + kk;
      const bool ok = c < Nc && i0 + tx < N;
      const size_t o = (size_t)c * N + i0 + tx;
      sTi[kk][tx] = ok ? T[o] : 0.0;
      sAi[kk][tx] = ok ? AT[o] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int kk = (t >> 5) + 8 * q, c = c0 + kk, jl = t & 31;
      const bool ok = c < Nc && j0 + jl < N;
      const size_t o = (size_t)c * N + j0 + jl;
      sTj[kk][jl] = ok ? T[o] : 0.0;
      sAj[kk][jl] = ok ? AT[o] : 0.0;
    }
    __syncthreads();
    const int kc = min(16, Nc - c0);
    for (int kk = 0; kk < kc; kk++) {
      // no contraction into fused multiply-adds here: the two products are rounded on their own, then added, so that
      // (i, j) and (j, i) add the same two numbers
#pragma clang fp contract(off)
      const double ti = sTi[kk][tx], ai = sAi[kk][tx];
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const double p1 = ti * sAj[kk][ty + 4 * q], p2 = ai * sTj[kk][ty + 4 * q];
        const double term = p1 + p2;
        acc[q] = acc[q] + term;
      }
    }
    __syncthreads();
  }
  if (i0 + tx >= N) return;
#pragma unroll
  for (int q = 0; q < 8; q++) {
    const int j = j0 + ty + 4 * q;
    if (j < N) {
      const size_t o = (size_t)j * N + i0 + tx;
      Fa[o] -= acc[q];  // lambda = -W
      Fb[o] += acc[q];
    }
  }
}

__global__ __launch_bounds__(256) void k_cuhf_delta(const double *__restrict__ Fa, const double *__restrict__ Fb, size_t len,
                                                    double *__restrict__ D) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < len; i += stride) D[i] = 0.5 * Fa[i] - 0.5 * Fb[i];
}
// lambda in the natural-orbital basis (ascending occupations: virtual 0 .. Nv-1, core n-Nc .. n-1): the core-virtual
// blocks of -Delta, everything else zero
__global__ void k_cuhf_no_lambda(double *__restrict__ D, int n, int Nc, int Nv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i >= n) return;
  const bool ic = i >= n - Nc, iv = i < Nv, jc = j >= n - Nc, jv = j < Nv;
  const size_t o = (size_t)j * n + i;
  D[o] = ((ic && jv) || (iv && jc)) ? -D[o] : 0.0;
}
__global__ __launch_bounds__(256) void k_cuhf_add(const double *__restrict__ L, size_t len, double *__restrict__ Fa, double *__restrict__ Fb) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < len; i += stride) {
    Fa[i] += L[i];
    Fb[i] -= L[i];
  }
}

unsigned stream_blocks(size_t len) { return (unsigned)std::min<size_t>((len + 255) / 256, 4096); }

}  // namespace

void cuhf_lowrank_dev(hfg_ctx *ctx, int N, const double *dS, const double *dCa, int nocca, const double *dCb, int noccb, double *dFa,
                      double *dFb) {
  const int r = nocca + noccb, Nc = std::min(nocca, noccb), Nw = std::max(nocca, noccb);
  if (Nc < 1 || nocca == noccb) return;
  if (r > CUHF_LR_MAXCOLS || r > N) throw std::logic_error("cuhf_lowrank_dev: nocca + noccb <= 128 and <= N\n");
  ProfScope ps(ctx, "cuhf_lowrank");
  hipStream_t s = ctx->stream;
  CuhfWork &w = ctx->work.get<CuhfWork>(WS_CUHF);
  const size_t Nr = (size_t)N * r;
  w.C.resize(Nr);
  w.SC.resize(Nr);
  w.G.resize((size_t)r * r);
  w.R.resize((size_t)r * r);
  w.lam.resize(r);
  w.Q.resize((size_t)r * Nw);
  w.Y.resize((size_t)N * Nw);
  w.T.resize((size_t)N * Nw);
  w.AT.resize((size_t)N * Nc);
  w.Mt.resize((size_t)Nw * Nc);
  HFG_HIP_CHECK(hipMemcpyAsync(w.C.p, dCa, sizeof(double) * N * (size_t)nocca, hipMemcpyDeviceToDevice, s));
  HFG_HIP_CHECK(hipMemcpyAsync(w.C.p + (size_t)N * nocca, dCb, sizeof(double) * N * (size_t)noccb, hipMemcpyDeviceToDevice, s));
  gemm_dev(ctx, false, false, N, r, N, 1.0, dS, N, w.C.p, N, 0.0, w.SC.p, N);
  hipLaunchKernelGGL(k_cuhf_gram, dim3(r, r), dim3(256), 0, s, w.C.p, w.SC.p, N, r, w.G.p);
  eig_sym_dev(ctx, r, w.G.p, w.lam.p, w.R.p);  // occupations ascending
  hipLaunchKernelGGL(k_cuhf_q, dim3((r + 63) / 64, Nw), dim3(64), 0, s, w.R.p, w.lam.p, r, w.Q.p);
  gemm_dev(ctx, false, false, N, Nw, r, 1.0, w.C.p, N, w.Q.p, r, 0.0, w.Y.p, N);   // Y_w
  gemm_dev(ctx, false, false, N, Nw, r, 1.0, w.SC.p, N, w.Q.p, r, 0.0, w.T.p, N);  // T_w
  hipLaunchKernelGGL(k_cuhf_a, dim3((N + 15) / 16), dim3(256), 0, s, dFa, dFb, w.Y.p, N, Nc, w.AT.p);
  gemm_dev(ctx, true, false, Nw, Nc, N, 1.0, w.Y.p, N, w.AT.p, N, 0.0, w.Mt.p, Nw);     // M^T = Y_w^T A^T
  gemm_dev(ctx, false, false, N, Nc, Nw, -1.0, w.T.p, N, w.Mt.p, Nw, 1.0, w.AT.p, N);  // A'^T = A^T - T_w M^T
  {
    ProfScope pa(ctx, "cuhf_apply");
    hipLaunchKernelGGL(k_cuhf_apply, dim3((N + 63) / 64, (N + 31) / 32), dim3(256), 0, s, w.T.p, w.AT.p, N, Nc, dFa, dFb);
  }
  HFG_HIP_CHECK(hipGetLastError());
}

void cuhf_dense_dev(hfg_ctx *ctx, int N, int n, const double *dP, const double *dSh, const double *dSinvh, int nocca, int noccb,
                    double *dFa, double *dFb) {
  const int Nc = std::min(nocca, noccb), Nv = n - std::max(nocca, noccb);
  if (Nc < 1 || nocca == noccb) return;
  if (n < 1 || n > N || Nv < 0) throw std::logic_error("cuhf_dense_dev: max(nocca, noccb) <= n <= N\n");
  ProfScope ps(ctx, "cuhf_dense");
  hipStream_t s = ctx->stream;
  CuhfWork &w = ctx->work.get<CuhfWork>(WS_CUHF);
  const size_t NN = (size_t)N * N;
  for (DevBuf<double> *b : {&w.T1, &w.T2, &w.Pvec, &w.A2N, &w.ShPv}) b->resize(NN);
  w.occ.resize(N);
  // the sequence of the device SCF driver (scf_device.hip, "scf::ROHF_update"), Sinvh with n <= N columns
  gemm_dev(ctx, false, false, N, n, N, 1.0, dP, N, dSh, N, 0.0, w.T1.p, N);
  gemm_dev(ctx, true, false, n, n, N, 1.0, dSh, N, w.T1.p, N, 0.0, w.T2.p, n);  // P in the orthonormal basis
  eig_sym_dev(ctx, n, w.T2.p, w.occ.p, w.Pvec.p);                                // natural orbitals, ascending
  gemm_dev(ctx, false, false, N, n, n, 1.0, dSinvh, N, w.Pvec.p, n, 0.0, w.A2N.p, N);
  gemm_dev(ctx, false, false, N, n, n, 1.0, dSh, N, w.Pvec.p, n, 0.0, w.ShPv.p, N);
  hipLaunchKernelGGL(k_cuhf_delta, dim3(stream_blocks(NN)), dim3(256), 0, s, dFa, dFb, NN, w.T1.p);
  gemm_dev(ctx, false, false, N, n, N, 1.0, w.T1.p, N, w.A2N.p, N, 0.0, w.T2.p, N);
  gemm_dev(ctx, true, false, n, n, N, 1.0, w.A2N.p, N, w.T2.p, N, 0.0, w.T1.p, n);  // Delta in the NO basis
  hipLaunchKernelGGL(k_cuhf_no_lambda, dim3((n + 255) / 256, n), dim3(256), 0, s, w.T1.p, n, Nc, Nv);
  gemm_dev(ctx, false, false, N, n, n, 1.0, w.ShPv.p, N, w.T1.p, n, 0.0, w.T2.p, N);
  gemm_dev(ctx, false, true, N, N, n, 1.0, w.T2.p, N, w.ShPv.p, N, 0.0, w.T1.p, N);  // lambda in the AO basis
  hipLaunchKernelGGL(k_cuhf_add, dim3(stream_blocks(NN)), dim3(256), 0, s, w.T1.p, NN, dFa, dFb);
  HFG_HIP_CHECK(hipGetLastError());
}

namespace {
// what the dense route needs and the entry does not get: S^{-1/2} (one block), its partner Sh = S Sinvh and P = Pa + Pb
void cuhf_dense_from_orbitals(hfg_ctx *ctx, int N, const double *dS, const double *dCa, int nocca, const double *dCb, int noccb,
                              double *dFa, double *dFb) {
  CuhfWork &w = ctx->work.get<CuhfWork>(WS_CUHF);
  const size_t NN = (size_t)N * N;
  {
    ProfScope ps(ctx, "cuhf_dense_metric");
    for (DevBuf<double> *b : {&w.Sinvh, &w.Sh, &w.P}) b->resize(NN);
    std::vector<int64_t> idx(N);
    for (int i = 0; i < N; i++) idx[i] = i;
    const int64_t ptr[2] = {0, N};
    form_sinvh_dev(ctx, N, dS, false, 1, ptr, idx.data(), w.Sinvh.p);
    HFG_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // idx lives on this stack frame
    gemm_dev(ctx, false, false, N, N, N, 1.0, dS, N, w.Sinvh.p, N, 0.0, w.Sh.p, N);
    gemm_dev(ctx, false, true, N, N, nocca, 1.0, dCa, N, dCa, N, 0.0, w.P.p, N);
    gemm_dev(ctx, false, true, N, N, noccb, 1.0, dCb, N, dCb, N, 1.0, w.P.p, N);
  }
  cuhf_dense_dev(ctx, N, N, w.P.p, w.Sh.p, w.Sinvh.p, nocca, noccb, dFa, dFb);
}

template <class Fn>
int guarded(Fn &&fn) {
  try {
    fn();
  } catch (const std::logic_error &e) {
    set_error(e.what());
    return 1;
  } catch (const std::runtime_error &e) {
    set_error(e.what());
    return 2;
  } catch (const std::exception &e) {
    set_error(e.what());
    return 3;
  }
  return 0;
}
}  // namespace

}  // namespace hfg

extern "C" {

int hfg_cuhf_update_devptr(hfg_ctx *ctx, int64_t N, const double *dS, const double *dCa, int64_t nocca, const double *dCb,
                           int64_t noccb, double *dFa, double *dFb) {
  return hfg::guarded([&] {
    if (!ctx) throw std::logic_error("hfg_cuhf_update_devptr: null context\n");
    if (N < 1 || N > 46340) throw std::logic_error("hfg_cuhf_update_devptr: 1 <= N <= 46340\n");
    if (nocca < 0 || noccb < 0 || nocca > N || noccb > N) throw std::logic_error("hfg_cuhf_update_devptr: 0 <= nocc <= N\n");
    if (nocca == noccb || nocca == 0 || noccb == 0) return;  // no core or no active space: lambda = 0
    if (!dS || !dCa || !dCb || !dFa || !dFb) throw std::logic_error("hfg_cuhf_update_devptr: null pointer\n");
    HFG_HIP_CHECK(hipSetDevice(ctx->device));
    if (nocca + noccb <= hfg::CUHF_LR_MAXCOLS && helfem::tuning_live().cuhf_lowrank)
      hfg::cuhf_lowrank_dev(ctx, (int)N, dS, dCa, (int)nocca, dCb, (int)noccb, dFa, dFb);
    else
      hfg::cuhf_dense_from_orbitals(ctx, (int)N, dS, dCa, (int)nocca, dCb, (int)noccb, dFa, dFb);
  });
}

int hfg_rohf_update(hfg_ctx *ctx, int64_t N, int64_t n, double *Fa, double *Fb, const double *P, const double *Sh,
                    const double *Sinvh, int64_t nocca, int64_t noccb) {
  return hfg::guarded([&] {
    if (!ctx) throw std::logic_error("hfg_rohf_update: null context\n");
    if (N < 1 || N > 46340 || n < 1 || n > N) throw std::logic_error("hfg_rohf_update: 1 <= n <= N <= 46340\n");
    if (nocca < 0 || noccb < 0 || nocca > n || noccb > n) throw std::logic_error("hfg_rohf_update: 0 <= nocc <= n\n");
    if (nocca == noccb || nocca == 0 || noccb == 0) return;
    if (!Fa || !Fb || !P || !Sh || !Sinvh) throw std::logic_error("hfg_rohf_update: null pointer\n");
    HFG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t NN = (size_t)N * N, Nn = (size_t)N * n;
    hfg::DevBuf<double> dFa, dFb, dP, dSh, dX;
    dFa.resize(NN);
    dFb.resize(NN);
    dP.resize(NN);
    dSh.resize(Nn);
    dX.resize(Nn);
    HFG_HIP_CHECK(hipMemcpyAsync(dFa.p, Fa, sizeof(double) * NN, hipMemcpyHostToDevice, s));
    HFG_HIP_CHECK(hipMemcpyAsync(dFb.p, Fb, sizeof(double) * NN, hipMemcpyHostToDevice, s));
    HFG_HIP_CHECK(hipMemcpyAsync(dP.p, P, sizeof(double) * NN, hipMemcpyHostToDevice, s));
    HFG_HIP_CHECK(hipMemcpyAsync(dSh.p, Sh, sizeof(double) * Nn, hipMemcpyHostToDevice, s));
    HFG_HIP_CHECK(hipMemcpyAsync(dX.p, Sinvh, sizeof(double) * Nn, hipMemcpyHostToDevice, s));
    hfg::cuhf_dense_dev(ctx, (int)N, (int)n, dP.p, dSh.p, dX.p, (int)nocca, (int)noccb, dFa.p, dFb.p);
    HFG_HIP_CHECK(hipMemcpyAsync(Fa, dFa.p, sizeof(double) * NN, hipMemcpyDeviceToHost, s));
    HFG_HIP_CHECK(hipMemcpyAsync(Fb, dFb.p, sizeof(double) * NN, hipMemcpyDeviceToHost, s));
    HFG_HIP_CHECK(hipStreamSynchronize(s));
  });
}

}  // extern "C"
