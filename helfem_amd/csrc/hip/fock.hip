// Coulomb and exchange-correlation Fock-matrix kernels for the diatomic basis (gfx950).
//
// What they replace (reference, /root/reference):
//   TwoDBasis::coulomb                src/diatomic/basis.cpp:1359-1530
//   DFTGrid::eval_Fxc (restricted)    src/diatomic/dftgrid.cpp:769-810 and the worker it drives
//                                     (:51-117 update_density, :343-458 compute_xc, :499-545 eval_Fxc,
//                                      :669-755 compute_bf, dftgrid.h:190-253 increment_lda/gga)
//
// Design notes (DESIGN.md has the long version):
//  * Both J and the XC matrix are block-banded in the radial index (two FEM functions only overlap
//    inside one element), and both only read the element-diagonal p x p blocks of P.  All work is
//    done on the "compact" layout X_c[x][y][e][j][i] (tables.h); dense N x N matrices appear only at
//    the API boundary (gather_compact / scatter_dense).
//  * XC: the reference forms the complex (A*p) x (ntheta*nphi) basis-function matrix for every radial
//    point and runs zgemm on it.  Here the product structure  bf = B_n(mu) Theta_lm(theta) e^{i m phi}
//    is used: contract the radial index (X1), the theta index per (m,m') group pair (X2), evaluate
//    the functional on the grid with the phi sums folded in (X3), and go back up (X4, X5).  Same
//    sums, different association order; ~2000x fewer flops, no O(Ng * ne) intermediates.
//  * No atomics anywhere: every output element has exactly one writer and a fixed summation order,
//    so results are bitwise reproducible run to run.
#include "internal.h"
#include "xc_device.h"
#include "../host/dftfuncs.h"
#include "../host/fock_need.h"
#include "../host/fock_plan.h"
#include <algorithm>
#include <cstring>

namespace hfg {

// -------------------------------------------------------------------------------------------------
// dense <-> compact
// -------------------------------------------------------------------------------------------------
// Xc[x][y][e][j][i] = P(pure(x,e*(p-1)+i), pure(y,e*(p-1)+j))
__global__ void k_gather_compact(const double *__restrict__ P, int N, int A, int R, int E, int p,
                                 const int *__restrict__ shell_off, const int *__restrict__ shell_skip,
                                 double *__restrict__ Xc, int *__restrict__ on) {
  int blk = blockIdx.x;  // (x*A+y)*E+e
  int e = blk % E;
  int xy = blk / E;
  int y = xy % A, x = xy / A;
  int pp = p * p;
  int live = 0;
  for (int t = threadIdx.x; t < pp; t += blockDim.x) {
    int i = t % p, j = t / p;
    int ni = e * (p - 1) + i, nj = e * (p - 1) + j;
    double v = 0.0;
    bool ok = (ni < R) && (nj < R) && !(shell_skip[x] && ni == 0) && !(shell_skip[y] && nj == 0);
    if (ok) v = P[(size_t)(shell_off[y] + nj) * N + (shell_off[x] + ni)];
    Xc[(size_t)blk * pp + t] = v;
    live |= (v != 0.0);  // true for a NaN: it stays "on" and propagates
  }
  // on[blk]: the block holds something other than zeros (DESIGN 3.1 "Skipped work"); one writer per flag
  if (on) {
    live = __syncthreads_or(live);
    if (threadIdx.x == 0) on[blk] = live;
  }
}

// gon[e][ga][gb]: some pair (a in group ga, b in group gb) is on in element e -- what X2 asks once per radial point
__global__ void k_skip_groups(const int *__restrict__ on, int A, int E, int G, const int *__restrict__ grp_off,
                              const int *__restrict__ grp_shell, int *__restrict__ gon) {
  int e = blockIdx.x, ga = blockIdx.y / G, gb = blockIdx.y % G;
  int a0 = grp_off[ga], na = grp_off[ga + 1] - a0;
  int b0 = grp_off[gb], nb = grp_off[gb + 1] - b0;
  int live = 0;
  for (int t = threadIdx.x; t < na * nb; t += blockDim.x) {
    int a = grp_shell[a0 + t / nb], b = grp_shell[b0 + t % nb];
    live |= on[((size_t)a * A + b) * E + e];
  }
  live = __syncthreads_or(live);
  if (threadIdx.x == 0) gon[((size_t)e * G + ga) * G + gb] = live;
}

// out(pure row, pure col) = sum over the (one or two) elements that contain both radial functions
__global__ void k_scatter_dense(const double *__restrict__ Xc, int N, int A, int R, int E, int p,
                                const int *__restrict__ pure_shell, const int *__restrict__ pure_n,
                                double *__restrict__ out) {
  int row = blockIdx.x * 64 + (threadIdx.x & 63);
  int col = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (row >= N || col >= N) return;
  int x = pure_shell[row], n = pure_n[row];
  int y = pure_shell[col], m = pure_n[col];
  int pm = p - 1, pp = p * p;
  // candidate elements of n: e1=n/pm (local n%pm) and, on a shared node, e1-1 (local pm)
  int e1 = n / pm, f1 = m / pm;
  double v = 0.0;
  const double *base = Xc + (size_t)(x * A + y) * E * pp;
  for (int ce = 0; ce < 2; ce++) {
    int e = e1 - ce;
    if (e < 0 || e >= E) continue;
    int i = n - e * pm;
    if (i < 0 || i > pm) continue;
    for (int cf = 0; cf < 2; cf++) {
      int f = f1 - cf;
      if (f != e) continue;
      int j = m - f * pm;
      if (j < 0 || j > pm) continue;
      v += base[(size_t)e * pp + j * p + i];
    }
  }
  out[(size_t)col * N + row] = v;
}

// F(row,col) = [blockid(row)==blockid(col)] * (H0(row,col) + scatter(Xc)(row,col))
// (Fock assembly + scf::enforce_fock_symmetry, src/diatomic/main.cpp:871-900, scf_helpers.cpp:249)
__global__ void k_fock_finish(const double *__restrict__ Xc, const double *__restrict__ H0,
                              const int *__restrict__ blockid, int N, int A, int R, int E, int p,
                              const int *__restrict__ pure_shell, const int *__restrict__ pure_n,
                              double *__restrict__ out) {
  int row = blockIdx.x * 64 + (threadIdx.x & 63);
  int col = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (row >= N || col >= N) return;
  size_t o = (size_t)col * N + row;
  if (blockid && blockid[row] != blockid[col]) {
    out[o] = 0.0;
    return;
  }
  int x = pure_shell[row], n = pure_n[row];
  int y = pure_shell[col], m = pure_n[col];
  int pm = p - 1, pp = p * p;
  int e1 = n / pm, f1 = m / pm;
  double v = H0 ? H0[o] : 0.0;
  const double *base = Xc + (size_t)(x * A + y) * E * pp;
  for (int ce = 0; ce < 2; ce++) {
    int e = e1 - ce;
    if (e < 0 || e >= E) continue;
    int i = n - e * pm;
    if (i < 0 || i > pm) continue;
    for (int cf = 0; cf < 2; cf++) {
      int f = f1 - cf;
      if (f != e) continue;
      int j = m - f * pm;
      if (j < 0 || j > pm) continue;
      v += base[(size_t)e * pp + j * p + i];
    }
  }
  out[o] = v;
}

__global__ void k_add_inplace(double *__restrict__ a, const double *__restrict__ b, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) a[i] += b[i];
}

// The gather of an unrestricted build: both spins in one pass, each as k_gather_compact gives it, with their sum
// Xt = Pa + Pb (the one add that the dense sum in front of coulomb_dev makes) and on[blk] = the block of EITHER spin holds
// something other than zeros -- a superset of what Xt alone would flag, so a skipped entry still only multiplies zeros
__global__ void k_gather_compact_pol(const double *__restrict__ Pa, const double *__restrict__ Pb, int N, int A, int R, int E,
                                     int p, const int *__restrict__ shell_off, const int *__restrict__ shell_skip,
                                     double *__restrict__ Xa, double *__restrict__ Xb, double *__restrict__ Xt,
                                     int *__restrict__ on) {
  int blk = blockIdx.x;  // (x*A+y)*E+e
  int e = blk % E;
  int xy = blk / E;
  int y = xy % A, x = xy / A;
  int pp = p * p;
  int live = 0;
  for (int t = threadIdx.x; t < pp; t += blockDim.x) {
    int i = t % p, j = t / p;
    int ni = e * (p - 1) + i, nj = e * (p - 1) + j;
    double va = 0.0, vb = 0.0;
    bool ok = (ni < R) && (nj < R) && !(shell_skip[x] && ni == 0) && !(shell_skip[y] && nj == 0);
    if (ok) {
      size_t o = (size_t)(shell_off[y] + nj) * N + (shell_off[x] + ni);
      va = Pa[o];
      vb = Pb[o];
    }
    size_t c = (size_t)blk * pp + t;
    Xa[c] = va;
    Xb[c] = vb;
    Xt[c] = va + vb;
    live |= (va != 0.0) | (vb != 0.0);  // true for a NaN in either spin
  }
  if (on) {
    live = __syncthreads_or(live);
    if (threadIdx.x == 0) on[blk] = live;
  }
}

// Fc[0 : nc] = J + XC_a, Fc[nc : 2 nc] = J + XC_b; J arrives in the second slab and is read once
__global__ void k_fock_combine_pol(double *__restrict__ Fc, const double *__restrict__ Xa, const double *__restrict__ Xb,
                                   size_t nc) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < nc; i += stride) {
    double j = Fc[nc + i];
    Fc[i] = j + Xa[i];
    Fc[nc + i] = j + Xb[i];
  }
}

// k_fock_finish for the two slabs of an unrestricted build: H0, the block ids and the index maps are read once, and each
// spin is summed in the order of k_fock_finish
__global__ void k_fock_finish_pol(const double *__restrict__ Xc, size_t nc, const double *__restrict__ H0,
                                  const int *__restrict__ blockid, int N, int A, int R, int E, int p,
                                  const int *__restrict__ pure_shell, const int *__restrict__ pure_n,
                                  double *__restrict__ outa, double *__restrict__ outb) {
  int row = blockIdx.x * 64 + (threadIdx.x & 63);
  int col = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (row >= N || col >= N) return;
  size_t o = (size_t)col * N + row;
  if (blockid && blockid[row] != blockid[col]) {
    outa[o] = 0.0;
    outb[o] = 0.0;
    return;
  }
  int x = pure_shell[row], n = pure_n[row];
  int y = pure_shell[col], m = pure_n[col];
  int pm = p - 1, pp = p * p;
  int e1 = n / pm, f1 = m / pm;
  double va = H0 ? H0[o] : 0.0, vb = va;
  const double *base = Xc + (size_t)(x * A + y) * E * pp;
  for (int ce = 0; ce < 2; ce++) {
    int e = e1 - ce;
    if (e < 0 || e >= E) continue;
    int i = n - e * pm;
    if (i < 0 || i > pm) continue;
    for (int cf = 0; cf < 2; cf++) {
      int f = f1 - cf;
      if (f != e) continue;
      int j = m - f * pm;
      if (j < 0 || j > pm) continue;
      size_t c = (size_t)e * pp + j * p + i;
      va += base[c];
      vb += base[nc + c];
    }
  }
  outa[o] = va;
  outb[o] = vb;
}

// -------------------------------------------------------------------------------------------------
// Coulomb
// -------------------------------------------------------------------------------------------------
// K1  ket contraction (basis.cpp:1380-1405), restricted to the element-diagonal blocks:
//     Paux{0,2}[iLM][e][t] = sum_{(x,y) in iLM} c{0,2} * Pc[x][y][e][t]
__global__ void k_coulomb_ket(const double *__restrict__ Pc, int A, int E, int pp, const int *__restrict__ lm_off,
                              const int *__restrict__ lm_x, const int *__restrict__ lm_y,
                              const double *__restrict__ lm_c0, const double *__restrict__ lm_c2, int NLM,
                              const int *__restrict__ LM_ilm, int rank, int nranks, double *__restrict__ Paux,
                              const int *__restrict__ on, int *__restrict__ chan) {
  int iLM = blockIdx.x, e = blockIdx.y;
  if (LM_ilm[iLM] % nranks != rank) return;  // (L,|M|) channels are the multi-GPU shards of J
  int beg = lm_off[iLM], end = lm_off[iLM + 1];
  if (on) {
    // a channel none of whose pairs carries density in this element is a sum of c * 0: zeros, and "channel off" for K2, K3.
    // (A live channel runs the full loop below: the entries of one (L, M) all have m_x - m_y = M, so with a density that
    // is block diagonal in m they are live or dead together.)
    int live = 0;
    for (int k = beg + threadIdx.x; k < end; k += blockDim.x) live |= on[((size_t)lm_x[k] * A + lm_y[k]) * E + e];
    live = __syncthreads_or(live);
    if (threadIdx.x == 0) chan[(size_t)iLM * E + e] = live;
    if (!live) {
      for (int t = threadIdx.x; t < pp; t += blockDim.x) {
        Paux[((size_t)(0 * NLM + iLM) * E + e) * pp + t] = 0.0;
        Paux[((size_t)(1 * NLM + iLM) * E + e) * pp + t] = 0.0;
      }
      return;
    }
  }
  for (int t = threadIdx.x; t < pp; t += blockDim.x) {
    double a0 = 0.0, a2 = 0.0;
    // eight entries in flight: the rolled "load P, two FMAs" loop paid one memory round trip per entry (~330 entries per
    // channel: 146 us for the kernel); the order of the additions is unchanged
    int k = beg;
    for (; k + 8 <= end; k += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) v[u] = Pc[((size_t)(lm_x[k + u] * A + lm_y[k + u]) * E + e) * pp + t];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        a0 += lm_c0[k + u] * v[u];
        a2 += lm_c2[k + u] * v[u];
      }
    }
    for (; k < end; k++) {
      double v = Pc[((size_t)(lm_x[k] * A + lm_y[k]) * E + e) * pp + t];
      a0 += lm_c0[k] * v;
      a2 += lm_c2[k] * v;
    }
    Paux[((size_t)(0 * NLM + iLM) * E + e) * pp + t] = a0;
    Paux[((size_t)(1 * NLM + iLM) * E + e) * pp + t] = a2;
  }
}

// K2b in-element integrals (basis.cpp:1472-1485): Y[tt][iLM][e][:] = tei_tt[ilm][e] * vec(Paux_{tt&1 ? 2:0}[iLM][e])
//     for iLM=(L,+|M|) and its partner (L,-|M|) in one pass over the p^2 x p^2 table (HBM-bound:
//     this is where the 4*Nlm*E*p^4*8 bytes of primitive integrals are streamed once per build).
__global__ void k_coulomb_tei(const double *__restrict__ tei, const double *__restrict__ Paux, int Ntab, int NLM,
                              int E, int pp, const int *__restrict__ lmpos /* [Nlm][2] iLM of +M and -M */,
                              const int *__restrict__ lm_tab, int rank, int nranks, double *__restrict__ Y,
                              const int *__restrict__ chan) {
  extern __shared__ double sh[];  // x_plus[pp], x_minus[pp]
  int ilm = blockIdx.x / E, e = blockIdx.x % E;
  if (ilm % nranks != rank) return;
  int tt = blockIdx.y;  // 0:00 1:02 2:20 3:22
  int iLMp = lmpos[2 * ilm], iLMm = lmpos[2 * ilm + 1];
  if (chan && !(iLMp >= 0 && chan[(size_t)iLMp * E + e]) && !(iLMm >= 0 && chan[(size_t)iLMm * E + e])) {
    // both right-hand sides are zero (K1 said so): the table is not read at all
    for (int r = threadIdx.x; r < pp; r += blockDim.x) {
      if (iLMp >= 0) Y[((size_t)(tt * NLM + iLMp) * E + e) * pp + r] = 0.0;
      if (iLMm >= 0) Y[((size_t)(tt * NLM + iLMm) * E + e) * pp + r] = 0.0;
    }
    return;
  }
  int which = (tt & 1);  // 00,20 act on Paux0 ; 02,22 act on Paux2
  double *xp = sh, *xm = sh + pp;
  for (int t = threadIdx.x; t < pp; t += blockDim.x) {
    xp[t] = (iLMp >= 0) ? Paux[((size_t)(which * NLM + iLMp) * E + e) * pp + t] : 0.0;
    xm[t] = (iLMm >= 0) ? Paux[((size_t)(which * NLM + iLMm) * E + e) * pp + t] : 0.0;
  }
  __syncthreads();
  const double *T = tei + (((size_t)tt * Ntab + lm_tab[ilm]) * E + e) * (size_t)pp * pp;
  for (int r = threadIdx.x; r < pp; r += blockDim.x) {
    double yp = 0.0, ym = 0.0;
#pragma unroll 5
    for (int c = 0; c < pp; c++) {
      double v = T[(size_t)c * pp + r];
      yp += v * xp[c];
      ym += v * xm[c];
    }
    if (iLMp >= 0) Y[((size_t)(tt * NLM + iLMp) * E + e) * pp + r] = yp;
    if (iLMm >= 0) Y[((size_t)(tt * NLM + iLMm) * E + e) * pp + r] = ym;
  }
}

// K2c per (L,M): disjoint (cross-element) part via the trace scalars + in-element part (basis.cpp:1424-1494).
//     full = 1: prolate kernel with the four P0/P2/Q0/Q2 and 00/02/20/22 tables; full = 0: spherical kernel
//     r_<^L/r_>^{L+1} with P0/Q0 and 00 only (atomic TwoDBasis.cpp:884-936), disj then holds [P0][Q0].
//     (the body is shared with k_coulomb_radial_batch, which runs it once per density of a batch)
__device__ __forceinline__ void coulomb_radial_body(const double *__restrict__ Paux, const double *__restrict__ Y,
                                                    const double *__restrict__ disj, const int *__restrict__ LM_ilm,
                                                    const int *__restrict__ LM_tab, const double *__restrict__ LM_fac, int Ntab,
                                                    int NLM, int E, int p, int full, int rank, int nranks,
                                                    double *__restrict__ Jaux, const int *__restrict__ chan = nullptr) {
  extern __shared__ double sh[];  // red[4*E*nwave], sc[4*E], big[E], small[E]
  int iLM = blockIdx.x;
  if (LM_ilm[iLM] % nranks != rank) return;
  int tab = LM_tab[iLM];
  double fac = LM_fac[iLM];
  int pp = p * p;
  if (chan) {
    // the elements couple through the trace scalars: only a channel that is off in every element is all zeros
    int live = 0;
    for (int e = threadIdx.x; e < E; e += blockDim.x) live |= chan[(size_t)iLM * E + e];
    if (!__syncthreads_or(live)) {
      for (int t = threadIdx.x; t < E * pp; t += blockDim.x) {
        Jaux[(size_t)(0 * NLM + iLM) * E * pp + t] = 0.0;
        Jaux[(size_t)(1 * NLM + iLM) * E * pp + t] = 0.0;
      }
      return;
    }
  }
  int nwave = blockDim.x / 64, wave = threadIdx.x / 64, lane = threadIdx.x & 63;
  double *red = sh;
  double *sc = red + 4 * E * nwave;
  double *big = sc + 4 * E, *small = big + E;
  const int tQ0 = full ? 2 : 1;
  const double *dP0 = disj + ((size_t)0 * Ntab + tab) * E * pp;
  const double *dQ0 = disj + ((size_t)tQ0 * Ntab + tab) * E * pp;
  const double *dP2 = full ? disj + ((size_t)1 * Ntab + tab) * E * pp : nullptr;
  const double *dQ2 = full ? disj + ((size_t)3 * Ntab + tab) * E * pp : nullptr;
  // traces: js[k][e], k: 0 small0=tr(P0*Psub0) 1 big0=tr(Q0*Psub0) 2 small2=tr(P2*Psub2) 3 big2=tr(Q2*Psub2)
  for (int e = 0; e < E; e++) {
    double a[4] = {0, 0, 0, 0};
    for (int t = threadIdx.x; t < pp; t += blockDim.x) {
      int i = t % p, j = t / p;
      double x0 = Paux[((size_t)(0 * NLM + iLM) * E + e) * pp + (i * p + j)];  // Psub(j,i)
      a[0] += dP0[(size_t)e * pp + t] * x0;
      a[1] += dQ0[(size_t)e * pp + t] * x0;
      if (full) {
        double x2 = Paux[((size_t)(1 * NLM + iLM) * E + e) * pp + (i * p + j)];
        a[2] += dP2[(size_t)e * pp + t] * x2;
        a[3] += dQ2[(size_t)e * pp + t] * x2;
      }
    }
    for (int k = 0; k < 4; k++) {
      double v = a[k];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
      if (lane == 0) red[(k * E + e) * nwave + wave] = v;
    }
  }
  __syncthreads();
  // (strided: 4 * E exceeds the workgroup from E = 17 at up to 8 nodes, E = 65 at 14 and more)
  for (int k = threadIdx.x; k < 4 * E; k += blockDim.x) {
    double v = 0.0;
    for (int w = 0; w < nwave; w++) v += red[k * nwave + w];
    sc[k] = fac * v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    // contributions to element e from jel>e use "big" of jel, from jel<e use "small" of jel
    double sb = 0.0, ss = 0.0;
    for (int jel = e + 1; jel < E; jel++) sb += sc[1 * E + jel] - sc[3 * E + jel];  // jbig0 - jbig2
    for (int jel = 0; jel < e; jel++) ss += sc[0 * E + jel] - sc[2 * E + jel];      // jsmall0 - jsmall2
    big[e] = sb;
    small[e] = ss;
  }
  __syncthreads();
  for (int e = 0; e < E; e++)
    for (int t = threadIdx.x; t < pp; t += blockDim.x) {
      double P0 = dP0[(size_t)e * pp + t], Q0 = dQ0[(size_t)e * pp + t];
      double y00 = Y[((size_t)(0 * NLM + iLM) * E + e) * pp + t];
      double j0 = P0 * big[e] + Q0 * small[e] + fac * y00;
      double j2 = 0.0;
      if (full) {
        double P2 = dP2[(size_t)e * pp + t], Q2 = dQ2[(size_t)e * pp + t];
        double y02 = Y[((size_t)(1 * NLM + iLM) * E + e) * pp + t];
        double y20 = Y[((size_t)(2 * NLM + iLM) * E + e) * pp + t], y22 = Y[((size_t)(3 * NLM + iLM) * E + e) * pp + t];
        j0 -= fac * y02;
        j2 = -P2 * big[e] - Q2 * small[e] - fac * y20 + fac * y22;
      }
      Jaux[((size_t)(0 * NLM + iLM) * E + e) * pp + t] = j0;
      Jaux[((size_t)(1 * NLM + iLM) * E + e) * pp + t] = j2;
    }
}
__global__ void k_coulomb_radial(const double *__restrict__ Paux, const double *__restrict__ Y,
                                 const double *__restrict__ disj, const int *__restrict__ LM_ilm,
                                 const int *__restrict__ LM_tab, const double *__restrict__ LM_fac, int Ntab, int NLM,
                                 int E, int p, int full, int rank, int nranks, double *__restrict__ Jaux,
                                 const int *__restrict__ chan) {
  coulomb_radial_body(Paux, Y, disj, LM_ilm, LM_tab, LM_fac, Ntab, NLM, E, p, full, rank, nranks, Jaux, chan);
}

// K3 bra expansion (basis.cpp:1498-1527): Jc[i][j][e][:] = sum_L c0(j,i,L) Jaux0[iLM] + c2(j,i,L) Jaux2[iLM]
__global__ void k_coulomb_bra(const double *__restrict__ Jaux, int A, int E, int pp, int NLM,
                              const int *__restrict__ pair_off, const int *__restrict__ ent_iLM,
                              const double *__restrict__ ent_c0, const double *__restrict__ ent_c2,
                              const int *__restrict__ LM_ilm, int rank, int nranks, double *__restrict__ Jc,
                              const int *__restrict__ need) {
  int ij = blockIdx.x, e = blockIdx.y;
  if (need && !need[ij]) {  // a block the caller does not read (hfg_ctx_set_fock_blocks): zeros, the buffer is summed over ranks
    for (int t = threadIdx.x; t < pp; t += blockDim.x) Jc[((size_t)ij * E + e) * pp + t] = 0.0;
    return;
  }
  int iang = ij / A, jang = ij % A;
  int pr = jang * A + iang;  // pair (x=jang, y=iang)
  int beg = pair_off[pr], end = pair_off[pr + 1];
  for (int t = threadIdx.x; t < pp; t += blockDim.x) {
    double acc = 0.0;
    // four entries (eight loads) in flight; entries of other ranks' channels contribute an exact zero in the same place
    int k = beg;
    for (; k + 4 <= end; k += 4) {
      double j0[4], j2[4], c0[4], c2[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int iLM = ent_iLM[k + u];
        const bool mine = (LM_ilm[iLM] % nranks == rank);
        j0[u] = Jaux[((size_t)(0 * NLM + iLM) * E + e) * pp + t];
        j2[u] = Jaux[((size_t)(1 * NLM + iLM) * E + e) * pp + t];
        c0[u] = mine ? ent_c0[k + u] : 0.0;
        c2[u] = mine ? ent_c2[k + u] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (c0[u] != 0.0 || c2[u] != 0.0) acc += c0[u] * j0[u] + c2[u] * j2[u];
    }
    for (; k < end; k++) {
      int iLM = ent_iLM[k];
      if (LM_ilm[iLM] % nranks != rank) continue;
      acc += ent_c0[k] * Jaux[((size_t)(0 * NLM + iLM) * E + e) * pp + t] +
             ent_c2[k] * Jaux[((size_t)(1 * NLM + iLM) * E + e) * pp + t];
    }
    Jc[((size_t)ij * E + e) * pp + t] = acc;
  }
}

// -------------------------------------------------------------------------------------------------
// Coulomb for a batch of densities (hfg_coulomb_batch, DESIGN 3.1 "Batched J")
// -------------------------------------------------------------------------------------------------
// Every buffer of the single build gains a leading density index with the stride the caller names: Pc[b][x][y][e][j][i],
// Paux[b][0/2][iLM][e][t], Y[b][tt][iLM][e][t], Jaux[b][0/2][iLM][e][t].  Same sums and the same order of additions per
// density as the kernels above; the in-element tables are read once for all densities of a pass.
constexpr int CB_DB = 4;  // densities per thread of the batched ket and bra kernels: one read of a coupling entry serves them all

// K1 for nb densities: blockIdx.z takes CB_DB of them
__global__ void k_coulomb_ket_batch(const double *__restrict__ Pc, size_t sPc, int nb, int A, int E, int pp,
                                    const int *__restrict__ lm_off, const int *__restrict__ lm_x, const int *__restrict__ lm_y,
                                    const double *__restrict__ lm_c0, const double *__restrict__ lm_c2, int NLM,
                                    const int *__restrict__ LM_ilm, int rank, int nranks, double *__restrict__ Paux, size_t sPaux) {
  const int iLM = blockIdx.x, e = blockIdx.y, b0 = blockIdx.z * CB_DB;
  if (LM_ilm[iLM] % nranks != rank) return;
  const int beg = lm_off[iLM], end = lm_off[iLM + 1];
  for (int t = threadIdx.x; t < pp; t += blockDim.x) {
    double a0[CB_DB], a2[CB_DB];
#pragma unroll
    for (int u = 0; u < CB_DB; u++) a0[u] = a2[u] = 0.0;
#pragma unroll 2
    for (int k = beg; k < end; k++) {
      const size_t o = ((size_t)(lm_x[k] * A + lm_y[k]) * E + e) * pp + t;
      const double c0 = lm_c0[k], c2 = lm_c2[k];
#pragma unroll
      for (int u = 0; u < CB_DB; u++) {
        const double v = (b0 + u < nb) ? Pc[(size_t)(b0 + u) * sPc + o] : 0.0;
        a0[u] += c0 * v;
        a2[u] += c2 * v;
      }
    }
#pragma unroll
    for (int u = 0; u < CB_DB; u++)
      if (b0 + u < nb) {
        double *out = Paux + (size_t)(b0 + u) * sPaux;
        out[((size_t)(0 * NLM + iLM) * E + e) * pp + t] = a0[u];
        out[((size_t)(1 * NLM + iLM) * E + e) * pp + t] = a2[u];
      }
  }
}

// K2b for a batch, small column counts: Y[pp x ncol] = tei[pp x pp] * X[pp x ncol] with the columns (sign s, density b) ->
//     s * nb + b of the +M channel and, where it exists, of its -M partner; NC >= ncol accumulators per thread (one row
//     of Y each), X in LDS as X[c][NC] so that all lanes read one address.  One pass over the table for all columns.
template <int NC>
__global__ void k_coulomb_tei_cols(const double *__restrict__ tei, const double *__restrict__ Paux, size_t sPaux, int nb, int Ntab,
                                   int NLM, int E, int pp, const int *__restrict__ lmpos, const int *__restrict__ lm_tab, int rank,
                                   int nranks, double *__restrict__ Y, size_t sY) {
  extern __shared__ double sh[];  // X[pp][NC]
  const int ilm = blockIdx.x / E, e = blockIdx.x % E;
  if (ilm % nranks != rank) return;
  const int tt = blockIdx.y;
  const int iLMp = lmpos[2 * ilm], iLMm = lmpos[2 * ilm + 1];
  const int which = (tt & 1);
  const int ncol = (iLMm >= 0 ? 2 : 1) * nb;  // host: ncol <= 2 nb <= NC
  for (int idx = threadIdx.x; idx < pp * NC; idx += blockDim.x) {
    const int j = idx / pp, c = idx - j * pp;
    double v = 0.0;
    if (j < ncol) {
      const int sg = (j >= nb) ? 1 : 0, b = j - sg * nb, iLM = sg ? iLMm : iLMp;
      if (iLM >= 0) v = Paux[(size_t)b * sPaux + ((size_t)(which * NLM + iLM) * E + e) * pp + c];
    }
    sh[c * NC + j] = v;
  }
  __syncthreads();
  const double *T = tei + (((size_t)tt * Ntab + lm_tab[ilm]) * E + e) * (size_t)pp * pp;
  for (int r = threadIdx.x; r < pp; r += blockDim.x) {
    double y[NC];
#pragma unroll
    for (int j = 0; j < NC; j++) y[j] = 0.0;
#pragma unroll 4
    for (int c = 0; c < pp; c++) {
      const double v = T[(size_t)c * pp + r];
#pragma unroll
      for (int j = 0; j < NC; j++) y[j] += v * sh[c * NC + j];
    }
#pragma unroll
    for (int j = 0; j < NC; j++)
      if (j < ncol) {
        const int sg = (j >= nb) ? 1 : 0, b = j - sg * nb, iLM = sg ? iLMm : iLMp;
        if (iLM >= 0) Y[(size_t)b * sY + ((size_t)(tt * NLM + iLM) * E + e) * pp + r] = y[j];
      }
  }
}

// K2b for a batch on the matrix cores: the same product with up to 16 NT columns, v_mfma_f64_16x16x4_f64 (operand maps:
//     hip/gemm.hip).  Issued as Y^T = X^T T^T: the a-operand is X^T from LDS (lane l: column l & 15 of the tile, table
//     column c = k0 + (l >> 4)), the b-operand comes straight from the table in HBM (lane l: T[c][row l & 15], 16
//     consecutive doubles per 16 lanes; every table entry is loaded by exactly one lane of one wave, once), and result
//     register r of lane l is Y[row l & 15][column (l >> 4) + 4 r] of the tile: a store writes 16 consecutive rows of four
//     columns.  X sits in LDS as X[c][16 NT], the columns padded with zeros there (never in the table) and, for even NT,
//     the 16-column halves swapped in odd rows so that the two rows a half-wave reads fall into different banks.  Four
//     waves; a wave owns four row tiles (64 rows of Y) for the whole K loop and keeps their 4 x NT result tiles in registers.
//     Rows beyond pp read the last row again and are not stored; the K tail (pp % 4 columns) is one guarded step.
typedef double cb_d4 __attribute__((ext_vector_type(4)));
template <int NT>
__global__ __launch_bounds__(256) void k_coulomb_tei_mfma(const double *__restrict__ tei, const double *__restrict__ Paux, size_t sPaux,
                                                          int nb, int Ntab, int NLM, int E, int pp, const int *__restrict__ lmpos,
                                                          const int *__restrict__ lm_tab, int rank, int nranks,
                                                          double *__restrict__ Y, size_t sY) {
  extern __shared__ double sh[];  // X[cpad][16 NT]
  constexpr int NP = 16 * NT, RT = 4;
  const int ilm = blockIdx.x / E, e = blockIdx.x % E;
  if (ilm % nranks != rank) return;
  const int tt = blockIdx.y;
  const int iLMp = lmpos[2 * ilm], iLMm = lmpos[2 * ilm + 1];
  const int which = (tt & 1);
  const int ncol = (iLMm >= 0 ? 2 : 1) * nb;  // host: ncol <= 2 nb <= NP
  const int cpad = (pp + 3) & ~3;
  // 32 lanes along a column of X (contiguous in Paux), eight columns at a time, eight loads in flight per thread
  for (int j = threadIdx.x >> 5; j < NP; j += 8) {
    const double *src = nullptr;
    if (j < ncol) {
      const int sg = (j >= nb) ? 1 : 0, b = j - sg * nb, iLM = sg ? iLMm : iLMp;
      if (iLM >= 0) src = Paux + (size_t)b * sPaux + ((size_t)(which * NLM + iLM) * E + e) * pp;
    }
    for (int c0 = threadIdx.x & 31; c0 < cpad; c0 += 256) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) v[u] = (src && c0 + 32 * u < pp) ? src[c0 + 32 * u] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int c = c0 + 32 * u;
        if (c < cpad) sh[c * NP + (j ^ ((NT % 2 == 0) ? ((c & 1) << 4) : 0))] = v[u];
      }
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int nrt = (pp + 15) / 16, kfull = pp & ~3;
  const double *T = tei + (((size_t)tt * Ntab + lm_tab[ilm]) * E + e) * (size_t)pp * pp;
  for (int rt0 = wave * RT; rt0 < nrt; rt0 += 4 * RT) {
    cb_d4 acc[RT][NT];
    int roff[RT];
#pragma unroll
    for (int i = 0; i < RT; i++) {
      roff[i] = min((rt0 + i) * 16 + l15, pp - 1);
#pragma unroll
      for (int j = 0; j < NT; j++) acc[i][j] = cb_d4{0.0, 0.0, 0.0, 0.0};
    }
#pragma unroll 4
    for (int k0 = 0; k0 < kfull; k0 += 4) {
      const int c = k0 + l4;
      const double *Tc = T + (size_t)c * pp;
      const double *Xc = sh + c * NP;
      const int sw = (NT % 2 == 0) ? ((c & 1) << 4) : 0;
      double tb[RT], xa[NT];
#pragma unroll
      for (int i = 0; i < RT; i++) tb[i] = Tc[roff[i]];
#pragma unroll
      for (int j = 0; j < NT; j++) xa[j] = Xc[(j * 16 + l15) ^ sw];
#pragma unroll
      for (int i = 0; i < RT; i++)
#pragma unroll
        for (int j = 0; j < NT; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[j], tb[i], acc[i][j], 0, 0, 0);
    }
    if (kfull < pp) {
      const int c = kfull + l4;  // < cpad: the rows of X from pp on hold zeros; the table has no such column
      const double *Tc = T + (size_t)min(c, pp - 1) * pp;
      const double *Xc = sh + c * NP;
      const int sw = (NT % 2 == 0) ? ((c & 1) << 4) : 0;
#pragma unroll
      for (int i = 0; i < RT; i++) {
        const double tb = (c < pp) ? Tc[roff[i]] : 0.0;
#pragma unroll
        for (int j = 0; j < NT; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(Xc[(j * 16 + l15) ^ sw], tb, acc[i][j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < RT; i++) {
      const int row = (rt0 + i) * 16 + l15;
      if (row >= pp) continue;
#pragma unroll
      for (int j = 0; j < NT; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int col = j * 16 + l4 + 4 * r;
          if (col >= ncol) continue;
          const int sg = (col >= nb) ? 1 : 0, b = col - sg * nb, iLM = sg ? iLMm : iLMp;
          if (iLM >= 0) Y[(size_t)b * sY + ((size_t)(tt * NLM + iLM) * E + e) * pp + row] = acc[i][j][r];
        }
    }
  }
}

// K2c for a batch: the single-density body once per (channel, density); the LDS scalars are per workgroup, so per density
__global__ void k_coulomb_radial_batch(const double *__restrict__ Paux, size_t sPaux, const double *__restrict__ Y, size_t sY,
                                       const double *__restrict__ disj, const int *__restrict__ LM_ilm,
                                       const int *__restrict__ LM_tab, const double *__restrict__ LM_fac, int Ntab, int NLM, int E,
                                       int p, int full, int rank, int nranks, double *__restrict__ Jaux, size_t sJaux) {
  const size_t b = blockIdx.y;
  coulomb_radial_body(Paux + b * sPaux, Y + b * sY, disj, LM_ilm, LM_tab, LM_fac, Ntab, NLM, E, p, full, rank, nranks,
                      Jaux + b * sJaux);
}

// K3 for nb densities: blockIdx.z takes CB_DB of them
__global__ void k_coulomb_bra_batch(const double *__restrict__ Jaux, size_t sJaux, int nb, int A, int E, int pp, int NLM,
                                    const int *__restrict__ pair_off, const int *__restrict__ ent_iLM,
                                    const double *__restrict__ ent_c0, const double *__restrict__ ent_c2,
                                    const int *__restrict__ LM_ilm, int rank, int nranks, double *__restrict__ Jc, size_t sJc) {
  const int ij = blockIdx.x, e = blockIdx.y, b0 = blockIdx.z * CB_DB;
  const int iang = ij / A, jang = ij % A;
  const int pr = jang * A + iang;
  const int beg = pair_off[pr], end = pair_off[pr + 1];
  for (int t = threadIdx.x; t < pp; t += blockDim.x) {
    double acc[CB_DB];
#pragma unroll
    for (int u = 0; u < CB_DB; u++) acc[u] = 0.0;
    for (int k = beg; k < end; k++) {
      const int iLM = ent_iLM[k];
      if (LM_ilm[iLM] % nranks != rank) continue;
      const double c0 = ent_c0[k], c2 = ent_c2[k];
      const size_t o0 = ((size_t)(0 * NLM + iLM) * E + e) * pp + t, o2 = ((size_t)(1 * NLM + iLM) * E + e) * pp + t;
#pragma unroll
      for (int u = 0; u < CB_DB; u++)
        if (b0 + u < nb) {
          const double *J = Jaux + (size_t)(b0 + u) * sJaux;
          acc[u] += c0 * J[o0] + c2 * J[o2];
        }
    }
#pragma unroll
    for (int u = 0; u < CB_DB; u++)
      if (b0 + u < nb) Jc[(size_t)(b0 + u) * sJc + ((size_t)ij * E + e) * pp + t] = acc[u];
  }
}

// W[a][b0 + b] = sum over the compact entries of Pc[a] * Jc[b] = tr(P_a J[P_b]) (both block-banded: the compact layout holds
//     every entry of J and the entries of P that meet them, each once).  Stage 1: workgroup (slice, a tile, b tile) sums
//     a 4 x 4 tile over its slice of the entries in a fixed order; stage 2 adds the slices in order.  No atomics.
constexpr int CB_WT = 4, CB_SLICE = 8192;
__global__ __launch_bounds__(256) void k_coulomb_energy_part(const double *__restrict__ Pc, int nP, const double *__restrict__ Jc, int nb,
                                                             size_t nc, double *__restrict__ part /* [slice][nP][nb] */) {
  __shared__ double red[4][CB_WT * CB_WT];
  const int a0 = blockIdx.y * CB_WT, b0 = blockIdx.z * CB_WT;
  const size_t beg = (size_t)blockIdx.x * CB_SLICE, end = min(nc, beg + CB_SLICE);
  double acc[CB_WT][CB_WT];
#pragma unroll
  for (int i = 0; i < CB_WT; i++)
#pragma unroll
    for (int j = 0; j < CB_WT; j++) acc[i][j] = 0.0;
  for (size_t k = beg + threadIdx.x; k < end; k += blockDim.x) {
    double pv[CB_WT], jv[CB_WT];
#pragma unroll
    for (int i = 0; i < CB_WT; i++) pv[i] = (a0 + i < nP) ? Pc[(size_t)(a0 + i) * nc + k] : 0.0;
#pragma unroll
    for (int j = 0; j < CB_WT; j++) jv[j] = (b0 + j < nb) ? Jc[(size_t)(b0 + j) * nc + k] : 0.0;
#pragma unroll
    for (int i = 0; i < CB_WT; i++)
#pragma unroll
      for (int j = 0; j < CB_WT; j++) acc[i][j] += pv[i] * jv[j];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < CB_WT; i++)
#pragma unroll
    for (int j = 0; j < CB_WT; j++) {
      double v = acc[i][j];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
      if (lane == 0) red[wave][i * CB_WT + j] = v;
    }
  __syncthreads();
  if (threadIdx.x < CB_WT * CB_WT) {
    const int i = threadIdx.x / CB_WT, j = threadIdx.x % CB_WT;
    if (a0 + i < nP && b0 + j < nb)
      part[((size_t)blockIdx.x * nP + (a0 + i)) * nb + (b0 + j)] =
          (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
  }
}
__global__ void k_coulomb_energy_sum(const double *__restrict__ part, int nslice, int nP, int nb, int b0, double *__restrict__ W) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // a * nb + b
  if (idx >= nP * nb) return;
  double v = 0.0;
  for (int s = 0; s < nslice; s++) v += part[(size_t)s * nP * nb + idx];
  const int a = idx / nb, b = idx % nb;
  W[(size_t)(b0 + b) * nP + a] = v;  // column-major nP x nP: W(a, b)
}

// -------------------------------------------------------------------------------------------------
// XC
// -------------------------------------------------------------------------------------------------
// X1 radial contraction of the density: D0[Q][x][y] = sum_ij B_i(q) Pc[x][y][e][j][i] B_j(q),
//    D1[Q][x][y] = sum_ij B'_i(q) Pc[..][j][i] B_j(q)            (replaces Pv = P conj(bf), dftgrid.cpp:62)
//    (meta-GGA: D2[Q][x][y] = sum_ij B'_i Pc B'_j for the kinetic energy density)
//    (Laplacian: D3[Q][x][y] = sum_ij B_i Pc L_j with the radial table L = g'' + 2 g'/r of the y shell's functions)
__global__ __launch_bounds__(256) void k_xc_density_radial(const double *__restrict__ Pc, const double *__restrict__ B,
                                                           const double *__restrict__ dB, const double *__restrict__ Lr, int A,
                                                           int E, int p, int nq, int do_grad, int do_tau, int do_lapl, int rank,
                                                           int nranks, double *__restrict__ D0, double *__restrict__ D1,
                                                           double *__restrict__ D2, double *__restrict__ D3,
                                                           const int *__restrict__ on) {
  // One workgroup per (shell pair, element).  The p x p block of P and the element's B, B' tables sit in LDS (the
  // tables transposed to [i][q]: consecutive q <-> consecutive banks); thread (q, jc) forms the rows j = jc, jc+NJ, ...
  // of T = P b(q), contracts them with b_j, b'_j, and the NJ partial results of a point are summed through LDS in a
  // fixed order.
  extern __shared__ double sh[];  // P[pp], Bt[p][nq], dBt[p][nq], part[3 (4 with do_lapl)][NJ][nq], Lt[p][nq] (do_lapl)
  const int xy = blockIdx.x, e = blockIdx.y;
  const int pp = p * p;
  if (on && !on[(size_t)xy * E + e]) {  // a block of zeros contracts to zeros: nothing is staged
    const size_t AA = (size_t)A * A;
    for (int q = threadIdx.x; q < nq; q += blockDim.x) {
      if ((e * nq + q) % nranks != rank) continue;
      const size_t Q = (size_t)e * nq + q;
      D0[Q * AA + xy] = 0.0;
      if (do_grad) D1[Q * AA + xy] = 0.0;
      if (do_tau) D2[Q * AA + xy] = 0.0;
      if (do_lapl) D3[Q * AA + xy] = 0.0;
    }
    return;
  }
  double *sP = sh, *sB = sh + pp, *sdB = sB + p * nq;
  const int NJ = blockDim.x / nq > 0 ? min((int)(blockDim.x / nq), p) : 1;
  double *part = sdB + p * nq;
  double *sL = part + (do_lapl ? 4 : 3) * NJ * nq;
  for (int t = threadIdx.x; t < pp; t += blockDim.x) sP[t] = Pc[((size_t)xy * E + e) * pp + t];
  for (int t = threadIdx.x; t < p * nq; t += blockDim.x) {
    int q = t / p, i = t % p;
    sB[i * nq + q] = B[((size_t)e * nq + q) * p + i];
    sdB[i * nq + q] = dB[((size_t)e * nq + q) * p + i];
    if (do_lapl) sL[i * nq + q] = Lr[((size_t)e * nq + q) * p + i];
  }
  __syncthreads();
  const size_t AA = (size_t)A * A;
  // work items (q, jc), q fastest; with nq <= blockDim.x every point is finished in one pass
  for (int q0 = 0; q0 < nq; q0 += blockDim.x / NJ) {
    const int ql = threadIdx.x % (blockDim.x / NJ), jc = threadIdx.x / (blockDim.x / NJ);
    const int q = q0 + ql;
    double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
    if (q < nq && jc < NJ)
      for (int j = jc; j < p; j += NJ) {
        double s0 = 0.0, s1 = 0.0;
        for (int i = 0; i < p; i++) {
          double pv = sP[j * p + i];
          s0 += sB[i * nq + q] * pv;
          s1 += sdB[i * nq + q] * pv;
        }
        d0 += s0 * sB[j * nq + q];
        d1 += s1 * sB[j * nq + q];
        d2 += s1 * sdB[j * nq + q];
        if (do_lapl) d3 += s0 * sL[j * nq + q];
      }
    if (q < nq && jc < NJ) {
      part[(0 * NJ + jc) * nq + q] = d0;
      part[(1 * NJ + jc) * nq + q] = d1;
      part[(2 * NJ + jc) * nq + q] = d2;
      if (do_lapl) part[(3 * NJ + jc) * nq + q] = d3;
    }
    __syncthreads();
    if (jc == 0 && q < nq && (e * nq + q) % nranks == rank) {  // radial quadrature points are the multi-GPU shards of XC
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      for (int k = 0; k < NJ; k++) {
        a0 += part[(0 * NJ + k) * nq + q];
        a1 += part[(1 * NJ + k) * nq + q];
        a2 += part[(2 * NJ + k) * nq + q];
        if (do_lapl) a3 += part[(3 * NJ + k) * nq + q];
      }
      const size_t Q = (size_t)e * nq + q;
      D0[Q * AA + xy] = a0;
      if (do_grad) D1[Q * AA + xy] = a1;
      if (do_tau) D2[Q * AA + xy] = a2;
      if (do_lapl) D3[Q * AA + xy] = a3;
    }
    __syncthreads();
  }
}

// X2 theta contraction per (m-group pair): V[k][Q][ga][gb][i],
//    k=0: sum Theta_a D0_ab Theta_b ; k=1: sum dTheta_a D0_ab Theta_b ; k=2: sum Theta_a D1_ab Theta_b
//    meta-GGA: k=3: sum Theta_a D2_ab Theta_b ; k=4: sum dTheta_a D0_ab dTheta_b
//    Laplacian: k=5: sum Theta_a (D3_ab - l_b(l_b+1)/r^2 D0_ab) Theta_b   (eval_lf, atomic/TwoDBasis.cpp:1423-1445)
__global__ void k_xc_density_theta(const double *__restrict__ D0, const double *__restrict__ D1,
                                   const double *__restrict__ D2, const double *__restrict__ D3, const double *__restrict__ Th,
                                   const double *__restrict__ dTh, const int *__restrict__ shell_l,
                                   const double *__restrict__ rad_sh, int A, int nth, int G,
                                   const int *__restrict__ grp_off, const int *__restrict__ grp_shell, int do_grad,
                                   int do_tau, int do_lapl, size_t NQ, int rank, int nranks, double *__restrict__ V, int nq,
                                   const int *__restrict__ gon) {
  extern __shared__ double sh[];  // d0[na*nb], d1[na*nb], d2[na*nb], d3[na*nb] (do_lapl)
  size_t Q = blockIdx.x;
  if ((int)(Q % nranks) != rank) return;
  int ga = blockIdx.y / G, gb = blockIdx.y % G;
  if (gon && !gon[(Q / nq) * G * G + blockIdx.y]) {  // every D of this group pair is zero in the element of Q (k_skip_groups)
    const size_t o = ((Q * G + ga) * G + gb) * nth, stride = NQ * G * G * nth;
    for (int i = threadIdx.x; i < nth; i += blockDim.x) {
      V[o + i] = 0.0;
      if (do_grad) V[stride + o + i] = V[2 * stride + o + i] = 0.0;
      if (do_tau) V[3 * stride + o + i] = V[4 * stride + o + i] = 0.0;
      if (do_lapl) V[5 * stride + o + i] = 0.0;
    }
    return;
  }
  int a0 = grp_off[ga], na = grp_off[ga + 1] - a0;
  int b0 = grp_off[gb], nb = grp_off[gb + 1] - b0;
  double *d0 = sh, *d1 = sh + na * nb, *d2 = sh + 2 * na * nb, *d3 = sh + 3 * na * nb;
  size_t AA = (size_t)A * A;
  const double ir2 = do_lapl ? 1.0 / (rad_sh[Q] * rad_sh[Q]) : 0.0;
  for (int t = threadIdx.x; t < na * nb; t += blockDim.x) {
    int ia = t / nb, ib = t % nb;
    int a = grp_shell[a0 + ia], b = grp_shell[b0 + ib];
    d0[t] = D0[Q * AA + (size_t)a * A + b];
    d1[t] = do_grad ? D1[Q * AA + (size_t)a * A + b] : 0.0;
    d2[t] = do_tau ? D2[Q * AA + (size_t)a * A + b] : 0.0;
    if (do_lapl) d3[t] = D3[Q * AA + (size_t)a * A + b] - (double)(shell_l[b] * (shell_l[b] + 1)) * ir2 * d0[t];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nth; i += blockDim.x) {
    double r = 0.0, s = 0.0, u = 0.0, k3 = 0.0, k4 = 0.0, k5 = 0.0;
    for (int ia = 0; ia < na; ia++) {
      int a = grp_shell[a0 + ia];
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s5 = 0.0;
      for (int ib = 0; ib < nb; ib++) {
        double tb = Th[(size_t)grp_shell[b0 + ib] * nth + i];
        s0 += d0[ia * nb + ib] * tb;
        s1 += d1[ia * nb + ib] * tb;
        if (do_tau) {
          s2 += d2[ia * nb + ib] * tb;
          s3 += d0[ia * nb + ib] * dTh[(size_t)grp_shell[b0 + ib] * nth + i];
        }
        if (do_lapl) s5 += d3[ia * nb + ib] * tb;
      }
      double ta = Th[(size_t)a * nth + i];
      r += ta * s0;
      if (do_grad) {
        s += dTh[(size_t)a * nth + i] * s0;
        u += ta * s1;
      }
      if (do_tau) {
        k3 += ta * s2;
        k4 += dTh[(size_t)a * nth + i] * s3;
      }
      if (do_lapl) k5 += ta * s5;
    }
    size_t o = ((Q * G + ga) * G + gb) * nth + i;
    size_t stride = NQ * G * G * nth;
    V[o] = r;
    if (do_grad) {
      V[stride + o] = s;
      V[2 * stride + o] = u;
    }
    if (do_tau) {
      V[3 * stride + o] = k3;
      V[4 * stride + o] = k4;
    }
    if (do_lapl) V[5 * stride + o] = k5;
  }
}

// Pieces that the two grid kernels below share, each in the operation order the kernels had them in.
// Scale factors of the radial-like, polar-like and azimuthal coordinates: prolate spheroidal (diatomic dftgrid.cpp:693-707),
// spherical (atomic dftgrid.cpp:724-743; shm holds r)
__device__ __forceinline__ void xc_scale_factors(int geom, double Rh, double shm, double sth, double &hmu, double &hnu, double &hphi) {
  if (geom == 0) {
    hmu = hnu = Rh * sqrt(shm * shm + sth * sth);
    hphi = Rh * shm * sth;
  } else {
    hmu = 1.0;
    hnu = shm;
    hphi = shm * sth;
  }
}
// ... and the volume weight w of theta point i (th_w) at a radial point of weight wr, dphi per point of the phi grid
__device__ __forceinline__ void xc_scale_factors_weight(int geom, double Rh, double shm, double sth, const double *__restrict__ th_w, int i,
                                                        double dphi, double wr, double &hmu, double &hnu, double &hphi, double &w) {
  if (geom == 0) {
    double h2 = shm * shm + sth * sth;
    hmu = hnu = Rh * sqrt(h2);
    hphi = Rh * shm * sth;
    w = th_w[i] * dphi * wr * Rh * Rh * Rh * shm * h2;
  } else {
    hmu = 1.0;
    hnu = shm;
    hphi = shm * sth;
    w = th_w[i] * dphi * wr * shm * shm;
  }
}
// Block reduction of the three scalars of a radial point into partial[3][NQ]; red: 3 * nwave doubles of LDS.  Fixed order
// (shuffle down 32 ... 1, then the wave sums in wave order) -> deterministic
__device__ __forceinline__ void xc_reduce_partials(double nel, double exc_sum, double kin_sum, double *red, size_t Q, size_t NQ,
                                                   double *__restrict__ partial) {
  int nwave = blockDim.x / 64, wave = threadIdx.x / 64, lane = threadIdx.x & 63;
  for (int o = 32; o > 0; o >>= 1) {
    nel += __shfl_down(nel, o, 64);
    exc_sum += __shfl_down(exc_sum, o, 64);
    kin_sum += __shfl_down(kin_sum, o, 64);
  }
  if (lane == 0) {
    red[wave] = nel;
    red[nwave + wave] = exc_sum;
    red[2 * nwave + wave] = kin_sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0, c2 = 0.0;
    for (int w = 0; w < nwave; w++) {
      a += red[w];
      b += red[nwave + w];
      c2 += red[2 * nwave + w];
    }
    partial[Q] = a;
    partial[NQ + Q] = b;
    partial[2 * NQ + Q] = c2;
  }
}
// Phi transform of one output (ga, gb, theta row i) of one spin: pot holds that spin's potential planes in LDS with stride
// ng, il is the row's place in them, Fs the spin's planes of Fo
__device__ __forceinline__ void xc_phi_transform(const double *pot, int ng, int il, int i, int ga, int gb, size_t Q, int G, int nth, int nphi,
                                                 const int *__restrict__ grp_m, const double *__restrict__ cosd,
                                                 const double *__restrict__ sind, int Dmax, const double *__restrict__ th_s, int geom,
                                                 double Rh, double shm, int do_grad, int do_tau, int do_lapl, size_t stride,
                                                 double *__restrict__ Fs) {
  int D = grp_m[ga] - grp_m[gb];
  const double *cd = cosd + (size_t)(D + Dmax) * nphi;
  const double *sd = sind + (size_t)(D + Dmax) * nphi;
  const double *p0 = pot, *p1 = p0 + ng, *p2 = p0 + 2 * ng, *p3 = p0 + 3 * ng, *p4 = p0 + 4 * ng, *p5 = p0 + 5 * ng;
  double fa = 0.0, fs = 0.0, fb = 0.0, ft = 0.0, fl = 0.0;
  double mga = grp_m[ga];
  for (int j = 0; j < nphi; j++) {
    int pt = il * nphi + j;
    fa += 0.5 * p0[pt] * cd[j];
    if (do_grad) {
      fa -= mga * p3[pt] * sd[j];
      fs += p2[pt] * cd[j];
      fb += p1[pt] * cd[j];
    }
    if (do_tau) ft += p4[pt] * cd[j];
    if (do_lapl) fl += p5[pt] * cd[j];
  }
  size_t o = ((Q * G + ga) * G + gb) * nth + i;
  if (do_lapl) Fs[5 * stride + o] = fl;
  if (do_tau) {
    // the three tau terms of eval_Fxc (dftgrid.cpp:533-540) share the phi sum; the scale factors depend on
    // theta only.  Halves as for the LDA term: the radial stage adds the (x,y) and (y,x) blocks.
    double hmu, hnu, hphi;
    xc_scale_factors(geom, Rh, shm, th_s[i], hmu, hnu, hphi);
    fa += 0.5 * mga * (double)grp_m[gb] * ft / (hphi * hphi);
    Fs[3 * stride + o] = 0.5 * ft / (hmu * hmu);
    Fs[4 * stride + o] = 0.5 * ft / (hnu * hnu);
  }
  Fs[o] = fa;
  if (do_grad) {
    Fs[stride + o] = fs;
    Fs[2 * stride + o] = fb;
  }
}

// X3 grid evaluation at one radial point: density & gradient on the (theta,phi) grid, functional,
//    energy/electron partial sums, and the phi-transformed potentials
//       Fo[0][Q][ga][gb][i] = sum_j (1/2 w vrho cos(D phi_j) - m_ga gr_phi sin(D phi_j))
//       Fo[1][..]           = sum_j gr_nu cos(D phi_j)
//       Fo[2][..]           = sum_j gr_mu cos(D phi_j)            D = m_ga - m_gb
//    (dftgrid.cpp:69-86, 412-416, 471-477, 510-531, 693-707)
//    Laplacian (do_lapl, atomic dftgrid.cpp:105-120, 557-571): lapl = 2 (kin + lap) with kin = 2 tau and lap = sum_j V5 cos,
//    the tau-type potential becomes w (vtau/2 + 2 vlapl), and Fo[5][..] = sum_j w vlapl cos(D phi_j) feeds the
//    increment_mgga_lapl term
//    EXT: the instantiation that also runs the xc::is_ext functionals (SCAN, SCAN0, PBEsol, revPBE); the host launches it
//    only when one of the two ids is one of them, so the instantiation for every other functional keeps its code
template <bool EXT>
__global__ void k_xc_grid(const double *__restrict__ V, const double *__restrict__ rad_w,
                          const double *__restrict__ rad_sh, const double *__restrict__ th_s,
                          const double *__restrict__ th_w, const int *__restrict__ grp_m,
                          const double *__restrict__ cosd, const double *__restrict__ sind, int Dmax, int G, int nth,
                          int nphi, double Rh, int geom, int x_func, int c_func, int do_grad, int do_tau, int do_lapl,
                          double thr, size_t NQ, int rank, int nranks, double *__restrict__ Fo,
                          double *__restrict__ partial /* [3][NQ] */) {
  extern __shared__ double sh[];  // pot[5 (6 with do_lapl)][nth*nphi], red[3*nwave]
  size_t Q = blockIdx.x;
  if ((int)(Q % nranks) != rank) {
    if (threadIdx.x == 0) {
      partial[Q] = 0.0;
      partial[NQ + Q] = 0.0;
      partial[2 * NQ + Q] = 0.0;
    }
    return;
  }
  int ng = nth * nphi;
  double *p0 = sh, *p1 = sh + ng, *p2 = sh + 2 * ng, *p3 = sh + 3 * ng, *p4 = sh + 4 * ng, *p5 = sh + 5 * ng;
  double *red = sh + (do_lapl ? 6 : 5) * ng;
  double shm = rad_sh[Q], wr = rad_w[Q];
  double dphi = 2.0 * HFG_PI / nphi;
  size_t stride = NQ * G * G * nth;
  double nel = 0.0, exc_sum = 0.0, kin_sum = 0.0;
  for (int pt = threadIdx.x; pt < ng; pt += blockDim.x) {
    int i = pt / nphi, j = pt % nphi;
    double hmu, hnu, hphi, w;
    xc_scale_factors_weight(geom, Rh, shm, th_s[i], th_w, i, dphi, wr, hmu, hnu, hphi, w);
    double rho = 0.0, gmu = 0.0, gnu = 0.0, gphi = 0.0, tau = 0.0, lap = 0.0;
    for (int ga = 0; ga < G; ga++)
      for (int gb = 0; gb < G; gb++) {
        int D = grp_m[ga] - grp_m[gb];
        double cd = cosd[(size_t)(D + Dmax) * nphi + j];
        size_t o = ((Q * G + ga) * G + gb) * nth + i;
        double vr = V[o];
        rho += cd * vr;
        if (do_lapl) lap += cd * V[5 * stride + o];
        if (do_tau)  // tau = 1/2 sum_c Re[(P conj d_c bf) . d_c bf] / h_c^2   (dftgrid.cpp:90-112)
          tau += 0.5 * cd * (V[3 * stride + o] / (hmu * hmu) + V[4 * stride + o] / (hnu * hnu) +
                             (double)(grp_m[ga] * grp_m[gb]) * vr / (hphi * hphi));
        if (do_grad) {
          double sd = sind[(size_t)(D + Dmax) * nphi + j];
          gnu += cd * V[stride + o];
          gmu += cd * V[2 * stride + o];
          gphi -= grp_m[ga] * sd * vr;
        }
      }
    double sigma = 0.0;
    if (do_grad) {
      gmu *= 2.0 / hmu;
      gnu *= 2.0 / hnu;
      gphi *= 2.0 / hphi;
      sigma = gmu * gmu + gnu * gnu + gphi * gphi;
    }
    double exc = 0.0, vrho = 0.0, vsig = 0.0, vtau = 0.0, vlap = 0.0;
    if (rho >= thr && rho > 0.0) {
      const bool live = 0.5 * rho >= thr;  // the spin channels of the exchange sum carry rho/2 each
      const double lapl = 2.0 * (2.0 * tau + lap);
      if (x_func > 0) HFG_XC_EVAL_POINT(EXT, x_func, rho, sigma, tau, lapl, live, exc, vrho, vsig, vtau, vlap);
      if (c_func > 0) HFG_XC_EVAL_POINT(EXT, c_func, rho, sigma, tau, lapl, live, exc, vrho, vsig, vtau, vlap);
      if (!isfinite(vlap)) vlap = 0.0;  // check_xc, dftgrid.cpp:336-339
    }
    nel += w * rho;
    exc_sum += w * exc * rho;
    kin_sum += w * tau;
    if (do_tau) p4[pt] = do_lapl ? w * (0.5 * vtau + 2.0 * vlap) : 0.5 * w * vtau;  // vt / vtl of dftgrid.cpp:534-535, 557-562
    if (do_lapl) p5[pt] = w * vlap;
    p0[pt] = w * vrho;
    if (do_grad) {
      double f = 2.0 * w * vsig;
      p1[pt] = f * gmu / hmu;
      p2[pt] = f * gnu / hnu;
      p3[pt] = f * gphi / hphi;
    }
  }
  xc_reduce_partials(nel, exc_sum, kin_sum, red, Q, NQ, partial);
  // phi transforms
  int nout = G * G * nth;
  for (int t = threadIdx.x; t < nout; t += blockDim.x) {
    int i = t % nth;
    int gab = t / nth;
    int ga = gab / G, gb = gab % G;
    xc_phi_transform(sh, ng, i, i, ga, gb, Q, G, nth, nphi, grp_m, cosd, sind, Dmax, th_s, geom, Rh, shm, do_grad, do_tau, do_lapl,
                     stride, Fo);
  }
}

// X3 for a spin-polarised density (DFTGridWorker::update_density(Pa,Pb), compute_xc, eval_Fxc(Ha,Hb,beta);
//    dftgrid.cpp:119-170, 343-458, 547-613): V and Fo hold the alpha planes (0..2) followed by the beta planes (3..5).
//    EXT as in k_xc_grid.
template <bool EXT>
__global__ void k_xc_grid_pol(const double *__restrict__ V, const double *__restrict__ rad_w,
                              const double *__restrict__ rad_sh, const double *__restrict__ th_s,
                              const double *__restrict__ th_w, const int *__restrict__ grp_m,
                              const double *__restrict__ cosd, const double *__restrict__ sind, int Dmax, int G, int nth,
                              int nphi, double Rh, int geom, int x_func, int c_func, int do_grad, int do_tau, int do_lapl,
                              double thr, size_t NQ, int rank, int nranks, double *__restrict__ Fo,
                              double *__restrict__ partial /* [3][NQ] */, int rowc) {
  // meta-GGA (do_tau): V and Fo carry five planes per spin (the tau planes 3, 4 as in k_xc_grid), LDS one more potential
  // plane per spin.  The theta rows go through LDS rowc at a time (the phi transform is row by row): rowc = nth unless the
  // planes of the whole grid exceed a CU's LDS (lmax beyond ~26 with mmax = 2).
  // Laplacian (do_lapl): a sixth plane per spin in V and Fo and in LDS (the vlapl potential), as in k_xc_grid.
  extern __shared__ double sh[];  // pot[2*npot][rowc*nphi] (npot = 4, 5 with tau, 6 with lapl), red[3*nwave]
  size_t Q = blockIdx.x;
  if ((int)(Q % nranks) != rank) {
    if (threadIdx.x == 0) {
      partial[Q] = 0.0;
      partial[NQ + Q] = 0.0;
      partial[2 * NQ + Q] = 0.0;
    }
    return;
  }
  const int ng = rowc * nphi;        // plane stride in LDS
  const int npl = do_lapl ? 6 : (do_tau ? 5 : 3);   // planes per spin in V and Fo
  const int npot = do_lapl ? 6 : (do_tau ? 5 : 4);  // potential planes per spin in LDS
  double *red = sh + 2 * npot * ng;
  double shm = rad_sh[Q], wr = rad_w[Q];
  double dphi = 2.0 * HFG_PI / nphi;
  size_t stride = NQ * G * G * nth;
  double nel = 0.0, exc_sum = 0.0, kin_sum = 0.0;
  for (int i0 = 0; i0 < nth; i0 += rowc) {
  const int rows = min(rowc, nth - i0);
  if (i0) __syncthreads();  // the previous chunk's planes have been transformed
  for (int pt = threadIdx.x; pt < rows * nphi; pt += blockDim.x) {
    int i = i0 + pt / nphi, j = pt % nphi;
    double hmu, hnu, hphi, w;
    xc_scale_factors_weight(geom, Rh, shm, th_s[i], th_w, i, dphi, wr, hmu, hnu, hphi, w);
    double rho[2] = {0.0, 0.0}, gmu[2] = {0.0, 0.0}, gnu[2] = {0.0, 0.0}, gphi[2] = {0.0, 0.0}, tau[2] = {0.0, 0.0};
    double lap[2] = {0.0, 0.0};
    for (int ga = 0; ga < G; ga++)
      for (int gb = 0; gb < G; gb++) {
        int D = grp_m[ga] - grp_m[gb];
        double cd = cosd[(size_t)(D + Dmax) * nphi + j];
        double sd = sind[(size_t)(D + Dmax) * nphi + j];
        size_t o = ((Q * G + ga) * G + gb) * nth + i;
        for (int sp = 0; sp < 2; sp++) {
          const double *Vs = V + (size_t)sp * npl * stride;
          double vr = Vs[o];
          rho[sp] += cd * vr;
          if (do_lapl) lap[sp] += cd * Vs[5 * stride + o];
          if (do_tau)  // dftgrid.cpp:159-200: tau of each spin density
            tau[sp] += 0.5 * cd * (Vs[3 * stride + o] / (hmu * hmu) + Vs[4 * stride + o] / (hnu * hnu) +
                                   (double)(grp_m[ga] * grp_m[gb]) * vr / (hphi * hphi));
          if (do_grad) {
            gnu[sp] += cd * Vs[stride + o];
            gmu[sp] += cd * Vs[2 * stride + o];
            gphi[sp] -= grp_m[ga] * sd * vr;
          }
        }
      }
    double saa = 0.0, sab = 0.0, sbb = 0.0;
    if (do_grad) {
      for (int sp = 0; sp < 2; sp++) {
        gmu[sp] *= 2.0 / hmu;
        gnu[sp] *= 2.0 / hnu;
        gphi[sp] *= 2.0 / hphi;
      }
      saa = gmu[0] * gmu[0] + gnu[0] * gnu[0] + gphi[0] * gphi[0];
      sab = gmu[0] * gmu[1] + gnu[0] * gnu[1] + gphi[0] * gphi[1];
      sbb = gmu[1] * gmu[1] + gnu[1] * gnu[1] + gphi[1] * gphi[1];
    }
    double exc = 0.0, va = 0.0, vb = 0.0, vsaa = 0.0, vsab = 0.0, vsbb = 0.0, vta = 0.0, vtb = 0.0, vla = 0.0, vlb = 0.0;
    const double rt = rho[0] + rho[1];
    if (rt >= thr && rt > 0.0) {
      double ra = fmax(rho[0], thr), rb = fmax(rho[1], thr);
      // dftgrid.cpp:206-229: lapl_s = 2 (kin_s + lap_s), kin_s = 2 tau_s
      const double la = 2.0 * (2.0 * tau[0] + lap[0]), lb = 2.0 * (2.0 * tau[1] + lap[1]);
      for (int f = 0; f < 2; f++) {
        const int id = f ? c_func : x_func;
        if (id <= 0) continue;
        HFG_XC_EVAL_POINT_POL(EXT, id, ra, rb, saa, sab, sbb, tau[0], tau[1], la, lb, rho[0] >= thr, rho[1] >= thr, exc, va, vb, vsaa, vsab,
                                vsbb, vta, vtb, vla, vlb);
      }
      if (!isfinite(vla)) vla = 0.0;  // check_xc, dftgrid.cpp:336-339
      if (!isfinite(vlb)) vlb = 0.0;
    }
    nel += w * rt;
    exc_sum += w * exc * rt;
    kin_sum += w * (tau[0] + tau[1]);
    sh[0 * ng + pt] = w * va;
    sh[npot * ng + pt] = w * vb;
    if (do_lapl) {  // vtl_a, vtl_b of dftgrid.cpp:643-660
      sh[4 * ng + pt] = w * (0.5 * vta + 2.0 * vla);
      sh[(npot + 4) * ng + pt] = w * (0.5 * vtb + 2.0 * vlb);
      sh[5 * ng + pt] = w * vla;
      sh[(npot + 5) * ng + pt] = w * vlb;
    } else if (do_tau) {
      sh[4 * ng + pt] = 0.5 * w * vta;
      sh[(npot + 4) * ng + pt] = 0.5 * w * vtb;
    }
    if (do_grad) {
      // gr_a = w (2 vs_aa grad rho_a + vs_ab grad rho_b) / h ; gr_b likewise   (dftgrid.cpp:583-601)
      sh[1 * ng + pt] = w * (2.0 * vsaa * gmu[0] + vsab * gmu[1]) / hmu;
      sh[2 * ng + pt] = w * (2.0 * vsaa * gnu[0] + vsab * gnu[1]) / hnu;
      sh[3 * ng + pt] = w * (2.0 * vsaa * gphi[0] + vsab * gphi[1]) / hphi;
      sh[(npot + 1) * ng + pt] = w * (2.0 * vsbb * gmu[1] + vsab * gmu[0]) / hmu;
      sh[(npot + 2) * ng + pt] = w * (2.0 * vsbb * gnu[1] + vsab * gnu[0]) / hnu;
      sh[(npot + 3) * ng + pt] = w * (2.0 * vsbb * gphi[1] + vsab * gphi[0]) / hphi;
    }
  }
  __syncthreads();
  int nout = G * G * rows;
  for (int t = threadIdx.x; t < 2 * nout; t += blockDim.x) {
    int sp = t / nout, tt = t % nout;
    const int il = tt % rows;
    int i = i0 + il;
    int gab = tt / rows;
    int ga = gab / G, gb = gab % G;
    xc_phi_transform(sh + (size_t)(npot * sp) * ng, ng, il, i, ga, gb, Q, G, nth, nphi, grp_m, cosd, sind, Dmax, th_s, geom, Rh, shm, do_grad,
                     do_tau, do_lapl, stride, Fo + (size_t)sp * npl * stride);
  }
  }  // theta chunks
  xc_reduce_partials(nel, exc_sum, kin_sum, red, Q, NQ, partial);
}

// X4 of a group pair none of whose shell pairs the caller reads (hfg_ctx_set_fock_blocks): zeros, never stale data
__device__ __forceinline__ void xc_fock_theta_zero(size_t Q, int A, int a0, int na, int b0, int nb,
                                                   const int *__restrict__ grp_shell, int do_grad, int do_tau, int do_lapl,
                                                   double *__restrict__ GA, double *__restrict__ GB, double *__restrict__ GC,
                                                   double *__restrict__ GL) {
  const size_t AA = (size_t)A * A;
  for (int t = threadIdx.x; t < na * nb; t += blockDim.x) {
    const int a = grp_shell[a0 + t / nb], b = grp_shell[b0 + t % nb];
    GA[Q * AA + (size_t)a * A + b] = 0.0;
    if (do_grad) GB[Q * AA + (size_t)a * A + b] = 0.0;
    if (do_tau) GC[Q * AA + (size_t)a * A + b] = 0.0;
    if (do_lapl) GL[Q * AA + (size_t)a * A + b] = 0.0;
  }
}

// X4 theta expansion: GA[Q][a][b] = sum_i Theta_a Theta_b Fo0 + dTheta_a Theta_b Fo1 ; GB[Q][a][b] = sum_i Theta_a Theta_b Fo2
//    meta-GGA: GA += sum_i dTheta_a dTheta_b Fo4 ; GC[Q][a][b] = sum_i Theta_a Theta_b Fo3
//    Laplacian: GL[Q][a][b] = sum_i Theta_a Theta_b Fo5
__global__ void k_xc_fock_theta(const double *__restrict__ Fo, const double *__restrict__ Th,
                                const double *__restrict__ dTh, int A, int nth, int G,
                                const int *__restrict__ grp_off, const int *__restrict__ grp_shell, int do_grad,
                                int do_tau, int do_lapl, size_t NQ, int rank, int nranks, double *__restrict__ GA,
                                double *__restrict__ GB, double *__restrict__ GC, double *__restrict__ GL,
                                const int *__restrict__ gneed) {
  // LDS: f0..f4[nth] (f5 with do_lapl), then the Theta / dTheta rows of the two shell groups, [i][shell] (the pair loop reads them with
  // consecutive b across threads; from global memory the loop was latency-bound: 0.26 ms per build at Nbf = 4230)
  extern __shared__ double sh[];
  size_t Q = blockIdx.x;
  if ((int)(Q % nranks) != rank) return;
  int ga = blockIdx.y / G, gb = blockIdx.y % G;
  int a0 = grp_off[ga], na = grp_off[ga + 1] - a0;
  int b0 = grp_off[gb], nb = grp_off[gb + 1] - b0;
  if (gneed && !gneed[blockIdx.y]) {
    xc_fock_theta_zero(Q, A, a0, na, b0, nb, grp_shell, do_grad, do_tau, do_lapl, GA, GB, GC, GL);
    return;
  }
  size_t stride = NQ * G * G * nth;
  size_t o = ((Q * G + ga) * G + gb) * nth;
  double *f0 = sh, *f1 = sh + nth, *f2 = sh + 2 * nth, *f3 = sh + 3 * nth, *f4 = sh + 4 * nth, *f5 = sh + 5 * nth;
  double *sTa = sh + (do_lapl ? 6 : 5) * nth, *sDa = sTa + (size_t)nth * na, *sTb = sDa + (size_t)nth * na, *sDb = sTb + (size_t)nth * nb;
  for (int i = threadIdx.x; i < nth; i += blockDim.x) {
    f0[i] = Fo[o + i];
    f1[i] = do_grad ? Fo[stride + o + i] : 0.0;
    f2[i] = do_grad ? Fo[2 * stride + o + i] : 0.0;
    f3[i] = do_tau ? Fo[3 * stride + o + i] : 0.0;
    f4[i] = do_tau ? Fo[4 * stride + o + i] : 0.0;
    if (do_lapl) f5[i] = Fo[5 * stride + o + i];
  }
  for (int t = threadIdx.x; t < nth * na; t += blockDim.x) {
    int ia = t / nth, i = t % nth;  // consecutive threads read consecutive theta points of one shell
    int a = grp_shell[a0 + ia];
    sTa[i * na + ia] = Th[(size_t)a * nth + i];
    sDa[i * na + ia] = dTh[(size_t)a * nth + i];
  }
  for (int t = threadIdx.x; t < nth * nb; t += blockDim.x) {
    int ib = t / nth, i = t % nth;
    int b = grp_shell[b0 + ib];
    sTb[i * nb + ib] = Th[(size_t)b * nth + i];
    sDb[i * nb + ib] = dTh[(size_t)b * nth + i];
  }
  __syncthreads();
  size_t AA = (size_t)A * A;
  for (int t = threadIdx.x; t < na * nb; t += blockDim.x) {
    const int ia = t / nb, ib = t % nb;
    int a = grp_shell[a0 + ia], b = grp_shell[b0 + ib];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int i = 0; i < nth; i++) {
      const double tai = sTa[i * na + ia], dai = sDa[i * na + ia], tbi = sTb[i * nb + ib];
      s0 += (tai * f0[i] + dai * f1[i]) * tbi;
      s1 += tai * f2[i] * tbi;
      if (do_tau) {
        s0 += dai * sDb[i * nb + ib] * f4[i];
        s2 += tai * tbi * f3[i];
      }
      if (do_lapl) s3 += tai * tbi * f5[i];
    }
    GA[Q * AA + (size_t)a * A + b] = s0;
    if (do_grad) GB[Q * AA + (size_t)a * A + b] = s1;
    if (do_tau) GC[Q * AA + (size_t)a * A + b] = s2;
    if (do_lapl) GL[Q * AA + (size_t)a * A + b] = s3;
  }
}

// X4 for shell groups whose Theta tables do not fit a CU's LDS (lmax beyond ~33 with mmax = 2): the theta points go
// through LDS nthc at a time and every thread keeps the sums of its (a, b) pairs in registers across the chunks
// (at most XC_FT_MAXPP pairs per thread: groups of up to 64 shells)
// (LAPL: the Laplacian plane Fo5 -> GL as in k_xc_fock_theta; a template parameter, so that the instance without it keeps
// its register budget)
using helfem::XC_FT_MAXPP;
template <bool LAPL>
__global__ __launch_bounds__(256) void k_xc_fock_theta_chunked(const double *__restrict__ Fo, const double *__restrict__ Th,
                                                               const double *__restrict__ dTh, int A, int nth, int G,
                                                               const int *__restrict__ grp_off, const int *__restrict__ grp_shell,
                                                               int do_grad, int do_tau, size_t NQ, int rank, int nranks,
                                                               double *__restrict__ GA, double *__restrict__ GB,
                                                               double *__restrict__ GC, double *__restrict__ GL, int nthc,
                                                               const int *__restrict__ gneed) {
  extern __shared__ double sh[];
  size_t Q = blockIdx.x;
  if ((int)(Q % nranks) != rank) return;
  int ga = blockIdx.y / G, gb = blockIdx.y % G;
  int a0 = grp_off[ga], na = grp_off[ga + 1] - a0;
  int b0 = grp_off[gb], nb = grp_off[gb + 1] - b0;
  if (gneed && !gneed[blockIdx.y]) {
    xc_fock_theta_zero(Q, A, a0, na, b0, nb, grp_shell, do_grad, do_tau, LAPL, GA, GB, GC, GL);
    return;
  }
  size_t stride = NQ * G * G * nth;
  size_t o = ((Q * G + ga) * G + gb) * nth;
  double *f0 = sh, *f1 = sh + nthc, *f2 = sh + 2 * nthc, *f3 = sh + 3 * nthc, *f4 = sh + 4 * nthc, *f5 = sh + 5 * nthc;
  double *sTa = sh + (LAPL ? 6 : 5) * nthc, *sDa = sTa + (size_t)nthc * na, *sTb = sDa + (size_t)nthc * na, *sDb = sTb + (size_t)nthc * nb;
  double s0[XC_FT_MAXPP], s1[XC_FT_MAXPP], s2[XC_FT_MAXPP], s3[LAPL ? XC_FT_MAXPP : 1];
#pragma unroll
  for (int q = 0; q < XC_FT_MAXPP; q++) s0[q] = s1[q] = s2[q] = 0.0;
  if (LAPL)
#pragma unroll
    for (int q = 0; q < (LAPL ? XC_FT_MAXPP : 1); q++) s3[q] = 0.0;
  for (int c0 = 0; c0 < nth; c0 += nthc) {
    const int len = min(nthc, nth - c0);
    if (c0) __syncthreads();
    for (int i = threadIdx.x; i < len; i += blockDim.x) {
      f0[i] = Fo[o + c0 + i];
      f1[i] = do_grad ? Fo[stride + o + c0 + i] : 0.0;
      f2[i] = do_grad ? Fo[2 * stride + o + c0 + i] : 0.0;
      f3[i] = do_tau ? Fo[3 * stride + o + c0 + i] : 0.0;
      f4[i] = do_tau ? Fo[4 * stride + o + c0 + i] : 0.0;
      if (LAPL) f5[i] = Fo[5 * stride + o + c0 + i];
    }
    for (int t = threadIdx.x; t < len * na; t += blockDim.x) {
      int ia = t / len, i = t % len;
      int a = grp_shell[a0 + ia];
      sTa[i * na + ia] = Th[(size_t)a * nth + c0 + i];
      sDa[i * na + ia] = dTh[(size_t)a * nth + c0 + i];
    }
    for (int t = threadIdx.x; t < len * nb; t += blockDim.x) {
      int ib = t / len, i = t % len;
      int b = grp_shell[b0 + ib];
      sTb[i * nb + ib] = Th[(size_t)b * nth + c0 + i];
      sDb[i * nb + ib] = dTh[(size_t)b * nth + c0 + i];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < XC_FT_MAXPP; q++) {
      const int t = threadIdx.x + q * 256;
      if (t < na * nb) {
        const int ia = t / nb, ib = t % nb;
        double t0 = s0[q], t1 = s1[q], t2 = s2[q], t3 = LAPL ? s3[LAPL ? q : 0] : 0.0;
        for (int i = 0; i < len; i++) {
          const double tai = sTa[i * na + ia], dai = sDa[i * na + ia], tbi = sTb[i * nb + ib];
          t0 += (tai * f0[i] + dai * f1[i]) * tbi;
          t1 += tai * f2[i] * tbi;
          if (do_tau) {
            t0 += dai * sDb[i * nb + ib] * f4[i];
            t2 += tai * tbi * f3[i];
          }
          if (LAPL) t3 += tai * tbi * f5[i];
        }
        s0[q] = t0;
        s1[q] = t1;
        s2[q] = t2;
        if (LAPL) s3[LAPL ? q : 0] = t3;
      }
    }
  }
  size_t AA = (size_t)A * A;
#pragma unroll
  for (int q = 0; q < XC_FT_MAXPP; q++) {
    const int t = threadIdx.x + q * 256;
    if (t < na * nb) {
      const int ia = t / nb, ib = t % nb;
      int a = grp_shell[a0 + ia], b = grp_shell[b0 + ib];
      GA[Q * AA + (size_t)a * A + b] = s0[q];
      if (do_grad) GB[Q * AA + (size_t)a * A + b] = s1[q];
      if (do_tau) GC[Q * AA + (size_t)a * A + b] = s2[q];
      if (LAPL) GL[Q * AA + (size_t)a * A + b] = s3[LAPL ? q : 0];
    }
  }
}

// X5 radial expansion into the compact Fock blocks:
//    Hc[x][y][e][n'][n] = sum_q B_n B_n' (GA_xy + GA_yx) + B'_n B_n' GB_xy + B_n B'_n' GB_yx
//    meta-GGA: + B'_n B'_n' (GC_xy + GC_yx)
//    Laplacian (increment_mgga_lapl, dftgrid.h:257-281): + B_n L_n' GL_xy + L_n B_n' GL_yx, and the shell part of eval_lf,
//    -(l_y(l_y+1) GL_xy + l_x(l_x+1) GL_yx)/r^2, folded into the B_n B_n' weight
__global__ void k_xc_fock_radial(const double *__restrict__ GA, const double *__restrict__ GB,
                                 const double *__restrict__ GC, const double *__restrict__ GL, const double *__restrict__ B,
                                 const double *__restrict__ dB, const double *__restrict__ Lr, const int *__restrict__ shell_l,
                                 const double *__restrict__ rad_sh, int A, int E, int p, int nq, int do_grad, int do_tau,
                                 int do_lapl, int rank, int nranks, double *__restrict__ Hc, const int *__restrict__ need) {
  // gs[nq], g1[nq], g2[nq], g3[nq], B[nq][p], dB[nq][p] of this element, U[nq][p], W[nq][p]; do_lapl: L[nq][p], V[nq][p]
  extern __shared__ double sh[];
  int xy = blockIdx.x, e = blockIdx.y;
  if (need && !need[xy]) {  // a block the caller does not read: zeros (the compact buffer is summed over ranks and scattered)
    for (int t = threadIdx.x; t < p * p; t += blockDim.x) Hc[((size_t)xy * E + e) * p * p + t] = 0.0;
    return;
  }
  int x = xy / A, y = xy % A;
  int yx = y * A + x;
  size_t AA = (size_t)A * A;
  double *gs = sh, *g1 = sh + nq, *g2 = sh + 2 * nq, *g3 = sh + 3 * nq;
  double *sB = sh + 4 * nq, *sdB = sB + nq * p;
  for (int q = threadIdx.x; q < nq; q += blockDim.x) {
    size_t Q = (size_t)e * nq + q;
    bool own = ((int)(Q % nranks) == rank);
    gs[q] = own ? GA[Q * AA + xy] + GA[Q * AA + yx] : 0.0;
    g1[q] = (own && do_grad) ? GB[Q * AA + xy] : 0.0;
    g2[q] = (own && do_grad) ? GB[Q * AA + yx] : 0.0;
    g3[q] = (own && do_tau) ? GC[Q * AA + xy] + GC[Q * AA + yx] : 0.0;
  }
  double *sU = sdB + nq * p, *sW = sU + nq * p;
  double *sL = sW + nq * p, *sV = sL + nq * p;
  for (int t = threadIdx.x; t < nq * p; t += blockDim.x) {
    sB[t] = B[(size_t)e * nq * p + t];
    sdB[t] = dB[(size_t)e * nq * p + t];
    if (do_lapl) sL[t] = Lr[(size_t)e * nq * p + t];
  }
  __syncthreads();
  // U[q][m] = gs B_m + g2 B'_m,  W[q][m] = g1 B_m + g3 B'_m:  H[n][m] = sum_q B_n U[q][m] + B'_n W[q][m]  (four LDS reads
  // per point and output instead of eight: the loop is LDS-bound)
  int pp = p * p;
  if (do_lapl) {
    // U += GL_xy L_m with the shell terms in the B B weight, V[q][m] = GL_yx B_m:  H[n][m] += sum_q L_n V[q][m]
    const int lx = shell_l[x] * (shell_l[x] + 1), ly = shell_l[y] * (shell_l[y] + 1);
    for (int t = threadIdx.x; t < nq * p; t += blockDim.x) {
      const int q = t / p;
      const size_t Q = (size_t)e * nq + q;
      const bool own = ((int)(Q % nranks) == rank);
      const double gl1 = own ? GL[Q * AA + xy] : 0.0, gl2 = own ? GL[Q * AA + yx] : 0.0;
      const double ir2 = 1.0 / (rad_sh[Q] * rad_sh[Q]);
      sU[t] = (gs[q] - (ly * gl1 + lx * gl2) * ir2) * sB[t] + g2[q] * sdB[t] + gl1 * sL[t];
      sW[t] = g1[q] * sB[t] + g3[q] * sdB[t];
      sV[t] = gl2 * sB[t];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < pp; t += blockDim.x) {
      int n = t % p, m = t / p;
      double acc = 0.0;
      for (int q = 0; q < nq; q++) acc += sB[q * p + n] * sU[q * p + m] + sdB[q * p + n] * sW[q * p + m] + sL[q * p + n] * sV[q * p + m];
      Hc[((size_t)xy * E + e) * pp + t] = acc;
    }
    return;
  }
  for (int t = threadIdx.x; t < nq * p; t += blockDim.x) {
    const int q = t / p;
    sU[t] = gs[q] * sB[t] + g2[q] * sdB[t];
    sW[t] = g1[q] * sB[t] + g3[q] * sdB[t];
  }
  __syncthreads();
  for (int t = threadIdx.x; t < pp; t += blockDim.x) {
    int n = t % p, m = t / p;
    double acc = 0.0;
    for (int q = 0; q < nq; q++) acc += sB[q * p + n] * sU[q * p + m] + sdB[q * p + n] * sW[q * p + m];
    Hc[((size_t)xy * E + e) * pp + t] = acc;
  }
}

__global__ void k_xc_sum_partials(const double *__restrict__ partial, size_t NQ, double *__restrict__ scal) {
  // one wave: lane l adds the points l, l + 64, ... in order, then a fixed shuffle tree (deterministic)
  if (blockIdx.x != 0 || threadIdx.x >= 64) return;
  double nel = 0.0, exc = 0.0, kin = 0.0;
  for (size_t q = threadIdx.x; q < NQ; q += 64) {
    nel += partial[q];
    exc += partial[NQ + q];
    kin += partial[2 * NQ + q];
  }
  for (int o = 32; o > 0; o >>= 1) {
    nel += __shfl_down(nel, o, 64);
    exc += __shfl_down(exc, o, 64);
    kin += __shfl_down(kin, o, 64);
  }
  if (threadIdx.x == 0) {
    scal[0] = exc;  // Exc
    scal[1] = nel;  // Nel
    scal[2] = kin;  // Ekin = integral of tau (zero unless a meta-GGA asked for tau; dftgrid.cpp:227-240)
  }
}

// -------------------------------------------------------------------------------------------------
// Model-potential matrix of the initial guess (TwoDGrid::model_potential, src/diatomic/twodquadrature.cpp:213-232,
// 351-375): H_ij = int phi_i [V_1(r_1) + V_2(r_2)] phi_j on the same (mu, nu) product grid as the XC quadrature.  The
// integrand does not depend on phi, so the phi transform of k_xc_grid collapses to the m-diagonal planes
// Fo[0][Q][g][g][i] = 1/2 nphi w v; the theta and radial expansions X4, X5 are reused unchanged.
struct DevModelPot {
  int kind, Z;
  double d, H;
};
__device__ inline double mp_potential(const DevModelPot &p, double r) {
  double zeff;
  if (p.kind == 0) zeff = (double)p.Z;
  else if (p.kind == 1) {
    const double Hz = (p.H > 0.0) ? p.H : p.d * pow((double)(p.Z - 1), 0.4);
    zeff = 1.0 + (p.Z - 1) / (1.0 + (exp(r / p.d) - 1.0) * Hz);
  } else {
    const double alpha = 0.7280642371, beta = -0.5430794693, gamma = 0.3612163121;
    const double x = r * cbrt(128.0 * p.Z / (9.0 * HFG_PI * HFG_PI)), sx = sqrt(x);
    const double f = 1.0 + alpha * sx + beta * x * exp(-gamma * sx);
    zeff = p.Z * f * f * exp(-2.0 * alpha * sx);
  }
  const double v = -zeff / r;
  return (isfinite(v) && v != 0.0 && fabs(v) >= 2.2250738585072014e-308) ? v : 0.0;  // std::isnormal, as the reference
}
__global__ void k_mp_fill(const double *__restrict__ rad_w, const double *__restrict__ rad_sh,
                          const double *__restrict__ th_c, const double *__restrict__ th_s,
                          const double *__restrict__ th_w, int G, int nth, int nphi, double Rh, int geom, DevModelPot p1,
                          DevModelPot p2, double *__restrict__ Fo) {
  const size_t Q = blockIdx.x;
  const double shm = rad_sh[Q], wr = rad_w[Q];
  const double dphi = 2.0 * HFG_PI / nphi;
  for (int t = threadIdx.x; t < G * G * nth; t += blockDim.x) {
    const int i = t % nth, gab = t / nth, ga = gab / G, gb = gab % G;
    double f = 0.0;
    if (ga == gb) {
      const double sth = th_s[i], cth = th_c[i];
      double w, v;
      if (geom == 0) {
        const double chm = sqrt(1.0 + shm * shm);
        w = th_w[i] * dphi * wr * Rh * Rh * Rh * shm * (shm * shm + sth * sth);
        v = mp_potential(p1, Rh * (chm + cth)) + mp_potential(p2, Rh * (chm - cth));
      } else {
        w = th_w[i] * dphi * wr * shm * shm;
        v = mp_potential(p1, shm);
      }
      f = 0.5 * nphi * w * v;
    }
    Fo[((Q * G + ga) * G + gb) * nth + i] = f;
  }
}

// launchers
// -------------------------------------------------------------------------------------------------
// Workgroup sizes, bytes of LDS, chunking and what is refused: host/fock_plan.h.  A refusal of the plan is thrown here.
using helfem::fock_block_threads;
static void refuse(const char *why) {
  if (why) throw std::runtime_error(why);
}
static size_t accepted(const helfem::FockLds &lds) {
  refuse(lds.refused);
  return lds.bytes;
}

// Launch with `bytes` of dynamic LDS: beyond what a kernel may have as it is, its attribute is raised first (the XC radial
// kernels need that for elements of more than ~24 nodes with the default 5 quadrature points per node)
template <typename K, typename... Args>
static void launch_lds(K kernel, dim3 grid, dim3 block, size_t bytes, hipStream_t stream, Args... args) {
  if (helfem::fock_lds_raise(bytes))
    HFG_HIP_CHECK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  hipLaunchKernelGGL(kernel, grid, block, bytes, stream, args...);
}

struct FockAux : Workspace {
  DevBuf<int> pure_shell, pure_n, lmpos;
  DevBuf<double> Pc, Jc, Pc2, Jc2, Pc3, Paux, Y, Jaux, D0, D1, D2, D3, V, Fo, GA, GB, GC, GL, partial, scal;
  DevBuf<int> on, gon, chan;  // density flags of the last flagged gather (FockSkip)
};

// What one build may skip (DESIGN 3.1 "Skipped work"); a null pointer switches that kind of skipping off, and a build that
// did not fill the flags itself passes FockSkip() -- the polarised XC path, the model potential and the batched Coulomb.
//   density side, found on the device by the gather, valid for any P:
//     on[(x*A+y)*E+e]    the block of Pc holds a non-zero (or a NaN)         -> X1, K1
//     gon[(e*G+ga)*G+gb] some pair of the m-group pair is on in element e    -> X2
//     chan[iLM*E+e]      K1's channel received something (written by K1)     -> K2, K3
//   output side, told by the caller through hfg_ctx_set_fock_blocks, otherwise null = everything is needed:
//     need[x*A+y], gneed[ga*G+gb]                                            -> X5, K4 and X4
// A skipped entry is always written as 0.
struct FockSkip {
  const int *on = nullptr, *gon = nullptr;
  int *chan = nullptr;
  const int *need = nullptr, *gneed = nullptr;
};

static void aux_setup(hfg_ctx *ctx, const hfg_dev_tables *t, FockAux *a) {
  std::vector<int> ps(t->N), pn(t->N);
  {
    size_t k = 0;
    for (int s = 0; s < t->A; s++)
      for (int n = (t->h_shell_skip[s] ? 1 : 0); n < t->R; n++, k++) {
        ps[k] = s;
        pn[k] = n;
      }
  }
  a->pure_shell.upload(ps, ctx->stream);
  a->pure_n.upload(pn, ctx->stream);
  std::vector<int> lmpos(2 * t->Nlm, -1);
  for (int i = 0; i < t->NLM; i++) {
    int M = t->h_LM_M[i];
    int ilm = t->h_LM_ilm[i];
    if (M >= 0) lmpos[2 * ilm] = i;
    if (M < 0) lmpos[2 * ilm + 1] = i;
  }
  a->lmpos.upload(lmpos, ctx->stream);
  HFG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
}
static FockAux &aux_for(hfg_ctx *ctx, hfg_basis *basis) {
  hfg_dev_tables *t = basis->dev;
  return t->work.get<FockAux>(WS_FOCK, [&](FockAux &a) { aux_setup(ctx, t, &a); });
}

static hfg_dev_tables *tables_of(hfg_ctx *ctx, hfg_basis *basis) {
  if (!basis->dev || !basis->dev->have_tei) throw std::logic_error("Primitive teis have not been computed!\n");
  if (basis->dev_device != ctx->device) throw std::logic_error("basis tables live on a different device\n");
  return basis->dev;
}

static void gather_compact(hfg_ctx *ctx, hfg_basis *basis, const double *dP, double *dPc) {
  hfg_dev_tables *t = basis->dev;
  hipLaunchKernelGGL(k_gather_compact, dim3(t->A * t->A * t->E), dim3(256), 0, ctx->stream, dP, t->N, t->A, t->R, t->E,
                     t->p, t->shell_off.p, t->shell_skip.p, dPc, (int *)nullptr);
}

// The flags that follow from on[] (filled by the gather just enqueued on the context's stream): the m-group flags, the
// buffer of K1's channel flags, and the caller's output-side flags
static void skip_flags_behind_on(hfg_ctx *ctx, hfg_dev_tables *t, FockAux &a, bool with_need, FockSkip &sk) {
  sk.on = a.on.p;
  sk.chan = a.chan.p;
  if (t->have_xc) {
    a.gon.resize((size_t)t->E * t->G * t->G);
    hipLaunchKernelGGL(k_skip_groups, dim3(t->E, t->G * t->G), dim3(256), 0, ctx->stream, a.on.p, t->A, t->E, t->G, t->grp_off.p,
                       t->grp_shell.p, a.gon.p);
    sk.gon = a.gon.p;
  }
  if (with_need && ctx->fock_need_tables == t && ctx->fock_need_A == t->A) {
    sk.need = ctx->fock_need.p;
    if (t->have_xc && ctx->fock_need_G == t->G) sk.gneed = ctx->fock_gneed.p;
  }
}

// The gather of a build that skips (HELFEM_FOCK_SKIP, read at every call): it also writes the density flags, into the
// table set's workspace and on the context's stream, so whatever is ordered behind Pc is ordered behind the flags.  The
// output-side flags are the context's, if hfg_ctx_set_fock_blocks gave it some for these very tables and with_need asks.
static FockSkip gather_compact_flagged(hfg_ctx *ctx, hfg_basis *basis, const double *dP, double *dPc, bool with_need) {
  hfg_dev_tables *t = basis->dev;
  FockSkip sk;
  if (!helfem::tuning_live().fock_skip) {
    gather_compact(ctx, basis, dP, dPc);
    return sk;
  }
  FockAux &a = aux_for(ctx, basis);
  a.on.resize((size_t)t->A * t->A * t->E);
  a.chan.resize((size_t)t->NLM * t->E);
  hipLaunchKernelGGL(k_gather_compact, dim3(t->A * t->A * t->E), dim3(256), 0, ctx->stream, dP, t->N, t->A, t->R, t->E,
                     t->p, t->shell_off.p, t->shell_skip.p, dPc, a.on.p);
  skip_flags_behind_on(ctx, t, a, with_need, sk);
  return sk;
}

// gather_compact_flagged for an unrestricted build: Pa, Pb and Pa + Pb into Pc, Pc2 and Pc3, the flags of the union of the spins
static FockSkip gather_compact_pol_flagged(hfg_ctx *ctx, hfg_basis *basis, const double *dPa, const double *dPb, bool with_need) {
  hfg_dev_tables *t = basis->dev;
  FockAux &a = aux_for(ctx, basis);
  FockSkip sk;
  const bool skip = helfem::tuning_live().fock_skip;
  if (skip) {
    a.on.resize((size_t)t->A * t->A * t->E);
    a.chan.resize((size_t)t->NLM * t->E);
  }
  hipLaunchKernelGGL(k_gather_compact_pol, dim3(t->A * t->A * t->E), dim3(256), 0, ctx->stream, dPa, dPb, t->N, t->A, t->R, t->E,
                     t->p, t->shell_off.p, t->shell_skip.p, a.Pc.p, a.Pc2.p, a.Pc3.p, skip ? a.on.p : (int *)nullptr);
  if (skip) skip_flags_behind_on(ctx, t, a, with_need, sk);
  return sk;
}

static void scatter_dense(hfg_ctx *ctx, hfg_basis *basis, const double *dXc, double *dOut) {
  hfg_dev_tables *t = basis->dev;
  FockAux &a = aux_for(ctx, basis);
  dim3 grid((t->N + 63) / 64, (t->N + 3) / 4);
  hipLaunchKernelGGL(k_scatter_dense, grid, dim3(256), 0, ctx->stream, dXc, t->N, t->A, t->R, t->E, t->p,
                     a.pure_shell.p, a.pure_n.p, dOut);
}

// J (compact) from P (compact)
static void coulomb_compact(hfg_ctx *ctx, hfg_basis *basis, const double *dPc, double *dJc, const FockSkip &sk = FockSkip()) {
  hfg_dev_tables *t = tables_of(ctx, basis);
  FockAux &a = aux_for(ctx, basis);
  const int pp = t->p * t->p;
  const size_t nb = (size_t)t->NLM * t->E * pp;
  a.Paux.resize(2 * nb);
  a.Y.resize(4 * nb);
  a.Jaux.resize(2 * nb);
  const int bs = fock_block_threads(pp);
  const int *chan = sk.on ? sk.chan : nullptr;  // K1 publishes the channel flags only when it has the density flags
  hipLaunchKernelGGL(k_coulomb_ket, dim3(t->NLM, t->E), dim3(bs), 0, ctx->stream, dPc, t->A, t->E, pp, t->lm_off.p,
                     t->lm_x.p, t->lm_y.p, t->lm_c0.p, t->lm_c2.p, t->NLM, t->LM_ilm.p, ctx->shard_rank, ctx->shard_n, a.Paux.p, sk.on,
                     sk.on ? sk.chan : (int *)nullptr);
  hipLaunchKernelGGL(k_coulomb_tei, dim3(t->Nlm * t->E, t->ntt), dim3(bs), 2 * pp * sizeof(double), ctx->stream,
                     t->tei.p, a.Paux.p, t->Ntab, t->NLM, t->E, pp, a.lmpos.p, t->lm_tab.p, ctx->shard_rank, ctx->shard_n,
                     a.Y.p, chan);
  hipLaunchKernelGGL(k_coulomb_radial, dim3(t->NLM), dim3(bs), helfem::coulomb_radial_lds(t->E, bs), ctx->stream, a.Paux.p, a.Y.p, t->disj.p,
                     t->LM_ilm.p, t->LM_tab.p, t->LM_fac.p, t->Ntab, t->NLM, t->E, t->p, t->ntt == 4 ? 1 : 0,
                     ctx->shard_rank, ctx->shard_n, a.Jaux.p, chan);
  hipLaunchKernelGGL(k_coulomb_bra, dim3(t->A * t->A, t->E), dim3(bs), 0, ctx->stream, a.Jaux.p, t->A, t->E, pp,
                     t->NLM, t->pair_off.p, t->ent_iLM.p, t->ent_c0.p, t->ent_c2.p, t->LM_ilm.p, ctx->shard_rank, ctx->shard_n, dJc,
                     sk.need);
  HFG_HIP_CHECK(hipGetLastError());
}

void coulomb_dev(hfg_ctx *ctx, hfg_basis *basis, const double *dP, double *dJ) {
  hfg_dev_tables *t = tables_of(ctx, basis);
  FockAux &a = aux_for(ctx, basis);
  const size_t nc = (size_t)t->A * t->A * t->E * t->p * t->p;
  a.Pc.resize(nc);
  a.Jc.resize(nc);
  ProfScope ps(ctx, "coulomb");
  const FockSkip sk = gather_compact_flagged(ctx, basis, dP, a.Pc.p, false);  // the whole J is returned: density side only
  coulomb_compact(ctx, basis, a.Pc.p, a.Jc.p, sk);
  scatter_dense(ctx, basis, a.Jc.p, dJ);
  HFG_HIP_CHECK(hipGetLastError());
}

// ---- J for a batch of densities -------------------------------------------------------------------------------------
struct CoulombBatchAux : Workspace {
  DevBuf<double> Pc, Jc, Paux, Y, Jaux, part;  // grown to the largest pass seen
};
static CoulombBatchAux &batch_aux_for(hfg_basis *basis) { return basis->dev->work.get<CoulombBatchAux>(WS_COULOMB_BATCH); }

// Densities per pass over the in-element tables: the LDS rule of host/fock_plan.h under HELFEM_COULOMB_BATCH_CHUNK
static int coulomb_batch_chunk(const hfg_dev_tables *t) {
  const helfem::CoulombBatchChunk c = helfem::coulomb_batch_chunk(t->p, helfem::tuning_live().coulomb_batch_chunk);
  refuse(c.refused);
  return c.chunk;
}

template <int NC>
static void launch_tei_cols(hfg_ctx *ctx, const hfg_dev_tables *t, const FockAux &a, CoulombBatchAux &w, int nb, size_t nbk, int bs) {
  const int pp = t->p * t->p;
  hipLaunchKernelGGL(k_coulomb_tei_cols<NC>, dim3(t->Nlm * t->E, t->ntt), dim3(bs), (size_t)pp * NC * sizeof(double), ctx->stream,
                     t->tei.p, w.Paux.p, 2 * nbk, nb, t->Ntab, t->NLM, t->E, pp, a.lmpos.p, t->lm_tab.p, ctx->shard_rank,
                     ctx->shard_n, w.Y.p, 4 * nbk);
}
template <int NT>
static void launch_tei_mfma(hfg_ctx *ctx, const hfg_dev_tables *t, const FockAux &a, CoulombBatchAux &w, int nb, size_t nbk) {
  const int pp = t->p * t->p;
  launch_lds(k_coulomb_tei_mfma<NT>, dim3(t->Nlm * t->E, t->ntt), dim3(256), helfem::coulomb_batch_tile_bytes(t->p) * NT, ctx->stream,
             t->tei.p, w.Paux.p, 2 * nbk, nb, t->Ntab, t->NLM, t->E, pp, a.lmpos.p, t->lm_tab.p, ctx->shard_rank, ctx->shard_n, w.Y.p,
             4 * nbk);
}

// J (compact) from P (compact) for the nb <= coulomb_batch_chunk densities of one pass, both with the stride of one
// compact matrix.  One density goes through the kernels of the single build.
static void coulomb_batch_compact(hfg_ctx *ctx, hfg_basis *basis, int nb, const double *dPc, double *dJc) {
  if (nb == 1) return coulomb_compact(ctx, basis, dPc, dJc);
  hfg_dev_tables *t = tables_of(ctx, basis);
  FockAux &a = aux_for(ctx, basis);
  CoulombBatchAux &w = batch_aux_for(basis);
  const int pp = t->p * t->p;
  const size_t nc = (size_t)t->A * t->A * t->E * pp, nbk = (size_t)t->NLM * t->E * pp;
  w.Paux.resize(nb * 2 * nbk);
  w.Y.resize(nb * 4 * nbk);
  w.Jaux.resize(nb * 2 * nbk);
  const int bs = fock_block_threads(pp);
  const unsigned zg = (nb + CB_DB - 1) / CB_DB;
  hipLaunchKernelGGL(k_coulomb_ket_batch, dim3(t->NLM, t->E, zg), dim3(bs), 0, ctx->stream, dPc, nc, nb, t->A, t->E, pp, t->lm_off.p,
                     t->lm_x.p, t->lm_y.p, t->lm_c0.p, t->lm_c2.p, t->NLM, t->LM_ilm.p, ctx->shard_rank, ctx->shard_n, w.Paux.p,
                     2 * nbk);
  {
    ProfScope ps(ctx, "coulomb_batch_tei");  // the pass over the tables alone (tools/coulomb_batch_time.py)
    const helfem::CoulombBatchTei v = helfem::coulomb_batch_tei(nb);
    static_assert(helfem::CB_MAX_NT == 4, "one instantiation of k_coulomb_tei_mfma per tile count the rule can return");
    if (v.n == 0) throw std::logic_error("coulomb_batch_compact: pass larger than coulomb_batch_chunk\n");
    if (!v.mfma && v.n == 4) launch_tei_cols<4>(ctx, t, a, w, nb, nbk, bs);
    else if (!v.mfma && v.n == 8) launch_tei_cols<8>(ctx, t, a, w, nb, nbk, bs);
    else if (!v.mfma) launch_tei_cols<14>(ctx, t, a, w, nb, nbk, bs);
    else if (v.n == 1) launch_tei_mfma<1>(ctx, t, a, w, nb, nbk);
    else if (v.n == 2) launch_tei_mfma<2>(ctx, t, a, w, nb, nbk);
    else if (v.n == 3) launch_tei_mfma<3>(ctx, t, a, w, nb, nbk);
    else launch_tei_mfma<4>(ctx, t, a, w, nb, nbk);
  }
  hipLaunchKernelGGL(k_coulomb_radial_batch, dim3(t->NLM, nb), dim3(bs), helfem::coulomb_radial_lds(t->E, bs), ctx->stream, w.Paux.p, 2 * nbk, w.Y.p, 4 * nbk, t->disj.p,
                     t->LM_ilm.p, t->LM_tab.p, t->LM_fac.p, t->Ntab, t->NLM, t->E, t->p, t->ntt == 4 ? 1 : 0, ctx->shard_rank,
                     ctx->shard_n, w.Jaux.p, 2 * nbk);
  hipLaunchKernelGGL(k_coulomb_bra_batch, dim3(t->A * t->A, t->E, zg), dim3(bs), 0, ctx->stream, w.Jaux.p, 2 * nbk, nb, t->A, t->E, pp,
                     t->NLM, t->pair_off.p, t->ent_iLM.p, t->ent_c0.p, t->ent_c2.p, t->LM_ilm.p, ctx->shard_rank, ctx->shard_n, dJc, nc);
  HFG_HIP_CHECK(hipGetLastError());
}

void coulomb_batch_dev(hfg_ctx *ctx, hfg_basis *basis, int64_t nP, const double *dP, double *dJ) {
  if (nP <= 0) return;
  hfg_dev_tables *t = tables_of(ctx, basis);
  CoulombBatchAux &w = batch_aux_for(basis);
  const size_t nc = (size_t)t->A * t->A * t->E * t->p * t->p, N2 = (size_t)t->N * t->N;
  const int64_t chunk = coulomb_batch_chunk(t);
  ProfScope ps(ctx, "coulomb_batch");
  for (int64_t b0 = 0; b0 < nP; b0 += chunk) {
    const int nb = (int)std::min(chunk, nP - b0);
    w.Pc.resize(nb * nc);
    w.Jc.resize(nb * nc);
    for (int b = 0; b < nb; b++) gather_compact(ctx, basis, dP + (size_t)(b0 + b) * N2, w.Pc.p + b * nc);
    coulomb_batch_compact(ctx, basis, nb, w.Pc.p, w.Jc.p);
    for (int b = 0; b < nb; b++) scatter_dense(ctx, basis, w.Jc.p + b * nc, dJ + (size_t)(b0 + b) * N2);
  }
  HFG_HIP_CHECK(hipGetLastError());
}

// W(a, b) = tr(P_a J[P_b]), nP x nP column-major in HBM, from the compact P and J; not symmetrised
void coulomb_energy_matrix_dev(hfg_ctx *ctx, hfg_basis *basis, int64_t nP, const double *dP, double *dW) {
  if (nP <= 0) return;
  hfg_dev_tables *t = tables_of(ctx, basis);
  CoulombBatchAux &w = batch_aux_for(basis);
  const size_t nc = (size_t)t->A * t->A * t->E * t->p * t->p, N2 = (size_t)t->N * t->N;
  const int64_t chunk = coulomb_batch_chunk(t);
  const unsigned nslice = (unsigned)((nc + CB_SLICE - 1) / CB_SLICE);
  ProfScope ps(ctx, "coulomb_batch");
  w.Pc.resize(nP * nc);  // every P stays: each meets every J
  w.Jc.resize(std::min(chunk, nP) * nc);
  w.part.resize((size_t)nslice * nP * std::min(chunk, nP));
  for (int64_t b = 0; b < nP; b++) gather_compact(ctx, basis, dP + (size_t)b * N2, w.Pc.p + b * nc);
  for (int64_t b0 = 0; b0 < nP; b0 += chunk) {
    const int nb = (int)std::min(chunk, nP - b0);
    coulomb_batch_compact(ctx, basis, nb, w.Pc.p + b0 * nc, w.Jc.p);
    hipLaunchKernelGGL(k_coulomb_energy_part, dim3(nslice, (unsigned)((nP + CB_WT - 1) / CB_WT), (nb + CB_WT - 1) / CB_WT), dim3(256), 0,
                       ctx->stream, w.Pc.p, (int)nP, w.Jc.p, nb, nc, w.part.p);
    hipLaunchKernelGGL(k_coulomb_energy_sum, dim3((unsigned)((nP * nb + 255) / 256)), dim3(256), 0, ctx->stream, w.part.p, (int)nslice,
                       (int)nP, nb, (int)b0, dW);
  }
  HFG_HIP_CHECK(hipGetLastError());
}

// What one XC build computes and launches, decided once from the rows of its two functionals (host/xc_funcs.h)
struct XCPlan {
  int do_grad, do_tau, do_lapl;  // the inputs beside rho that the density stage forms and the Fock stage consumes
  bool ext;                      // the EXT instantiation of the grid kernel
  double thr;                    // density threshold
  int maxgrp;                    // largest m group of the angular basis
  size_t NQ, AA, nv;             // radial points, angular pairs, entries of one V / Fo plane
  int rank, nranks;              // the shard of the radial points that this build computes: the context's
};
static int max_group(const hfg_dev_tables *t) {
  int maxgrp = 0;
  for (int g = 0; g < t->G; g++) maxgrp = std::max(maxgrp, t->h_grp_off[g + 1] - t->h_grp_off[g]);
  return maxgrp;
}
// (no functional at all, ids 0 and 0: the plain plan of the model potential -- no gradient, no tau, no Laplacian)
static XCPlan xc_plan(const hfg_ctx *ctx, const hfg_dev_tables *t, int x_func, int c_func, double thr) {
  if (!t->have_xc) throw std::runtime_error("XC grid tables were not uploaded (hfg_basis_upload with ldft,mdft > 0)\n");
  auto either = [&](bool (*is)(int)) { return (x_func > 0 && is(x_func)) || (c_func > 0 && is(c_func)); };
  if ((x_func > 0 && !xc::is_supported(x_func)) || (c_func > 0 && !xc::is_supported(c_func)))
    throw std::runtime_error("Functional not found!");
  XCPlan pl;
  pl.do_grad = either(xc::is_gga);
  // Laplacian-dependent meta-GGAs (the atomic program only; both available ones need tau as well)
  pl.do_lapl = either(xc::is_mgga_lapl);
  if (pl.do_lapl && t->geom != 1) throw std::logic_error("Laplacian not implemented!\n");  // diatomic dftgrid.cpp:115-116, 209-210
  pl.do_tau = either(xc::is_mgga) || pl.do_lapl;
  pl.ext = either(xc::is_ext);
  // meta-GGAs: a floor under the density threshold.  Below 1e-50 the tau-dependent expressions overflow (tau_unif ~ n^(5/3),
  // p ~ sigma / n^(8/3)) and return NaN where the point carries nothing; libxc keeps such points out with its own tau and
  // sigma thresholds, --dftthr 0 would switch the density threshold off.  Far-field densities of an SCF density are
  // rounding noise of the eigensolver at that level (tests/test_gpu_fullsize.py::test_fullsize_xc_without_density_threshold).
  pl.thr = pl.do_tau ? std::max(thr, 1e-40) : thr;
  pl.maxgrp = max_group(t);
  pl.NQ = (size_t)t->E * t->nq;
  pl.AA = (size_t)t->A * t->A;
  pl.nv = pl.NQ * t->G * t->G * t->ntheta;
  pl.rank = ctx->shard_rank;
  pl.nranks = ctx->shard_n;
  return pl;
}

// work arrays of one XC build; planes: how many V and Fo hold in all, as the grid kernel indexes them
static void xc_buffers(FockAux &a, const XCPlan &pl, int planes) {
  a.D0.resize(pl.NQ * pl.AA);
  a.D1.resize(pl.NQ * pl.AA);
  a.GA.resize(pl.NQ * pl.AA);
  a.GB.resize(pl.NQ * pl.AA);
  if (pl.do_tau) {
    a.D2.resize(pl.NQ * pl.AA);
    a.GC.resize(pl.NQ * pl.AA);
  }
  if (pl.do_lapl) {
    a.D3.resize(pl.NQ * pl.AA);
    a.GL.resize(pl.NQ * pl.AA);
  }
  a.V.resize(planes * pl.nv);
  a.Fo.resize(planes * pl.nv);
  a.partial.resize(3 * pl.NQ);
}

// density stage of one spin: compact density -> the planes of V at dV
static void xc_density_stage(hfg_ctx *ctx, const hfg_dev_tables *t, FockAux &a, const XCPlan &pl, const double *dPc, double *dV,
                             const FockSkip &sk = FockSkip()) {
  const int A = t->A, E = t->E, p = t->p, nq = t->nq, G = t->G, nth = t->ntheta;
  launch_lds(k_xc_density_radial, dim3(A * A, E), dim3(256), accepted(helfem::xc_density_radial_lds(p, nq, pl.do_lapl)), ctx->stream, dPc,
             t->rad_B.p, t->rad_dB.p, t->rad_L.p, A, E, p, nq, pl.do_grad, pl.do_tau, pl.do_lapl, pl.rank, pl.nranks, a.D0.p,
             a.D1.p, a.D2.p, a.D3.p, sk.on);
  hipLaunchKernelGGL(k_xc_density_theta, dim3((unsigned)pl.NQ, G * G), dim3(fock_block_threads(nth)),
                     helfem::xc_density_theta_lds(pl.maxgrp, pl.do_lapl), ctx->stream, a.D0.p, a.D1.p, (const double *)a.D2.p,
                     (const double *)a.D3.p, t->Th.p, t->dTh.p, t->shell_l.p, t->rad_sh.p, A, nth, G, t->grp_off.p, t->grp_shell.p,
                     pl.do_grad, pl.do_tau, pl.do_lapl, pl.NQ, pl.rank, pl.nranks, dV, nq, sk.gon);
}

// X4: the one-pass kernel when its tables fit the LDS the plan allows, the chunked one otherwise
static void launch_xc_fock_theta(hfg_ctx *ctx, const hfg_dev_tables *t, FockAux &a, const XCPlan &pl, const double *dFo, const FockSkip &sk) {
  const helfem::XcFockThetaPlan th = helfem::xc_fock_theta_plan(t->ntheta, pl.maxgrp, pl.do_lapl, tuning().xc_lds_limit);
  refuse(th.refused);
  const dim3 grid((unsigned)pl.NQ, t->G * t->G), block(256);
  if (!th.chunked)
    launch_lds(k_xc_fock_theta, grid, block, th.bytes, ctx->stream, dFo, t->Th.p, t->dTh.p, t->A, t->ntheta, t->G, t->grp_off.p,
               t->grp_shell.p, pl.do_grad, pl.do_tau, pl.do_lapl, pl.NQ, pl.rank, pl.nranks, a.GA.p, a.GB.p, a.GC.p, a.GL.p,
               sk.gneed);
  else if (pl.do_lapl)
    launch_lds(k_xc_fock_theta_chunked<true>, grid, block, th.bytes, ctx->stream, dFo, t->Th.p, t->dTh.p, t->A, t->ntheta, t->G,
               t->grp_off.p, t->grp_shell.p, pl.do_grad, pl.do_tau, pl.NQ, pl.rank, pl.nranks, a.GA.p, a.GB.p, a.GC.p, a.GL.p,
               th.nthc, sk.gneed);
  else
    launch_lds(k_xc_fock_theta_chunked<false>, grid, block, th.bytes, ctx->stream, dFo, t->Th.p, t->dTh.p, t->A, t->ntheta, t->G,
               t->grp_off.p, t->grp_shell.p, pl.do_grad, pl.do_tau, pl.NQ, pl.rank, pl.nranks, a.GA.p, a.GB.p, a.GC.p,
               (double *)nullptr, th.nthc, sk.gneed);
}

// Fock stage of one spin: the planes of Fo at dFo -> compact matrix
static void xc_fock_stage(hfg_ctx *ctx, const hfg_dev_tables *t, FockAux &a, const XCPlan &pl, const double *dFo, double *dHc,
                          const FockSkip &sk = FockSkip()) {
  const int A = t->A, E = t->E, p = t->p, nq = t->nq;
  launch_xc_fock_theta(ctx, t, a, pl, dFo, sk);
  launch_lds(k_xc_fock_radial, dim3(A * A, E), dim3(fock_block_threads(p * p)), accepted(helfem::xc_fock_radial_lds(p, nq, pl.do_lapl)),
             ctx->stream, a.GA.p, a.GB.p, a.GC.p, a.GL.p, t->rad_B.p, t->rad_dB.p, t->rad_L.p, t->shell_l.p, t->rad_sh.p, A, E, p, nq,
             pl.do_grad, pl.do_tau, pl.do_lapl, pl.rank, pl.nranks, dHc, sk.need);
}

// the grid kernel of one build: its EXT instantiation if the plan asks for it, shb bytes of dynamic LDS, one workgroup per
// radial point; tail: the arguments behind the tables that both grid kernels share
template <typename K, typename... Tail>
static void launch_xc_grid(hfg_ctx *ctx, const hfg_dev_tables *t, FockAux &a, const XCPlan &pl, K k_ext, K k_plain, size_t shb,
                           int x_func, int c_func, Tail... tail) {
  launch_lds(pl.ext ? k_ext : k_plain, dim3((unsigned)pl.NQ), dim3(256), shb, ctx->stream, a.V.p, t->rad_w.p, t->rad_sh.p, t->th_s.p,
             t->th_w.p, t->grp_m.p, t->cosd.p, t->sind.p, t->Dmax, t->G, t->ntheta, t->nphi, t->Rhalf, t->geom, x_func, c_func, pl.do_grad,
             pl.do_tau, pl.do_lapl, pl.thr, pl.NQ, pl.rank, pl.nranks, a.Fo.p, a.partial.p, tail...);
}

static void xc_compact(hfg_ctx *ctx, hfg_basis *basis, int x_func, int c_func, const double *dPc, double *dHc, double *dScal,
                       double thr, const FockSkip &sk = FockSkip()) {
  hfg_dev_tables *t = tables_of(ctx, basis);
  const XCPlan pl = xc_plan(ctx, t, x_func, c_func, thr);
  FockAux &a = aux_for(ctx, basis);
  const int npl = pl.do_lapl ? 6 : 5;  // planes of V and Fo, and of the kernel's LDS potentials
  xc_buffers(a, pl, npl);
  xc_density_stage(ctx, t, a, pl, dPc, a.V.p, sk);
  launch_xc_grid(ctx, t, a, pl, k_xc_grid<true>, k_xc_grid<false>, accepted(helfem::xc_grid_lds(npl, t->ntheta, t->nphi)), x_func, c_func);
  xc_fock_stage(ctx, t, a, pl, a.Fo.p, dHc, sk);
  hipLaunchKernelGGL(k_xc_sum_partials, dim3(1), dim3(64), 0, ctx->stream, a.partial.p, pl.NQ, dScal);
  HFG_HIP_CHECK(hipGetLastError());
}

/// The n external parameters of functional id into the XCPar fields its row names, in order (host/xc_funcs.h); the count has
/// passed check_xc_params.  A range-separation constant must be positive.
static void fill_xcpar(xc::XCPar &par, int id, const double *pars, int n) {
  const helfem::XCFunc *f = helfem::find_xc_func(id);
  const char *name = f ? f->pars : "";
  for (int i = 0; i < n; i++) {
    const size_t len = strcspn(name, ",");
    double *field = nullptr;
#define FIELD(m) \
  if (len == strlen(#m) && !strncmp(name, #m, len)) field = &par.m;
    FIELD(x_alpha) FIELD(x_kappa) FIELD(x_mu) FIELD(c_beta) FIELD(c_gamma) FIELD(c_BB) FIELD(x_omega)
#undef FIELD
    if (!field) throw std::logic_error("xc_funcs.h names an XCPar field that does not exist\n");
    if (field == &par.x_omega && !(pars[i] > 0.0)) throw std::runtime_error("The range-separation constant omega must be positive.\n");
    *field = pars[i];
    name += len + (name[len] == ',');
  }
}

/// External functional parameters for the following XC builds on this stream (NULL / 0: the functional's defaults), libxc's
/// parameter lists as the npar / pars columns of host/xc_funcs.h give them; anything else throws (std::runtime_error, as
/// libxc's "number of parameters" check does through the reference).
void set_xc_params(hfg_ctx *ctx, int x_func, const double *x_pars, int nx, int c_func, const double *c_pars, int nc) {
  xc::XCPar par = HFG_XCPAR_DEFAULTS;
  if (nx > 0 && !x_pars) throw std::runtime_error("Exchange functional parameters missing.\n");
  if (nc > 0 && !c_pars) throw std::runtime_error("Correlation functional parameters missing.\n");
  helfem::check_xc_params(x_func, nx, c_func, nc);
  fill_xcpar(par, x_func, x_pars, nx);
  fill_xcpar(par, c_func, c_pars, nc);
  // the host copy must stay valid until the asynchronous copy has run: a small per-thread ring
  static thread_local xc::XCPar staged[8];
  static thread_local int slot = 0;
  staged[slot] = par;
  HFG_HIP_CHECK(hipMemcpyToSymbolAsync(HIP_SYMBOL(xc::c_xcpar), &staged[slot], sizeof(par), 0, hipMemcpyHostToDevice, ctx->stream));
  slot = (slot + 1) % 8;
}

/// libxc's xc_mgga_exc_vxc array layout on host arrays for one functional id (hfg_xc_eval): the point code of the grid kernels,
/// compiled for the host, with their threshold rules (density threshold, the meta-GGA floor 1e-40 under it, exchange channels
/// below it left out, non-finite vlapl zeroed).  nspin 1: rho, sigma, lapl, tau, exc, vrho, vsigma, vlapl, vtau hold one value
/// per point; nspin 2: rho[2], sigma[3] (aa, ab, bb), lapl[2], tau[2] per point, and the potentials likewise.  Missing inputs
/// (NULL) are zero, missing outputs are skipped.
void xc_eval_host(int id, int nspin, size_t np, const double *rho, const double *sigma, const double *lapl, const double *tau,
                  double *exc, double *vrho, double *vsigma, double *vlapl, double *vtau, double thr) {
  if (id <= 0 || !xc::is_supported(id)) throw std::runtime_error("Functional not found!");
  if (nspin != 1 && nspin != 2) throw std::logic_error("hfg_xc_eval: nspin must be 1 or 2\n");
  if (!rho) throw std::logic_error("hfg_xc_eval: rho is required\n");
  if (xc::is_mgga(id) || xc::is_mgga_lapl(id)) thr = std::max(thr, 1e-40);
  auto in = [](const double *a, size_t i) { return a ? a[i] : 0.0; };
  auto out = [](double *a, size_t i, double v) {
    if (a) a[i] = v;
  };
  for (size_t i = 0; i < np; i++) {
    if (nspin == 1) {
      const double r = rho[i], s = in(sigma, i), l = in(lapl, i), t = in(tau, i);
      double e = 0.0, vr = 0.0, vs = 0.0, vt = 0.0, vl = 0.0;
      if (r >= thr && r > 0.0) {
        const bool live = 0.5 * r >= thr;
        HFG_XC_EVAL_POINT(true, id, r, s, t, l, live, e, vr, vs, vt, vl);
        if (!std::isfinite(vl)) vl = 0.0;
      }
      out(exc, i, e);
      out(vrho, i, vr);
      out(vsigma, i, vs);
      out(vlapl, i, vl);
      out(vtau, i, vt);
      continue;
    }
    const double r0 = rho[2 * i], r1 = rho[2 * i + 1], rt = r0 + r1;
    double e = 0.0, va = 0.0, vb = 0.0, vsaa = 0.0, vsab = 0.0, vsbb = 0.0, vta = 0.0, vtb = 0.0, vla = 0.0, vlb = 0.0;
    if (rt >= thr && rt > 0.0) {
      const double ra = std::max(r0, thr), rb = std::max(r1, thr);
      const double saa = in(sigma, 3 * i), sab = in(sigma, 3 * i + 1), sbb = in(sigma, 3 * i + 2);
      const double ta = in(tau, 2 * i), tb = in(tau, 2 * i + 1), la = in(lapl, 2 * i), lb = in(lapl, 2 * i + 1);
      HFG_XC_EVAL_POINT_POL(true, id, ra, rb, saa, sab, sbb, ta, tb, la, lb, r0 >= thr, r1 >= thr, e, va, vb, vsaa, vsab, vsbb, vta, vtb, vla, vlb);
      if (!std::isfinite(vla)) vla = 0.0;
      if (!std::isfinite(vlb)) vlb = 0.0;
    }
    out(exc, i, e);
    out(vrho, 2 * i, va);
    out(vrho, 2 * i + 1, vb);
    out(vsigma, 3 * i, vsaa);
    out(vsigma, 3 * i + 1, vsab);
    out(vsigma, 3 * i + 2, vsbb);
    out(vlapl, 2 * i, vla);
    out(vlapl, 2 * i + 1, vlb);
    out(vtau, 2 * i, vta);
    out(vtau, 2 * i + 1, vtb);
  }
}

/// xc_eval_host with external parameters for this call (hfg_xc_eval_ext): pars as set_xc_params takes them for the id as an
/// exchange (lda_x, gga_x_pbe, the short-range GGA primitives) or correlation (gga_c_pbe) functional
void xc_eval_host_ext(int id, const double *pars, int npars, int nspin, size_t np, const double *rho, const double *sigma,
                      const double *lapl, const double *tau, double *exc, double *vrho, double *vsigma, double *vlapl, double *vtau,
                      double thr) {
  if (npars > 0 && !pars) throw std::runtime_error("Functional parameters missing.\n");
  xc::XCPar par = HFG_XCPAR_DEFAULTS;
  if (npars > 0) {
    // in the role of its row; an id that takes no parameters is refused in the words for an exchange functional
    const helfem::XCFunc *f = helfem::find_xc_func(id);
    if (f && f->npar > 0 && !strcmp(f->role, "c")) helfem::check_xc_params(0, 0, id, npars);
    else helfem::check_xc_params(id, npars, 0, 0);
    fill_xcpar(par, id, pars, npars);
  }
  struct Reset {  // the defaults come back whatever happens
    ~Reset() { xc::host_xcpar() = xc::XCPar HFG_XCPAR_DEFAULTS; }
  } reset;
  xc::host_xcpar() = par;
  xc_eval_host(id, nspin, np, rho, sigma, lapl, tau, exc, vrho, vsigma, vlapl, vtau, thr);
}

void xc_fock_dev(hfg_ctx *ctx, hfg_basis *basis, int x_func, int c_func, const double *dP, double *dH, double *dScal,
                 double thr) {
  hfg_dev_tables *t = tables_of(ctx, basis);
  FockAux &a = aux_for(ctx, basis);
  const size_t nc = (size_t)t->A * t->A * t->E * t->p * t->p;
  a.Pc.resize(nc);
  a.Jc.resize(nc);
  ProfScope ps(ctx, "xc");
  const FockSkip sk = gather_compact_flagged(ctx, basis, dP, a.Pc.p, false);  // the whole matrix is returned: density side only
  xc_compact(ctx, basis, x_func, c_func, a.Pc.p, a.Jc.p, dScal, thr, sk);
  scatter_dense(ctx, basis, a.Jc.p, dH);
  HFG_HIP_CHECK(hipGetLastError());
}

// dynamic LDS of k_xc_grid_pol and the theta rows that go through it per pass
static helfem::XcGridPolPlan xc_grid_pol_plan(const hfg_dev_tables *t, const XCPlan &pl) {
  const helfem::XcGridPolPlan g = helfem::xc_grid_pol_plan(t->ntheta, t->nphi, pl.do_tau, pl.do_lapl, tuning().xc_lds_limit);
  refuse(g.refused);
  return g;
}

// spin-polarised XC: Hc_a, Hc_b (compact) from Pc_a, Pc_b (compact); dScal = (Exc, Nel, 0).  sk: flags that hold for both
// spins (gather_compact_pol_flagged); xc_fock_pol_dev passes none
static void xc_compact_pol(hfg_ctx *ctx, hfg_basis *basis, int x_func, int c_func, const double *dPca, const double *dPcb,
                           double *dHca, double *dHcb, double *dScal, double thr, const FockSkip &sk = FockSkip()) {
  hfg_dev_tables *t = tables_of(ctx, basis);
  const XCPlan pl = xc_plan(ctx, t, x_func, c_func, thr);
  FockAux &a = aux_for(ctx, basis);
  const int npl = pl.do_lapl ? 6 : (pl.do_tau ? 5 : 3);  // planes of V and Fo per spin
  xc_buffers(a, pl, 2 * npl);
  for (int sp = 0; sp < 2; sp++) xc_density_stage(ctx, t, a, pl, sp ? dPcb : dPca, a.V.p + (size_t)sp * npl * pl.nv, sk);
  const helfem::XcGridPolPlan g = xc_grid_pol_plan(t, pl);
  launch_xc_grid(ctx, t, a, pl, k_xc_grid_pol<true>, k_xc_grid_pol<false>, g.bytes, x_func, c_func, g.rowc);
  for (int sp = 0; sp < 2; sp++) xc_fock_stage(ctx, t, a, pl, a.Fo.p + (size_t)sp * npl * pl.nv, sp ? dHcb : dHca, sk);
  hipLaunchKernelGGL(k_xc_sum_partials, dim3(1), dim3(64), 0, ctx->stream, a.partial.p, pl.NQ, dScal);
  HFG_HIP_CHECK(hipGetLastError());
}

void xc_fock_pol_dev(hfg_ctx *ctx, hfg_basis *basis, int x_func, int c_func, const double *dPa, const double *dPb,
                     double *dHa, double *dHb, double *dScal, double thr) {
  hfg_dev_tables *t = tables_of(ctx, basis);
  FockAux &a = aux_for(ctx, basis);
  const size_t nc = (size_t)t->A * t->A * t->E * t->p * t->p;
  a.Pc.resize(nc);
  a.Jc.resize(nc);
  a.Pc2.resize(nc);
  a.Jc2.resize(nc);
  ProfScope ps(ctx, "xc");
  gather_compact(ctx, basis, dPa, a.Pc.p);
  gather_compact(ctx, basis, dPb, a.Pc2.p);
  xc_compact_pol(ctx, basis, x_func, c_func, a.Pc.p, a.Pc2.p, a.Jc.p, a.Jc2.p, dScal, thr);
  scatter_dense(ctx, basis, a.Jc.p, dHa);
  scatter_dense(ctx, basis, a.Jc2.p, dHb);
  HFG_HIP_CHECK(hipGetLastError());
}

void model_potential_dev(hfg_ctx *ctx, hfg_basis *basis, int kind1, int Z1, double d1, double H1, int kind2, int Z2,
                         double d2, double H2, double *dH) {
  hfg_dev_tables *t = tables_of(ctx, basis);
  XCPlan pl = xc_plan(ctx, t, 0, 0, 0.0);  // the plain plan: the Fock stage reads the one plane that k_mp_fill writes
  pl.rank = 0, pl.nranks = 1;              // the whole matrix on every rank: the guess is not summed over them
  for (int k : {kind1, kind2})
    if (k != 0 && k != 1 && k != 3) throw std::logic_error("Unsupported guess\n");
  if ((kind1 == 1 && !(d1 > 0.0)) || (kind2 == 1 && !(d2 > 0.0)))
    throw std::logic_error("GSZ guess: the screening length d_Z must be given\n");
  FockAux &a = aux_for(ctx, basis);
  a.Jc.resize(pl.AA * t->E * t->p * t->p);
  a.GA.resize(pl.NQ * pl.AA);
  a.GB.resize(pl.NQ * pl.AA);
  a.Fo.resize(5 * pl.nv);
  DevModelPot p1{kind1, Z1, d1, H1}, p2{kind2, Z2, d2, H2};
  hipLaunchKernelGGL(k_mp_fill, dim3((unsigned)pl.NQ), dim3(256), 0, ctx->stream, t->rad_w.p, t->rad_sh.p, t->th_c.p, t->th_s.p,
                     t->th_w.p, t->G, t->ntheta, t->nphi, t->Rhalf, t->geom, p1, p2, a.Fo.p);
  xc_fock_stage(ctx, t, a, pl, a.Fo.p, a.Jc.p);
  scatter_dense(ctx, basis, a.Jc.p, dH);
  HFG_HIP_CHECK(hipGetLastError());
}

size_t fock_compact_size(hfg_basis *basis) {
  return (size_t)basis->Nang() * basis->Nang() * basis->Nel() * basis->max_Nprim() * basis->max_Nprim();
}

// hfg_ctx_set_fock_blocks: the pairs of the compact matrix that the caller of fock_compact_dev reads, from the symmetry
// block of every basis function (device array of N ints, as fock_finish_dev takes it; null: everything again).  Kept in
// the context, for the table set the basis has now: another basis, or tables uploaded anew, are built in full.
void set_fock_blocks(hfg_ctx *ctx, hfg_basis *basis, const int *dBlockId) {
  ctx->fock_need_tables = nullptr;
  if (!dBlockId) return;
  if (!basis->dev || basis->dev_device != ctx->device) throw std::logic_error("hfg_ctx_set_fock_blocks: the basis tables are not on this context's device\n");
  const hfg_dev_tables *t = basis->dev;
  const int A = t->A;
  std::vector<int> blockid(t->N), nfunc(A), need((size_t)A * A);
  HFG_HIP_CHECK(hipDeviceSynchronize());  // set-up call: whichever stream filled dBlockId has finished
  HFG_HIP_CHECK(hipMemcpy(blockid.data(), dBlockId, sizeof(int) * t->N, hipMemcpyDeviceToHost));
  for (int x = 0; x < A; x++) nfunc[x] = t->R - (t->h_shell_skip[x] ? 1 : 0);
  helfem::fock_need_pairs(A, nfunc.data(), blockid.data(), need.data());
  ctx->fock_need.upload(need, ctx->stream);
  ctx->fock_need_A = A;
  ctx->fock_need_G = 0;
  if (t->have_xc) {  // m groups in the order of tables.cpp: ascending distinct m
    std::vector<int> ms(t->h_shell_m.begin(), t->h_shell_m.begin() + A);
    std::sort(ms.begin(), ms.end());
    ms.erase(std::unique(ms.begin(), ms.end()), ms.end());
    const int G = (int)ms.size();
    if (G != t->G) throw std::logic_error("hfg_ctx_set_fock_blocks: m groups do not match the XC tables\n");
    std::vector<int> gneed((size_t)G * G, 0);
    auto grp = [&](int x) { return (int)(std::lower_bound(ms.begin(), ms.end(), t->h_shell_m[x]) - ms.begin()); };
    for (int x = 0; x < A; x++)
      for (int y = 0; y < A; y++)
        if (need[(size_t)x * A + y]) gneed[(size_t)grp(x) * G + grp(y)] = 1;
    ctx->fock_gneed.upload(gneed, ctx->stream);
    ctx->fock_need_G = G;
  }
  HFG_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the host vectors go out of scope
  ctx->fock_need_tables = t;
}

// J beside XC, for the restricted and the unrestricted compact build.  J and the XC matrices are independent given the
// compact densities: the Coulomb kernels (one of them streams the 1 GB of primitive integrals: HBM-bound) run on the
// context's side stream beside the XC kernels (LDS- and latency-bound); HELFEM_FOCK_OVERLAP=0, or a context that has given
// its side stream up: one after the other on the main stream.  gather() enqueues the compact densities and returns their
// flags, coulomb(sk) and xc(sk) enqueue on ctx->stream, combine() adds what the two left.
template <typename Gather, typename Coulomb, typename XC, typename Combine>
static void fock_j_beside_xc(hfg_ctx *ctx, Gather gather, Coulomb coulomb, XC xc, Combine combine) {
  if (!(tuning().fock_overlap && !ctx->avoid_side)) {
    FockSkip sk;
    {
      ProfScope ps(ctx, "coulomb");
      sk = gather();
      coulomb(sk);
    }
    ProfScope ps(ctx, "xc");
    xc(sk);
    combine();
    HFG_HIP_CHECK(hipGetLastError());
    return;
  }
  const hipStream_t main = ctx->stream, q = ctx->side();
  const FockSkip sk = gather();  // (the flags go under the event that guards the compact densities)
  HFG_HIP_CHECK(hipEventRecord(ctx->side_ev[0], main));
  HFG_HIP_CHECK(hipStreamWaitEvent(q, ctx->side_ev[0], 0));
  {
    struct OnStream {  // ctx->stream is q in this scope and main again behind it, also when coulomb() throws
      hfg_ctx *ctx;
      hipStream_t back;
      ~OnStream() { ctx->stream = back; }
    } on_side{ctx, main};
    ctx->stream = q;
    ProfScope ps(ctx, "coulomb");  // (its events go to the side stream with the kernels)
    coulomb(sk);
  }
  HFG_HIP_CHECK(hipEventRecord(ctx->side_ev[1], q));
  ProfScope ps(ctx, "xc");
  try {
    xc(sk);
  } catch (...) {  // J is under way into the caller's buffer: whatever the caller enqueues after the error comes behind it
    (void)hipStreamWaitEvent(main, ctx->side_ev[1], 0);
    throw;
  }
  HFG_HIP_CHECK(hipStreamWaitEvent(main, ctx->side_ev[1], 0));
  combine();
  HFG_HIP_CHECK(hipGetLastError());
}

// This shard's part of J + XC in the compact layout (to be summed over ranks), dScal = partial (Exc, Nel, 0)
void fock_compact_dev(hfg_ctx *ctx, hfg_basis *basis, int x_func, int c_func, const double *dP, double *dFc,
                      double *dScal, double thr) {
  tables_of(ctx, basis);
  FockAux &a = aux_for(ctx, basis);
  const size_t nc = fock_compact_size(basis);
  a.Pc.resize(nc);
  a.Jc.resize(nc);
  if (!(x_func > 0 || c_func > 0)) {
    {
      ProfScope ps(ctx, "coulomb");
      const FockSkip sk = gather_compact_flagged(ctx, basis, dP, a.Pc.p, true);
      coulomb_compact(ctx, basis, a.Pc.p, dFc, sk);
    }
    HFG_HIP_CHECK(hipMemsetAsync(dScal, 0, 3 * sizeof(double), ctx->stream));
    HFG_HIP_CHECK(hipGetLastError());
    return;
  }
  fock_j_beside_xc(
      ctx, [&] { return gather_compact_flagged(ctx, basis, dP, a.Pc.p, true); },
      [&](const FockSkip &sk) { coulomb_compact(ctx, basis, a.Pc.p, dFc, sk); },
      [&](const FockSkip &sk) { xc_compact(ctx, basis, x_func, c_func, a.Pc.p, a.Jc.p, dScal, thr, sk); },
      [&] { hipLaunchKernelGGL(k_add_inplace, dim3(2048), dim3(256), 0, ctx->stream, dFc, a.Jc.p, nc); });
}

// F = enforce_fock_symmetry(H0 + J + XC) from the (rank-summed) compact matrix
void fock_finish_dev(hfg_ctx *ctx, hfg_basis *basis, const double *dFc, const double *dH0, const int *dBlockId,
                     double *dF) {
  hfg_dev_tables *t = tables_of(ctx, basis);
  FockAux &a = aux_for(ctx, basis);
  ProfScope ps(ctx, "scatter");
  dim3 grid((t->N + 63) / 64, (t->N + 3) / 4);
  hipLaunchKernelGGL(k_fock_finish, grid, dim3(256), 0, ctx->stream, dFc, dH0, dBlockId, t->N, t->A, t->R, t->E, t->p,
                     a.pure_shell.p, a.pure_n.p, dF);
  HFG_HIP_CHECK(hipGetLastError());
}

// fock_compact_dev for an unrestricted build: this shard's part of Fc[0 : nc] = J[Pa + Pb] + XC_a and
// Fc[nc : 2 nc] = J[Pa + Pb] + XC_b (nc = fock_compact_size), dScal = partial (Exc, Nel, Ekin); Hartree-Fock: both slabs J
void fock_compact_pol_dev(hfg_ctx *ctx, hfg_basis *basis, int x_func, int c_func, const double *dPa, const double *dPb,
                          double *dFc, double *dScal, double thr) {
  hfg_dev_tables *t = tables_of(ctx, basis);
  const bool with_xc = x_func > 0 || c_func > 0;
  if (with_xc) xc_grid_pol_plan(t, xc_plan(ctx, t, x_func, c_func, thr));  // what the XC build would refuse is refused before the first launch
  FockAux &a = aux_for(ctx, basis);
  const size_t nc = fock_compact_size(basis);
  a.Pc.resize(nc);
  a.Pc2.resize(nc);
  a.Pc3.resize(nc);
  double *dJc = dFc + nc;  // J goes to the second slab; k_fock_combine_pol spreads it
  if (!with_xc) {
    ProfScope ps(ctx, "coulomb");
    const FockSkip sk = gather_compact_pol_flagged(ctx, basis, dPa, dPb, true);
    coulomb_compact(ctx, basis, a.Pc3.p, dJc, sk);
    HFG_HIP_CHECK(hipMemcpyAsync(dFc, dJc, nc * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    HFG_HIP_CHECK(hipMemsetAsync(dScal, 0, 3 * sizeof(double), ctx->stream));
    return;
  }
  a.Jc.resize(nc);
  a.Jc2.resize(nc);
  fock_j_beside_xc(
      ctx, [&] { return gather_compact_pol_flagged(ctx, basis, dPa, dPb, true); },
      [&](const FockSkip &sk) { coulomb_compact(ctx, basis, a.Pc3.p, dJc, sk); },
      [&](const FockSkip &sk) { xc_compact_pol(ctx, basis, x_func, c_func, a.Pc.p, a.Pc2.p, a.Jc.p, a.Jc2.p, dScal, thr, sk); },
      [&] { hipLaunchKernelGGL(k_fock_combine_pol, dim3(2048), dim3(256), 0, ctx->stream, dFc, a.Jc.p, a.Jc2.p, nc); });
}

// fock_finish_dev for the two slabs of fock_compact_pol_dev, one launch
void fock_finish_pol_dev(hfg_ctx *ctx, hfg_basis *basis, const double *dFc, const double *dH0, const int *dBlockId,
                         double *dFa, double *dFb) {
  hfg_dev_tables *t = tables_of(ctx, basis);
  FockAux &a = aux_for(ctx, basis);
  ProfScope ps(ctx, "scatter");
  dim3 grid((t->N + 63) / 64, (t->N + 3) / 4);
  hipLaunchKernelGGL(k_fock_finish_pol, grid, dim3(256), 0, ctx->stream, dFc, fock_compact_size(basis), dH0, dBlockId, t->N, t->A,
                     t->R, t->E, t->p, a.pure_shell.p, a.pure_n.p, dFa, dFb);
  HFG_HIP_CHECK(hipGetLastError());
}

}  // namespace hfg
