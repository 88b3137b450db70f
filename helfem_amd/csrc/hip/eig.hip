// Dense symmetric / symmetric-definite generalized eigensolver on gfx950.
//
// Replaces (reference, /root/reference):
//   scf::eig_gsym      src/general/scf_helpers.cpp:131-140   Forth = Sinvh^T F Sinvh; eig_sym; C = Sinvh C
//   scf::eig_gsym_sub  src/general/scf_helpers.cpp:142-186   the same per symmetry block + global sort
//   arma::eig_sym      (LAPACK dsyevd) as called there and in utils::invh, libhelfem/src/utils.cpp:172
//
// Pipeline per (symmetry) block, all blocks batched in the same launches (grid.y = block):
//   1. gather F(idx,idx), Sinvh(idx,cols)                       k_gather_block
//   2. Forth = X^T (F X)                                        FP64 MFMA GEMM (gemm.hip)
//   3. Householder tridiagonalisation, two launches per column   k_trd_gemv / k_trd_update
//        (symv-like sweep over the trailing matrix: bandwidth bound, matrix resident in L2/MALL)
//   4. tridiagonal eigenproblem                                  implicit QL, rotations logged then
//                                                                applied row-parallel (k_tql_*)
//   5. back-transformation Z <- H_0 ... H_{n-3} Z                k_backtransform (column-parallel, no
//                                                                inter-workgroup dependency at all)
//   6. C = X Z                                                   GEMM, then rank sort + scatter
#include "internal.h"
#include "wave.h"
#include "../host/eigsel_count.h"
#include "../host/eig_band_plan.h"
#include <cstdlib>
#include <cstring>
#include <functional>

namespace hfg {

constexpr int MAXB = 8;
struct EigBatch {
  int nblk;
  int n[MAXB];
  double *A[MAXB];    // n x n, lda = n; on exit Householder vectors below the subdiagonal
  double *d[MAXB];    // n
  double *e[MAXB];    // n
  double *tau[MAXB];  // n
  double *v[MAXB];    // n   current Householder vector (v[0]=1 stored explicitly)
  double *pp[MAXB];   // NCS x n partial gemv results
  double *dots[MAXB];  // partial v^T A v per gemv workgroup
  double *Z[MAXB];    // n x nz eigenvectors
  int nz[MAXB];       // columns of Z: n, or the wanted ones of a selected solve
  double *rot[MAXB];  // rotation log (c,s pairs)
  int *sweeps[MAXB];  // (l, m, offset, count) per QL sweep; sweeps[0] = number of sweeps, [1]=status
  long rotcap[MAXB];
};

constexpr int TRD_NCS = 8;  // column slabs of the gemv

// ---- 1. gather -----------------------------------------------------------------------------------
__global__ void k_gather_block(const double *__restrict__ F, const double *__restrict__ S, int N,
                               const int64_t *__restrict__ rows, const int64_t *__restrict__ cols, int n,
                               double *__restrict__ Fb, double *__restrict__ Xb) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int j = blockIdx.y;
  if (i >= n) return;
  Fb[(size_t)j * n + i] = F[(size_t)rows[j] * N + rows[i]];
  Xb[(size_t)j * n + i] = S[(size_t)cols[j] * N + rows[i]];
}

// F(idx,idx) alone: X of this block is already in the context's cache (EigWork::Xc)
__global__ void k_gather_f(const double *__restrict__ F, int N, const int64_t *__restrict__ rows, int n, double *__restrict__ Fb) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int j = blockIdx.y;
  if (i >= n) return;
  Fb[(size_t)j * n + i] = F[(size_t)rows[j] * N + rows[i]];
}

// F(irows, jrows): the rows of the block in another order than its columns (the banded F X: rows radial-major)
__global__ void k_gather_f2(const double *__restrict__ F, int N, const int64_t *__restrict__ irows, const int64_t *__restrict__ jrows,
                            int n, double *__restrict__ Fb) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int j = blockIdx.y;
  if (i >= n) return;
  Fb[(size_t)j * n + i] = F[(size_t)jrows[j] * N + irows[i]];
}

// column support of Sinvh on the block rows (scf_helpers.cpp:150-157): flag[c] = any(Sinvh(rows,c) != 0)
__global__ void k_col_support(const double *__restrict__ S, int N, const int64_t *__restrict__ rows, int n,
                              int *__restrict__ flag) {
  int c = blockIdx.x;
  int any = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x)
    if (S[(size_t)c * N + rows[i]] != 0.0) any = 1;
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) flag[c] = any;
}

// ---- 3. tridiagonalisation -----------------------------------------------------------------------
// Householder vector of column k (LAPACK dlarfg), computed identically by every workgroup.
__device__ inline void householder_of_column(const double *__restrict__ A, int n, int k, double *vsh, double *red,
                                             double &tau, double &beta) {
  const int m = n - k - 1;  // length of x = A[k+1:n, k]
  const double *x = A + (size_t)k * n + k + 1;
  double s = 0.0;
  for (int i = 1 + threadIdx.x; i < m; i += blockDim.x) s += x[i] * x[i];
  s = wave_sum(s);
  int nwave = blockDim.x / 64;
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  double xn2 = 0.0;
  for (int w = 0; w < nwave; w++) xn2 += red[w];
  double alpha = x[0];
  double scale;
  if (xn2 == 0.0) {
    tau = 0.0;
    beta = alpha;
    scale = 0.0;
  } else {
    double nrm = sqrt(alpha * alpha + xn2);
    beta = (alpha >= 0.0) ? -nrm : nrm;
    tau = (beta - alpha) / beta;
    scale = 1.0 / (alpha - beta);
  }
  for (int i = threadIdx.x; i < m; i += blockDim.x) vsh[i] = (i == 0) ? 1.0 : x[i] * scale;
  __syncthreads();
}

// S1: partial p = A22 v over (64-row slab) x (column slab); partial v^T A22 v
__global__ __launch_bounds__(256) void k_trd_gemv(EigBatch b, int k) {
  extern __shared__ double sh[];  // v[nmax], red[4*64 + 8]
  const int blk = blockIdx.y;
  const int n = b.n[blk];
  if (k > n - 3) return;
  const int m = n - k - 1;
  const int nrs = (m + 63) / 64;
  const int rs = blockIdx.x / TRD_NCS, cs = blockIdx.x % TRD_NCS;
  if (rs >= nrs) return;
  double *A = b.A[blk];
  double *vsh = sh;
  double *red = sh + n;
  double tau, beta;
  householder_of_column(A, n, k, vsh, red, tau, beta);
  if (blockIdx.x == 0) {
    for (int i = threadIdx.x; i < m; i += blockDim.x) b.v[blk][i] = vsh[i];
    if (threadIdx.x == 0) {
      b.tau[blk][k] = tau;
      b.e[blk][k] = beta;
      b.d[blk][k] = A[(size_t)k * n + k];
    }
  }
  const int cchunk = (m + TRD_NCS - 1) / TRD_NCS;
  const int c0 = cs * cchunk, c1 = min(m, c0 + cchunk);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = rs * 64 + lane;  // local index in trailing block
  double acc = 0.0;
  if (row < m) {
    const double *a = A + (size_t)(k + 1) * n + (k + 1) + row;  // A22(row, 0)
    for (int c = c0 + wave; c < c1; c += 4) acc += a[(size_t)c * n] * vsh[c];
  }
  __syncthreads();
  red[wave * 64 + lane] = acc;
  __syncthreads();
  if (wave == 0) {
    double p = red[lane] + red[64 + lane] + red[128 + lane] + red[192 + lane];
    if (row < m) b.pp[blk][(size_t)cs * n + row] = p;
    double dv = (row < m) ? p * vsh[row] : 0.0;
    dv = wave_sum(dv);
    if (lane == 0) b.dots[blk][blockIdx.x] = dv;
  }
}

// S2: w = tau*p - (tau^2/2)(v^T A v) v ; A22 -= v w^T + w v^T on a 64x64 tile; first tile stores v into column k
__global__ __launch_bounds__(256) void k_trd_update(EigBatch b, int k) {
  __shared__ double vr[64], vc[64], wr[64], wc[64];
  __shared__ double Ksh;
  const int blk = blockIdx.y;
  const int n = b.n[blk];
  if (k > n - 3) return;
  const int m = n - k - 1;
  const int nt = (m + 63) / 64;
  if ((int)blockIdx.x >= nt * nt) return;
  const int tr = blockIdx.x % nt, tc = blockIdx.x / nt;
  double *A = b.A[blk];
  const double tau = b.tau[blk][k];
  if (threadIdx.x == 0) {
    const int nrs = (m + 63) / 64;
    double s = 0.0;
    for (int i = 0; i < nrs * TRD_NCS; i++) s += b.dots[blk][i];
    Ksh = 0.5 * tau * tau * s;  // (tau/2) * p^T v with p = tau A v
  }
  __syncthreads();
  if (threadIdx.x < 128) {
    int which = threadIdx.x >> 6, l = threadIdx.x & 63;
    int idx = (which ? tc : tr) * 64 + l;
    double v = 0.0, w = 0.0;
    if (idx < m) {
      v = b.v[blk][idx];
      double p = 0.0;
      for (int cs = 0; cs < TRD_NCS; cs++) p += b.pp[blk][(size_t)cs * n + idx];
      w = tau * p - Ksh * v;
    }
    if (which) {
      vc[l] = v;
      wc[l] = w;
    } else {
      vr[l] = v;
      wr[l] = w;
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = tr * 64 + lane;
  if (row < m) {
    double *a = A + (size_t)(k + 1) * n + (k + 1) + row;
    for (int c = wave; c < 64; c += 4) {
      int col = tc * 64 + c;
      if (col < m) a[(size_t)col * n] -= vr[lane] * wc[c] + wr[lane] * vc[c];
    }
  }
  if (blockIdx.x == 0) {
    // store v (without the implicit leading 1) below the subdiagonal of column k, beta on the subdiagonal
    for (int i = 1 + threadIdx.x; i < m; i += blockDim.x) A[(size_t)k * n + k + 1 + i] = b.v[blk][i];
  }
}

__global__ void k_trd_finish(EigBatch b) {
  int blk = blockIdx.x;
  if (threadIdx.x != 0) return;
  int n = b.n[blk];
  double *A = b.A[blk];
  if (n >= 2) {
    b.d[blk][n - 2] = A[(size_t)(n - 2) * n + (n - 2)];
    b.e[blk][n - 2] = A[(size_t)(n - 2) * n + (n - 1)];
    b.tau[blk][n - 2] = 0.0;
  }
  b.d[blk][n - 1] = A[(size_t)(n - 1) * n + (n - 1)];
  b.e[blk][n - 1] = 0.0;
}

// ---- 4. tridiagonal eigenproblem: implicit-shift QL, rotations logged --------------------------------
__global__ void k_tql_values(EigBatch b) {
  int blk = blockIdx.x;
  if (threadIdx.x != 0) return;
  const int n = b.n[blk];
  double *d = b.d[blk], *e = b.e[blk];
  double *rot = b.rot[blk];
  int *sw = b.sweeps[blk];
  long nrot = 0;
  int nsw = 0;
  int status = 0;
  const long cap = b.rotcap[blk];
  for (int l = 0; l < n && !status; l++) {
    int iter = 0;
    int m;
    do {
      for (m = l; m + 1 < n; m++) {
        double dd = fabs(d[m]) + fabs(d[m + 1]);
        if (fabs(e[m]) <= 2.220446049250313e-16 * dd) break;
      }
      if (m != l) {
        if (iter++ == 300) {
          status = 1;
          break;
        }
        if (nrot + (m - l) > cap || 4 * (nsw + 1) + 2 >= 4 * 64 * n) {
          status = 2;
          break;
        }
        double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
        double r = hypot(g, 1.0);
        g = d[m] - d[l] + e[l] / (g + (g >= 0.0 ? fabs(r) : -fabs(r)));
        double s = 1.0, c = 1.0, p = 0.0;
        int cnt = 0;
        bool under = false;
        int i;
        for (i = m - 1; i >= l; i--) {
          double f = s * e[i], bb = c * e[i];
          r = hypot(f, g);
          e[i + 1] = r;
          if (r == 0.0) {
            d[i + 1] -= p;
            e[m] = 0.0;
            under = true;
            break;
          }
          s = f / r;
          c = g / r;
          g = d[i + 1] - p;
          r = (d[i] - g) * s + 2.0 * c * bb;
          p = s * r;
          d[i + 1] = g + p;
          g = c * r - bb;
          rot[2 * (nrot + cnt)] = c;
          rot[2 * (nrot + cnt) + 1] = s;
          cnt++;
        }
        sw[2 + 4 * nsw + 0] = l;
        sw[2 + 4 * nsw + 1] = m;
        sw[2 + 4 * nsw + 2] = (int)(nrot & 0x7fffffff);
        sw[2 + 4 * nsw + 3] = cnt;
        // offsets beyond 2^31 are reconstructed by the consumer as a running sum of cnt
        nsw++;
        nrot += cnt;
        if (under) continue;
        d[l] -= p;
        e[l] = g;
        e[m] = 0.0;
      }
    } while (m != l);
  }
  sw[0] = nsw;
  sw[1] = status;
}

__global__ void k_set_identity(EigBatch b) {
  int blk = blockIdx.z;
  int n = b.n[blk];
  int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i < n && j < n) b.Z[blk][(size_t)j * n + i] = (i == j) ? 1.0 : 0.0;
}

// apply the logged rotations to the rows of Z; one thread per row, columns walked as tql2 does
__global__ void k_tql_apply(EigBatch b) {
  int blk = blockIdx.y;
  int n = b.n[blk];
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  double *Z = b.Z[blk] + k;
  const double *rot = b.rot[blk];
  const int *sw = b.sweeps[blk];
  int nsw = sw[0];
  long off = 0;
  for (int q = 0; q < nsw; q++) {
    int m = sw[2 + 4 * q + 1], cnt = sw[2 + 4 * q + 3];
    double hi = Z[(size_t)m * n];
    int i = m - 1;
    for (int t = 0; t < cnt; t++, i--) {
      double c = rot[2 * (off + t)], s = rot[2 * (off + t) + 1];
      double lo = Z[(size_t)i * n];
      Z[(size_t)(i + 1) * n] = s * lo + c * hi;
      hi = c * lo - s * hi;
    }
    Z[(size_t)(i + 1) * n] = hi;
    off += cnt;
  }
}

// ---- 5. back-transformation ----------------------------------------------------------------------------
// Each wave owns one column z of Z (kept in registers, strided over the lanes) and applies
// H_{n-3} ... H_0 in turn:  z[k+1:] -= tau_k v_k (v_k^T z[k+1:]).
template <int NR>
__global__ __launch_bounds__(256) void k_backtransform(EigBatch b) {
  int blk = blockIdx.y;
  int n = b.n[blk];
  int col = blockIdx.x * 4 + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (col >= b.nz[blk]) return;
  const double *A = b.A[blk];
  const double *tau = b.tau[blk];
  double *z = b.Z[blk] + (size_t)col * n;
  double zr[NR];
#pragma unroll
  for (int r = 0; r < NR; r++) {
    int i = lane + 64 * r;
    zr[r] = (i < n) ? z[i] : 0.0;
  }
  for (int k = n - 3; k >= 0; k--) {
    double t = tau[k];
    if (t == 0.0) continue;
    const double *v = A + (size_t)k * n;  // v_i for i>k+1 at v[i], v_{k+1}=1
    double s = 0.0;
    double vr[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) {
      int i = lane + 64 * r;
      double vi = 0.0;
      if (i == k + 1) vi = 1.0;
      else if (i > k + 1 && i < n) vi = v[i];
      vr[r] = vi;
      s += vi * zr[r];
    }
    s = wave_sum(s);
    s *= t;
#pragma unroll
    for (int r = 0; r < NR; r++) zr[r] -= s * vr[r];
  }
#pragma unroll
  for (int r = 0; r < NR; r++) {
    int i = lane + 64 * r;
    if (i < n) z[i] = zr[r];
  }
}

// generic (any n) version: column kept in LDS
__global__ __launch_bounds__(256) void k_backtransform_lds(EigBatch b) {
  extern __shared__ double sh[];  // 4 * n
  int blk = blockIdx.y;
  int n = b.n[blk];
  int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int col = blockIdx.x * 4 + wave;
  if (col >= b.nz[blk]) return;
  const double *A = b.A[blk];
  const double *tau = b.tau[blk];
  double *z = b.Z[blk] + (size_t)col * n;
  double *zs = sh + (size_t)wave * n;
  for (int i = lane; i < n; i += 64) zs[i] = z[i];
  for (int k = n - 3; k >= 0; k--) {
    double t = tau[k];
    if (t == 0.0) continue;
    const double *v = A + (size_t)k * n;
    double s = 0.0;
    for (int i = k + 1 + lane; i < n; i += 64) s += ((i == k + 1) ? 1.0 : v[i]) * zs[i];
    s = wave_sum(s);
    s *= t;
    for (int i = k + 1 + lane; i < n; i += 64) zs[i] -= s * ((i == k + 1) ? 1.0 : v[i]);
  }
  for (int i = lane; i < n; i += 64) z[i] = zs[i];
}

// ---- 6. sort + scatter ---------------------------------------------------------------------------------
// rank[i] = number of eigenvalues ordered before E[i] (ties by index).  Grid (ceil(n/256), segments): a workgroup
// compares its 256 values with one segment of E staged through LDS in chunks of 256; the segment counts are integer
// atomic adds into the zero-initialised rank array (order independent).
constexpr int RANK_SEG = 8;
__global__ __launch_bounds__(256) void k_rank(const double *__restrict__ E, int n, int *__restrict__ rank) {
  __shared__ double sE[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const double ei = (i < n) ? E[i] : 0.0;
  const int seg = (n + RANK_SEG - 1) / RANK_SEG;
  const int j0 = blockIdx.y * seg, j1 = min(n, j0 + seg);
  int r = 0;
  for (int c = j0; c < j1; c += 256) {
    __syncthreads();
    sE[threadIdx.x] = (c + (int)threadIdx.x < j1) ? E[c + threadIdx.x] : 0.0;
    __syncthreads();
    const int m = min(256, j1 - c);
    if (m == 256) {
#pragma unroll 16
      for (int jj = 0; jj < 256; jj++) {
        const double ej = sE[jj];
        r += (ej < ei) || (ej == ei && c + jj < i);
      }
    } else {
      for (int jj = 0; jj < m; jj++) {
        const double ej = sE[jj];
        r += (ej < ei) || (ej == ei && c + jj < i);
      }
    }
  }
  if (i < n && r) atomicAdd(&rank[i], r);
}
static void launch_rank(hfg_ctx *ctx, const double *E, int n, int *rank) {
  HFG_HIP_CHECK(hipMemsetAsync(rank, 0, sizeof(int) * n, ctx->stream));
  hipLaunchKernelGGL(k_rank, dim3((n + 255) / 256, RANK_SEG), dim3(256), 0, ctx->stream, E, n, rank);
}

// Eout[rank[i]] = E[i]: the eigenvalues at their ranked places (the one-call entries, whose eigenvectors the last product places)
__global__ void k_place_values(const double *__restrict__ E, int n, const int *__restrict__ rank, double *__restrict__ Eout) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) Eout[rank[i]] = E[i];
}

// Cout(rows[i], rank[coff+j]) = Cb(i,j) ; Eout[rank[coff+j]] = Eb[j]   (rows==nullptr: identity)
__global__ void k_scatter_cols(const double *__restrict__ Cb, int nrow, int ncol, const int64_t *__restrict__ rows,
                               const int *__restrict__ rank, int coff, const double *__restrict__ Eb, int ldc,
                               double *__restrict__ Cout, double *__restrict__ Eout) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int j = blockIdx.y;
  if (i >= nrow) return;
  int c = rank[coff + j];
  size_t r = rows ? (size_t)rows[i] : (size_t)i;
  Cout[(size_t)c * ldc + r] = Cb[(size_t)j * nrow + i];
  if (i == 0) Eout[c] = Eb[j];
}

// selected solve through the full one: column j of Z (n x n) with rank[j] < nev goes to column rank[j] of Zs (n x nev), its
// eigenvalue to Ws[rank[j]]
__global__ void k_take_lowest(const double *__restrict__ Z, const double *__restrict__ E, int n, int nev, const int *__restrict__ rank,
                              double *__restrict__ Zs, double *__restrict__ Ws) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int j = blockIdx.y;
  int c = rank[j];
  if (i >= n || c >= nev) return;
  Zs[(size_t)c * n + i] = Z[(size_t)j * n + i];
  if (i == 0) Ws[c] = E[j];
}

// -------------------------------------------------------------------------------------------------
// host-side drivers
// -------------------------------------------------------------------------------------------------
// ---- 5b. back-transformation through compact-WY blocks on the matrix cores --------------------------------------
// Q = H_0 ... H_{n-3} = Q_0 ... Q_{P-1},  Q_p = I - V_p T_p V_p^T over BT_KB consecutive reflectors (dlarft,
// forward / columnwise), applied from the last block to the first:  Z <- Z - (V_p T_p)(V_p^T Z).
constexpr int BT_KB = 64;

// explicit reflector matrix: Vx[g, j] = 1 at g = j+1, A[g, j] below, 0 above; columns j > n-3 are zero
__global__ void k_bt_extract(EigBatch b, double *const *__restrict__ Vx) {
  const int blk = blockIdx.z;
  const int n = b.n[blk];
  const int j = blockIdx.y;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n || g >= n) return;
  double v = 0.0;
  if (j <= n - 3) {
    if (g == j + 1) v = 1.0;
    else if (g > j + 1) v = b.A[blk][(size_t)j * n + g];
  }
  Vx[blk][(size_t)j * n + g] = v;
}

// Two consecutive reflector blocks are applied in one pass over Z:  Q_p Q_{p+1} Z = Z - [VT_p | VT_{p+1}] [W0; W1] with
//   W1 = V_{p+1}^T Z,   W0 = V_p^T Z - (V_p^T VT_{p+1}) W1.
// The split-K product delivers S = [V_p | V_{p+1}]^T Z in BT_S slabs (2 BT_KB x n each, ld 2 BT_KB); this kernel adds the
// slabs and applies the coupling C = V_p^T VT_{p+1} (itself the sum of BT_GS partial products).  Workgroup = 4 columns.
constexpr int BT_PW = 2 * BT_KB;  // rows of the pair's W
constexpr int BT_WREP = 4;         // passes of 4 columns per workgroup of k_bt_wpair
__global__ __launch_bounds__(256) void k_bt_wpair(EigBatch b, double *const *__restrict__ Wpart, double *const *__restrict__ W,
                                                  double *const *__restrict__ Cc, int S, int GS, int npair, int pair,
                                                  int mirror) {
  __shared__ double sC[BT_KB][BT_KB + 1];
  __shared__ double s1[4][BT_KB];
  const int blk = blockIdx.y;
  const int n = b.n[blk];
  const int j0 = pair * BT_PW;
  if (j0 > n - 3) return;
  const int kb1 = min(BT_KB, n - 2 - (j0 + BT_KB));  // reflectors of the pair's second block (<= 0: there is none)
  const int tid = threadIdx.x, cl = tid >> 6, i = tid & 63;
  if (kb1 > 0) {
    // all loads of a slab in flight together (a rolled "load GS values, add, store" loop over the 16 elements of a
    // thread paid 16 memory round trips: 30 of this kernel's 37 us)
    constexpr int NE = BT_KB * BT_KB / 256;
    double c[NE];
#pragma unroll
    for (int u = 0; u < NE; u++) c[u] = 0.0;
    for (int sl = 0; sl < GS; sl++) {
      const double *src = Cc[blk] + ((size_t)sl * npair + pair) * BT_KB * BT_KB + tid;
#pragma unroll
      for (int u = 0; u < NE; u++) c[u] += src[256 * u];
    }
#pragma unroll
    for (int u = 0; u < NE; u++) {
      const int t = tid + 256 * u;
      sC[t % BT_KB][t / BT_KB] = c[u];  // C is column-major, ld BT_KB: element (row t % KB, col t / KB)
    }
  }
  // 16 columns per workgroup, four at a time: the 64 x 64 coupling (GS slabs to add) is staged once for all of them
  // (with 4 columns per workgroup its 128 KB of loads per workgroup made this kernel 43 us per pair)
  const size_t tot = (size_t)BT_PW * n;
  // the slab sums of all 16 columns first (independent loads, one memory round trip), then the coupling pass by pass
  double a0[BT_WREP], a1[BT_WREP];
#pragma unroll
  for (int rep = 0; rep < BT_WREP; rep++) {
    const int col = (blockIdx.x * BT_WREP + rep) * 4 + cl;
    a0[rep] = 0.0;
    a1[rep] = 0.0;
    if (col < n) {
      for (int sl = 0; sl < S; sl++) {
        a0[rep] += Wpart[blk][(size_t)sl * tot + (size_t)col * BT_PW + i];
        a1[rep] += Wpart[blk][(size_t)sl * tot + (size_t)col * BT_PW + BT_KB + i];
      }
    }
  }
  if (mirror) {
    // right application (X Q_p Q_p+1, worked on Y = X^T): rows 0..63 pass through, rows 64.. get the coupling,
    //   W1 = A1 - C^T A0   (C = V_p^T VT_p+1 as above)
    const int kb0 = min(BT_KB, n - 2 - j0);
#pragma unroll
    for (int rep = 0; rep < BT_WREP; rep++) {
      const int col = (blockIdx.x * BT_WREP + rep) * 4 + cl;
      __syncthreads();
      s1[cl][i] = (i < kb0) ? a0[rep] : 0.0;
      __syncthreads();
      if (col < n) {
        double r1 = 0.0;
        if (kb1 > 0 && i < kb1) {
          double corr = 0.0;
          for (int j = 0; j < kb0; j++) corr += sC[j][i] * s1[cl][j];
          r1 = a1[rep] - corr;
        }
        W[blk][(size_t)col * BT_PW + i] = a0[rep];
        W[blk][(size_t)col * BT_PW + BT_KB + i] = r1;
      }
    }
    return;
  }
#pragma unroll
  for (int rep = 0; rep < BT_WREP; rep++) {
    const int col = (blockIdx.x * BT_WREP + rep) * 4 + cl;
    __syncthreads();  // s1 of the previous four columns has been read (first pass: sC is complete)
    s1[cl][i] = (kb1 > 0 && i < kb1) ? a1[rep] : 0.0;
    __syncthreads();
    if (col < n) {
      double r0 = a0[rep];
      if (kb1 > 0) {
        double corr = 0.0;
        for (int j = 0; j < kb1; j++) corr += sC[i][j] * s1[cl][j];
        r0 -= corr;
      }
      W[blk][(size_t)col * BT_PW + i] = r0;
      W[blk][(size_t)col * BT_PW + BT_KB + i] = (kb1 > 0 && i < kb1) ? a1[rep] : 0.0;
    }
  }
}

// T_p from the Gram matrix G_p = V_p^T V_p and tau (one workgroup per block p of one matrix):
//   T(i,i) = tau_i,   T(0:i, i) = -tau_i T(0:i,0:i) G(0:i, i)
constexpr int BT_GS = 4;  // split-K slabs of the Gram products (K = rows of the reflector block, one 64 x 64 tile each)
__global__ __launch_bounds__(64) void k_bt_T(EigBatch b, double *const *__restrict__ G, double *const *__restrict__ T,
                                             int P) {
  __shared__ double sT[BT_KB][BT_KB + 1];
  __shared__ double sG[BT_KB][BT_KB + 1];
  __shared__ double sg[BT_KB];
  const int blk = blockIdx.y, p = blockIdx.x;
  const int n = b.n[blk];
  const int j0 = p * BT_KB;
  if (j0 > n - 3) return;
  const int kb = min(BT_KB, n - 2 - j0);
  double *Tp = T[blk] + (size_t)p * BT_KB * BT_KB;
  const int t = threadIdx.x;
  // Gram matrix = sum of the BT_GS partial products (fixed order), staged in LDS
  // (16 columns x BT_GS slabs of loads in flight at a time: the rolled "load, add, store" loop over the 64 columns paid
  // 64 memory round trips, 100 of this kernel's 115 us)
  for (int c0 = 0; c0 < BT_KB; c0 += 16) {
    double g[16];
#pragma unroll
    for (int u = 0; u < 16; u++) g[u] = 0.0;
#pragma unroll
    for (int sl = 0; sl < BT_GS; sl++) {
      const double *src = G[blk] + ((size_t)sl * P + p) * BT_KB * BT_KB + (size_t)c0 * BT_KB + t;
#pragma unroll
      for (int u = 0; u < 16; u++) g[u] += src[(size_t)u * BT_KB];
    }
#pragma unroll
    for (int u = 0; u < 16; u++) {
      sG[c0 + u][t] = g[u];  // column c of G
      sT[t][c0 + u] = 0.0;
    }
  }
  __shared__ double stau[BT_KB];
  stau[t] = (t < kb) ? b.tau[blk][j0 + t] : 0.0;  // one load per lane instead of one memory round trip per column
  __syncthreads();
  for (int i = 0; i < kb; i++) {
    const double ti = stau[i];
    sg[t] = (t < i) ? sG[i][t] : 0.0;
    __syncthreads();
    if (t < i) {
      // row t of the triangle times G(0:i, i).  Full-length and unrolled: T(t, k) is still zero for k < t and for the
      // columns >= i not built yet, sg is zero from i on; the rolled loop over k = t .. i-1 was bound by the latency of
      // its two LDS reads per term (2016 dependent terms per block: 85 of the kernel's 100 us)
      double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
#pragma unroll
      for (int k = 0; k < BT_KB; k += 4) {
        acc0 += sT[t][k] * sg[k];
        acc1 += sT[t][k + 1] * sg[k + 1];
        acc2 += sT[t][k + 2] * sg[k + 2];
        acc3 += sT[t][k + 3] * sg[k + 3];
      }
      sT[t][i] = -ti * ((acc0 + acc1) + (acc2 + acc3));
    }
    if (t == i) sT[i][i] = ti;
    __syncthreads();
  }
  for (int c = 0; c < BT_KB; c++) Tp[(size_t)c * BT_KB + t] = sT[t][c];
}

struct EigWork : Workspace {
  std::vector<int64_t> asm_rows;  // eig_assemble_dev: the index list whose device copy is asm_rows_dev
  DevBuf<long long> asm_rows_dev;
  bool folded = false;      // the last batch formed Y = (X Q)^T beside the divide-and-conquer stage (bt_wy_fold_x)
  DevBuf<double> Y[MAXB];
  DevBuf<GemmTask> btslabR, btupdR;
  std::vector<GemmTask> h_btslabR, h_btupdR;
  DevBuf<double> A[MAXB], d[MAXB], e[MAXB], tau[MAXB], v[MAXB], pp[MAXB], dots[MAXB], Z[MAXB], rot[MAXB];
  DevBuf<double> Zs[MAXB], Ws[MAXB];  // selected solve: the wanted eigenvectors (n x nev, ld n) and eigenvalues, ascending
  DevBuf<int> selrank;
  DevBuf<int> sweeps[MAXB];
  DevBuf<int> ibuf1, ibuf2;
  DevBuf<GemmTask> gtasks, bttasks, btslab, btgram, btcpl, btupd;
  std::vector<GemmTask> h_gtasks, h_bttasks, h_btslab, h_btgram, h_btcpl, h_btupd;  // host copies (upload_cached)
  std::vector<double *> h_btptr;
  DevBuf<double> Vx[MAXB], G[MAXB], T[MAXB], VT[MAXB], Wb[MAXB], Wp[MAXB], Cc[MAXB];
  DevBuf<double *> btptr;
  bool used_dc = true;
  // block row / column index lists of the last eig_blocks_dev call, and what they were derived from (hfg_ctx_fix_sinvh)
  DevBuf<double> idx;  // raw storage for int64 rows + cols
  const double *sup_S = nullptr;
  unsigned long sup_gen = 0;
  int sup_N = 0;
  std::vector<int64_t> sup_ptr, sup_idx;
  // the blocks' X = Sinvh(rows, cols), block ib (n x n, ld n) at offset sum_{b < ib} n_b^2, gathered once while the lists above
  // are valid (so only under hfg_ctx_fix_sinvh); xc_have[ib]: block ib has been gathered.  Cleared with the lists.
  DevBuf<double> Xc;
  std::vector<char> xc_have;
  // the declared radial-element pattern of F (hfg_ctx_declare_fock_band) as applied to the lists above (eig_band_plan.h),
  // derived with them.  band_rows: the caller's index list with every block ordered radial-major (empty: no declaration in
  // force) -- the ROWS of the gathered F under the pattern; its columns, X and everything downstream keep the caller's order.
  // band_pos[blk_ptr[ib] + i]: position in block ib of its radial-major row i (where row i of F X is stored).  band_ks: the k
  // steps of all row tiles, tile t of block ib at band_ks[band_koff[band_toff[ib] + t] ...).
  std::vector<int64_t> band_rows, band_pos;
  std::vector<int> band_ks, band_koff, band_toff;
  bool band_any = false;  // some block takes the row tasks
  DevBuf<long long> band_rows_dev, band_pos_dev;
  DevBuf<int> band_ks_dev, band_iota_dev;
  DevBuf<GemmTask> fxtasks;
  std::vector<GemmTask> h_fxtasks;
  // one-call entries: the divide-and-conquer status word is copied home behind that stage and waited for through the event,
  // so that the host returns while the last product is still running
  int *h_status = nullptr;
  hipEvent_t status_ev = nullptr;
  ~EigWork() {
    if (h_status) (void)hipHostFree(h_status);
    if (status_ev) (void)hipEventDestroy(status_ev);
  }
};
static EigWork &work_for(hfg_ctx *ctx) { return ctx->work.get<EigWork>(WS_EIG); }

/// Eigen-decomposition of nblk symmetric matrices already in w.A[blk] (n x n); eigenvalues end up in
/// w.d[blk] (unsorted), eigenvectors in w.Z[blk].
// (1) buffers and task lists (host work + one stream synchronisation: done before the tridiagonalisation is queued),
// (2) the part that needs only the reflectors -- explicit V, Gram matrices, T, V T -- queued on the context's side
//     stream so that it runs beside the divide-and-conquer stage (which keeps few CUs busy),
// (3) the sweep over the reflector blocks on the main stream.
// up to 16 short vectors copied by ONE launch (eigenvalues into / out of the block slots: a device-to-device
// hipMemcpyAsync costs 15-20 us of stream time each, seven of them 0.13 ms per step)
struct CopySlices {
  const double *src[16];
  double *dst[16];
  int n[16];
};
__global__ void k_copy_slices(CopySlices c) {
  const int q = blockIdx.y;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < c.n[q]; i += gridDim.x * blockDim.x) c.dst[q][i] = c.src[q][i];
}
/// The eigenvalues of `count` blocks to where they are read next: src(q), dst(q) and n(q) give block q's vector, its place
/// and its length.  The one builder of the copy lists: the direct path, the block slots and eig_assemble_dev differ in
/// their rules only.
template <class Src, class Dst, class Len>
static void publish_values(hipStream_t s, int count, Src src, Dst dst, Len n) {
  for (int q0 = 0; q0 < count; q0 += 16) {
    CopySlices c{};
    const int m = std::min(16, count - q0);
    int nmax = 0;
    for (int q = 0; q < m; q++) {
      c.src[q] = src(q0 + q);
      c.dst[q] = dst(q0 + q);
      c.n[q] = n(q0 + q);
      nmax = std::max(nmax, c.n[q]);
    }
    if (nmax > 0) hipLaunchKernelGGL(k_copy_slices, dim3((nmax + 255) / 256, m), dim3(256), 0, s, c);
  }
}

// Y = X^T for every matrix of the batch (64 x 64 blocks through LDS)
struct TrPtrs {
  const double *src[MAXB];
  double *dst[MAXB];
  int n[MAXB];
};
__global__ __launch_bounds__(256) void k_transpose_batch(TrPtrs t) {
  __shared__ double tile[64][65];
  const int blk = blockIdx.z, n = t.n[blk];
  const int bi = blockIdx.x * 64, bj = blockIdx.y * 64;
  if (bi >= n || bj >= n) return;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int c = ty; c < 64; c += 4) {
    const int gm = bi + tx, gn = bj + c;
    tile[c][tx] = (gm < n && gn < n) ? t.src[blk][(size_t)gn * n + gm] : 0.0;
  }
  __syncthreads();
  for (int c = ty; c < 64; c += 4) {
    const int gm = bj + tx, gn = bi + c;  // dst(gm, gn) = src(gn, gm)
    if (gm < n && gn < n) t.dst[blk][(size_t)gn * n + gm] = tile[tx][c];
  }
}

/// b.nz: the columns of b.Z that the left application (bt_wy_apply) works on
static void bt_wy_setup(hfg_ctx *ctx, EigWork &w, const EigBatch &b, int nblk, const int *ns, int nmax, bool fold = false) {
  hipStream_t s = ctx->stream;
  const int P = (nmax - 3) / BT_KB + 1;  // reflector blocks of the largest matrix
  const int NP = (P + 1) / 2;            // pairs of blocks, applied together (k_bt_wpair)
  constexpr int BT_S = 6;                // split-K slabs of the skinny product S = [V_p | V_p+1]^T Z
  std::vector<double *> ptrs(6 * (size_t)nblk);
  for (int k = 0; k < nblk; k++) {
    const int n = ns[k];
    w.Vx[k].resize((size_t)n * n);
    w.G[k].resize((size_t)BT_GS * P * BT_KB * BT_KB);
    w.T[k].resize((size_t)P * BT_KB * BT_KB);
    w.VT[k].resize((size_t)n * P * BT_KB);
    w.Wb[k].resize((size_t)BT_PW * n);
    w.Wp[k].resize((size_t)BT_S * BT_PW * n);
    w.Cc[k].resize((size_t)BT_GS * NP * BT_KB * BT_KB);
    ptrs[k] = w.Vx[k].p;
    ptrs[nblk + k] = w.G[k].p;
    ptrs[2 * nblk + k] = w.T[k].p;
    ptrs[3 * nblk + k] = w.Wp[k].p;
    ptrs[4 * nblk + k] = w.Wb[k].p;
    ptrs[5 * nblk + k] = w.Cc[k].p;
  }
  upload_cached(w.btptr, w.h_btptr, ptrs, s);
  GemmTask none;  // inactive
  none.A = none.B = nullptr;
  none.C = nullptr;
  none.M = none.N = none.K = 0;
  none.lda = none.ldb = none.ldc = 1;
  auto kb_of = [&](int k, int p) { return std::max(0, std::min(BT_KB, ns[k] - 2 - p * BT_KB)); };
  auto chunk_of = [](int len, int parts) { return ((len + parts - 1) / parts + 15) / 16 * 16; };

  // ---- per block p: Gram products (split over BT_GS row slabs) and VT = V T.  The VT columns of an odd block are
  //      formed from the first row of its PAIR on (V is zero there), so that [VT_p | VT_p+1] is one operand ----
  std::vector<GemmTask> gram((size_t)BT_GS * P * nblk, none), vt((size_t)P * nblk, none);
  for (int p = 0; p < P; p++)
    for (int k = 0; k < nblk; k++) {
      const int n = ns[k], j0 = p * BT_KB, kb = kb_of(k, p);
      if (kb <= 0) continue;
      const int r0 = j0 + 1, mr = n - r0;  // first row where the block's reflectors are non-zero
      const double *Vp = w.Vx[k].p + (size_t)j0 * n + r0;
      const int chunk = chunk_of(mr, BT_GS);
      for (int sl = 0; sl < BT_GS; sl++) {
        GemmTask g = none;
        const int k0 = sl * chunk, kk = std::max(0, std::min(chunk, mr - k0));
        g.A = g.B = Vp + (kk > 0 ? k0 : 0);
        g.C = w.G[k].p + ((size_t)sl * P + p) * BT_KB * BT_KB;
        g.tA = 1;
        g.M = g.N = kb;
        g.K = kk;  // K = 0 writes zeros
        g.lda = g.ldb = n;
        g.ldc = BT_KB;
        gram[((size_t)sl * P + p) * nblk + k] = g;
      }
      const int rp = (p & ~1) * BT_KB + 1;  // first row of the pair
      GemmTask g = none;
      g.A = w.Vx[k].p + (size_t)j0 * n + rp;
      g.B = w.T[k].p + (size_t)p * BT_KB * BT_KB;
      g.C = w.VT[k].p + (size_t)j0 * n + rp;
      g.M = n - rp;
      g.N = g.K = kb;
      g.lda = n;
      g.ldb = BT_KB;
      g.ldc = n;
      vt[(size_t)p * nblk + k] = g;
    }
  upload_cached(w.btgram, w.h_btgram, gram, s);
  upload_cached(w.bttasks, w.h_bttasks, vt, s);

  // ---- per pair: coupling C = V_p^T VT_p+1 (split over BT_GS slabs), S = [V_p | V_p+1]^T Z (BT_S slabs), the update ----
  std::vector<GemmTask> cpl((size_t)BT_GS * NP * nblk, none), slab((size_t)NP * BT_S * nblk, none), upd((size_t)NP * nblk, none);
  for (int g2 = 0; g2 < NP; g2++)
    for (int k = 0; k < nblk; k++) {
      const int n = ns[k], p0 = 2 * g2, j0 = p0 * BT_KB;
      const int kb0 = kb_of(k, p0), kb1 = (p0 + 1 < P) ? kb_of(k, p0 + 1) : 0;
      if (kb0 <= 0) continue;
      const int r0 = j0 + 1, mr = n - r0, kbp = kb0 + kb1;
      if (kb1 > 0) {
        const int r1 = j0 + BT_KB + 1, m1 = n - r1;  // rows where V_p+1 (and VT_p+1) are non-zero
        const int chunk = chunk_of(m1, BT_GS);
        for (int sl = 0; sl < BT_GS; sl++) {
          GemmTask c = none;
          const int k0 = sl * chunk, kk = std::max(0, std::min(chunk, m1 - k0));
          c.A = w.Vx[k].p + (size_t)j0 * n + r1 + (kk > 0 ? k0 : 0);
          c.B = w.VT[k].p + (size_t)(j0 + BT_KB) * n + r1 + (kk > 0 ? k0 : 0);
          c.C = w.Cc[k].p + ((size_t)sl * NP + g2) * BT_KB * BT_KB;
          c.tA = 1;
          c.M = kb0;
          c.N = kb1;
          c.K = kk;
          c.lda = c.ldb = n;
          c.ldc = BT_KB;
          cpl[((size_t)sl * NP + g2) * nblk + k] = c;
        }
      }
      const int chunk = chunk_of(mr, BT_S);
      for (int sl = 0; sl < BT_S; sl++) {
        GemmTask q = none;
        const int k0 = sl * chunk, kk = std::max(0, std::min(chunk, mr - k0));
        q.A = w.Vx[k].p + (size_t)j0 * n + r0 + (kk > 0 ? k0 : 0);
        q.B = b.Z[k] + r0 + (kk > 0 ? k0 : 0);
        q.C = w.Wp[k].p + (size_t)sl * BT_PW * n;
        q.tA = 1;
        q.M = kbp;
        q.N = b.nz[k];
        q.K = kk;  // empty slab: K = 0 writes zeros
        q.lda = q.ldb = n;
        q.ldc = BT_PW;
        slab[((size_t)g2 * BT_S + sl) * nblk + k] = q;
      }
      GemmTask u = none;
      u.A = w.VT[k].p + (size_t)j0 * n + r0;
      u.B = w.Wb[k].p;
      u.C = b.Z[k] + r0;
      u.M = mr;
      u.N = b.nz[k];
      u.K = kbp;
      u.lda = n;
      u.ldb = BT_PW;
      u.ldc = n;
      u.alpha = -1.0;
      u.beta = 1.0;
      upd[(size_t)g2 * nblk + k] = u;
    }
  upload_cached(w.btcpl, w.h_btcpl, cpl, s);
  upload_cached(w.btslab, w.h_btslab, slab, s);
  upload_cached(w.btupd, w.h_btupd, upd, s);
  if (fold) {
    // ---- the same pairs applied from the RIGHT to X, worked on Y = X^T (eig_blocks_dev: C = (X Q) Z):
    //   X Q_p Q_p+1 = X - B0 V_p^T - (B1 - B0 C) V_p+1^T,  B = X [VT_p | VT_p+1]   <=>
    //   Y <- Y - [V_p | V_p+1] [W0; W1],  W0 = VT_p^T Y,  W1 = VT_p+1^T Y - C^T W0
    // i.e. the tasks above with V and VT exchanged, on Y, pairs first to last; needs only the reflectors, not Z ----
    std::vector<GemmTask> slabR((size_t)NP * BT_S * nblk, none), updR((size_t)NP * nblk, none);
    for (int g2 = 0; g2 < NP; g2++)
      for (int k = 0; k < nblk; k++) {
        const int n = ns[k], p0 = 2 * g2, j0 = p0 * BT_KB;
        const int kb0 = kb_of(k, p0), kb1 = (p0 + 1 < P) ? kb_of(k, p0 + 1) : 0;
        if (kb0 <= 0) continue;
        const int r0 = j0 + 1, mr = n - r0, kbp = kb0 + kb1;
        const int chunk = chunk_of(mr, BT_S);
        for (int sl = 0; sl < BT_S; sl++) {
          GemmTask q = none;
          const int k0 = sl * chunk, kk = std::max(0, std::min(chunk, mr - k0));
          q.A = w.VT[k].p + (size_t)j0 * n + r0 + (kk > 0 ? k0 : 0);
          q.B = w.Y[k].p + r0 + (kk > 0 ? k0 : 0);
          q.C = w.Wp[k].p + (size_t)sl * BT_PW * n;
          q.tA = 1;
          q.M = kbp;
          q.N = n;
          q.K = kk;
          q.lda = q.ldb = n;
          q.ldc = BT_PW;
          slabR[((size_t)g2 * BT_S + sl) * nblk + k] = q;
        }
        GemmTask u = none;
        u.A = w.Vx[k].p + (size_t)j0 * n + r0;
        u.B = w.Wb[k].p;
        u.C = w.Y[k].p + r0;
        u.M = mr;
        u.N = n;
        u.K = kbp;
        u.lda = n;
        u.ldb = BT_PW;
        u.ldc = n;
        u.alpha = -1.0;
        u.beta = 1.0;
        updR[(size_t)g2 * nblk + k] = u;
      }
    upload_cached(w.btslabR, w.h_btslabR, slabR, s);
    upload_cached(w.btupdR, w.h_btupdR, updR, s);
  }
}

static void bt_wy_prepare(hfg_ctx *ctx, EigWork &w, const EigBatch &b, int nblk, int nmax, bool on_side = false) {
  const int P = (nmax - 3) / BT_KB + 1;
  // HELFEM_BT_SIDE=1 queues this part on a second stream beside the divide-and-conquer stage.  Measured: the 0.25 ms it
  // hides are outweighed by what a second live stream costs every launch on the framework's null stream (the
  // tridiagonalisation alone went from 17.4 to 19.1 ms), so the default keeps everything on the context's stream.
  // (Round 3: with X Q folded beside the divide-and-conquer stage -- bt_wy_fold_x, which needs these operands -- the set-up
  // goes to the side stream with it; the launch chain whose launches a second stream slowed is no longer the default.)
  const bool use_side = (tuning().bt_side && !ctx->avoid_side) || on_side;
  hipStream_t main = ctx->stream, q = main;
  const bool prof = ctx->profiling;
  if (use_side) {
    q = ctx->side();
    HFG_HIP_CHECK(hipEventRecord(ctx->side_ev[0], main));  // reflectors and tau are complete
    HFG_HIP_CHECK(hipStreamWaitEvent(q, ctx->side_ev[0], 0));
    ctx->profiling = false;  // the profiling brackets are events of the main stream
    ctx->stream = q;
  }
  try {
    double *const *dptr = w.btptr.p;
    hipLaunchKernelGGL(k_bt_extract, dim3((nmax + 255) / 256, nmax, nblk), dim3(256), 0, q, b, dptr);
    gemm_tasklist_dev(ctx, w.btgram.p, BT_GS * P * nblk, BT_KB, BT_KB, {GemmTile::T64});
    hipLaunchKernelGGL(k_bt_T, dim3(P, nblk), dim3(BT_KB), 0, q, b, dptr + nblk, dptr + 2 * nblk, P);
    gemm_tasklist_dev(ctx, w.bttasks.p, P * nblk, nmax, BT_KB, {GemmTile::T64});
    gemm_tasklist_dev(ctx, w.btcpl.p, BT_GS * ((P + 1) / 2) * nblk, BT_KB, BT_KB, {GemmTile::T64});
  } catch (...) {
    ctx->stream = main;
    ctx->profiling = prof;
    throw;
  }
  ctx->stream = main;
  ctx->profiling = prof;
  if (use_side) HFG_HIP_CHECK(hipEventRecord(ctx->side_ev[1], q));
}

static void bt_wy_apply(hfg_ctx *ctx, EigWork &w, const EigBatch &b, int nblk, int nmax) {
  hipStream_t s = ctx->stream;
  const int P = (nmax - 3) / BT_KB + 1, NP = (P + 1) / 2;
  constexpr int BT_S = 6;
  double *const *dptr = w.btptr.p;
  if (tuning().bt_side && !ctx->avoid_side) HFG_HIP_CHECK(hipStreamWaitEvent(s, ctx->side_ev[1], 0));  // (not reached when X Q was folded)
  // pairs of reflector blocks, last to first: three launches and one read-modify-write of Z per 128 reflectors
  for (int g = NP - 1; g >= 0; g--) {
    gemm_tasklist_dev(ctx, w.btslab.p + (size_t)g * BT_S * nblk, BT_S * nblk, BT_PW, nmax, {GemmTile::T64});
    // (summing the slabs inside the update's operand loads instead was measured: 2.73 -> 3.11 ms, six times the operand
    // traffic on every tile's critical path)
    hipLaunchKernelGGL(k_bt_wpair, dim3((nmax + 4 * BT_WREP - 1) / (4 * BT_WREP), nblk), dim3(256), 0, s, b, dptr + 3 * nblk, dptr + 4 * nblk,
                       dptr + 5 * nblk, BT_S, BT_GS, NP, g, 0);
    gemm_tasklist_dev(ctx, w.btupd.p + (size_t)g * nblk, nblk, nmax, nmax, {tuning().acc_tile != 128 ? GemmTile::T64 : GemmTile::T128, /*acc*/ true});
  }
  HFG_HIP_CHECK(hipGetLastError());
}

// X Q on the side stream, beside the divide-and-conquer stage (which needs d and e only and keeps few CUs busy):
// the compact-WY set-up (bt_wy_prepare, same stream), Y = X^T, then the pairs of reflector blocks first to last.
// side_ev[0]: reflectors and tau are complete (main stream); side_ev[1]: Y = (X Q)^T is complete.
static void bt_wy_fold_x(hfg_ctx *ctx, EigWork &w, const EigBatch &b, int nblk, const int *ns, int nmax, const double *const *X) {
  const int P = (nmax - 3) / BT_KB + 1, NP = (P + 1) / 2;
  constexpr int BT_S = 6;
  hipStream_t main = ctx->stream, q = ctx->side();  // (bt_wy_prepare ran on q behind the tridiagonalisation: stream order)
  const bool prof = ctx->profiling;
  ctx->profiling = false;  // the profiling brackets are events of the main stream
  ctx->stream = q;
  try {
    TrPtrs t;
    for (int k = 0; k < MAXB; k++) {
      t.src[k] = k < nblk ? X[k] : nullptr;
      t.dst[k] = k < nblk ? w.Y[k].p : nullptr;
      t.n[k] = k < nblk ? ns[k] : 0;
    }
    hipLaunchKernelGGL(k_transpose_batch, dim3((nmax + 63) / 64, (nmax + 63) / 64, nblk), dim3(256), 0, q, t);
    double *const *dptr = w.btptr.p;
    for (int g = 0; g < NP; g++) {
      gemm_tasklist_dev(ctx, w.btslabR.p + (size_t)g * BT_S * nblk, BT_S * nblk, BT_PW, nmax, {GemmTile::T64});
      hipLaunchKernelGGL(k_bt_wpair, dim3((nmax + 4 * BT_WREP - 1) / (4 * BT_WREP), nblk), dim3(256), 0, q, b, dptr + 3 * nblk, dptr + 4 * nblk,
                         dptr + 5 * nblk, BT_S, BT_GS, NP, g, 1);
      gemm_tasklist_dev(ctx, w.btupdR.p + (size_t)g * nblk, nblk, nmax, nmax, {GemmTile::T64, /*acc*/ true});
    }
  } catch (...) {
    ctx->stream = main;
    ctx->profiling = prof;
    throw;
  }
  ctx->stream = main;
  ctx->profiling = prof;
  HFG_HIP_CHECK(hipGetLastError());
  HFG_HIP_CHECK(hipEventRecord(ctx->side_ev[1], q));
}

/// foldX != nullptr (device pointers of the blocks' X, n x n, ld n): the caller wants C = X Q Z; then X Q is formed beside
/// the divide-and-conquer stage (w.Y = (X Q)^T, w.folded = true), w.Z keeps the tridiagonal matrix's eigenvectors and
/// the caller multiplies Y^T Z.  Otherwise (and when the compact-WY path does not apply) Z <- Q Z as before.
/// nev != nullptr (1 <= nev[i] <= ns[i]): the lowest nev[i] eigenpairs only, eigenvalues ascending in w.Ws[i], eigenvectors
/// in w.Zs[i] (n x nev[i], ld n) in place of w.d and w.Z.  Two paths, chosen by eigsel_takes_stein: multisection and inverse
/// iteration (stsel.hip), or the full tridiagonal solve followed by taking the lowest columns; the back-transformation
/// works on the nev[i] columns in either.
// Crossover of the selected solve: multisection and inverse iteration cost O(nev n) per block, all of it in serial chains
// of about seven passes over n per vector; divide and conquer costs O(n^2) to O(n^3) whatever nev is.  The first value
// from those counts was 1/8 of the columns.  Measured (n = 1470): the two curves do not meet, stein is
// slower at 1/64, 1/16, 1/4 and 1/2 of the columns (8.8 ms against 0.73 ms at 1/64: dstein's clusters run their members one
// after the other), so the crossover is 0 and sends every fraction to dc.  HELFEM_EIGSEL forces either path.
constexpr double EIGSEL_CROSS = 0.0;  // stein where sum nev_b <= EIGSEL_CROSS sum n_b
static bool eigsel_takes_stein(int nblk, const int *ns, const int *nev) {
  const helfem::EigSel how = tuning().eigsel;
  if (how != helfem::EigSel::crossover) return how == helfem::EigSel::stein;
  long want = 0, all = 0;
  for (int i = 0; i < nblk; i++) {
    want += nev[i];
    all += ns[i];
  }
  return (double)want <= EIGSEL_CROSS * (double)all;
}
/// after_solve: queued on the main stream as soon as the eigenvalues (w.d, or w.Ws of a selected solve) are final, ahead of
/// the back-transformation or of the wait for X Q
static void eig_sym_batch(hfg_ctx *ctx, EigWork &w, int nblk, const int *ns, const double *const *foldX = nullptr,
                          const int *nev = nullptr, const std::function<void()> &after_solve = nullptr) {
  EigBatch b;
  b.nblk = nblk;
  int nmax = 0, nzmax = 0;
  const bool stein = nev && eigsel_takes_stein(nblk, ns, nev);
  for (int i = 0; i < nblk; i++) {
    int n = ns[i];
    nmax = std::max(nmax, n);
    b.n[i] = n;
    b.nz[i] = nev ? nev[i] : n;
    nzmax = std::max(nzmax, b.nz[i]);
    if (nev) {
      if (nev[i] < 1 || nev[i] > n) throw std::logic_error("eig_sym_batch: 1 <= nev <= n violated\n");
      w.Zs[i].resize((size_t)n * nev[i]);
      w.Ws[i].resize(nev[i]);
    }
    w.d[i].resize(n);
    w.e[i].resize(n);
    w.tau[i].resize(n);
    w.v[i].resize(n);
    w.pp[i].resize((size_t)TRD_NCS * n);
    w.dots[i].resize((size_t)TRD_NCS * ((n + 63) / 64) + 8);
    if (!stein) w.Z[i].resize((size_t)n * n);
    long cap = 3L * n * n + 1024;
    w.rot[i].resize(2 * (size_t)cap);
    w.sweeps[i].resize((size_t)4 * 64 * n + 8);
    b.rotcap[i] = cap;
    b.A[i] = w.A[i].p;
    b.d[i] = w.d[i].p;
    b.e[i] = w.e[i].p;
    b.tau[i] = w.tau[i].p;
    b.v[i] = w.v[i].p;
    b.pp[i] = w.pp[i].p;
    b.dots[i] = w.dots[i].p;
    b.Z[i] = stein ? nullptr : w.Z[i].p;  // (the tridiagonal stage's output; a selected solve continues on w.Zs below)
    b.rot[i] = w.rot[i].p;
    b.sweeps[i] = w.sweeps[i].p;
  }
  hipStream_t s = ctx->stream;
  const bool bt_wy = !tuning().bt_column && nmax >= 4 * BT_KB;
  if (tridiagonalize_takes_chain(nblk, ns)) {  // thousands of dependent launches ahead: no second stream beside them
    ctx->avoid_side = true;
    ctx->drop_side();
  }
  const bool fold = bt_wy && foldX != nullptr && tuning().bt_fold && !ctx->avoid_side;
  w.folded = fold;
  if (fold)
    for (int i = 0; i < nblk; i++) w.Y[i].resize((size_t)ns[i] * ns[i]);
  EigBatch bz = b;  // the batch as the back-transformation sees it: Z = the wanted columns
  if (nev)
    for (int i = 0; i < nblk; i++) bz.Z[i] = w.Zs[i].p;
  if (bt_wy) bt_wy_setup(ctx, w, bz, nblk, ns, nmax, fold);
  {
    ProfScope ps(ctx, "eig_tridiag");
    if (tuning().trd_mode == TrdMode::unblocked) {
      // first-generation path (rank-2 update of the whole trailing matrix at every column), kept for A/B runs
      size_t shb = (size_t)(nmax + 4 * 64 + 8) * sizeof(double);
      if (shb > 64 * 1024)
        HFG_HIP_CHECK(hipFuncSetAttribute((const void *)k_trd_gemv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shb));
      for (int k = 0; k <= nmax - 3; k++) {
        int m = nmax - k - 1;
        int nrs = (m + 63) / 64;
        hipLaunchKernelGGL(k_trd_gemv, dim3(nrs * TRD_NCS, nblk), dim3(256), shb, s, b, k);
        hipLaunchKernelGGL(k_trd_update, dim3(nrs * nrs, nblk), dim3(256), 0, s, b, k);
      }
      hipLaunchKernelGGL(k_trd_finish, dim3(nblk), dim3(64), 0, s, b);
    } else {
      double *Ap[MAXB], *dp[MAXB], *ep[MAXB], *tp[MAXB];
      for (int i = 0; i < nblk; i++) {
        Ap[i] = w.A[i].p;
        dp[i] = w.d[i].p;
        ep[i] = w.e[i].p;
        tp[i] = w.tau[i].p;
      }
      tridiagonalize_batch(ctx, nblk, ns, Ap, dp, ep, tp);
    }
  }
  if (bt_wy) bt_wy_prepare(ctx, w, b, nblk, nmax, fold);
  if (fold) bt_wy_fold_x(ctx, w, b, nblk, ns, nmax, foldX);
  if (stein) {
    ProfScope ps(ctx, "eig_tridiag_sel");
    w.used_dc = true;  // the status word of this path is the divide-and-conquer stage's
    double *dp[MAXB], *ep[MAXB], *wp[MAXB], *zp[MAXB];
    for (int i = 0; i < nblk; i++) {
      dp[i] = w.d[i].p;
      ep[i] = w.e[i].p;
      wp[i] = w.Ws[i].p;
      zp[i] = w.Zs[i].p;
    }
    tridiag_sel_batch(ctx, nblk, ns, nev, dp, ep, wp, zp);
  } else {
    ProfScope ps(ctx, "eig_tridiag_solve");
    w.used_dc = !tuning().tridiag_ql;
    if (!w.used_dc) {
      // reference implementation kept for cross-checks: implicit QL by one lane, rotations logged then applied
      hipLaunchKernelGGL(k_set_identity, dim3((nmax + 255) / 256, nmax, nblk), dim3(256), 0, s, b);
      hipLaunchKernelGGL(k_tql_values, dim3(nblk), dim3(64), 0, s, b);
      hipLaunchKernelGGL(k_tql_apply, dim3((nmax + 63) / 64, nblk), dim3(64), 0, s, b);
    } else {
      double *dp[MAXB], *ep[MAXB], *zp[MAXB];
      for (int i = 0; i < nblk; i++) {
        dp[i] = w.d[i].p;
        ep[i] = w.e[i].p;
        zp[i] = w.Z[i].p;
      }
      tridiag_dc_batch(ctx, nblk, ns, dp, ep, zp);
    }
    if (nev) {  // the lowest columns of the full solve, in ascending order
      size_t off = 0;
      for (int i = 0; i < nblk; i++) off += ns[i] + 8;
      w.selrank.resize(off);
      off = 0;
      for (int i = 0; i < nblk; i++) {
        launch_rank(ctx, w.d[i].p, ns[i], w.selrank.p + off);
        hipLaunchKernelGGL(k_take_lowest, dim3((ns[i] + 255) / 256, ns[i]), dim3(256), 0, s, w.Z[i].p, w.d[i].p, ns[i], nev[i],
                           w.selrank.p + off, w.Zs[i].p, w.Ws[i].p);
        off += ns[i] + 8;
      }
    }
  }
  if (after_solve) after_solve();
  {
    ProfScope ps(ctx, "eig_backtransform");
    if (fold) {
      HFG_HIP_CHECK(hipStreamWaitEvent(s, ctx->side_ev[1], 0));  // Y = (X Q)^T is complete
    } else if (bt_wy) {
      bt_wy_apply(ctx, w, bz, nblk, nmax);
    } else {
    dim3 grid((nzmax + 3) / 4, nblk);
    if (nmax <= 64 * 8)
      hipLaunchKernelGGL(k_backtransform<8>, grid, dim3(256), 0, s, bz);
    else if (nmax <= 64 * 24)
      hipLaunchKernelGGL(k_backtransform<24>, grid, dim3(256), 0, s, bz);
    else {
      size_t shb = (size_t)4 * nmax * sizeof(double);
      if (shb > 64 * 1024)
        HFG_HIP_CHECK(
            hipFuncSetAttribute((const void *)k_backtransform_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shb));
      hipLaunchKernelGGL(k_backtransform_lds, grid, dim3(256), shb, s, bz);
    }
    }
  }
  HFG_HIP_CHECK(hipGetLastError());
}

static void check_status(hfg_ctx *ctx, EigWork &w, int nblk) {
  if (w.used_dc) {
    if (dc_status(ctx) != 0) throw std::logic_error("Eigendecomposition failed!\n");
    trdp_check_status(ctx);  // the stream has just been synchronised: the status word of a persistent launch is home
    return;
  }
  for (int i = 0; i < nblk; i++) {
    int st[2];
    HFG_HIP_CHECK(hipMemcpyAsync(st, w.sweeps[i].p, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HFG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (st[1] != 0) throw std::logic_error("Eigendecomposition failed!\n");
  }
}

// E (n), C (n x n) <- eig_sym(A) ; all device pointers
void eig_sym_dev(hfg_ctx *ctx, int n, const double *dA, double *dE, double *dC) {
  EigWork &w = work_for(ctx);
  w.A[0].resize((size_t)n * n + 2);
  HFG_HIP_CHECK(hipMemcpyAsync(w.A[0].p, dA, sizeof(double) * n * n, hipMemcpyDeviceToDevice, ctx->stream));
  eig_sym_batch(ctx, w, 1, &n);
  DevBuf<int> &rank = w.ibuf1;
  rank.resize(n + 8);
  launch_rank(ctx, w.d[0].p, n, rank.p);
  hipLaunchKernelGGL(k_scatter_cols, dim3((n + 255) / 256, n), dim3(256), 0, ctx->stream, w.Z[0].p, n, n,
                     (const int64_t *)nullptr, rank.p, 0, w.d[0].p, n, dC, dE);
  check_status(ctx, w, 1);
}

// the lowest nev eigenpairs: E (nev, ascending), C (n x nev) ; all device pointers
void eig_sym_sel_dev(hfg_ctx *ctx, int n, const double *dA, int nev, double *dE, double *dC) {
  if (nev < 1) throw std::logic_error("eig_sym_sel: nev must be at least 1\n");
  if (n < 1) throw std::logic_error("eig_sym_sel: empty matrix\n");
  nev = std::min(nev, n);
  EigWork &w = work_for(ctx);
  w.A[0].resize((size_t)n * n + 2);
  HFG_HIP_CHECK(hipMemcpyAsync(w.A[0].p, dA, sizeof(double) * n * n, hipMemcpyDeviceToDevice, ctx->stream));
  eig_sym_batch(ctx, w, 1, &n, nullptr, &nev);
  HFG_HIP_CHECK(hipMemcpyAsync(dC, w.Zs[0].p, sizeof(double) * (size_t)n * nev, hipMemcpyDeviceToDevice, ctx->stream));
  HFG_HIP_CHECK(hipMemcpyAsync(dE, w.Ws[0].p, sizeof(double) * nev, hipMemcpyDeviceToDevice, ctx->stream));
  check_status(ctx, w, 1);
}

// scf::eig_gsym: F N x N, Sinvh N x n  ->  E (n), C (N x n)
void eig_gsym_dev(hfg_ctx *ctx, int N, int n, const double *dF, const double *dS, double *dE, double *dC) {
  EigWork &w = work_for(ctx);
  w.A[0].resize((size_t)n * n + 2);
  DevBuf<double> &T1 = ctx->ws[0];
  DevBuf<double> &Ctmp = ctx->ws[1];
  T1.resize((size_t)N * n);
  Ctmp.resize((size_t)N * n);
  {
    ProfScope ps(ctx, "eig_reduce");
    gemm_dev(ctx, false, false, N, n, N, 1.0, dF, N, dS, N, 0.0, T1.p, N);
    gemm_dev(ctx, true, false, n, n, N, 1.0, dS, N, T1.p, N, 0.0, w.A[0].p, n);
  }
  eig_sym_batch(ctx, w, 1, &n);
  {
    ProfScope ps(ctx, "eig_backtransform");
    gemm_dev(ctx, false, false, N, n, n, 1.0, dS, N, w.Z[0].p, n, 0.0, Ctmp.p, N);
  }
  DevBuf<int> &rank = w.ibuf1;
  rank.resize(n + 8);
  launch_rank(ctx, w.d[0].p, n, rank.p);
  hipLaunchKernelGGL(k_scatter_cols, dim3((N + 255) / 256, n), dim3(256), 0, ctx->stream, Ctmp.p, N, n,
                     (const int64_t *)nullptr, rank.p, 0, w.d[0].p, N, dC, dE);
  check_status(ctx, w, 1);
}

// scf::eig_gsym_sub, phase 1: the symmetry blocks owned by this shard (block ib belongs to rank ib % nranks).
// dBlockBuf: nblk slots of (nmax*nmax + nmax) doubles, slot ib = [C block (n x n, ld n) | pad | eigenvalues (n) at
// offset nmax*nmax]; slots of blocks owned by other ranks are zeroed so that a sum all-reduce over ranks
// completes the buffer.
size_t eig_block_buf_size(int nblk, const int64_t *blk_ptr) {
  const size_t nmax = helfem::eig_block_nmax(nblk, blk_ptr);
  return (size_t)nblk * (nmax * nmax + nmax);
}
int64_t eig_sel_count(int nblk, const int64_t *blk_ptr, int64_t nev) { return helfem::eig_sel_count(nblk, blk_ptr, nev); }

/// the switches of the product rules (host/eig_plan.h): this file reads them here and nowhere else
static helfem::EigSwitches eig_switches() {
  return {tuning().gemm_tile, tuning().gemm_splitk, tuning().gemm_rect, tuning().mfma_4x4x4};
}

// ---- the blocked driver, stage by stage (eig_blocks_multi_dev below calls them in this order) -------------------------------
/// Column supports of the symmetry blocks of a block-structured Sinvh (scf_helpers.cpp:150-157): cols[blk_ptr[ib] ...] = the
/// columns with support on block ib's rows, ascending.  Uploads blk_idx to drows (N values on the device) on the way; the
/// stream is drained on return.
static void block_supports(hfg_ctx *ctx, int N, const double *dS, int nblk, const int64_t *blk_ptr, const int64_t *blk_idx,
                           int64_t *drows, DevBuf<int> &flag, std::vector<int64_t> &cols) {
  hipStream_t s = ctx->stream;
  HFG_HIP_CHECK(hipMemcpyAsync(drows, blk_idx, sizeof(int64_t) * N, hipMemcpyHostToDevice, s));
  flag.resize((size_t)N * nblk + 8);
  for (int ib = 0; ib < nblk; ib++) {
    int n = (int)(blk_ptr[ib + 1] - blk_ptr[ib]);
    hipLaunchKernelGGL(k_col_support, dim3(N), dim3(256), 0, s, dS, N, drows + blk_ptr[ib], n, flag.p + (size_t)ib * N);
  }
  std::vector<int> hflag((size_t)N * nblk);
  HFG_HIP_CHECK(hipMemcpyAsync(hflag.data(), flag.p, sizeof(int) * hflag.size(), hipMemcpyDeviceToHost, s));
  HFG_HIP_CHECK(hipStreamSynchronize(s));
  cols.clear();
  for (int ib = 0; ib < nblk; ib++) {
    int cnt = 0;
    for (int c = 0; c < N; c++)
      if (hflag[(size_t)ib * N + c]) {
        cols.push_back(c);
        cnt++;
      }
    if (cnt != (int)(blk_ptr[ib + 1] - blk_ptr[ib]))
      throw std::logic_error("eig_gsym_sub: Sinvh is not block structured (columns with support != block size)\n");
  }
}

/// The declared pattern of F applied to these blocks (EigWork::band_*, eig_band_plan.h), and the lists' device copies
static void band_lists(hfg_ctx *ctx, EigWork &w, int N, int nblk, const int64_t *blk_ptr, const int64_t *blk_idx) {
  hipStream_t s = ctx->stream;
  w.band_rows.resize(N);
  w.band_pos.resize(N);
  std::vector<int> nd, ks, toff;
  int64_t nbig = 0;
  for (int ib = 0; ib < nblk; ib++) {
    const int64_t o = blk_ptr[ib], n = blk_ptr[ib + 1] - o;
    nbig = std::max(nbig, n);
    nd.resize(n);
    for (int64_t i = 0; i < n; i++) {
      if (blk_idx[o + i] < 0 || blk_idx[o + i] >= N) throw std::logic_error("eig_gsym_sub: block index out of range\n");
      nd[i] = ctx->band_node[blk_idx[o + i]];
    }
    helfem::eig_band_order(n, nd.data(), w.band_pos.data() + o);
    for (int64_t i = 0; i < n; i++) w.band_rows[o + i] = blk_idx[o + w.band_pos[o + i]];
    if (helfem::eig_band_plan(n, nd.data(), w.band_pos.data() + o, ctx->band_pm, ctx->band_E, ks, toff)) w.band_any = true;
    for (size_t t = 0; t + 1 < toff.size(); t++) w.band_koff.push_back((int)w.band_ks.size() + toff[t + 1]);
    w.band_ks.insert(w.band_ks.end(), ks.begin(), ks.end());
    w.band_toff.push_back((int)w.band_koff.size() - 1);
  }
  std::vector<int> iota(nbig);
  for (int64_t i = 0; i < nbig; i++) iota[i] = (int)i;
  w.band_rows_dev.resize(N);
  w.band_pos_dev.resize(N);
  w.band_ks_dev.resize(w.band_ks.size() + 1);
  w.band_iota_dev.resize(nbig);
  HFG_HIP_CHECK(hipMemcpyAsync(w.band_rows_dev.p, w.band_rows.data(), sizeof(int64_t) * N, hipMemcpyHostToDevice, s));
  HFG_HIP_CHECK(hipMemcpyAsync(w.band_pos_dev.p, w.band_pos.data(), sizeof(int64_t) * N, hipMemcpyHostToDevice, s));
  HFG_HIP_CHECK(hipMemcpyAsync(w.band_ks_dev.p, w.band_ks.data(), sizeof(int) * w.band_ks.size(), hipMemcpyHostToDevice, s));
  HFG_HIP_CHECK(hipMemcpyAsync(w.band_iota_dev.p, iota.data(), sizeof(int) * nbig, hipMemcpyHostToDevice, s));
  HFG_HIP_CHECK(hipStreamSynchronize(s));  // iota lives on this stack frame
}

/// The blocks' row and column index lists on the device (w.idx): drows = blk_idx, dcols = the column support of every block.
/// The supports depend on Sinvh and the blocks only: when the caller has declared Sinvh fixed (hfg_ctx_fix_sinvh) the lists
/// of the previous call, the band lists derived with them and the X cache are still good.
struct BlockLists {
  const int64_t *drows, *dcols;
};
static BlockLists block_lists(hfg_ctx *ctx, EigWork &w, int N, const double *dS, int nblk, const int64_t *blk_ptr, const int64_t *blk_idx) {
  hipStream_t s = ctx->stream;
  w.idx.resize(2 * (size_t)N + 16);
  int64_t *drows = (int64_t *)w.idx.p, *dcols = drows + N;
  // the declared pattern of F: valid beside the declared Sinvh only, ignored under HELFEM_EIG_BAND=0 (read at every call)
  const bool want_band = ctx->fixed_sinvh && ctx->fixed_sinvh == dS && ctx->band_state == 1 && ctx->band_node.size() == (size_t)N &&
                         helfem::tuning_live().eig_band;
  const bool cached = ctx->fixed_sinvh && ctx->fixed_sinvh == dS && w.sup_S == dS && w.sup_gen == ctx->fixed_gen &&
                      w.sup_N == N && want_band == !w.band_rows.empty() &&
                      w.sup_ptr.size() == (size_t)nblk + 1 && std::equal(w.sup_ptr.begin(), w.sup_ptr.end(), blk_ptr) &&
                      w.sup_idx.size() == (size_t)N && std::equal(w.sup_idx.begin(), w.sup_idx.end(), blk_idx);
  if (cached) return {drows, dcols};
  w.sup_S = nullptr;
  w.xc_have.clear();  // the gathered X blocks belong to the lists that go
  HFG_HIP_CHECK(hipStreamSynchronize(s));  // the band lists may still be the source of an earlier copy
  w.band_rows.clear();
  w.band_pos.clear();
  w.band_ks.clear();
  w.band_koff.assign(1, 0);
  w.band_toff.assign(1, 0);
  w.band_any = false;
  if (want_band) band_lists(ctx, w, N, nblk, blk_ptr, blk_idx);
  std::vector<int64_t> allcols;
  block_supports(ctx, N, dS, nblk, blk_ptr, blk_idx, drows, w.ibuf2, allcols);
  HFG_HIP_CHECK(hipMemcpyAsync(dcols, allcols.data(), sizeof(int64_t) * N, hipMemcpyHostToDevice, s));
  HFG_HIP_CHECK(hipStreamSynchronize(s));  // allcols lives on this stack frame
  if (ctx->fixed_sinvh == dS) {
    w.sup_S = dS;
    w.sup_gen = ctx->fixed_gen;
    w.sup_N = N;
    w.sup_ptr.assign(blk_ptr, blk_ptr + nblk + 1);
    w.sup_idx.assign(blk_idx, blk_idx + N);
  }
  return {drows, dcols};
}

/// One call of the driver: its arguments and what is derived from them once
struct BlocksCall {
  hfg_ctx *ctx;
  EigWork &w;
  int N, nF, nblk;
  const int64_t *blk_ptr;
  const double *const *dFs;
  const double *dS;
  double *const *dBlockBufs;  // the slot path's buffers, one per matrix
  int nev;
  double *const *dEs, *const *dCs;  // the direct path's outputs, one per matrix
  bool direct;
  BlockLists lists;
  size_t nmax, slot;    // order of the largest block, doubles of a block slot
  bool keep_x;          // X of every block stays in w.Xc, block ib at xoff[ib]
  const size_t *xoff;
  const int64_t *koff;  // block ib's values start at koff[ib] among the K of a matrix (eig_value_offsets)
  int K;
  int order(int ib) const { return (int)(blk_ptr[ib + 1] - blk_ptr[ib]); }
  // batch member k: its gathered F, its F X, its X when that is not cached
  double *Fk(int k) const { return ctx->ws[5].p + (size_t)k * nmax * nmax; }
  double *Tk(int k) const { return ctx->ws[0].p + (size_t)k * nmax * nmax; }
  double *Xk(int k) const { return ctx->ws[4].p + (size_t)k * nmax * nmax; }
  // direct: ranks and eigenvalues of matrix f
  int *rank(int f) const { return w.ibuf1.p + (size_t)f * (N + 8); }
  double *Etmp(int f) const { return ctx->ws[3].p + (size_t)f * N; }
};

/// One batch: at most MAXB (matrix, block) pairs, whose products and decompositions share their launches
struct EigChunk {
  int nb = 0, nm = 0;         // pairs, largest order among them
  int ib[MAXB], f[MAXB];      // block and matrix of pair k
  int ns[MAXB], nevs[MAXB];   // order, eigenpairs wanted
  const double *Xptr[MAXB];   // X = Sinvh(rows, cols) of the block
  helfem::EigProductPlan plan;
  helfem::EigLastProduct last;
  double *slot(const BlocksCall &c, int k) const { return c.dBlockBufs[f[k]] + (size_t)ib[k] * c.slot; }
  const double *values(const BlocksCall &c, int k) const { return c.nev > 0 ? c.w.Ws[k].p : c.w.d[k].p; }  // final behind the solve
};
/// items: nb entries matrix * nblk + block.  Sizes the batch's matrices in the workspace as well.
static EigChunk fill_chunk(const BlocksCall &c, const int *items, int nb) {
  EigWork &w = c.w;
  EigChunk b;
  b.nb = nb;
  for (int k = 0; k < nb; k++) {
    const int ib = items[k] % c.nblk, n = c.order(ib);
    b.ib[k] = ib;
    b.f[k] = items[k] / c.nblk;
    b.ns[k] = n;
    b.nevs[k] = c.nev > 0 ? std::min(c.nev, n) : n;
    b.nm = std::max(b.nm, n);
    w.A[k].resize((size_t)n * n + 2);  // + 2: the sweep's 16-byte row pairs may straddle the last element
    if (c.nev > 0) w.Zs[k].resize((size_t)n * b.nevs[k]);
    else w.Z[k].resize((size_t)n * n);
    w.Y[k].resize((size_t)n * n);
    b.Xptr[k] = c.keep_x ? w.Xc.p + c.xoff[ib] : c.Xk(k);
  }
  return b;
}

/// The three products of every block (F X, X^T (F X), X Z) go through one task-list launch each, so that the blocks fill
/// the chip together.  [k]: F X, [nb + k]: X^T (F X), [2 nb + k]: X Z, [3 nb + k]: the last product when X Q was folded
/// (eig_sym_batch): (X Q) Z = Y^T Z
static std::vector<GemmTask> build_tasks(const BlocksCall &c, const EigChunk &b) {
  EigWork &w = c.w;
  const int nb = b.nb;
  std::vector<GemmTask> gt(4 * (size_t)nb);
  for (int k = 0; k < nb; k++) {
    const int ib = b.ib[k], n = b.ns[k];
    double *Xb = const_cast<double *>(b.Xptr[k]);
    GemmTask g;
    g.M = g.N = g.K = n;
    g.lda = g.ldb = g.ldc = n;
    g.A = c.Fk(k);
    g.B = Xb;
    g.C = c.Tk(k);
    gt[k] = g;
    g.A = Xb;
    g.tA = 1;
    g.B = c.Tk(k);
    g.C = w.A[k].p;
    g.sym = 1;  // X^T (F X): the lower tiles are computed, the upper ones mirrored
    gt[nb + k] = g;
    g.sym = 0;
    g.tA = 0;
    g.A = Xb;
    g.B = c.nev > 0 ? w.Zs[k].p : w.Z[k].p;
    g.N = b.nevs[k];
    if (c.direct) {
      g.C = c.dCs[b.f[k]];
      g.ldc = c.N;
      g.rmap = c.lists.drows + c.blk_ptr[ib];
      g.cmap = c.rank(b.f[k]) + c.koff[ib];
    } else
      g.C = b.slot(c, k);
    gt[2 * nb + k] = g;
    g.A = w.Y[k].p;
    g.tA = 1;
    gt[3 * nb + k] = g;
  }
  return gt;
}

/// F X under the declared pattern: one task per 64 rows of F in radial-major ROW order (the gather of reduce_stage), its k
/// loop over the tile's step list alone, the rows stored at their places in the caller's order (rmap).  Columns of F, X and T
/// are in the caller's order, so T is bit for bit the dense product.  Once one block of the batch takes row tasks every
/// block does (a dense one with all steps), and the grid stays that of a 64-row product.  Longest lists first: the launch
/// hands out the tasks in order, the short ones fill the tail.  Empty: no pattern in force.
static std::vector<GemmTask> build_row_tasks(const BlocksCall &c, const EigChunk &b, const std::vector<GemmTask> &gt) {
  const EigWork &w = c.w;
  std::vector<GemmTask> fx;
  if (!(w.band_any && !w.band_rows.empty())) return fx;
  for (int k = 0; k < b.nb; k++) {
    const int ib = b.ib[k];
    const int n = b.ns[k], nt = w.band_toff[ib + 1] - w.band_toff[ib];
    for (int t = 0; t < nt; t++) {
      const int i0 = t * helfem::EIG_BAND_TILE, q = w.band_toff[ib] + t;
      GemmTask g = gt[k];
      g.A = gt[k].A + i0;
      g.M = std::min(helfem::EIG_BAND_TILE, n - i0);
      g.rmap = (const int64_t *)w.band_pos_dev.p + c.blk_ptr[ib] + i0;
      g.cmap = w.band_iota_dev.p;
      g.kstart = w.band_ks_dev.p + w.band_koff[q];
      g.nk = w.band_koff[q + 1] - w.band_koff[q];
      fx.push_back(g);
    }
  }
  std::stable_sort(fx.begin(), fx.end(), [](const GemmTask &a, const GemmTask &b) { return a.nk > b.nk; });
  return fx;
}

/// Forth = X^T (F X) of every pair of the batch into w.A: the gathers, the zeroing that the plan asks for, the two task-list
/// launches and the mirror.  nfx: row tasks in w.fxtasks.
static void reduce_stage(const BlocksCall &c, const EigChunk &b, int nfx) {
  hfg_ctx *ctx = c.ctx;
  EigWork &w = c.w;
  hipStream_t s = ctx->stream;
  const helfem::EigProductPlan &p = b.plan;
  const int nb = b.nb, nm = b.nm;
  const int64_t *drows = c.lists.drows, *dcols = c.lists.dcols;
  ProfScope ps(ctx, "eig_reduce");
  for (int k = 0; k < nb; k++) {
    const int ib = b.ib[k], n = b.ns[k];
    const double *dF = c.dFs[b.f[k]];
    double *Fk = c.Fk(k);
    if (!(c.keep_x && w.xc_have[ib]))
      hipLaunchKernelGGL(k_gather_block, dim3((n + 255) / 256, n), dim3(256), 0, s, dF, c.dS, c.N, drows + c.blk_ptr[ib],
                         dcols + c.blk_ptr[ib], n, Fk, const_cast<double *>(b.Xptr[k]));
    else if (!p.band_fx)
      hipLaunchKernelGGL(k_gather_f, dim3((n + 255) / 256, n), dim3(256), 0, s, dF, c.N, drows + c.blk_ptr[ib], n, Fk);
    if (p.band_fx)  // the rows of F radial-major, its columns in the caller's order
      hipLaunchKernelGGL(k_gather_f2, dim3((n + 255) / 256, n), dim3(256), 0, s, dF, c.N, (const int64_t *)w.band_rows_dev.p + c.blk_ptr[ib],
                         drows + c.blk_ptr[ib], n, Fk);
    if (c.keep_x) w.xc_have[ib] = 1;
  }
  ProfScope pp3(ctx, "eig_products");  // the N^3 products alone (bench.py: MFMA fraction of the tile engine)
  if (p.zero_fx)
    for (int k = 0; k < nb; k++) HFG_HIP_CHECK(hipMemsetAsync(c.Tk(k), 0, sizeof(double) * (size_t)b.ns[k] * b.ns[k], s));
  if (p.band_fx) {
    GemmHow how;
    how.tile = GemmTile::T64;
    how.scatter = how.klist = true;
    gemm_tasklist_dev(ctx, w.fxtasks.p, nfx, helfem::EIG_BAND_TILE, nm, how);
  } else
    gemm_tasklist_dev(ctx, w.gtasks.p, nb, nm, nm, p.full);
  if (p.zero_low)
    for (int k = 0; k < nb; k++) HFG_HIP_CHECK(hipMemsetAsync(w.A[k].p, 0, sizeof(double) * (size_t)b.ns[k] * b.ns[k], s));
  gemm_tasklist_dev(ctx, w.gtasks.p + nb, nb, nm, nm, p.low);
  gemm_mirror_lower_dev(ctx, w.gtasks.p + nb, nb, nm);  // the tridiagonalisation sweeps the full square
}

/// Direct path, the after_solve hook of eig_sym_batch: everything that needs the eigenvalues alone, on the main stream
/// between the divide-and-conquer stage and the wait for X Q (the side stream ends after that stage: the main stream would
/// idle there).  The values go to Etmp, are ranked and placed in dEs; C is zeroed ahead of the product that stores into it.
static void publish_direct(const BlocksCall &c, const EigChunk &b) {
  hfg_ctx *ctx = c.ctx;
  EigWork &w = c.w;
  hipStream_t s = ctx->stream;
  if (w.used_dc) {  // the status word goes home now; the host waits for this point only
    if (!w.h_status) HFG_HIP_CHECK(hipHostMalloc((void **)&w.h_status, sizeof(int), hipHostMallocDefault));
    if (!w.status_ev) HFG_HIP_CHECK(hipEventCreateWithFlags(&w.status_ev, hipEventDisableTiming));
    HFG_HIP_CHECK(hipMemcpyAsync(w.h_status, dc_status_word(ctx), sizeof(int), hipMemcpyDeviceToHost, s));
    HFG_HIP_CHECK(hipEventRecord(w.status_ev, s));
  }
  ProfScope ps(ctx, "scatter");
  publish_values(
      s, b.nb, [&](int k) { return b.values(c, k); }, [&](int k) { return c.Etmp(b.f[k]) + c.koff[b.ib[k]]; },
      [&](int k) { return b.nevs[k]; });
  for (int f = 0; f < c.nF; f++) {
    launch_rank(ctx, c.Etmp(f), c.K, c.rank(f));
    hipLaunchKernelGGL(k_place_values, dim3((c.K + 255) / 256), dim3(256), 0, s, c.Etmp(f), c.K, c.rank(f), c.dEs[f]);
    if (b.last.zero_out)  // (stream order: ahead of the product, split K adds into it)
      HFG_HIP_CHECK(hipMemsetAsync(c.dCs[f], 0, sizeof(double) * (size_t)c.N * c.K, s));
  }
}

/// Slot path: the eigenvalues are final, their copy into the slots goes ahead of the last product, not behind it
static void publish_slots(const BlocksCall &c, const EigChunk &b) {
  hipStream_t s = c.ctx->stream;
  if (b.last.zero_out && c.ctx->shard_n == 1)  // (more ranks: the whole buffer was zeroed at the start of the call)
    for (int k = 0; k < b.nb; k++) HFG_HIP_CHECK(hipMemsetAsync(b.slot(c, k), 0, sizeof(double) * (size_t)b.ns[k] * b.ns[k], s));
  publish_values(
      s, b.nb, [&](int k) { return b.values(c, k); }, [&](int k) { return b.slot(c, k) + c.nmax * c.nmax; },
      [&](int k) { return b.nevs[k]; });
}

/// C = X Z, or Y^T Z when X Q was folded: into the slots, or through the maps straight into C
static void last_product(const BlocksCall &c, const EigChunk &b) {
  ProfScope pp3(c.ctx, "eig_products");
  const GemmTask *last = c.w.gtasks.p + (c.w.folded ? 3 : 2) * (size_t)b.nb;
  gemm_tasklist_dev(c.ctx, last, b.nb, b.nm, c.nev > 0 ? *std::max_element(b.nevs, b.nevs + b.nb) : b.nm, b.last.how);
}

static void wait_status(const BlocksCall &c, int nb) {
  EigWork &w = c.w;
  if (c.direct && w.used_dc) {
    // everything is queued: the one host wait, for the status word behind the divide-and-conquer stage (the persistent
    // tridiagonalisation's words, written before it, are home by then too)
    HFG_HIP_CHECK(hipEventSynchronize(w.status_ev));
    if (*w.h_status != 0) throw std::logic_error("Eigendecomposition failed!\n");
    trdp_check_status(c.ctx);
  } else
    check_status(c.ctx, w, nb);
}

// nF Fock matrices at once (the two spins of an unrestricted iteration): their blocks join ONE batch -- the
// tridiagonalisation is a chain of dependent launches whose length does not depend on the number of blocks in it, so two
// spins cost about what one costs
/// nev > 0: the lowest min(nev, n_b) eigenpairs of every block only; slot ib then holds that many columns (ld n_b) and values
/// dEs, dCs (the one-call entries on one device, nF * nblk <= MAXB; dBlockBufs is not used): no block slots.  The K =
/// eig_sel_count eigenvalues of matrix f are ranked as soon as they are final and go to dEs[f]; the last product stores
/// element (i, j) of block ib at row blk_idx[blk_ptr[ib] + i], column rank[koff[ib] + j] of dCs[f] (N x K, zeroed here),
/// with the tiles and the k order of the slot path, so that E and C are bit for bit those of eig_assemble_dev.
static void eig_blocks_multi_dev(hfg_ctx *ctx, int N, int nF, const double *const *dFs, const double *dS, int nblk, const int64_t *blk_ptr,
                                 const int64_t *blk_idx, double *const *dBlockBufs, int nev = 0, double *const *dEs = nullptr,
                                 double *const *dCs = nullptr) {
  EigWork &w = work_for(ctx);
  hipStream_t s = ctx->stream;
  const bool direct = dEs != nullptr;
  if (direct && (ctx->shard_n != 1 || nF * nblk > MAXB)) throw std::logic_error("eig_blocks_multi_dev: direct path needs one rank and one batch\n");
  if (blk_ptr[nblk] != N) throw std::logic_error("Symmetry mismatch in eig_gsym_sub\n");
  for (int ib = 0; ib < nblk; ib++)
    if (blk_ptr[ib + 1] == blk_ptr[ib]) throw std::logic_error("eig_gsym_sub: empty symmetry block\n");
  const BlockLists lists = block_lists(ctx, w, N, dS, nblk, blk_ptr, blk_idx);

  const size_t nmax = helfem::eig_block_nmax(nblk, blk_ptr), slot = nmax * nmax + nmax;
  // the slots of the other ranks' blocks are zero so that a sum over the ranks completes the buffer.  One rank writes every
  // word that is read afterwards (eig_assemble_dev: n x nev columns and nev values per slot; the collectives of
  // helfem_amd.parallel move whole buffers or whole slots and read nothing themselves), so nothing is zeroed for it --
  // except the products' own outputs where two half-K workgroups add into them (eig_product_plan, eig_last_product).
  if (!direct && ctx->shard_n > 1)
    for (int f = 0; f < nF; f++) HFG_HIP_CHECK(hipMemsetAsync(dBlockBufs[f], 0, sizeof(double) * slot * nblk, s));
  // X = Sinvh(rows, cols) of every block, kept across calls while the lists above are (hfg_ctx_fix_sinvh): w.Xc
  const bool keep_x = w.sup_S == dS && w.sup_S != nullptr;
  std::vector<size_t> xoff(nblk + 1, 0);
  for (int ib = 0; ib < nblk; ib++) xoff[ib + 1] = xoff[ib] + (size_t)(blk_ptr[ib + 1] - blk_ptr[ib]) * (size_t)(blk_ptr[ib + 1] - blk_ptr[ib]);
  if (keep_x && (w.xc_have.size() != (size_t)nblk || w.Xc.n < xoff[nblk])) {
    w.Xc.resize(xoff[nblk]);
    w.xc_have.assign(nblk, 0);
  }
  // direct: ranks and eigenvalues of matrix f at ibuf1 + f (N + 8), ws[3] + f N; block ib's values start at koff[ib]
  std::vector<int64_t> koff(nblk + 1);
  const int K = (int)helfem::eig_value_offsets(nblk, blk_ptr, nev, koff.data());
  if (direct) {
    w.ibuf1.resize((size_t)nF * (N + 8));
    ctx->ws[3].resize((size_t)nF * N);
  }
  // work items: (matrix, block) pairs; `mine` holds matrix * nblk + block
  std::vector<int> mine;
  for (int f = 0; f < nF; f++)
    for (int ib = 0; ib < nblk; ib++)
      if (ib % ctx->shard_n == ctx->shard_rank) mine.push_back(f * nblk + ib);
  ctx->ws[5].resize(nmax * nmax * MAXB);
  ctx->ws[0].resize(nmax * nmax * MAXB);
  ctx->ws[4].resize(nmax * nmax * MAXB);
  const BlocksCall c{ctx, w, N, nF, nblk, blk_ptr, dFs, dS, dBlockBufs, nev, dEs, dCs, direct, lists, nmax, slot, keep_x, xoff.data(), koff.data(), K};
  const helfem::EigSwitches sw = eig_switches();
  for (size_t c0 = 0; c0 < mine.size(); c0 += MAXB) {
    EigChunk b = fill_chunk(c, mine.data() + c0, (int)std::min<size_t>(MAXB, mine.size() - c0));
    const std::vector<GemmTask> gt = build_tasks(c, b);
    upload_cached(w.gtasks, w.h_gtasks, gt, s);
    const std::vector<GemmTask> fx = build_row_tasks(c, b, gt);
    if (!fx.empty()) upload_cached(w.fxtasks, w.h_fxtasks, fx, s);
    b.plan = helfem::eig_product_plan(b.nb, b.ns, gemm_tile_slots(ctx), !fx.empty(), sw);
    b.last = helfem::eig_last_product(b.plan.full, nev > 0, direct);
    reduce_stage(c, b, (int)fx.size());
    if (direct)
      eig_sym_batch(ctx, w, b.nb, b.ns, b.Xptr, nev > 0 ? b.nevs : nullptr, [&] { publish_direct(c, b); });
    else
      eig_sym_batch(ctx, w, b.nb, b.ns, b.Xptr, nev > 0 ? b.nevs : nullptr);
    {
      ProfScope ps(ctx, "eig_backtransform");
      if (!direct) publish_slots(c, b);
      last_product(c, b);
    }
    wait_status(c, b.nb);
  }
  HFG_HIP_CHECK(hipGetLastError());
}
void eig_blocks_dev(hfg_ctx *ctx, int N, const double *dF, const double *dS, int nblk, const int64_t *blk_ptr,
                    const int64_t *blk_idx, double *dBlockBuf) {
  eig_blocks_multi_dev(ctx, N, 1, &dF, dS, nblk, blk_ptr, blk_idx, &dBlockBuf);
}

// phase 2: global sort of all eigenvalues and scatter of the block eigenvectors into C (N x N)
/// nev > 0: slot ib holds the lowest min(nev, n_b) pairs of its block; the ranking runs over their K = eig_sel_count values
/// (ties by position in block order, as over all N values), C is N x K
static void eig_assemble_sel_dev(hfg_ctx *ctx, int N, int nblk, const int64_t *blk_ptr, const int64_t *blk_idx, const double *dBlockBuf,
                                 double *dE, double *dC, int nev) {
  EigWork &w = work_for(ctx);
  hipStream_t s = ctx->stream;
  ProfScope ps(ctx, "scatter");
  // the row indices of the blocks: uploaded once per index list (an SCF run passes the same list every iteration; the copy
  // from pageable host memory cost 25 us of stream time per call)
  if (w.asm_rows.size() != (size_t)N || !std::equal(w.asm_rows.begin(), w.asm_rows.end(), blk_idx)) {
    w.asm_rows.assign(blk_idx, blk_idx + N);
    w.asm_rows_dev.resize((size_t)N + 2);
    HFG_HIP_CHECK(hipMemcpyAsync(w.asm_rows_dev.p, w.asm_rows.data(), sizeof(int64_t) * N, hipMemcpyHostToDevice, s));
  }
  int64_t *drows = (int64_t *)w.asm_rows_dev.p;
  const size_t nmax = helfem::eig_block_nmax(nblk, blk_ptr), slot = nmax * nmax + nmax;
  DevBuf<double> &Etmp = ctx->ws[3];
  Etmp.resize(N);
  std::vector<int64_t> koff(nblk + 1);  // first of block ib's values among the K wanted ones (all of them: blk_ptr)
  const int K = (int)helfem::eig_value_offsets(nblk, blk_ptr, nev, koff.data());
  publish_values(
      s, nblk, [&](int ib) { return dBlockBuf + (size_t)ib * slot + nmax * nmax; }, [&](int ib) { return Etmp.p + koff[ib]; },
      [&](int ib) { return (int)(koff[ib + 1] - koff[ib]); });
  DevBuf<int> &rank = w.ibuf1;
  rank.resize(N + 8);
  HFG_HIP_CHECK(hipMemsetAsync(dC, 0, sizeof(double) * (size_t)N * K, s));
  launch_rank(ctx, Etmp.p, K, rank.p);
  for (int ib = 0; ib < nblk; ib++) {
    int n = (int)(blk_ptr[ib + 1] - blk_ptr[ib]), nc = (int)(koff[ib + 1] - koff[ib]);
    hipLaunchKernelGGL(k_scatter_cols, dim3((n + 255) / 256, nc), dim3(256), 0, s, dBlockBuf + (size_t)ib * slot, n, nc,
                       drows + blk_ptr[ib], rank.p, (int)koff[ib], Etmp.p + koff[ib], N, dC, dE);
  }
  HFG_HIP_CHECK(hipGetLastError());
}
void eig_assemble_dev(hfg_ctx *ctx, int N, int nblk, const int64_t *blk_ptr, const int64_t *blk_idx,
                      const double *dBlockBuf, double *dE, double *dC) {
  eig_assemble_sel_dev(ctx, N, nblk, blk_ptr, blk_idx, dBlockBuf, dE, dC, 0);
}

/// the context as one rank for the lifetime of the guard; its shard comes back on every way out
struct OneRankGuard {
  hfg_ctx *ctx;
  const int rank, n;
  explicit OneRankGuard(hfg_ctx *c) : ctx(c), rank(c->shard_rank), n(c->shard_n) { ctx->shard_rank = 0, ctx->shard_n = 1; }
  ~OneRankGuard() { ctx->shard_rank = rank, ctx->shard_n = n; }
  OneRankGuard(const OneRankGuard &) = delete;
};

// The one-call entries: scf::eig_gsym_sub on one device, whatever the context's shard.  nF matrices with the same Sinvh and
// blocks; nev > 0: the lowest min(nev, n_b) pairs of every block.  By default nothing goes through block slots
// (eig_blocks_multi_dev, direct); HELFEM_EIG_DIRECT=0, or more (matrix, block) pairs than one batch holds, takes the two
// phases through ws[6] -- the checker: same E, same C, bit for bit.
static void eig_gsym_sub_multi_dev(hfg_ctx *ctx, int N, int nF, const double *const *dFs, const double *dS, int nblk, const int64_t *blk_ptr,
                                   const int64_t *blk_idx, int nev, double *const *dEs, double *const *dCs) {
  const OneRankGuard one_rank(ctx);
  if (helfem::tuning_live().eig_direct && nF * nblk <= MAXB) {  // (read at every call)
    eig_blocks_multi_dev(ctx, N, nF, dFs, dS, nblk, blk_ptr, blk_idx, nullptr, nev, dEs, dCs);
    return;
  }
  const size_t sz = eig_block_buf_size(nblk, blk_ptr);
  DevBuf<double> &buf = ctx->ws[6];
  buf.resize(nF * sz);
  double *bufs[MAXB];
  if (nF > MAXB) throw std::logic_error("eig_gsym_sub: too many matrices in one call\n");
  for (int f = 0; f < nF; f++) bufs[f] = buf.p + f * sz;
  eig_blocks_multi_dev(ctx, N, nF, dFs, dS, nblk, blk_ptr, blk_idx, bufs, nev);
  for (int f = 0; f < nF; f++) eig_assemble_sel_dev(ctx, N, nblk, blk_ptr, blk_idx, bufs[f], dEs[f], dCs[f], nev);
}

void eig_gsym_sub_dev(hfg_ctx *ctx, int N, const double *dF, const double *dS, int nblk, const int64_t *blk_ptr,
                      const int64_t *blk_idx, double *dE, double *dC) {
  eig_gsym_sub_multi_dev(ctx, N, 1, &dF, dS, nblk, blk_ptr, blk_idx, 0, &dE, &dC);
}

// the lowest min(nev, n_b) eigenpairs of every block on one device: E (K = eig_sel_count values, ascending), C (N x K)
void eig_gsym_sub_sel_dev(hfg_ctx *ctx, int N, const double *dF, const double *dS, int nblk, const int64_t *blk_ptr,
                          const int64_t *blk_idx, int nev, double *dE, double *dC) {
  if (nev < 1) throw std::logic_error("eig_gsym_sub_sel: nev must be at least 1\n");
  eig_gsym_sub_multi_dev(ctx, N, 1, &dF, dS, nblk, blk_ptr, blk_idx, nev, &dE, &dC);
}

/// column supports of the symmetry blocks of a block-structured Sinvh (scf_helpers.cpp:150-157): cols[blk_ptr[ib] ...] =
/// the columns with support on block ib's rows, ascending; throws like eig_blocks_dev when Sinvh is not block structured
void eig_block_supports(hfg_ctx *ctx, int N, const double *dS, int nblk, const int64_t *blk_ptr, const int64_t *blk_idx,
                        std::vector<int64_t> &cols) {
  DevBuf<int64_t> drows;
  DevBuf<int> flag;
  drows.resize(N);
  block_supports(ctx, N, dS, nblk, blk_ptr, blk_idx, drows.p, flag, cols);
}

// flag = 1 when H (N x N) has a non-zero entry, inside a symmetry block (blockid null: anywhere), whose two radial
// functions share no element
__global__ void k_band_outside(const double *__restrict__ H, int N, const int *__restrict__ node, const int *__restrict__ blockid,
                               int pm, int E, int *__restrict__ flag) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x, col = blockIdx.y;
  int bad = 0;
  if (row < N && (!blockid || blockid[row] == blockid[col]) && !helfem::eig_band_share(node[row], node[col], pm, E))
    bad = H[(size_t)col * N + row] != 0.0;  // (a NaN counts)
  bad = __syncthreads_or(bad);
  if (bad && threadIdx.x == 0) atomicOr(flag, 1);
}

/// hfg_ctx_declare_fock_band: node (N values, host) = radial node of every basis function, pm = p - 1, E elements; dH0
/// (device, N x N, may be null) is checked against the pattern inside the blocks of dBlockId (device, N ids, may be null)
/// by one reduction.  Returns the context's band_state: 1 declared, 2 refused.  Needs hfg_ctx_fix_sinvh first.
int eig_declare_band(hfg_ctx *ctx, int N, const int *node, int pm, int E, const double *dH0, const int *dBlockId) {
  if (!ctx->fixed_sinvh) throw std::logic_error("hfg_ctx_declare_fock_band: no Sinvh is declared fixed (hfg_ctx_fix_sinvh)\n");
  if (N < 1 || pm < 1 || E < 1 || !node) throw std::logic_error("hfg_ctx_declare_fock_band: invalid pattern\n");
  for (int i = 0; i < N; i++)
    if (node[i] < 0 || node[i] > pm * E) throw std::logic_error("hfg_ctx_declare_fock_band: radial node outside the elements\n");
  ctx->band_node.clear();
  ctx->band_state = 0;
  EigWork &w = work_for(ctx);
  w.sup_S = nullptr;  // lists and plans derived under an earlier declaration go
  if (dH0) {
    hipStream_t s = ctx->stream;
    DevBuf<int> &buf = w.ibuf2;
    buf.resize((size_t)N + 8);
    int flag = 0;
    HFG_HIP_CHECK(hipMemcpyAsync(buf.p + 1, node, sizeof(int) * N, hipMemcpyHostToDevice, s));
    HFG_HIP_CHECK(hipMemsetAsync(buf.p, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_band_outside, dim3((N + 255) / 256, N), dim3(256), 0, s, dH0, N, buf.p + 1, dBlockId, pm, E, buf.p);
    HFG_HIP_CHECK(hipMemcpyAsync(&flag, buf.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HFG_HIP_CHECK(hipStreamSynchronize(s));
    if (flag) {
      ctx->band_state = 2;
      return 2;
    }
  }
  ctx->band_node.assign(node, node + N);
  ctx->band_pm = pm;
  ctx->band_E = E;
  ctx->band_state = 1;
  return 1;
}

// scf::eig_gsym_sub for the two spin matrices of an unrestricted iteration in one batch (diatomic/main.cpp:936-958 calls
// it twice in a row with the same Sinvh and symmetry blocks)
void eig_gsym_sub_pair_dev(hfg_ctx *ctx, int N, const double *dFa, const double *dFb, const double *dS, int nblk, const int64_t *blk_ptr,
                           const int64_t *blk_idx, double *dEa, double *dCa, double *dEb, double *dCb) {
  const double *Fs[2] = {dFa, dFb};
  double *Es[2] = {dEa, dEb}, *Cs[2] = {dCa, dCb};
  eig_gsym_sub_multi_dev(ctx, N, 2, Fs, dS, nblk, blk_ptr, blk_idx, 0, Es, Cs);
}

}  // namespace hfg
