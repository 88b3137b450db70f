// Selected eigenpairs of symmetric tridiagonal matrices on gfx950: the lowest nev eigenvalues by Sturm-count multisection,
// their eigenvectors by inverse iteration.  The second algorithm of the tridiagonal stage beside divide and conquer
// (dc.hip): independent work per eigenpair instead of a merge tree, for callers that want a few columns of a large block
// (LAPACK: dstebz + dstein, as dsyevx calls them with range = 'I').
//
//   k_stsel_values   one wave per wanted eigenvalue.  The 64 lanes evaluate the Sturm count at 64 shifts that divide the
//                    current interval into 65 parts (the recurrence of dlaebz, pivmin safeguard included); a ballot picks
//                    the part whose counts bracket the index.  Nine rounds take the Gershgorin interval to 2^-53 of its
//                    width.  d and e^2 are staged in LDS once per workgroup of four waves up to STSEL_LDS_N rows, read
//                    from global memory beyond.
//   k_stsel_vectors  one wave per CLUSTER (dstein: consecutive eigenvalues closer than 1e-3 ||T||_1), its members in
//                    order.  dlagtf / dlagts (factor T - lambda I with partial pivoting, solve) are serial recurrences
//                    on lane 0; scaling, norms and the modified Gram-Schmidt sweep against the earlier vectors of the
//                    cluster go over the lanes.  The factors and the iterate live in LDS up to STSEL_LDS_N rows (41 bytes
//                    per row), in a global work array beyond.  A cluster of c members costs O(c^2 n) in one wave: slow
//                    for a large cluster, accepted (the crossover in eig.hip sends large nev / n to divide and conquer).
//
// The matrix is not split at zero couplings: an eigenvalue repeated in decoupled parts is a cluster like any other, the
// 10 eps |lambda| perturbation of dstein separates its members and the Gram-Schmidt sweep makes them orthonormal.  The
// start vectors are a fixed hash of (column, row): results repeat bitwise.  Nothing is read back and nothing is
// synchronised; failures (an interval that does not close, an iterate that does not grow in five iterations) set the
// status word of the divide-and-conquer stage (dc_status).
#include "internal.h"
#include "wave.h"
#include <cfloat>

namespace hfg {

constexpr int STSEL_MAXB = 8;
constexpr int STSEL_LDS_N = 3072;  // largest order whose rows are staged in LDS (41 bytes per row in k_stsel_vectors: 123 KB)
constexpr int STSEL_ROUNDS = 256;  // multisection rounds at most (nine reach full precision of a well-scaled interval)
constexpr int STSEL_MAXITS = 5;    // dstein: MAXITS
constexpr int STSEL_EXTRA = 2;     // dstein: EXTRA
constexpr double STSEL_EPS = 2.220446049250313e-16;  // dlamch('P')
constexpr double STSEL_SFMIN = DBL_MIN;

struct StselBatch {
  int n[STSEL_MAXB], nev[STSEL_MAXB];
  const double *d[STSEL_MAXB], *e[STSEL_MAXB];  // e[i] couples rows i and i + 1
  double *W[STSEL_MAXB], *Z[STSEL_MAXB];        // nev values (ascending); n x nev, ld n
  double *work[STSEL_MAXB];                     // orders above STSEL_LDS_N: 6 n doubles per column
};

// Gershgorin bounds widened as in dstebz, pivmin, ||T||_1; every lane returns the same values
__device__ __forceinline__ void stsel_bounds(const double *__restrict__ d, const double *__restrict__ e, int n, int lane, double &gl,
                                             double &gu, double &pivmin, double &onenrm) {
  double lo = DBL_MAX, hi = -DBL_MAX, e2max = 0.0, nrm = 0.0;
  for (int i = lane; i < n; i += 64) {
    const double el = i > 0 ? fabs(e[i - 1]) : 0.0, er = i + 1 < n ? fabs(e[i]) : 0.0;
    lo = fmin(lo, d[i] - el - er);
    hi = fmax(hi, d[i] + el + er);
    e2max = fmax(e2max, er * er);
    nrm = fmax(nrm, fabs(d[i]) + el + er);
  }
  gl = -wave_max(-lo);
  gu = wave_max(hi);
  e2max = wave_max(e2max);
  onenrm = wave_max(nrm);
  pivmin = STSEL_SFMIN * fmax(1.0, e2max);
  const double tnorm = fmax(fabs(gl), fabs(gu));
  const double widen = 2.1 * tnorm * STSEL_EPS * n + 4.2 * pivmin;
  gl -= widen;
  gu += widen;
}

// number of eigenvalues <= sigma (dlaebz): negative pivots of the LDL^T factorisation of T - sigma I
template <bool LDS>
__device__ __forceinline__ int stsel_count(const double *dv, const double *e2v, const double *__restrict__ d, const double *__restrict__ e, int n,
                                           double sigma, double pivmin) {
  double q = (LDS ? dv[0] : d[0]) - sigma;
  if (fabs(q) < pivmin) q = -pivmin;
  int c = q <= 0.0;
  for (int i = 1; i < n; i++) {
    double di, e2;
    if (LDS) {
      di = dv[i];
      e2 = e2v[i - 1];
    } else {
      di = d[i];
      e2 = e[i - 1] * e[i - 1];
    }
    q = di - e2 / q - sigma;
    if (fabs(q) < pivmin) q = -pivmin;
    c += q <= 0.0;
  }
  return c;
}

template <bool LDS>
__global__ __launch_bounds__(256) void k_stsel_values(StselBatch b, int *__restrict__ status) {
  extern __shared__ double sh[];  // LDS: d[n], e^2[n]
  const int blk = blockIdx.y;
  const int n = b.n[blk], nev = b.nev[blk];
  const double *__restrict__ d = b.d[blk], *__restrict__ e = b.e[blk];
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blockIdx.x * 4 >= nev) return;  // the whole workgroup
  if (LDS) {
    for (int i = threadIdx.x; i < n; i += 256) {
      sh[i] = d[i];
      sh[n + i] = i + 1 < n ? e[i] * e[i] : 0.0;
    }
    __syncthreads();
  }
  if (k >= nev) return;  // the whole wave
  double lo, hi, pivmin, onenrm;
  stsel_bounds(d, e, n, lane, lo, hi, pivmin, onenrm);
  bool closed = false;
  for (int it = 0; it < STSEL_ROUNDS; it++) {
    if (hi - lo <= 2.0 * STSEL_EPS * fmax(fabs(lo), fabs(hi)) + pivmin) {
      closed = true;
      break;
    }
    const double h = (hi - lo) / 65.0;
    const double sigma = fma((double)(lane + 1), h, lo);
    const int c = stsel_count<LDS>(sh, sh + n, d, e, n, sigma, pivmin);
    const unsigned long long mask = __ballot(c > k);  // lanes whose shift has the k-th eigenvalue at or below it
    double nlo = lo, nhi = hi;
    if (mask == 0ull)
      nlo = fma(64.0, h, lo);
    else {
      const int j = __builtin_ctzll(mask);
      nhi = fma((double)(j + 1), h, lo);
      if (j > 0) nlo = fma((double)j, h, lo);
    }
    nlo = fmax(nlo, lo);  // rounding of the shifts never widens the interval
    nhi = fmin(nhi, hi);
    if (nlo == lo && nhi == hi) {  // the shifts have collapsed onto the ends: the interval is a few ulps wide
      closed = hi - lo <= 8.0 * STSEL_EPS * fmax(fabs(lo), fabs(hi)) + pivmin;
      break;
    }
    lo = nlo;
    hi = nhi;
  }
  if (lane == 0) {
    b.W[blk][k] = 0.5 * (lo + hi);
    if (!closed) atomicOr(status, 1);
  }
}

// start vector: uniform in (-1, 1), a fixed function of (column, row)
__device__ __forceinline__ double stsel_start(unsigned col, unsigned row) {
  unsigned long long z = ((unsigned long long)(col + 1) << 32) ^ (unsigned long long)(row + 0x9e3779b9u);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return ((double)(z >> 11) + 0.5) * (2.0 / 9007199254740992.0) - 1.0;
}

// index-free maximum of |x| over the rows, in every lane
__device__ __forceinline__ double stsel_amax(const double *x, int n, int lane) {
  double m = 0.0;
  for (int i = lane; i < n; i += 64) m = fmax(m, fabs(x[i]));
  return wave_max(m);
}

template <bool LDS>
__global__ __launch_bounds__(64) void k_stsel_vectors(StselBatch b, int *__restrict__ status) {
  extern __shared__ double sh[];  // LDS: a, bb, c, dd, x (n doubles each), in (n bytes)
  const int blk = blockIdx.y;
  const int n = b.n[blk], nev = b.nev[blk];
  const int lane = threadIdx.x;
  const int j0 = blockIdx.x;
  if (j0 >= nev) return;
  const double *__restrict__ d = b.d[blk], *__restrict__ e = b.e[blk];
  const double *__restrict__ W = b.W[blk];
  double *__restrict__ Z = b.Z[blk];
  double gl, gu, pivmin, onenrm;
  stsel_bounds(d, e, n, lane, gl, gu, pivmin, onenrm);
  const double ortol = 1e-3 * onenrm;
  if (j0 > 0 && W[j0] - W[j0 - 1] <= ortol) return;  // a later member of its cluster: the cluster's first wave computes it
  if (n == 1) {
    if (lane == 0) Z[0] = 1.0;
    return;
  }
  double *base = LDS ? sh : b.work[blk] + (size_t)j0 * 6 * n;
  double *a = base, *bb = base + n, *c = base + 2 * (size_t)n, *dd = base + 3 * (size_t)n, *x = base + 4 * (size_t)n;
  unsigned char *in = (unsigned char *)(base + 5 * (size_t)n);
  const double dtpcrt = sqrt(0.1 / n);
  double xjm = 0.0;
  for (int j = j0; j < nev; j++) {
    if (j > j0 && W[j] - W[j - 1] > ortol) break;  // the next cluster
    double xj = W[j];
    if (j > j0) {  // dstein: equal computed eigenvalues are separated
      const double pertol = 10.0 * fabs(STSEL_EPS * xj);
      if (xj - xjm < pertol) xj = xjm + pertol;
    }
    for (int i = lane; i < n; i += 64) {
      a[i] = d[i] - xj;
      bb[i] = c[i] = i + 1 < n ? e[i] : 0.0;
      dd[i] = 0.0;
      x[i] = stsel_start((unsigned)j, (unsigned)i);
    }
    __syncthreads();
    // ---- dlagtf: T - xj I = P L U, partial pivoting; U has the diagonals a, bb, dd; the multipliers are c ----
    if (lane == 0) {
      double scale1 = fabs(a[0]) + fabs(bb[0]);
      for (int k = 0; k < n - 1; k++) {
        const double ak = a[k], ck = c[k], ak1 = a[k + 1], bk = bb[k];
        double scale2 = fabs(ck) + fabs(ak1);
        if (k < n - 2) scale2 += fabs(bb[k + 1]);
        const double piv1 = ak == 0.0 ? 0.0 : fabs(ak) / scale1;
        if (ck == 0.0) {
          in[k] = 0;
          scale1 = scale2;
        } else {
          const double piv2 = fabs(ck) / scale2;
          if (piv2 <= piv1) {
            in[k] = 0;
            scale1 = scale2;
            const double m = ck / ak;
            c[k] = m;
            a[k + 1] = ak1 - m * bk;
          } else {
            in[k] = 1;
            const double m = ak / ck;
            a[k] = ck;
            a[k + 1] = bk - m * ak1;
            if (k < n - 2) {
              const double t = bb[k + 1];
              dd[k] = t;
              bb[k + 1] = -m * t;
            }
            bb[k] = ak1;
            c[k] = m;
          }
        }
      }
      in[n - 1] = 0;
    }
    __syncthreads();
    // dlagts's own tolerance (job = -1, tol = 0 on entry)
    double tol = 0.0;
    for (int i = lane; i < n; i += 64) tol = fmax(tol, fmax(fabs(a[i]), fmax(fabs(bb[i]), fabs(dd[i]))));
    tol = wave_max(tol) * STSEL_EPS;
    if (tol == 0.0) tol = STSEL_EPS;
    const double ulast = fabs(a[n - 1]);
    int its = 0, nrmchk = 0;
    bool failed = false;
    for (;;) {
      if (++its > STSEL_MAXITS) {
        failed = true;
        break;
      }
      // scale the right-hand side
      const double scl = n * onenrm * fmax(STSEL_EPS, ulast) / stsel_amax(x, n, lane);
      for (int i = lane; i < n; i += 64) x[i] *= scl;
      __syncthreads();
      // ---- dlagts, job = -1: solve with the factors, small pivots perturbed ----
      if (lane == 0) {
        for (int k = 1; k < n; k++) {
          if (in[k - 1] == 0)
            x[k] -= c[k - 1] * x[k - 1];
          else {
            const double t = x[k - 1];
            x[k - 1] = x[k];
            x[k] = t - c[k - 1] * x[k];
          }
        }
        const double bignum = 1.0 / STSEL_SFMIN;
        double y1 = 0.0, y2 = 0.0;  // x[k + 1], x[k + 2]
        for (int k = n - 1; k >= 0; k--) {
          double t = x[k];
          if (k <= n - 2) t -= bb[k] * y1;
          if (k <= n - 3) t -= dd[k] * y2;
          double ak = a[k];
          double pert = copysign(tol, ak);
          for (;;) {
            const double absak = fabs(ak);
            if (absak < 1.0) {
              if (absak < STSEL_SFMIN) {
                if (absak == 0.0 || fabs(t) * STSEL_SFMIN > absak) {
                  ak += pert;
                  pert *= 2.0;
                  continue;
                }
                t *= bignum;
                ak *= bignum;
              } else if (fabs(t) > absak * bignum) {
                ak += pert;
                pert *= 2.0;
                continue;
              }
            }
            break;
          }
          t = t / ak;
          x[k] = t;
          y2 = y1;
          y1 = t;
        }
      }
      __syncthreads();
      // ---- modified Gram-Schmidt against the earlier vectors of the cluster ----
      for (int q = j0; q < j; q++) {
        const double *zq = Z + (size_t)q * n;
        double s = 0.0;
        for (int i = lane; i < n; i += 64) s += x[i] * zq[i];
        s = wave_sum(s);
        for (int i = lane; i < n; i += 64) x[i] -= s * zq[i];
      }
      // ---- dstein's growth criterion ----
      const double nrm = stsel_amax(x, n, lane);
      if (!(nrm >= dtpcrt)) continue;  // (a NaN iterate keeps iterating and fails)
      if (++nrmchk < STSEL_EXTRA + 1) continue;
      break;
    }
    // normalise; the component of largest magnitude is made positive (the first such row)
    double s = 0.0, m = 0.0;
    for (int i = lane; i < n; i += 64) {
      s += x[i] * x[i];
      m = fmax(m, fabs(x[i]));
    }
    s = wave_sum(s);
    m = wave_max(m);
    int first = n;
    for (int i = lane; i < n; i += 64)
      if (fabs(x[i]) == m) {
        first = i;
        break;
      }
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o));
    double f = 1.0 / sqrt(s);
    if (first < n && x[first] < 0.0) f = -f;
    if (failed || !(s > 0.0) || !(f == f) || isinf(f)) {  // never a wrong vector silently
      if (lane == 0) atomicOr(status, 1);
      f = 0.0;
    }
    double *zj = Z + (size_t)j * n;
    for (int i = lane; i < n; i += 64) zj[i] = failed ? 0.0 : x[i] * f;
    __threadfence_block();
    __syncthreads();  // the column is read back by the cluster's later members (same wave)
    xjm = xj;
  }
}

struct StselWork : Workspace {
  DevBuf<double> work[STSEL_MAXB];
};

/// The lowest nev[blk] eigenpairs of nblk symmetric tridiagonal matrices (d[blk], e[blk]; not overwritten): eigenvalues
/// ascending in W[blk], eigenvectors in Z[blk] (n x nev, ld n).  Queued on the context's stream.
void tridiag_sel_batch(hfg_ctx *ctx, int nblk, const int *ns, const int *nev, double *const *d, double *const *e, double *const *W,
                       double *const *Z) {
  if (nblk > STSEL_MAXB) throw std::logic_error("tridiag_sel_batch: too many blocks");
  StselWork *wp = &ctx->work.get<StselWork>(WS_STSEL);
  hipStream_t s = ctx->stream;
  StselBatch b;
  int nmax = 0, nevmax = 0;
  for (int i = 0; i < STSEL_MAXB; i++) {
    const bool on = i < nblk;
    if (on && (ns[i] < 1 || nev[i] < 1 || nev[i] > ns[i])) throw std::logic_error("tridiag_sel_batch: 1 <= nev <= n violated");
    b.n[i] = on ? ns[i] : 0;
    b.nev[i] = on ? nev[i] : 0;
    b.d[i] = on ? d[i] : nullptr;
    b.e[i] = on ? e[i] : nullptr;
    b.W[i] = on ? W[i] : nullptr;
    b.Z[i] = on ? Z[i] : nullptr;
    b.work[i] = nullptr;
    if (on) {
      nmax = std::max(nmax, ns[i]);
      nevmax = std::max(nevmax, nev[i]);
    }
  }
  const bool lds = nmax <= STSEL_LDS_N;
  if (!lds)
    for (int i = 0; i < nblk; i++) {
      wp->work[i].resize((size_t)nev[i] * 6 * ns[i]);
      b.work[i] = wp->work[i].p;
    }
  int *status = dc_status_word(ctx);
  HFG_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int) * 4, s));
  const dim3 gv((nevmax + 3) / 4, nblk), gz(nevmax, nblk);
  if (lds) {
    const size_t shv = (size_t)2 * nmax * sizeof(double), shz = (size_t)5 * nmax * sizeof(double) + ((size_t)nmax + 7) / 8 * 8;
    if (shz > 64 * 1024)
      HFG_HIP_CHECK(hipFuncSetAttribute((const void *)k_stsel_vectors<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shz));
    hipLaunchKernelGGL(k_stsel_values<true>, gv, dim3(256), shv, s, b, status);
    hipLaunchKernelGGL(k_stsel_vectors<true>, gz, dim3(64), shz, s, b, status);
  } else {
    hipLaunchKernelGGL(k_stsel_values<false>, gv, dim3(256), 0, s, b, status);
    hipLaunchKernelGGL(k_stsel_vectors<false>, gz, dim3(64), 0, s, b, status);
  }
  HFG_HIP_CHECK(hipGetLastError());
}

}  // namespace hfg
