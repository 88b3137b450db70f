// FP64 special functions of the range-separated exchange tables, for device code (hip/rs_tei_dev.hip): the modified
// spherical Bessel functions i_L, k_L and the radial function Phi_L of the Legendre expansion of erfc(mu r12)/r12
// (Angyan, Gerber, Marsman, J. Phys. A 39, 8613 (2006)).  Device counterparts of bessel_il, bessel_kl and erfc_Phi in
// host/special.cpp, which are written in plain double already: the formulations chosen here are the host's own --
//   i_L  ascending series (all terms positive) below the switch, upward recurrence from sinh / cosh for x > 30 and x > 4L,
//        where x >> L keeps the subtraction of the recurrence harmless;
//   k_L  upward recurrence from exp(-x)/x (k_L is the dominant solution, upward is the stable direction);
//   Phi  the published short-range series (eq 30, paired terms, at most 32) for xi < 0.4 or (Xi < 0.5 and xi < 2 Xi), the
//        closed form (eqs 21-24) elsewhere, xi == 0 answered before the series, exact or reference binomials by `mode`
// -- with the operations in the host's order and without contraction into fused multiply-adds, so that the two sides differ
// by the last bits of exp, erfc, sinh, cosh and pow only.  Every function also compiles for the host (tests).
#pragma once
#include <hip/hip_runtime.h>

namespace hfg {
namespace sf {

#define HFG_SF __host__ __device__ inline

HFG_SF double bessel_il(double x, int L) {
#pragma clang fp contract(off)
  x = fabs(x);
  if (x == 0.0) return L == 0 ? 1.0 : 0.0;
  if (x > 30.0 && x > 4.0 * L) {
    double im = sinh(x) / x;
    if (L == 0) return im;
    double ic = (x * cosh(x) - sinh(x)) / (x * x);
    for (int n = 1; n < L; n++) {
      double ip = im - (2 * n + 1) / x * ic;
      im = ic;
      ic = ip;
    }
    return ic;
  }
  double pref = 1.0;
  for (int n = 1; n <= L; n++) pref *= x / (2 * n + 1);
  const double h = 0.5 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 2000; k++) {
    term *= h / ((double)k * (2 * L + 2 * k + 1));
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return pref * sum;
}

HFG_SF double bessel_kl(double x, int L) {
#pragma clang fp contract(off)
  const double ex = exp(-x);
  double km = ex / x;
  if (L == 0) return km;
  double kc = ex * (1.0 + 1.0 / x) / x;
  for (int n = 1; n < L; n++) {
    double kp = km + (2 * n + 1) / x * kc;
    km = kc;
    kc = kp;
  }
  return kc;
}

HFG_SF double factorial(int n) {
  double f = 1.0;
  for (int i = 2; i <= n; i++) f *= i;
  return f;
}
HFG_SF double double_factorial(int n) {
  double f = 1.0;
  for (int i = n; i > 1; i -= 2) f *= i;
  return f;
}
// C(n,m) = n (n-1) ... (n-m+1) / m! for any integer n
HFG_SF double gen_binomial(int n, int m) {
#pragma clang fp contract(off)
  if (m < 0) return 0.0;
  double c = 1.0;
  for (int i = 0; i < m; i++) c = c * (n - i) / (i + 1);
  return round(c);
}
// the reference's helper (mode 1), its recursion for n < 0 unrolled into a loop: each step multiplies by (-1)^m
HFG_SF double ref_binomial(int n, int m) {
  double sg = 1.0;
  const double sm = (m % 2) ? -1.0 : 1.0;
  for (;;) {
    if (n == -1) return sg * sm;
    if (n == 0) return m == 0 ? sg : 0.0;
    if (m == 0) return sg;
    if (m == 1) return sg * n;
    if (n > 0 && m > n) return 0.0;
    if (n > 0) return sg * gen_binomial(n, m);
    sg *= sm;
    n += m - 1;
  }
}

// eq 22
HFG_SF double erfc_F(int n, double Xi, double xi) {
#pragma clang fp contract(off)
  const double ep = exp(-(Xi + xi) * (Xi + xi)), em = exp(-(Xi - xi) * (Xi - xi));
  const double q = -1.0 / (4.0 * Xi * xi);
  double s = 0.0, qp = q;
  for (int p = 0; p <= n; p++) {
    const double sg = ((n - p) % 2) ? -1.0 : 1.0;
    s += qp * (factorial(n + p) / (factorial(p) * factorial(n - p))) * (sg * ep - em);
    qp *= q;
  }
  return 2.0 / sqrt(M_PI) * s;
}
// eq 24
HFG_SF double erfc_H(int n, double Xi, double xi) {
#pragma clang fp contract(off)
  const double A = pow(Xi, (double)(2 * n + 1)), a = pow(xi, (double)(2 * n + 1));
  return ((A + a) * erfc(Xi + xi) - (A - a) * erfc(Xi - xi)) / (2.0 * pow(xi * Xi, (double)(n + 1)));
}
// eq 21
HFG_SF double erfc_phi_general(int n, double Xi, double xi) {
#pragma clang fp contract(off)
  double s = erfc_F(n, Xi, xi) + erfc_H(n, Xi, xi);
  for (int m = 1; m <= n; m++) {
    const double Am = pow(Xi, (double)m), am = pow(xi, (double)m);
    s += erfc_F(n - m, Xi, xi) * ((Am * Am + am * am) / (Am * am));
  }
  return s;
}
// eqs 28, 29
HFG_SF double erfc_D(int n, int k, double Xi, int mode) {
#pragma clang fp contract(off)
  const double pref = exp(-Xi * Xi) / sqrt(M_PI) * pow(2.0, (double)(n + 1)) * pow(Xi, (double)(2 * n + 1));
  if (k == 0) {
    double s = 0.0;
    for (int m = 1; m <= n; m++) s += 1.0 / (double_factorial(2 * (n - m) + 1) * pow(2 * Xi * Xi, (double)m));
    return erfc(Xi) + pref * s;
  }
  double s = 0.0;
  for (int m = 1; m <= k; m++) {
    const double c = mode ? ref_binomial(m - k - 1, m - 1) : gen_binomial(m - k - 1, m - 1);
    s += c * pow(2 * Xi * Xi, (double)(k - m)) / double_factorial(2 * (n + k - m) + 1);
  }
  return pref * (2.0 * n + 1.0) / (factorial(k) * (2.0 * (n + k) + 1.0)) * s;
}
// eq 30
HFG_SF double erfc_phi_short(int n, double Xi, double xi, int mode) {
#pragma clang fp contract(off)
  if (xi == 0.0 && n > 0) return 0.0;
  if (n == 0 && xi == 0.0 && Xi == 0.0) return 1.0;
  double phi = 0.0;
  for (int k = 0; k <= 30; k += 2) {
    const double d = erfc_D(n, k, Xi, mode) * pow(xi, (double)(n + 2 * k)) + erfc_D(n, k + 1, Xi, mode) * pow(xi, (double)(n + 2 * (k + 1)));
    phi += d;
    if (fabs(d) < 2.220446049250313e-16 * fabs(phi)) break;
  }
  return phi / pow(Xi, (double)(n + 1));
}

HFG_SF double erfc_phi(int n, double Xi, double xi, int mode) {
  if (Xi < xi) {
    const double t = Xi;
    Xi = xi;
    xi = t;
  }
  if (xi < 0.4 || (Xi < 0.5 && xi < 2 * Xi)) return erfc_phi_short(n, Xi, xi, mode);
  return erfc_phi_general(n, Xi, xi);
}

#undef HFG_SF

}  // namespace sf
}  // namespace hfg
