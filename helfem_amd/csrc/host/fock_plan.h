// The host-side choices of the Fock build (hip/fock.hip): workgroup sizes, bytes of dynamic LDS, what a launcher refuses, the
// theta chunking of the XC kernels and the chunk and kernel variant of the batched Coulomb build, from plain integers alone.
// The launchers ask these functions and keep no copy of a rule; the LDS threshold and limits are named here and nowhere else.
// A refusal comes back as the text of the std::runtime_error that fock.hip throws (null: accepted).  Host only:
// tests/cpp/fock_plan_check.cpp includes nothing else.
#pragma once
#include <algorithm>
#include <cstddef>

namespace helfem {
constexpr size_t FOCK_LDS_PLAIN = 64 * 1024;  // dynamic LDS a kernel may have as it is; more: its attribute is raised first
constexpr size_t FOCK_LDS_MAX = 150 * 1024;   // bytes of LDS the XC kernels accept (and HELFEM_XC_LDS_LIMIT plans with)
constexpr size_t FOCK_LDS_CU = 160 * 1024;    // LDS of a CU: the one-pass theta kernel and the batched-Coulomb panel go this far
constexpr int XC_FT_MAXPP = 16;  // (a, b) pairs per thread of k_xc_fock_theta_chunked (256 threads): groups of up to 64 shells
constexpr int CB_MAX_NT = 4;     // column tiles of k_coulomb_tei_mfma at most: 16 result registers of 4 doubles per lane
constexpr int CB_TILE_NB = 8;    // densities per column tile: 16 columns, +M and -M of each

struct FockLds {
  size_t bytes;
  const char *refused;
};

inline bool fock_lds_raise(size_t bytes) { return bytes > FOCK_LDS_PLAIN; }
inline int round_up64(int n) { return ((n + 63) / 64) * 64; }
/// workgroup of the kernels that stride over pp items: the Coulomb kernels and k_xc_fock_radial (pp = p^2), k_xc_density_theta (ntheta)
inline int fock_block_threads(int pp) { return std::min(256, round_up64(pp)); }

// ---- Coulomb ----
/// k_coulomb_radial: red[4 E nwave], sc[4 E], big[E], small[E]
inline size_t coulomb_radial_lds(int E, int bs) {
  const int nwave = bs / 64;
  return (size_t)(4 * E * nwave + 4 * E + 2 * E) * sizeof(double);
}

/// the X panel of one column tile of k_coulomb_tei_mfma: round_up4(p^2) rows of 16 columns
inline size_t coulomb_batch_tile_bytes(int p) { return (size_t)((p * p + 3) & ~3) * 16 * sizeof(double); }

struct CoulombBatchChunk {
  int chunk;
  const char *refused;
};
/// Densities per pass over the in-element tables: as many column tiles as fit 64 KB (two workgroups per CU), CB_MAX_NT at
/// most; where not even one fits (p >= 23), as many as fit the 160 KB of a CU.  forced > 0 (HELFEM_COULOMB_BATCH_CHUNK): fewer.
inline CoulombBatchChunk coulomb_batch_chunk(int p, int forced) {
  const size_t tile = coulomb_batch_tile_bytes(p);
  int nt = (int)std::min<size_t>(CB_MAX_NT, FOCK_LDS_PLAIN / tile);
  if (nt == 0) nt = (int)std::min<size_t>(CB_MAX_NT, FOCK_LDS_CU / tile);
  if (nt == 0) return {0, "elements of more than 35 nodes: the batched Coulomb kernel's LDS panel does not fit\n"};
  return {forced > 0 ? std::min(forced, CB_TILE_NB * nt) : CB_TILE_NB * nt, nullptr};
}

struct CoulombBatchTei {
  bool mfma;  // k_coulomb_tei_mfma<n> (n column tiles), else k_coulomb_tei_cols<n> (n columns)
  int n;      // 0: a pass larger than any coulomb_batch_chunk
};
/// the kernel of a pass of nb >= 2 densities, 2 nb columns (+M and -M of each): matrix cores from 16 columns on,
/// register-blocked FMAs below
inline CoulombBatchTei coulomb_batch_tei(int nb) {
  if (nb <= 2) return {false, 4};
  if (nb <= 4) return {false, 8};
  if (nb <= 7) return {false, 14};
  const int nt = (nb + CB_TILE_NB - 1) / CB_TILE_NB;
  return {true, nt <= CB_MAX_NT ? nt : 0};
}

// ---- XC ----
/// k_xc_density_radial (256 threads): P block, the two transposed tables, the partial sums of the NJ classes of j; with the
/// Laplacian a fourth partial sum and the table L
inline FockLds xc_density_radial_lds(int p, int nq, int lapl) {
  const int NJ = (256 / nq > 0) ? std::min(256 / nq, p) : 1;
  const size_t shb = (size_t)(p * p + 2 * p * nq + 3 * NJ * nq + (lapl ? NJ * nq + p * nq : 0)) * sizeof(double);
  return {shb, shb > FOCK_LDS_MAX ? "radial quadrature too large for the XC density kernel's LDS tables" : nullptr};
}
/// k_xc_density_theta: the D blocks of one pair of m groups
inline size_t xc_density_theta_lds(int maxgrp, int lapl) { return (lapl ? 4 : 3) * maxgrp * maxgrp * sizeof(double); }

/// k_xc_fock_radial: four weights per point and four (six with the Laplacian) tables [nq][p]
inline FockLds xc_fock_radial_lds(int p, int nq, int lapl) {
  const size_t shb = (size_t)(4 * nq + (lapl ? 6 : 4) * nq * p) * sizeof(double);
  return {shb, shb > FOCK_LDS_MAX ? "radial quadrature too large for the XC Fock kernel's LDS tables" : nullptr};
}

struct XcFockThetaPlan {
  bool chunked;  // k_xc_fock_theta_chunked, nthc theta points at a time; else k_xc_fock_theta with all nth
  int nthc;
  size_t bytes;
  const char *refused;
};
/// X4: five (six with the Laplacian) potential rows and the Theta, dTheta rows of two shell groups in LDS; the one-pass
/// kernel when that fits lds_limit, the chunked one with the most theta points that do otherwise
inline XcFockThetaPlan xc_fock_theta_plan(int nth, int maxgrp, int lapl, size_t lds_limit) {
  const int nf = lapl ? 6 : 5;  // potential rows
  const size_t need = (size_t)(nf * nth + 4 * nth * maxgrp) * sizeof(double);
  if (need <= lds_limit)
    return {false, nth, need, need > FOCK_LDS_CU ? "angular grid too large for the XC Fock kernel's LDS tables" : nullptr};
  if (maxgrp * maxgrp > XC_FT_MAXPP * 256)
    return {true, 0, 0, "angular basis too large for the XC Fock kernels (more than 64 shells of one m)"};
  int nthc = (int)(lds_limit / sizeof(double) / (nf + 4 * maxgrp));
  if (nthc < 4) return {true, nthc, 0, "angular basis too large for the XC Fock kernels' LDS tables"};
  nthc = std::min(nthc, nth);
  return {true, nthc, (size_t)(nf * nthc + 4 * nthc * maxgrp) * sizeof(double), nullptr};
}

/// k_xc_grid: the potential planes of the whole angular grid (5, 6 with the Laplacian) and the reduction scratch; only the
/// six-plane build checks the limit itself
inline FockLds xc_grid_lds(int planes, int nth, int nphi) {
  const size_t shb = (size_t)(planes * nth * nphi + 3 * 4) * sizeof(double);
  return {shb, planes > 5 && shb > FOCK_LDS_MAX ? "XC angular grid too large for the grid kernel's LDS planes" : nullptr};
}

struct XcGridPolPlan {
  int rowc;  // theta rows that go through LDS per pass
  size_t bytes;
  const char *refused;
};
/// k_xc_grid_pol: 8 potential planes for both spins (10 with tau, 12 with the Laplacian) of rowc theta rows; rowc is halved
/// from nth until the planes fit lds_limit
inline XcGridPolPlan xc_grid_pol_plan(int nth, int nphi, int tau, int lapl, size_t lds_limit) {
  const int npot2 = lapl ? 12 : (tau ? 10 : 8);
  int rowc = nth;
  while ((size_t)(npot2 * rowc * nphi + 3 * 4) * sizeof(double) > lds_limit && rowc > 1) rowc = (rowc + 1) / 2;
  const size_t shb = (size_t)(npot2 * rowc * nphi + 3 * 4) * sizeof(double);
  return {rowc, shb, shb > FOCK_LDS_MAX ? "XC angular grid too large for the polarised grid kernel's LDS tile" : nullptr};
}
}  // namespace helfem
