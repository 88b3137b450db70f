// The host-side rules of the Fock build (helfem_amd/csrc/host/fock_plan.h) as a stand-alone program (host only: it includes
// that header and nothing else of the library).  The reference functions below are the expressions the launchers of
// hip/fock.hip held before the header existed, as they stood, throwing where the launchers threw; every rule of the header is
// compared with them over a sweep of shapes, then on both sides of each threshold, then for the shapes of the benchmark and
// of tests/xc_chunk_worker.py with values worked out by hand.  tests/test_fock_plan_cpu.py compiles it with
// -fsanitize=address,undefined and runs it.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../helfem_amd/csrc/host/fock_plan.h"

using namespace helfem;

static int failures = 0;
static long cases = 0;
static void expect(bool ok, const char *what) {
  cases++;
  if (!ok && failures++ < 20) std::printf("%s: FAILED\n", what);
}
#define EXPECT(cond) expect((cond), #cond)

// ---- the launchers' own expressions ----
namespace ref {
static int round_up64(int n) { return ((n + 63) / 64) * 64; }
static int bs(int pp) { return std::min(256, round_up64(pp)); }
static size_t coulomb_radial(int E, int bs) {
  int nwave = bs / 64;
  size_t shb = (size_t)(4 * E * nwave + 4 * E + 2 * E) * sizeof(double);
  return shb;
}
static size_t xc_fock_radial_lds(int p, int nq, int do_lapl) {
  const size_t shb = (size_t)(4 * nq + (do_lapl ? 6 : 4) * nq * p) * sizeof(double);
  if (shb > 150 * 1024) throw std::runtime_error("radial quadrature too large for the XC Fock kernel's LDS tables");
  return shb;
}
static size_t xc_fock_theta_lds(int nth, int maxgrp, int do_lapl) {
  size_t shb = (size_t)((do_lapl ? 6 : 5) * nth + 4 * nth * maxgrp) * sizeof(double);
  if (shb > 160 * 1024) throw std::runtime_error("angular grid too large for the XC Fock kernel's LDS tables");
  return shb;
}
constexpr int XC_FT_MAXPP = 16;
struct Theta {
  bool chunked;
  int nthc;
  size_t bytes;
};
static Theta launch_xc_fock_theta(int nth, int maxgrp, int do_lapl, size_t xc_lds_limit) {
  const int nf = do_lapl ? 6 : 5;  // potential rows
  const size_t need = (size_t)(nf * nth + 4 * nth * maxgrp) * sizeof(double);
  if (need <= xc_lds_limit) return {false, nth, xc_fock_theta_lds(nth, maxgrp, do_lapl)};
  if (maxgrp * maxgrp > XC_FT_MAXPP * 256) throw std::runtime_error("angular basis too large for the XC Fock kernels (more than 64 shells of one m)");
  int nthc = (int)(xc_lds_limit / sizeof(double) / (nf + 4 * maxgrp));
  if (nthc < 4) throw std::runtime_error("angular basis too large for the XC Fock kernels' LDS tables");
  nthc = std::min(nthc, nth);
  const size_t shb = (size_t)(nf * nthc + 4 * nthc * maxgrp) * sizeof(double);
  return {true, nthc, shb};
}
static size_t xc_density_radial_lds(int p, int nq, int do_lapl) {
  const int NJ = (256 / nq > 0) ? std::min(256 / nq, p) : 1;
  size_t shb = (size_t)(p * p + 2 * p * nq + 3 * NJ * nq + (do_lapl ? NJ * nq + p * nq : 0)) * sizeof(double);
  if (shb > 150 * 1024) throw std::runtime_error("radial quadrature too large for the XC density kernel's LDS tables");
  return shb;
}
static size_t xc_density_theta(int maxgrp, int do_lapl) { return (do_lapl ? 4 : 3) * maxgrp * maxgrp * sizeof(double); }
static size_t xc_grid(int do_lapl, int ntheta, int nphi) {
  const int npl = do_lapl ? 6 : 5;
  size_t shb = (size_t)(npl * ntheta * nphi + 3 * 4) * sizeof(double);
  if (do_lapl && shb > 150 * 1024) throw std::runtime_error("XC angular grid too large for the grid kernel's LDS planes");
  return shb;
}
static size_t xc_grid_pol_lds(int ntheta, int nphi, int do_tau, int do_lapl, size_t xc_lds_limit, int *rowc) {
  const int npot2 = do_lapl ? 12 : (do_tau ? 10 : 8);  // LDS potential planes, both spins
  *rowc = ntheta;
  while ((size_t)(npot2 * *rowc * nphi + 3 * 4) * sizeof(double) > xc_lds_limit && *rowc > 1) *rowc = (*rowc + 1) / 2;
  const size_t shb = (size_t)(npot2 * *rowc * nphi + 3 * 4) * sizeof(double);
  if (shb > 150 * 1024) throw std::runtime_error("XC angular grid too large for the polarised grid kernel's LDS tile");
  return shb;
}
constexpr int CB_MAX_NT = 4;
static int coulomb_batch_chunk(int p, int forced) {
  const size_t tile = (size_t)((p * p + 3) & ~3) * 16 * sizeof(double);
  int nt = (int)std::min<size_t>(CB_MAX_NT, (64 * 1024) / tile);
  if (nt == 0) nt = (int)std::min<size_t>(CB_MAX_NT, (160 * 1024) / tile);
  if (nt == 0) throw std::runtime_error("elements of more than 35 nodes: the batched Coulomb kernel's LDS panel does not fit\n");
  return forced > 0 ? std::min(forced, 8 * nt) : 8 * nt;
}
template <int NT>
static size_t tei_mfma_lds(int p) {
  const int pp = p * p;
  const size_t shb = (size_t)((pp + 3) & ~3) * 16 * NT * sizeof(double);
  return shb;
}
// the ladder of coulomb_batch_compact: 100 * mfma + NC or NT, 0 where it threw std::logic_error
static int ladder(int nb) {
  if (nb <= 2) return 4;
  else if (nb <= 4) return 8;
  else if (nb <= 7) return 14;
  else if (nb <= 8) return 101;
  else if (nb <= 16) return 102;
  else if (nb <= 24) return 103;
  else if (nb <= 8 * CB_MAX_NT) return 104;
  else return 0;
}
}  // namespace ref

// the reference's answer or the text it threw, against a rule's {bytes, refused}
template <typename F>
static void same_lds(const FockLds &got, F want, const char *what) {
  try {
    const size_t bytes = want();
    expect(!got.refused && got.bytes == bytes, what);
  } catch (const std::runtime_error &e) {
    expect(got.refused && !std::strcmp(got.refused, e.what()), what);
  }
}

static void sweep() {
  const size_t limits[] = {2500, 4096, 65536, 150 * 1024};
  for (int p = 2; p <= 40; p++) {
    expect(fock_block_threads(p * p) == ref::bs(p * p), "fock_block_threads");
    expect(coulomb_batch_tile_bytes(p) == ref::tei_mfma_lds<1>(p) && coulomb_batch_tile_bytes(p) * 2 == ref::tei_mfma_lds<2>(p) &&
               coulomb_batch_tile_bytes(p) * 3 == ref::tei_mfma_lds<3>(p) && coulomb_batch_tile_bytes(p) * 4 == ref::tei_mfma_lds<4>(p),
           "coulomb_batch_tile_bytes");
    for (int forced : {0, 1, 8, 9, 17, 40}) {
      const CoulombBatchChunk c = coulomb_batch_chunk(p, forced);
      try {
        const int want = ref::coulomb_batch_chunk(p, forced);
        expect(!c.refused && c.chunk == want, "coulomb_batch_chunk");
        // the ladder has a kernel for every pass the chunk rule allows, and its panel is the one the rule counted on
        const CoulombBatchTei v = coulomb_batch_tei(c.chunk);
        expect(c.chunk == 1 || v.n > 0, "a kernel for the largest pass");
        if (c.chunk > 1 && v.mfma) expect(coulomb_batch_tile_bytes(p) * v.n <= FOCK_LDS_CU, "the panel of the largest pass fits a CU");
      } catch (const std::runtime_error &e) {
        expect(c.refused && !std::strcmp(c.refused, e.what()), "coulomb_batch_chunk refusal");
      }
    }
    for (int nq : {p, 3 * p, 5 * p, 8 * p})
      for (int lapl = 0; lapl < 2; lapl++) {
        same_lds(xc_density_radial_lds(p, nq, lapl), [&] { return ref::xc_density_radial_lds(p, nq, lapl); }, "xc_density_radial_lds");
        same_lds(xc_fock_radial_lds(p, nq, lapl), [&] { return ref::xc_fock_radial_lds(p, nq, lapl); }, "xc_fock_radial_lds");
      }
  }
  for (int E = 1; E <= 70; E++)
    for (int bs : {64, 128, 192, 256}) expect(coulomb_radial_lds(E, bs) == ref::coulomb_radial(E, bs), "coulomb_radial_lds");
  for (int nth = 1; nth <= 140; nth++) {
    expect(fock_block_threads(nth) == ref::bs(nth), "fock_block_threads(nth)");
    for (int lapl = 0; lapl < 2; lapl++) {
      for (size_t limit : limits)
        for (int maxgrp = 1; maxgrp <= 70; maxgrp++) {
          const XcFockThetaPlan got = xc_fock_theta_plan(nth, maxgrp, lapl, limit);
          try {
            const ref::Theta want = ref::launch_xc_fock_theta(nth, maxgrp, lapl, limit);
            expect(!got.refused && got.chunked == want.chunked && got.nthc == want.nthc && got.bytes == want.bytes, "xc_fock_theta_plan");
          } catch (const std::runtime_error &e) {
            expect(got.refused && !std::strcmp(got.refused, e.what()), "xc_fock_theta_plan refusal");
          }
        }
      for (int nphi : {5, 9, 13, 21, 45}) {
        same_lds(xc_grid_lds(lapl ? 6 : 5, nth, nphi), [&] { return ref::xc_grid(lapl, nth, nphi); }, "xc_grid_lds");
        for (int tau = 0; tau < 2; tau++)
          for (size_t limit : limits) {
            const XcGridPolPlan got = xc_grid_pol_plan(nth, nphi, tau, lapl, limit);
            int rowc = 0;
            try {
              const size_t bytes = ref::xc_grid_pol_lds(nth, nphi, tau, lapl, limit, &rowc);
              expect(!got.refused && got.rowc == rowc && got.bytes == bytes, "xc_grid_pol_plan");
            } catch (const std::runtime_error &e) {
              expect(got.refused && !std::strcmp(got.refused, e.what()), "xc_grid_pol_plan refusal");
            }
          }
      }
    }
  }
  for (int maxgrp = 1; maxgrp <= 70; maxgrp++)
    for (int lapl = 0; lapl < 2; lapl++) expect(xc_density_theta_lds(maxgrp, lapl) == ref::xc_density_theta(maxgrp, lapl), "xc_density_theta_lds");
  for (int nb = 1; nb <= 33; nb++) {
    const CoulombBatchTei v = coulomb_batch_tei(nb);
    expect((v.n ? 100 * v.mfma + v.n : 0) == ref::ladder(nb), "coulomb_batch_tei");
  }
}

int main() {
  sweep();
  std::printf("%ld cases in the sweep\n", cases);

  // ---- the constants ----
  EXPECT(FOCK_LDS_PLAIN == 65536 && FOCK_LDS_MAX == 153600 && FOCK_LDS_CU == 163840 && CB_MAX_NT == 4 && XC_FT_MAXPP == 16);
  // the attribute is raised beyond 64 KB, not at it
  EXPECT(!fock_lds_raise(64 * 1024) && fock_lds_raise(64 * 1024 + 8) && !fock_lds_raise(0));

  // ---- workgroup sizes ----
  EXPECT(fock_block_threads(1) == 64 && fock_block_threads(64) == 64 && fock_block_threads(65) == 128 && fock_block_threads(192) == 192 &&
         fock_block_threads(193) == 256 && fock_block_threads(256) == 256 && fock_block_threads(257) == 256 && fock_block_threads(1600) == 256);

  // ---- X4: one pass at need == limit, chunked one double later ----
  {
    const size_t need = (size_t)(5 * 92 + 4 * 92 * 21) * 8;  // 65504
    XcFockThetaPlan a = xc_fock_theta_plan(92, 21, 0, need), b = xc_fock_theta_plan(92, 21, 0, need - 8);
    EXPECT(!a.refused && !a.chunked && a.nthc == 92 && a.bytes == need);
    EXPECT(!b.refused && b.chunked && b.nthc == 91 && b.bytes == (size_t)(5 * 91 + 4 * 91 * 21) * 8);  // 8187 doubles / 89 per point
    // a limit beyond a CU's LDS: the one-pass kernel refuses from 160 KB on; 20480 doubles = 5 * 128 + 4 * 128 * 38.75
    EXPECT(!xc_fock_theta_plan(128, 38, 0, 1 << 20).refused && xc_fock_theta_plan(128, 39, 0, 1 << 20).refused);
    EXPECT(xc_fock_theta_plan(128, 38, 0, 1 << 20).bytes == (size_t)(640 + 19456) * 8);
    EXPECT(!std::strcmp(xc_fock_theta_plan(140, 70, 0, 1 << 20).refused, "angular grid too large for the XC Fock kernel's LDS tables"));
    // chunked: 64 shells of one m at most (16 pairs per thread of 256), and four theta points at least
    EXPECT(!xc_fock_theta_plan(140, 64, 0, 65536).refused && xc_fock_theta_plan(140, 64, 0, 65536).chunked);
    EXPECT(!std::strcmp(xc_fock_theta_plan(140, 65, 0, 65536).refused, "angular basis too large for the XC Fock kernels (more than 64 shells of one m)"));
    EXPECT(xc_fock_theta_plan(100, 18, 1, 2500).nthc == 4 && !xc_fock_theta_plan(100, 18, 1, 2500).refused);  // 312 doubles / 78
    EXPECT(!std::strcmp(xc_fock_theta_plan(100, 19, 1, 2500).refused, "angular basis too large for the XC Fock kernels' LDS tables"));  // 312 / 82 = 3
    EXPECT(!xc_fock_theta_plan(3, 19, 1, 2500).refused && !xc_fock_theta_plan(3, 19, 1, 2500).chunked);  // three points in all: one pass
  }

  // ---- polarised grid kernel: rowc halves down to 1 ----
  {
    XcGridPolPlan g = xc_grid_pol_plan(28, 17, 0, 0, 100);
    EXPECT(g.rowc == 1 && g.bytes == (8 * 17 + 12) * 8 && !g.refused);
    EXPECT(xc_grid_pol_plan(28, 17, 0, 0, 30560).rowc == 28 && xc_grid_pol_plan(28, 17, 0, 0, 30559).rowc == 14);
    EXPECT(xc_grid_pol_plan(5, 9, 0, 0, (8 * 3 * 9 + 12) * 8).rowc == 3 && xc_grid_pol_plan(5, 9, 0, 0, (8 * 3 * 9 + 12) * 8 - 1).rowc == 2);
    g = xc_grid_pol_plan(140, 45, 1, 1, 1 << 20);  // fits the limit asked for, not the kernel's
    EXPECT(g.rowc == 140 && g.refused && !std::strcmp(g.refused, "XC angular grid too large for the polarised grid kernel's LDS tile"));
    EXPECT(!xc_grid_pol_plan(140, 45, 1, 1, 150 * 1024).refused && xc_grid_pol_plan(140, 45, 1, 1, 150 * 1024).rowc == 35);  // 12 * 35 * 45 + 12 = 18912 doubles
    // one row that does not fit: 12 * 1599 + 12 = 19200 doubles is the last that does
    EXPECT(!xc_grid_pol_plan(1, 1599, 0, 1, 150 * 1024).refused && xc_grid_pol_plan(1, 1600, 0, 1, 150 * 1024).refused &&
           !xc_grid_pol_plan(1, 1600, 0, 0, 150 * 1024).refused);
  }

  // ---- restricted grid kernel: only the six-plane build refuses; 19200 doubles = 6 * 246 * 13 + 12 ----
  EXPECT(xc_grid_lds(6, 246, 13).bytes == 150 * 1024 && !xc_grid_lds(6, 246, 13).refused && xc_grid_lds(6, 247, 13).refused);
  EXPECT(!xc_grid_lds(5, 400, 13).refused && xc_grid_lds(5, 400, 13).bytes == (5 * 400 * 13 + 12) * 8);
  EXPECT(!std::strcmp(xc_grid_lds(6, 140, 45).refused, "XC angular grid too large for the grid kernel's LDS planes"));

  // ---- radial kernels: 150 KiB = 19200 doubles ----
  EXPECT(xc_fock_radial_lds(24, 192, 0).bytes == 150 * 1024 && !xc_fock_radial_lds(24, 192, 0).refused);  // 192 * (4 + 4 * 24)
  EXPECT(!std::strcmp(xc_fock_radial_lds(24, 193, 0).refused, "radial quadrature too large for the XC Fock kernel's LDS tables"));
  EXPECT(xc_fock_radial_lds(24, 129, 1).bytes == (size_t)129 * 148 * 8 && !xc_fock_radial_lds(24, 129, 1).refused && xc_fock_radial_lds(24, 130, 1).refused);
  // density kernel, NJ = 1 from nq = 129 on: p^2 + nq (2 p + 3); p = 30: 900 + 63 nq, nq = 290 gives 19170, 291 gives 19233
  EXPECT(xc_density_radial_lds(30, 290, 0).bytes == 19170 * 8 && !xc_density_radial_lds(30, 290, 0).refused);
  EXPECT(!std::strcmp(xc_density_radial_lds(30, 291, 0).refused, "radial quadrature too large for the XC density kernel's LDS tables"));
  // the NJ rule: 256 / nq classes of j, p at most, one at least
  EXPECT(xc_density_radial_lds(4, 10, 0).bytes == (16 + 80 + 3 * 4 * 10) * 8);     // 25 -> p = 4
  EXPECT(xc_density_radial_lds(8, 40, 0).bytes == (64 + 640 + 3 * 6 * 40) * 8);    // 6
  EXPECT(xc_density_radial_lds(8, 40, 1).bytes == (64 + 640 + 4 * 6 * 40 + 320) * 8);
  EXPECT(xc_density_radial_lds(30, 128, 0).bytes == (900 + 7680 + 3 * 2 * 128) * 8 && xc_density_radial_lds(30, 129, 0).bytes == (900 + 7740 + 3 * 129) * 8);
  EXPECT(xc_density_radial_lds(30, 256, 0).bytes == (900 + 15360 + 3 * 256) * 8 && xc_density_radial_lds(30, 257, 0).bytes == (900 + 15420 + 3 * 257) * 8);

  // ---- batched Coulomb: kernel by nb ----
  {
    auto is = [](int nb, bool mfma, int n) {
      const CoulombBatchTei v = coulomb_batch_tei(nb);
      return v.mfma == mfma && v.n == n;
    };
    EXPECT(is(2, false, 4) && is(3, false, 8) && is(4, false, 8) && is(5, false, 14) && is(7, false, 14) && is(8, true, 1));
    EXPECT(is(9, true, 2) && is(16, true, 2) && is(17, true, 3) && is(24, true, 3) && is(25, true, 4) && is(32, true, 4));
    EXPECT(coulomb_batch_tei(33).n == 0 && coulomb_batch_tei(1000).n == 0);
    // columns: +M and -M of every density fit the kernel the ladder names
    for (int nb = 2; nb <= 32; nb++) {
      const CoulombBatchTei v = coulomb_batch_tei(nb);
      expect(2 * nb <= (v.mfma ? 16 * v.n : v.n), "2 nb columns fit");
    }
  }
  // ---- batched Coulomb: chunk by p.  One tile = round_up4(p^2) * 128 bytes: p = 22 the last in 64 KB, p = 35 the last in 160 KB ----
  EXPECT(coulomb_batch_tile_bytes(22) == 484 * 128 && coulomb_batch_tile_bytes(23) == 532 * 128 && coulomb_batch_tile_bytes(9) == 84 * 128);
  EXPECT(coulomb_batch_chunk(22, 0).chunk == 8 && coulomb_batch_chunk(23, 0).chunk == 16);   // 65536 / 61952 = 1; 163840 / 68096 = 2
  EXPECT(coulomb_batch_chunk(11, 0).chunk == 32 && coulomb_batch_chunk(12, 0).chunk == 24);  // four tiles of 124 rows, three of 144
  EXPECT(coulomb_batch_chunk(35, 0).chunk == 8 && !coulomb_batch_chunk(35, 0).refused);      // 1228 * 128 = 157184
  EXPECT(coulomb_batch_chunk(36, 0).chunk == 0 &&
         !std::strcmp(coulomb_batch_chunk(36, 0).refused, "elements of more than 35 nodes: the batched Coulomb kernel's LDS panel does not fit\n"));
  EXPECT(coulomb_batch_chunk(8, 5).chunk == 5 && coulomb_batch_chunk(8, 40).chunk == 32 && coulomb_batch_chunk(8, -3).chunk == 32);

  // ---- the benchmark's shapes: n2_pbe_nbf4230 (p 15, nq 75, E 5, 92 x 13 angular grid, 21 shells of m = 0), PBE ----
  EXPECT(fock_block_threads(225) == 256 && fock_block_threads(92) == 128 && coulomb_radial_lds(5, 256) == 880);
  EXPECT(xc_density_radial_lds(15, 75, 0).bytes == 25200 && xc_density_theta_lds(21, 0) == 10584 && xc_fock_radial_lds(15, 75, 0).bytes == 38400);
  EXPECT(xc_fock_theta_plan(92, 21, 0, 150 * 1024).bytes == 65504 && !xc_fock_theta_plan(92, 21, 0, 150 * 1024).chunked);
  EXPECT(xc_grid_lds(5, 92, 13).bytes == 47936 && xc_grid_pol_plan(92, 13, 0, 0, 150 * 1024).rowc == 92 &&
         xc_grid_pol_plan(92, 13, 0, 0, 150 * 1024).bytes == 76640);
  EXPECT(coulomb_batch_chunk(15, 0).chunk == 16 && coulomb_batch_tile_bytes(15) == 29184);
  // n2_pbe_small, n2_pbe0_small (p 8, nq 40, E 3, 36 x 13, 7 shells of m = 0)
  EXPECT(fock_block_threads(64) == 64 && fock_block_threads(36) == 64 && coulomb_radial_lds(3, 64) == 240);
  EXPECT(xc_density_radial_lds(8, 40, 0).bytes == 11392 && xc_density_theta_lds(7, 0) == 1176 && xc_fock_radial_lds(8, 40, 0).bytes == 11520);
  EXPECT(xc_fock_theta_plan(36, 7, 0, 150 * 1024).bytes == 9504 && !xc_fock_theta_plan(36, 7, 0, 150 * 1024).chunked);
  EXPECT(xc_grid_lds(5, 36, 13).bytes == 18816 && coulomb_batch_chunk(8, 0).chunk == 32);

  // ---- tests/xc_chunk_worker.py under HELFEM_XC_LDS_LIMIT=2500: 28 x 17 angular grid, 5 shells of m = 0 ----
  {
    const XcFockThetaPlan th = xc_fock_theta_plan(28, 5, 0, 2500);  // 700 doubles needed, 312 allowed, 25 per theta point
    EXPECT(th.chunked && th.nthc == 12 && th.bytes == 2400 && !th.refused);
    const XcGridPolPlan g = xc_grid_pol_plan(28, 17, 0, 0, 2500), gt = xc_grid_pol_plan(28, 17, 1, 0, 2500);
    EXPECT(g.rowc == 2 && g.bytes == 2272 && !g.refused);     // 28 -> 14 -> 7 -> 4 -> 2
    EXPECT(gt.rowc == 1 && gt.bytes == 1456 && !gt.refused);  // ten planes: two rows are 2816 bytes
    EXPECT(xc_grid_lds(5, 28, 17).bytes == 19136);            // the restricted kernel does not chunk
  }

  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("fock plan check ok\n");
  return 0;
}
