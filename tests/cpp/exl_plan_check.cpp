// The choices of the low-rank exchange build (helfem_amd/csrc/host/exl_plan.h) on both sides of every threshold and under
// every value of the switches, as a stand-alone program (host only: it includes that header and nothing else of the
// library).  The expected values are written out here as the rules are documented (the switch table), not
// derived from the header.  tests/test_exl_plan_cpu.py compiles it with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../helfem_amd/csrc/host/exl_plan.h"

using namespace helfem;

static int failures = 0;
static void expect(bool ok, const char *what) {
  if (!ok) {
    std::printf("%s: FAILED\n", what);
    failures++;
  }
}
#define EXPECT(cond) expect((cond), #cond)

static bool same(const ExlCross &a, bool split, ExlTile tile, bool wl) { return a.split == split && a.tile == tile && a.worklist == wl; }
static bool same(const ExlElem &a, ExlTile tile, bool wl) { return a.tile == tile && a.worklist == wl; }

int main() {
  const ExlSwitches def;
  EXPECT(def.rb == 0 && def.mgroups && def.rect == -1 && def.wl && def.splitk && def.crect);  // the defaults of the switch table

  // ---- what the builds decline ----
  EXPECT(exl_order_fits(16384) && !exl_order_fits(16385));
  EXPECT(exl_run_fits(256) && !exl_run_fits(257));
  // pair tables: ntt Ntab E^2 p^4 doubles against the limit (4 * 10 * 9 * 10^4 * 8 bytes = 28.8e6)
  EXPECT(exl_pair_tables_fit(4, 10, 3, 10, 28.8e6) && !exl_pair_tables_fit(4, 10, 3, 10, 28.8e6 - 1.0));

  // ---- alpha kernel: p 16 / 17, E p 512 / 513, the column of V in 150 KiB of LDS ----
  EXPECT(exl_alpha_lds(4, 1000) == 16000 && exl_alpha_lds(1, 1000) == 8000 && exl_alpha_lds(2, 1000) == 8000);
  EXPECT(exl_alpha_fast(16, 2, 1000) && !exl_alpha_fast(17, 2, 1000));
  EXPECT(exl_alpha_fast(16, 32, 1000) && !exl_alpha_fast(16, 33, 1000));  // E p = 512, 528
  EXPECT(exl_alpha_fast(8, 64, 1000) && !exl_alpha_fast(9, 57, 1000));    // E p = 512, 513
  EXPECT(exl_alpha_fast(10, 3, 150 * 1024) && !exl_alpha_fast(10, 3, 150 * 1024 + 8));
  EXPECT(exl_alpha_fast(10, 3, exl_alpha_lds(4, 9600)) && !exl_alpha_fast(10, 3, exl_alpha_lds(4, 9601)));  // Nd at the edge, two types
  EXPECT(exl_alpha_fast(10, 3, exl_alpha_lds(2, 19200)) && !exl_alpha_fast(10, 3, exl_alpha_lds(2, 19201)));

  // ---- grouped by m: more than one run, the fast alpha kernel, no pair tables, the switch ----
  for (int mg = 0; mg < 2; mg++)
    for (int pair = 0; pair < 2; pair++)
      for (int fast = 0; fast < 2; fast++)
        for (int nruns = 1; nruns <= 3; nruns++) {
          ExlSwitches sw;
          sw.mgroups = mg != 0;
          expect(exl_grouped(pair != 0, nruns, fast != 0, sw) == (mg && !pair && fast && nruns > 1), "exl_grouped");
        }

  // ---- RB kernel ----
  for (int rb : {-1, 0, 1, 2, 3, 4, 5})
    for (int p : {2, 15, 16, 17, 20}) {
      ExlSwitches sw;
      sw.rb = rb;
      expect(exl_rb_kernel(true, p, sw) == ExlRB::pair, "pair tables take k_exl_RB_pair");
      const ExlRB want = (rb == 1 || p > 16) ? ExlRB::one_pair : rb == 4 ? ExlRB::rb4 : ExlRB::mfma;
      expect(exl_rb_kernel(false, p, sw) == want, "exl_rb_kernel");
    }
  // the one-pair kernels stage (4 p + 1) max_nch r doubles: 150 KiB = 19200 doubles; p = 11, max_nch = 6, r = 71 gives 19170, r = 72 19440
  EXPECT(exl_one_pair_lds(6, 71, 11) == 19170 * sizeof(double));
  EXPECT(exl_rb_fits(ExlRB::one_pair, 6, 71, 11) && !exl_rb_fits(ExlRB::one_pair, 6, 72, 11));
  EXPECT(exl_rb_fits(ExlRB::pair, 6, 71, 11) && !exl_rb_fits(ExlRB::pair, 6, 72, 11));
  EXPECT(exl_rb_fits(ExlRB::mfma, 6, 72, 11) && exl_rb_fits(ExlRB::rb4, 6, 72, 11));  // they stage in slices
  // 150 KiB exactly: p = 1, max_nch = 64, r = 60 gives 5 * 3840 = 19200 doubles
  EXPECT(exl_rb_fits(ExlRB::one_pair, 64, 60, 1) && exl_one_pair_lds(64, 60, 1) == 150 * 1024 && !exl_rb_fits(ExlRB::one_pair, 64, 61, 1));

  // ---- cross products: every value of SPLITK, CRECT, WL, grouped or not, 511 / 512 columns, 2047 / 2048 tiles ----
  EXPECT(exl_tiles128(128, 128) == 1 && exl_tiles128(129, 128) == 2 && exl_tiles128(135, 135) == 4 && exl_tiles128(1, 257) == 3);
  for (int splitk = 0; splitk < 2; splitk++)
    for (int crect = 0; crect < 2; crect++)
      for (int wl = 0; wl < 2; wl++)
        for (int grouped = 0; grouped < 2; grouped++)
          for (long ncol : {1L, 511L, 512L, 513L, 100000L})
            for (long tiles : {0L, 1L, 2047L, 2048L, 2049L}) {
              ExlSwitches sw;
              sw.splitk = splitk != 0, sw.crect = crect != 0, sw.wl = wl != 0;
              const ExlCross c = exl_cross(ncol, tiles, grouped != 0, sw);
              const bool split = splitk && ncol >= 512 && tiles < 2048;
              if (!split) expect(same(c, false, ExlTile::Auto, false), "plain cross products: the default task-list tiles");
              else if (crect && grouped) expect(same(c, true, ExlTile::T128x64, wl != 0), "split cross products, 128 x 64: work list unless WL=0");
              else expect(same(c, true, ExlTile::T128, false), "split cross products, 128 x 128: task list");
            }
  // (the element switch does not reach the cross products)
  for (int rect : {-1, 0, 1, 2}) {
    ExlSwitches sw;
    sw.rect = rect;
    expect(same(exl_cross(512, 100, true, sw), true, ExlTile::T128x64, true), "RECT leaves the cross products alone");
  }

  // ---- element GEMM: every value of RECT and WL, 1499.x / 1500 pairs per task on average ----
  for (int wl = 0; wl < 2; wl++) {
    ExlSwitches sw;
    sw.wl = wl != 0;
    const ExlTile shortl = wl ? ExlTile::T64 : ExlTile::T128x64, longl = wl ? ExlTile::T128 : ExlTile::Auto;
    expect(same(exl_elem(1499.0 * 7 + 6.0, 7, sw), shortl, wl != 0), "1499 6/7 pairs on average: short lists");
    expect(same(exl_elem(1500.0 * 7, 7, sw), longl, wl != 0), "1500 pairs on average: long lists");
    expect(same(exl_elem(1500.0 * 7 + 1.0, 7, sw), longl, wl != 0), "more than 1500 pairs on average: long lists");
    expect(same(exl_elem(3.0, 1, sw), shortl, wl != 0), "one task of 3 pairs");
    for (double pairs : {3.0, 1e9}) {  // a forced shape wins over the lengths
      sw.rect = 0;
      expect(same(exl_elem(pairs, 4, sw), wl ? ExlTile::T128 : ExlTile::Auto, wl != 0), "RECT=0: 128 x 128 (task list: the launcher's choice)");
      sw.rect = 1;
      expect(same(exl_elem(pairs, 4, sw), ExlTile::T128x64, wl != 0), "RECT=1: 128 x 64");
      sw.rect = 2;
      expect(same(exl_elem(pairs, 4, sw), wl ? ExlTile::T64 : ExlTile::T128x64, wl != 0), "RECT=2: 64 x 64 (task list: 128 x 64)");
      sw.rect = 3;
      expect(same(exl_elem(pairs, 4, sw), wl ? ExlTile::T128 : ExlTile::T128x64, wl != 0), "RECT=3: not a shape, 128 x 128 on the work list");
      sw.rect = -1;
    }
  }
  // (the cross switches do not reach the element GEMM)
  for (int k = 0; k < 4; k++) {
    ExlSwitches sw;
    sw.splitk = k & 1, sw.crect = (k & 2) != 0;
    expect(same(exl_elem(10.0, 2, sw), ExlTile::T64, true), "SPLITK and CRECT leave the element GEMM alone");
  }

  // ---- batched build ----
  {
    const int runs_ok[3] = {256, 1, 30}, runs_long[3] = {10, 257, 30};
    EXPECT(exl_batch_takes(16384, false, 16, 32, 4, 9600, runs_ok, 3, def));
    EXPECT(!exl_batch_takes(16385, false, 16, 32, 4, 9600, runs_ok, 3, def));
    EXPECT(!exl_batch_takes(16384, true, 16, 32, 4, 9600, runs_ok, 3, def));
    EXPECT(!exl_batch_takes(16384, false, 17, 2, 4, 9600, runs_ok, 3, def));
    EXPECT(!exl_batch_takes(16384, false, 16, 33, 4, 9600, runs_ok, 3, def));
    EXPECT(!exl_batch_takes(16384, false, 16, 32, 4, 9601, runs_ok, 3, def));
    EXPECT(exl_batch_takes(16384, false, 16, 32, 2, 19200, runs_ok, 3, def));
    EXPECT(!exl_batch_takes(16384, false, 16, 32, 4, 9600, runs_long, 3, def));
    EXPECT(exl_batch_takes(100, false, 5, 2, 4, 100, runs_ok, 0, def));
    for (int rb : {0, 1, 2, 4}) {
      ExlSwitches sw;
      sw.rb = rb;
      expect(exl_batch_takes(100, false, 5, 2, 4, 100, runs_ok, 3, sw) == (rb != 1 && rb != 4), "the checkers of the RB kernel loop over the single build");
    }
    // what the batch takes is what takes the fast kernels in the single build
    for (int p : {15, 16, 17})
      for (int E : {2, 32, 33})
        for (int pair = 0; pair < 2; pair++)
          for (int rb : {0, 1, 4})
            for (int Nd : {9600, 9601}) {
              ExlSwitches sw;
              sw.rb = rb;
              const bool single = exl_rb_kernel(pair != 0, p, sw) == ExlRB::mfma && exl_alpha_fast(p, E, exl_alpha_lds(4, Nd));
              expect(exl_batch_takes(1000, pair != 0, p, E, 4, Nd, runs_ok, 3, sw) == single, "batch takes what the single build's fast kernels take");
            }
  }
  // A member of a chunk gets what the single build of that density alone gets: both builds call exl_cross with the
  // member's own NLM r and tile count and exl_elem with ONE density's pair count.  Restated on a chunk of ranks (r_hi, 2,
  // r_lo) around the threshold for NLM = 18, 31 and 64, under every switch setting: the members that split are exactly
  // those with NLM r >= 512, and tile and launcher are the same for every member that splits.
  for (int NLM : {18, 31, 64})
    for (int k = 0; k < 16; k++) {
      ExlSwitches sw;
      sw.splitk = k & 1, sw.crect = (k & 2) != 0, sw.wl = (k & 4) != 0, sw.mgroups = (k & 8) != 0;
      const int r_hi = (512 + NLM - 1) / NLM, r_lo = r_hi - 1;
      const bool grouped = exl_grouped(false, 2, true, sw);
      const int ranks[3] = {r_hi, 2, r_lo};
      const bool want[3] = {sw.splitk, false, false};
      ExlCross first;
      for (int b = 0; b < 3; b++) {
        const ExlCross c = exl_cross((long)NLM * ranks[b], 12, grouped, sw);
        expect(c.split == want[b], "member split as its single build");
        if (c.split) first = c;
      }
      if (sw.splitk) expect(first.tile == ((sw.crect && grouped) ? ExlTile::T128x64 : ExlTile::T128) && first.worklist == (sw.crect && grouped && sw.wl), "split members' tile");
    }

  // ---- the record ----
  {
    ExlPlanRecord r;
    EXPECT(exl_plan_json(r) == "null");
    r.chunks = 2;
    r.start(true, 31, 8, 21, 2, 5);
    EXPECT(r.valid && r.batch && r.chunks == 2 && r.NLM == 31 && r.A == 8 && r.Ntab == 21 && r.E == 2 && r.p == 5 && r.ranks.empty());
    r.run_shells = {4, 2, 2};
    r.ranks = {17, 2, 16};
    r.cross_split = {1, 0, 0};
    r.grouped = r.alpha_fast = true;
    r.cross_split_tile = ExlTile::T128x64;
    r.cross_worklist = true;
    r.elem_tile = ExlTile::T64;
    r.cross_task(40);
    r.cross_task(12);
    r.cross_task(90);
    EXPECT(r.cross_minK == 12 && r.cross_maxK == 90);
    const std::string s = exl_plan_json(r);
    EXPECT(s.find("\"ranks\": [17, 2, 16]") != std::string::npos && s.find("\"cross_split\": [1, 0, 0]") != std::string::npos);
    EXPECT(s.find("\"cross_split_tile\": \"T128x64\"") != std::string::npos && s.find("\"cross_launcher\": \"worklist\"") != std::string::npos);
    EXPECT(s.find("\"alpha\": \"k_exl_alpha\"") != std::string::npos && s.find("\"rb\": \"mfma\"") != std::string::npos);
    EXPECT(s.find("\"chunks\": 2") != std::string::npos && s.front() == '{' && s.back() == '}');
    r.start(false, 1, 1, 1, 1, 1);
    EXPECT(!r.batch && r.run_shells.empty() && r.cross_split.empty() && r.cross_split_tile == ExlTile::Auto);
  }
  std::printf(failures ? "exl plan check FAILED\n" : "exl plan check ok\n");
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
