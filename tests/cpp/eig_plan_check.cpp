// The rules of the blocked eigensolve's products (helfem_amd/csrc/host/eig_plan.h) on both sides of every threshold and
// under every value of their switches, the benchmark's shapes pinned, and the whole of it against the expressions the
// driver carried in its own body before the header existed, restated here.  A stand-alone program (host only: it includes
// that header and nothing else of the library); tests/test_eig_plan_cpu.py compiles it with -fsanitize=address,undefined
// and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../helfem_amd/csrc/host/eig_plan.h"

using namespace helfem;

static int failures = 0;
static void expect(bool ok, const char *what) {
  if (!ok) {
    if (failures < 20) std::printf("%s: FAILED\n", what);
    failures++;
  }
}
#define EXPECT(cond) expect((cond), #cond)

static bool same(const GemmHow &a, const GemmHow &b) {
  return a.tile == b.tile && a.acc == b.acc && a.split2 == b.split2 && a.map == b.map && a.scatter == b.scatter && a.klist == b.klist;
}
static bool is(const GemmHow &a, GemmTile tile, bool split2, bool scatter = false) {
  GemmHow b;
  b.tile = tile, b.split2 = split2, b.scatter = scatter;
  return same(a, b);
}
static EigProductPlan plan(const std::vector<int> &ns, int slots, bool rows, const EigSwitches &sw) {
  std::vector<int> heap(ns);  // (heap-allocated: the sanitizer sees a read past the list)
  heap.shrink_to_fit();
  return eig_product_plan((int)heap.size(), heap.data(), slots, rows, sw);
}

// ---- the driver's expressions as they stood in eig_blocks_multi_dev and gemm_prefers_128, switches as parameters ----
struct Old {
  GemmHow full, low, last;
  bool band_fx, zero_T, zero_A, zero_slot, zero_C;
};
static bool old_prefers_128(long tiles128, int slots, int gemm_tile) {
  if (gemm_tile) return gemm_tile == 128;
  const long rounds = (tiles128 + slots - 1) / slots;
  return tiles128 >= slots / 2 && (double)tiles128 >= 0.85 * (double)(rounds * slots);
}
static Old old_rules(const std::vector<int> &ns, int slots, bool fx_not_empty, const EigSwitches &sw, int nev, bool direct) {
  const int nb = (int)ns.size();
  int nm = 0;
  for (int k = 0; k < nb; k++) nm = std::max(nm, ns[k]);
  const int force_split = sw.gemm_splitk;
  long full_tiles = 0, low_tiles = 0;
  for (int k = 0; k < nb; k++) {
    const long t1 = (ns[k] + 127) / 128;
    full_tiles += t1 * t1;
    low_tiles += t1 * (t1 + 1) / 2;
  }
  const bool band_fx = fx_not_empty && force_split < 0 && !old_prefers_128(full_tiles, slots, sw.gemm_tile) && !sw.mfma_4x4x4;
  const bool split_full = force_split >= 0 ? force_split != 0 : (full_tiles < slots && nm >= 256);
  const bool split_low = force_split >= 0 ? force_split != 0 : (low_tiles < slots && nm >= 256);
  const bool tile64 = force_split < 0 && !old_prefers_128(full_tiles, slots, sw.gemm_tile);
  GemmHow full, low;
  if (tile64) full.tile = low.tile = GemmTile::T64;
  else {
    if (split_full) full.tile = GemmTile::T128, full.split2 = true;
    else if (sw.gemm_rect) full.tile = GemmTile::T128x64;
    if (split_low) low.tile = GemmTile::T128, low.split2 = true;
  }
  Old o;
  o.full = full, o.low = low, o.band_fx = band_fx;
  o.zero_T = full.split2;  // "if (full.split2) ... hipMemsetAsync(T1 ...)"
  o.zero_A = low.split2;   // "if (low.split2) ... hipMemsetAsync(w.A[k] ...)"
  GemmHow how = nev > 0 ? GemmHow{GemmTile::T64} : full;
  how.scatter = direct;
  o.last = how;
  o.zero_slot = nev <= 0 && full.split2;  // the slot path's condition (one rank)
  o.zero_C = true;                        // the direct path zeroed all of C at every call
  return o;
}

int main() {
  const EigSwitches def;
  EXPECT(def.gemm_tile == 0 && def.gemm_splitk == -1 && !def.gemm_rect && !def.mfma_4x4x4);  // the defaults of the switch table

  // ---- gemm_prefers_128 on 512 slots: slots / 2, 0.85 of one round (435.2), of two rounds (870.4) ----
  EXPECT(!gemm_prefers_128(255, 512, 0) && !gemm_prefers_128(256, 512, 0));  // 256 passes slots / 2 and misses 85 %
  EXPECT(!gemm_prefers_128(435, 512, 0) && gemm_prefers_128(436, 512, 0));
  EXPECT(gemm_prefers_128(512, 512, 0) && !gemm_prefers_128(513, 512, 0));
  EXPECT(!gemm_prefers_128(870, 512, 0) && gemm_prefers_128(871, 512, 0));
  // both clauses hold at once or not at all for a product with tiles (85 % of a round is more than half of it): slots / 2
  // decides alone for the empty product, which fills its zero rounds
  EXPECT(!gemm_prefers_128(0, 512, 0) && !gemm_prefers_128(0, 2, 0) && gemm_prefers_128(0, 1, 0));
  // on 2 slots one tile is 50 % of a round and stays small, on 1 slot it fills its round
  EXPECT(!gemm_prefers_128(1, 2, 0) && gemm_prefers_128(2, 2, 0) && gemm_prefers_128(1, 1, 0));
  // 6 slots: 3 tiles reach slots / 2 but 50 %, 5 tiles miss 85 % (5.1), 6 fill the round
  EXPECT(!gemm_prefers_128(2, 6, 0) && !gemm_prefers_128(3, 6, 0) && !gemm_prefers_128(5, 6, 0) && gemm_prefers_128(6, 6, 0));
  for (long tiles : {0L, 1L, 255L, 436L, 513L, 871L, 100000L}) {
    expect(gemm_prefers_128(tiles, 512, 128), "HELFEM_GEMM_TILE=128 forces the large tiles");
    expect(!gemm_prefers_128(tiles, 512, 64) && !gemm_prefers_128(tiles, 512, 7), "another non-zero HELFEM_GEMM_TILE forces the small ones");
  }

  // ---- split K: blocks of order 256 at least, fewer tiles than slots; seen where the large tiles are in force ----
  {
    EigSwitches big;
    big.gemm_tile = 128;
    EXPECT(is(plan({255}, 512, false, big).full, GemmTile::Auto, false) && is(plan({255}, 512, false, big).low, GemmTile::Auto, false));
    EXPECT(is(plan({256}, 512, false, big).full, GemmTile::T128, true) && is(plan({256}, 512, false, big).low, GemmTile::T128, true));
    EXPECT(plan({256}, 512, false, big).zero_fx && plan({256}, 512, false, big).zero_low && !plan({255}, 512, false, big).zero_fx &&
           !plan({255}, 512, false, big).zero_low);
    EXPECT(is(plan({64, 255, 256}, 512, false, big).full, GemmTile::T128, true));  // (the largest block counts)
    // order 256: 4 full tiles, 3 lower ones.  tiles == slots keeps one workgroup per tile, slots - 1 splits
    EXPECT(!plan({256}, 4, false, big).full.split2 && plan({256}, 4, false, big).low.split2);
    EXPECT(plan({256}, 5, false, big).full.split2 && !plan({256}, 3, false, big).low.split2 && !plan({256}, 3, false, big).full.split2);
    // forced: 0 off, 1 (any other non-negative) on, whatever the sizes; both products alike
    for (int force : {0, 1, 2})
      for (int n : {1, 255, 256, 2600}) {
        EigSwitches sw;
        sw.gemm_splitk = force;
        const EigProductPlan p = plan({n}, 512, true, sw);
        expect(p.full.split2 == (force != 0) && p.low.split2 == (force != 0) && p.zero_fx == (force != 0) && p.zero_low == (force != 0), "forced split");
        expect(p.full.tile == (force ? GemmTile::T128 : GemmTile::Auto) && p.low.tile == (force ? GemmTile::T128 : GemmTile::Auto), "forced split: large tiles");
        expect(!p.band_fx, "a forced split keeps the dense F X");
      }
    // gemm_rect: the full products that are not split; never the lower-triangle product
    EigSwitches rect = big;
    rect.gemm_rect = true;
    EXPECT(is(plan({255}, 512, false, rect).full, GemmTile::T128x64, false) && is(plan({255}, 512, false, rect).low, GemmTile::Auto, false));
    EXPECT(is(plan({256}, 512, false, rect).full, GemmTile::T128, true) && is(plan({256}, 512, false, rect).low, GemmTile::T128, true));
    rect.gemm_splitk = 0;
    EXPECT(is(plan({256}, 512, false, rect).full, GemmTile::T128x64, false) && is(plan({256}, 512, false, rect).low, GemmTile::Auto, false));
    rect = EigSwitches();
    rect.gemm_rect = true;  // the small tiles are not touched by it
    EXPECT(is(plan({256}, 512, false, rect).full, GemmTile::T64, false) && is(plan({256}, 512, false, rect).low, GemmTile::T64, false));
  }
  // ---- gemm_tile 0 / 64 / 128 on a batch whose large tiles fill the chip (2600: 21 x 21 = 441 of 512) and one that does not ----
  {
    EigSwitches sw;
    EXPECT(is(plan({2600}, 512, false, sw).full, GemmTile::T128, true) && is(plan({2600}, 512, false, sw).low, GemmTile::T128, true));  // 441, 231 < 512
    EXPECT(is(plan({1380}, 512, false, sw).full, GemmTile::T64, false) && is(plan({1380}, 512, false, sw).low, GemmTile::T64, false));
    sw.gemm_tile = 64;
    EXPECT(is(plan({2600}, 512, false, sw).full, GemmTile::T64, false) && is(plan({2600}, 512, false, sw).low, GemmTile::T64, false));
    sw.gemm_tile = 128;
    EXPECT(is(plan({1380}, 512, false, sw).full, GemmTile::T128, true) && is(plan({1380}, 512, false, sw).low, GemmTile::T128, true));
    EXPECT(is(plan({64}, 512, false, sw).full, GemmTile::Auto, false));  // large tiles asked for, nothing to split: the launcher's own choice
  }
  // ---- band_fx: row tasks, unforced split, small tiles, the 16x16x4 instruction ----
  {
    EigSwitches sw;
    EXPECT(plan({1380}, 512, true, sw).band_fx && !plan({1380}, 512, false, sw).band_fx);
    EXPECT(!plan({2600}, 512, true, sw).band_fx);  // the large tiles are in force
    sw.mfma_4x4x4 = true;
    EXPECT(!plan({1380}, 512, true, sw).band_fx && is(plan({1380}, 512, true, sw).full, GemmTile::T64, false));
    sw = EigSwitches();
    sw.gemm_splitk = 0;
    EXPECT(!plan({1380}, 512, true, sw).band_fx);
    sw.gemm_splitk = 1;
    EXPECT(!plan({1380}, 512, true, sw).band_fx);
    sw = EigSwitches();
    sw.gemm_tile = 128;
    EXPECT(!plan({1380}, 512, true, sw).band_fx);
    sw.gemm_tile = 64;
    EXPECT(plan({2600}, 512, true, sw).band_fx);
  }
  // ---- the last product ----
  {
    GemmHow split;
    split.tile = GemmTile::T128, split.split2 = true;
    GemmHow small;
    small.tile = GemmTile::T64;
    EXPECT(is(eig_last_product(split, false, false).how, GemmTile::T128, true, false) && eig_last_product(split, false, false).zero_out);
    EXPECT(is(eig_last_product(split, false, true).how, GemmTile::T128, true, true) && eig_last_product(split, false, true).zero_out);
    EXPECT(is(eig_last_product(small, false, false).how, GemmTile::T64, false, false) && !eig_last_product(small, false, false).zero_out);
    EXPECT(is(eig_last_product(small, false, true).how, GemmTile::T64, false, true) && eig_last_product(small, false, true).zero_out);
    // selected (n x nev): small tiles and no split whatever the full products take; the slots are then not zeroed
    EXPECT(is(eig_last_product(split, true, false).how, GemmTile::T64, false, false) && !eig_last_product(split, true, false).zero_out);
    EXPECT(is(eig_last_product(split, true, true).how, GemmTile::T64, false, true) && eig_last_product(split, true, true).zero_out);
    GemmHow rect;
    rect.tile = GemmTile::T128x64;
    EXPECT(is(eig_last_product(rect, false, true).how, GemmTile::T128x64, false, true) && is(eig_last_product(rect, true, false).how, GemmTile::T64, false, false));
  }

  // ---- the benchmark's shapes: 1380 / 1470 / 1380 have 11^2 + 12^2 + 11^2 = 386 large tiles, both spins 772 ----
  {
    const std::vector<int> one = {1380, 1470, 1380}, pair = {1380, 1470, 1380, 1380, 1470, 1380};
    EXPECT((1380 + 127) / 128 == 11 && (1470 + 127) / 128 == 12 && 121 + 144 + 121 == 386);
    EXPECT(!gemm_prefers_128(386, 512, 0) && !gemm_prefers_128(772, 512, 0));  // 75 % of one round, of two
    for (const std::vector<int> &ns : {one, pair})
      for (int rows = 0; rows < 2; rows++) {
        const EigProductPlan p = plan(ns, 512, rows != 0, def);
        expect(is(p.full, GemmTile::T64, false) && is(p.low, GemmTile::T64, false) && !p.zero_fx && !p.zero_low, "flagship: 64 x 64 tiles, no split");
        expect(p.band_fx == (rows != 0), "flagship: banded F X exactly when row tasks exist");
        expect(is(eig_last_product(p.full, false, true).how, GemmTile::T64, false, true), "flagship: last product scattered, small tiles");
      }
  }

  // ---- against the restated expressions: one to three sizes, both slot counts, every combination of the switches ----
  {
    const int sizes[] = {1, 64, 65, 128, 129, 255, 256, 257, 1380, 1470, 2600};
    const int nsz = (int)(sizeof(sizes) / sizeof(sizes[0]));
    std::vector<std::vector<int> > lists;
    for (int a = 0; a < nsz; a++) {
      lists.push_back({sizes[a]});
      for (int b = 0; b < nsz; b++) {
        lists.push_back({sizes[a], sizes[b]});
        for (int c = 0; c < nsz; c++) lists.push_back({sizes[a], sizes[b], sizes[c]});
      }
    }
    EXPECT(lists.size() == 11 + 121 + 1331);
    long compared = 0;
    for (const std::vector<int> &ns : lists)
      for (int slots : {208, 512})
        for (int splitk : {-1, 0, 1})
          for (int tile : {0, 64, 128})
            for (int bits = 0; bits < 8; bits++) {
              EigSwitches sw;
              sw.gemm_splitk = splitk, sw.gemm_tile = tile, sw.gemm_rect = bits & 1, sw.mfma_4x4x4 = (bits & 2) != 0;
              const bool rows = (bits & 4) != 0;
              const EigProductPlan p = plan(ns, slots, rows, sw);
              for (int nev : {0, 3})
                for (int direct = 0; direct < 2; direct++) {
                  const Old o = old_rules(ns, slots, rows, sw, nev, direct != 0);
                  const EigLastProduct l = eig_last_product(p.full, nev > 0, direct != 0);
                  expect(same(p.full, o.full) && same(p.low, o.low) && p.band_fx == o.band_fx && p.zero_fx == o.zero_T && p.zero_low == o.zero_A,
                         "eig_product_plan against the driver's expressions");
                  expect(same(l.how, o.last) && l.zero_out == (direct ? o.zero_C : o.zero_slot), "eig_last_product against the driver's expressions");
                  expect(!(p.band_fx && p.full.split2), "the banded F X is never a split product");
                  compared++;
                }
            }
    EXPECT(compared == 1463L * 2 * 3 * 3 * 8 * 4);
    for (long t = 0; t <= 2100; t++)
      for (int slots : {1, 2, 208, 512})
        for (int tile : {0, 64, 128}) expect(gemm_prefers_128(t, slots, tile) == old_prefers_128(t, slots, tile), "gemm_prefers_128 against its old body");
  }

  // ---- value offsets and the largest block against direct sums ----
  for (const std::vector<int64_t> &sz : std::vector<std::vector<int64_t> >{{1}, {1380, 1470, 1380}, {1, 2, 3, 5, 31, 33}, {7}, {4, 4}, {200, 1, 17}})
    for (int64_t nev : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)3, (int64_t)4, (int64_t)32, (int64_t)200, (int64_t)1470, (int64_t)5000}) {
      std::vector<int64_t> ptr(1, 0);
      for (int64_t s : sz) ptr.push_back(ptr.back() + s);
      ptr.shrink_to_fit();
      const int nblk = (int)sz.size();
      std::vector<int64_t> koff(nblk + 1, -7);
      koff.shrink_to_fit();
      const int64_t K = eig_value_offsets(nblk, ptr.data(), nev, koff.data());
      int64_t sum = 0, big = 0;
      bool ok = koff[0] == 0;
      for (int ib = 0; ib < nblk; ib++) {
        sum += (nev > 0 && nev < sz[ib]) ? nev : sz[ib];
        big = sz[ib] > big ? sz[ib] : big;
        ok = ok && koff[ib + 1] == sum;
      }
      expect(ok && K == sum && eig_value_offsets(nblk, ptr.data(), nev, nullptr) == sum, "eig_value_offsets against the direct sum");
      if (nev <= 0) expect(K == ptr.back(), "all values: koff is blk_ptr");
      expect(eig_block_nmax(nblk, ptr.data()) == (size_t)big, "eig_block_nmax");
    }
  {
    const int64_t none[1] = {0};
    EXPECT(eig_value_offsets(0, none, 3, nullptr) == 0 && eig_block_nmax(0, none) == 0);
  }
  std::printf(failures ? "eig plan check FAILED\n" : "eig plan check ok\n");
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
