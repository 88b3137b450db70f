// The choices of the low-rank exchange build (hip/exchange_lr.hip): which kernel, tile shape and launcher a build takes, from
// sizes and switches alone, and the record of what the last build on a table set took (hfg_exl_last_plan).  The single
// build (exchange_lowrank_dev) and the batched one (exchange_batch_chunk) both ask these functions, so that a member of a
// batch gets what its single build gets.  Host only: tests/cpp/exl_plan_check.cpp includes nothing else.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

namespace helfem {
constexpr int EXL_RMAX = 64;  // factors of one group (one pass over the tables)
constexpr int EXL_QMAX = 16;  // rows per thread in the factorisation kernel: N <= 1024 * EXL_QMAX
constexpr int EXL_AG = 4;     // groups of shells per workgroup of k_exl_alpha at most
constexpr int EXL_AP = 16;    // nodes per element the fast alpha kernel and the matrix-core RB kernel take at most
constexpr int EXL_RUN_MAX = 256;                 // k_exl_V lists at most 256 coupled shells: the longest run of shells of one m
constexpr size_t EXL_LDS_MAX = 150 * 1024;       // bytes of LDS the alpha kernel and the one-pair RB kernels plan with
constexpr long EXL_SPLIT_MIN_COLS = 512;         // cross products are split over K from NLM * r columns ...
constexpr long EXL_SPLIT_MAX_TILES = 2048;       // ... while they have fewer 128 x 128 tiles than this
constexpr double EXL_ELEM_LONG_PAIRS = 1500.0;   // element GEMM: 128 x 128 tiles from this many shell pairs per task on average

enum class ExlTile { Auto, T64, T128, T128x64 };  // Auto: the task-list launcher's own choice between T64 and T128
enum class ExlRB { mfma, rb4, one_pair, pair };   // k_exl_RBm, k_exl_RB4, k_exl_RB, k_exl_RB_pair

/// the switches the choices read (tuning.h: HELFEM_EXL_RB, _MGROUPS, _RECT, _WL, _SPLITK, _CRECT)
struct ExlSwitches {
  int rb = 0;
  bool mgroups = true;
  int rect = -1;
  bool wl = true, splitk = true, crect = true;
};

// ---- what the builds decline ----
inline bool exl_order_fits(long N) { return !(N > 1024 * EXL_QMAX); }
/// the exchange-ordered copy of the pair (erfc) tables against the largest the path takes
inline bool exl_pair_tables_fit(int ntt, int Ntab, int E, int p, double max_bytes) {
  return !((double)ntt * Ntab * E * E * p * p * p * p * sizeof(double) > max_bytes);
}
inline bool exl_run_fits(int nj) { return !(nj > EXL_RUN_MAX); }

// ---- angular stage ----
inline size_t exl_alpha_lds(int ntt, int Nd) { return (size_t)(ntt == 4 ? 2 : 1) * Nd * sizeof(double); }
/// k_exl_alpha (true) or k_exl_alpha_gen
inline bool exl_alpha_fast(int p, int E, size_t alds) { return !(p > EXL_AP || E * p > 512 || alds > EXL_LDS_MAX); }
/// cross products by blocks of equal m: they need the M-major column order, which only the fast alpha kernel writes
inline bool exl_grouped(bool pair, int nruns, bool alpha_fast, const ExlSwitches &sw) {
  return !pair && nruns > 1 && alpha_fast && sw.mgroups;
}

// ---- RB kernel ----
inline ExlRB exl_rb_kernel(bool pair, int p, const ExlSwitches &sw) {
  if (pair) return ExlRB::pair;
  const bool rb_one = sw.rb == 1, rb_four = sw.rb == 4;
  if (!rb_one && !rb_four && p <= 16) return ExlRB::mfma;
  if (rb_one || p > 16) return ExlRB::one_pair;
  return ExlRB::rb4;
}
/// LDS of the one-pair kernels (k_exl_RB, k_exl_RB_pair), which stage all (channel, factor) columns at once
inline size_t exl_one_pair_lds(int max_nch, int r, int p) { return (size_t)(4 * max_nch * r * p + max_nch * r) * sizeof(double); }
/// false: the build declines (the largest group's columns do not fit)
inline bool exl_rb_fits(ExlRB rb, int max_nch, int rmax, int p) {
  const bool one_pair = rb == ExlRB::pair || rb == ExlRB::one_pair;
  return !(one_pair && exl_one_pair_lds(max_nch, rmax, p) > EXL_LDS_MAX);
}

// ---- cross-element products ----
inline long exl_tiles128(long M, long N) { return ((M + 127) / 128) * ((N + 127) / 128); }
struct ExlCross {
  bool split = false;             // two half-K workgroups per tile into a zeroed G (split2)
  ExlTile tile = ExlTile::Auto;   // Auto: the default task-list tiles
  bool worklist = false;          // XCD-contiguous work list; else the task-list grid
};
/// ncol = NLM * r columns of ONE density (group), tiles = its products' 128 x 128 tiles
inline ExlCross exl_cross(long ncol, long tiles, bool grouped, const ExlSwitches &sw) {
  ExlCross c;
  c.split = sw.splitk && tiles < EXL_SPLIT_MAX_TILES && ncol >= EXL_SPLIT_MIN_COLS;
  if (!c.split) return c;
  c.tile = (sw.crect && grouped) ? ExlTile::T128x64 : ExlTile::T128;
  c.worklist = c.tile == ExlTile::T128x64 && sw.wl;
  return c;
}

// ---- element GEMM ----
struct ExlElem {
  ExlTile tile = ExlTile::Auto;   // Auto (task list only): the launcher's choice
  bool worklist = false;
};
/// pairs: pair columns of ONE density over all tasks; ntasks: tasks of the build
inline ExlElem exl_elem(double pairs, size_t ntasks, const ExlSwitches &sw) {
  const int rect_env = sw.rect;
  const bool rect_tiles = rect_env >= 0 ? rect_env != 0 : (pairs < EXL_ELEM_LONG_PAIRS * (double)ntasks);
  ExlElem e;
  e.worklist = sw.wl;
  if (sw.wl) {
    const int tile_mode = rect_env >= 0 ? rect_env : (rect_tiles ? 2 : 0);
    e.tile = tile_mode == 2 ? ExlTile::T64 : tile_mode == 1 ? ExlTile::T128x64 : ExlTile::T128;
  } else
    e.tile = rect_tiles ? ExlTile::T128x64 : ExlTile::Auto;
  return e;
}

// ---- batched build ----
/// the table sets whose batches run the batched stages: those whose single build takes the matrix-core RB kernel and the
/// fast alpha kernel; run_nj: shells per m-run
inline bool exl_batch_takes(long N, bool pair, int p, int E, int ntt, int Nd, const int *run_nj, int nruns, const ExlSwitches &sw) {
  if (!exl_order_fits(N)) return false;
  if (exl_rb_kernel(pair, p, sw) != ExlRB::mfma) return false;
  if (!exl_alpha_fast(p, E, exl_alpha_lds(ntt, Nd))) return false;
  for (int g = 0; g < nruns; g++)
    if (!exl_run_fits(run_nj[g])) return false;
  return true;
}

// ---- the record of a build ----
struct ExlPlanRecord {
  bool valid = false, batch = false;
  bool declined = false;  // handed to the general kernels (nothing below the ranks is then meaningful)
  int NLM = 0, A = 0, Ntab = 0, E = 0, p = 0;
  std::vector<int> run_shells;   // shells per m-run
  std::vector<int> ranks;        // factor groups of the single build, members of the chunk
  std::vector<int> cross_split;  // per group / member: were its cross products split
  bool alpha_fast = false, grouped = false;
  ExlRB rb = ExlRB::mfma;
  ExlTile cross_split_tile = ExlTile::Auto, cross_plain_tile = ExlTile::Auto, elem_tile = ExlTile::Auto;
  bool cross_worklist = false, elem_worklist = false;
  int n_cross_split = 0, n_cross_plain = 0, n_elem = 0;  // tasks (single build: of the last group)
  int cross_maxM = 0, cross_maxN = 0, max_pairs = 0;
  int cross_minK = 0, cross_maxK = 0;  // shortest and longest sum of a cross task
  int cross_skipped = 0;               // grouped: blocks (run, run) of one element pair that no channel reaches (G stays zero)
  bool elem_over = false;  // the element tasks carry the over-read flags
  int chunks = 0;          // batched build: chunks the last call ran through the batched stages

  /// a cross task of K summed columns
  void cross_task(int K) {
    cross_minK = (cross_minK == 0 || K < cross_minK) ? K : cross_minK;
    cross_maxK = K > cross_maxK ? K : cross_maxK;
  }
  void start(bool is_batch, int NLM_, int A_, int Ntab_, int E_, int p_) {
    const int keep = chunks;
    *this = ExlPlanRecord();
    chunks = keep;
    valid = true;
    batch = is_batch;
    NLM = NLM_, A = A_, Ntab = Ntab_, E = E_, p = p_;
  }
};

inline const char *exl_tile_name(ExlTile t) {
  return t == ExlTile::T64 ? "T64" : t == ExlTile::T128 ? "T128" : t == ExlTile::T128x64 ? "T128x64" : "Auto";
}
inline const char *exl_rb_name(ExlRB k) {
  return k == ExlRB::mfma ? "mfma" : k == ExlRB::rb4 ? "rb4" : k == ExlRB::one_pair ? "one_pair" : "pair";
}
inline std::string exl_plan_json(const ExlPlanRecord &r) {
  if (!r.valid) return "null";
  auto list = [](const std::vector<int> &v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); i++) s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "]";
  };
  auto flag = [](bool b) { return std::string(b ? "true" : "false"); };
  auto str = [](const char *s) { return "\"" + std::string(s) + "\""; };
  std::string s = "{";
  s += "\"batch\": " + flag(r.batch) + ", \"declined\": " + flag(r.declined);
  s += ", \"NLM\": " + std::to_string(r.NLM) + ", \"A\": " + std::to_string(r.A) + ", \"Ntab\": " + std::to_string(r.Ntab);
  s += ", \"E\": " + std::to_string(r.E) + ", \"p\": " + std::to_string(r.p);
  s += ", \"run_shells\": " + list(r.run_shells) + ", \"ranks\": " + list(r.ranks) + ", \"cross_split\": " + list(r.cross_split);
  s += ", \"alpha\": " + str(r.alpha_fast ? "k_exl_alpha" : "k_exl_alpha_gen") + ", \"grouped\": " + flag(r.grouped);
  s += ", \"rb\": " + str(exl_rb_name(r.rb));
  s += ", \"cross_split_tile\": " + str(exl_tile_name(r.cross_split_tile)) + ", \"cross_plain_tile\": " + str(exl_tile_name(r.cross_plain_tile));
  s += ", \"cross_launcher\": " + str(r.cross_worklist ? "worklist" : "tasklist");
  s += ", \"elem_tile\": " + str(exl_tile_name(r.elem_tile)) + ", \"elem_launcher\": " + str(r.elem_worklist ? "worklist" : "tasklist");
  s += ", \"elem_over\": " + flag(r.elem_over);
  s += ", \"n_cross_split\": " + std::to_string(r.n_cross_split) + ", \"n_cross_plain\": " + std::to_string(r.n_cross_plain);
  s += ", \"n_elem\": " + std::to_string(r.n_elem) + ", \"cross_maxM\": " + std::to_string(r.cross_maxM);
  s += ", \"cross_maxN\": " + std::to_string(r.cross_maxN) + ", \"max_pairs\": " + std::to_string(r.max_pairs);
  s += ", \"cross_minK\": " + std::to_string(r.cross_minK) + ", \"cross_maxK\": " + std::to_string(r.cross_maxK);
  s += ", \"cross_skipped\": " + std::to_string(r.cross_skipped);
  s += ", \"chunks\": " + std::to_string(r.chunks) + "}";
  return s;
}
}  // namespace helfem
