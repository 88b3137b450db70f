// The planner of the banded F X (helfem_amd/csrc/host/eig_band_plan.h) against brute force, as a stand-alone program (host
// only: it includes the planner's header and nothing else of the library).  tests/test_eig_band_cpu.py compiles it with
// -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../helfem_amd/csrc/host/eig_band_plan.h"

static int failures = 0;
static void fail(const char *what, const char *why) {
  std::printf("%s: %s\n", what, why);
  failures++;
}

// two radial nodes share an element: restated from the elements' node lists, not from the planner's range
static bool share(int n, int m, int pm, int E) {
  for (int e = 0; e < E; e++)
    if (n >= e * pm && n <= e * pm + pm && m >= e * pm && m <= e * pm + pm) return true;
  return false;
}

// one symmetry block in the callers' order: shell-major, `skip` shells without the first node, the last node absent
static void check(const char *what, int E, int p, int shells, int skip, bool want_dense) {
  const int pm = p - 1, R = E * pm;  // nodes 0 .. R-1 (the boundary function at the far end is not in the basis)
  std::vector<int> node;
  for (int s = 0; s < shells; s++)
    for (int n = (s < skip ? 1 : 0); n < R; n++) node.push_back(n);
  const int64_t n = (int64_t)node.size();
  const int nt = (int)((n + 63) / 64);
  std::vector<int64_t> perm(n, -1);  // exactly n entries: a write beyond them is the sanitizer's to find
  std::vector<int> kstart, toff;
  helfem::eig_band_order(n, node.data(), perm.data());
  std::vector<char> seen(n, 0);
  for (int64_t i = 0; i < n; i++) {
    if (perm[i] < 0 || perm[i] >= n || seen[perm[i]]) return fail(what, "perm is no permutation");
    seen[perm[i]] = 1;
    if (i && (node[perm[i]] < node[perm[i - 1]] || (node[perm[i]] == node[perm[i - 1]] && perm[i] < perm[i - 1])))
      return fail(what, "not ordered by (node, position)");
  }
  const bool banded = helfem::eig_band_plan(n, node.data(), perm.data(), pm, E, kstart, toff);
  if (banded == want_dense) return fail(what, want_dense ? "expected the dense product" : "expected row tasks");
  if ((int)toff.size() != nt + 1 || toff[0] != 0 || toff[nt] != (int)kstart.size()) return fail(what, "tile offsets");
  double covered = 0.0;
  for (int t = 0; t < nt; t++) {
    if (toff[t + 1] <= toff[t]) return fail(what, "a tile without steps");
    for (int q = toff[t]; q < toff[t + 1]; q++) {
      if (kstart[q] < 0 || kstart[q] >= n || kstart[q] % helfem::EIG_BAND_K0_ALIGN != 0) return fail(what, "step outside [0, n) or not aligned");
      if (q > toff[t] && kstart[q] < kstart[q - 1] + helfem::EIG_BAND_KSTEP) return fail(what, "steps overlap or descend");
    }
    if (!banded && toff[t + 1] - toff[t] != (int)((n + 15) / 16)) return fail(what, "a dense block with steps left out");
    covered += (double)(toff[t + 1] - toff[t]);
  }
  // rows radial-major, columns in the callers' order
  for (int64_t i = 0; i < n; i++)
    for (int64_t j = 0; j < n; j++)
      if (share(node[perm[i]], node[j], pm, E)) {
        const int t = (int)(i / 64);
        bool in = false;
        for (int q = toff[t]; q < toff[t + 1]; q++) in = in || (j >= kstart[q] && j < kstart[q] + helfem::EIG_BAND_KSTEP);
        if (!in) return fail(what, "a pair that shares an element lies in no step of its tile");
      }
  std::printf("%s: ok (n = %ld, %d tiles, %s, %.0f %% of the dense k steps)\n", what, (long)n, nt, banded ? "row tasks" : "dense",
              100.0 * covered / ((double)nt * (double)((n + 15) / 16)));
}

int main() {
  check("(E, p, shells) = (3, 8, 7)", 3, 8, 7, 0, false);
  check("(3, 8, 7), first node missing in 3 shells", 3, 8, 7, 3, false);
  check("(5, 15, 3)", 5, 15, 3, 0, false);
  check("(5, 15, 3), first node missing in 1 shell", 5, 15, 3, 1, false);
  check("(2, 4, 1): a single row tile", 2, 4, 1, 0, true);
  check("(5, 15, 21): the benchmark's block", 5, 15, 21, 7, false);
  check("(5, 8, 5): order 175, no multiple of 64", 5, 8, 5, 0, false);
  check("(1, 15, 9): one element, everything shares it", 1, 15, 9, 0, true);
  check("(4, 9, 13), odd order 411", 4, 9, 13, 5, false);
  check("(4, 5, 13): elements of 4 nodes, finer than a k step", 4, 5, 13, 5, true);
  std::printf(failures ? "band plan check FAILED\n" : "band plan check ok\n");
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
