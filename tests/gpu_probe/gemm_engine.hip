// Direct access to the launchers of the FP64 GEMM tile engine (helfem_amd/csrc/hip/gemm.hip) for
// tests/test_gpu_gemm_engine.py: one call uploads the operand buffers and a list of task descriptions, runs ONE named
// launcher once and copies the WHOLE C buffer back, padding included.  A probe library of its own
// (tests/gpu_probe/libgemm_engine_probe.so, linked against libhelfem_amd.so); the product library gains no entry point.
#include "../../helfem_amd/csrc/hip/internal.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>

using namespace hfg;
#define HFG_TRY try {
#define HFG_CATCH                       \
  }                                     \
  catch (const std::exception &e) {     \
    hfg::set_error(e.what());           \
    return 2;                           \
  }                                     \
  return 0;

namespace {
// launcher numbers of probe_gemm_launch (tests/gemm_engine_worker.py holds the same table)
enum Launcher {
  L_GEMM = 0,         // gemm_dev on task 0
  L_TASKLIST = 1,     // gemm_tasklist_dev, {}: Auto
  L_TASKLIST64 = 2,   // {T64}
  L_RECT = 3,         // {T128x64}
  L_ACC = 4,          // {T64 (flag != 0) or T128, acc}
  L_MAP64 = 5,        // {T64, map}
  L_SPLIT2 = 6,       // {T128, split2}
  L_SPLIT2_RECT = 7,  // {T128x64, split2}
  L_WL = 8,           // gemm_worklist_dev, flag = tiles (0: T128, 1: T128x64, 2: T64)
  L_WL_SPLIT2_RECT = 9,  // gemm_worklist_dev, T128x64 with split2
  L_MIRROR = 10       // gemm_mirror_lower_dev (maxN)
};
constexpr int TI = 16;  // integers per task description
}  // namespace

extern "C" {
int probe_gemm_launch(hfg_ctx *ctx, int launcher, int flag, int ntasks, const int64_t *ti, const double *td, const double *A,
                      int64_t nA, const double *B, int64_t nB, double *C, int64_t nC, const int *maps, int64_t nmaps, int maxM,
                      int maxN, int *nwg_out);
int probe_gemm_worklist(int ntasks, const int *mn, int tile, int split2, int *out, int cap, int *n_out);

// ti[t * 16 + ...]: 0 offA, 1 offB, 2 offC (elements inside the buffers A, B, C), 3 M, 4 N, 5 K, 6 lda, 7 ldb, 8 ldc, 9 tA,
// 10 tB, 11 sym, 12 over, 13 / 14 offsets of amap / cmap inside `maps` (-1: none); td[t * 2 + ...]: alpha, beta.
// The work-list launchers get their list from gemm_worklist, as exchange_lr.hip does; *nwg_out receives its length.
int probe_gemm_launch(hfg_ctx *ctx, int launcher, int flag, int ntasks, const int64_t *ti, const double *td, const double *A,
                      int64_t nA, const double *B, int64_t nB, double *C, int64_t nC, const int *maps, int64_t nmaps, int maxM,
                      int maxN, int *nwg_out) {
  HFG_TRY
  HFG_HIP_CHECK(hipSetDevice(ctx->device));
  if (ntasks < 1) throw std::logic_error("probe_gemm_launch: no task");
  DevBuf<double> dA, dB, dC;
  DevBuf<int> dmaps;
  DevBuf<GemmTask> dtasks;
  DevBuf<int2> dwl;
  dA.resize((size_t)std::max<int64_t>(nA, 1));
  dB.resize((size_t)std::max<int64_t>(nB, 1));
  dC.resize((size_t)std::max<int64_t>(nC, 1));
  dmaps.resize((size_t)std::max<int64_t>(nmaps, 1));
  if (nA > 0) HFG_HIP_CHECK(hipMemcpy(dA.p, A, sizeof(double) * nA, hipMemcpyHostToDevice));
  if (nB > 0) HFG_HIP_CHECK(hipMemcpy(dB.p, B, sizeof(double) * nB, hipMemcpyHostToDevice));
  if (nC > 0) HFG_HIP_CHECK(hipMemcpy(dC.p, C, sizeof(double) * nC, hipMemcpyHostToDevice));
  if (nmaps > 0) HFG_HIP_CHECK(hipMemcpy(dmaps.p, maps, sizeof(int) * nmaps, hipMemcpyHostToDevice));
  std::vector<GemmTask> tasks(ntasks);
  for (int t = 0; t < ntasks; t++) {
    const int64_t *q = ti + (size_t)t * TI;
    GemmTask &g = tasks[t];
    memset((void *)&g, 0, sizeof(g));
    if (q[0] < 0 || q[0] > nA || q[1] < 0 || q[1] > nB || q[2] < 0 || q[2] > nC) throw std::logic_error("probe_gemm_launch: operand offset outside its buffer");
    g.A = dA.p + q[0];
    g.B = dB.p + q[1];
    g.C = dC.p + q[2];
    g.M = (int)q[3], g.N = (int)q[4], g.K = (int)q[5];
    g.lda = (int)q[6], g.ldb = (int)q[7], g.ldc = (int)q[8];
    g.tA = (int)q[9], g.tB = (int)q[10];
    g.alpha = td[2 * t], g.beta = td[2 * t + 1];
    g.sym = (int)q[11], g.over = (int)q[12];
    g.amap = q[13] >= 0 ? dmaps.p + q[13] : nullptr;
    g.cmap = q[14] >= 0 ? dmaps.p + q[14] : nullptr;
  }
  dtasks.resize(tasks.size());
  HFG_HIP_CHECK(hipMemcpy((void *)dtasks.p, (const void *)tasks.data(), sizeof(GemmTask) * tasks.size(), hipMemcpyHostToDevice));
  int nwg = 0;
  GemmTile wl_tile = GemmTile::Auto;
  if (launcher == L_WL || launcher == L_WL_SPLIT2_RECT) {
    wl_tile = launcher == L_WL_SPLIT2_RECT ? GemmTile::T128x64 : flag == 2 ? GemmTile::T64 : flag == 1 ? GemmTile::T128x64 : GemmTile::T128;
    std::vector<int2> wl;
    gemm_worklist(tasks, wl_tile, launcher == L_WL_SPLIT2_RECT, wl);
    nwg = (int)wl.size();
    dwl.resize(wl.size() ? wl.size() : 1);
    if (nwg) HFG_HIP_CHECK(hipMemcpy((void *)dwl.p, (const void *)wl.data(), sizeof(int2) * wl.size(), hipMemcpyHostToDevice));
  }
  if (nwg_out) *nwg_out = nwg;
  const GemmTask &g0 = tasks[0];
  switch (launcher) {
    case L_GEMM: gemm_dev(ctx, g0.tA != 0, g0.tB != 0, g0.M, g0.N, g0.K, g0.alpha, g0.A, g0.lda, g0.B, g0.ldb, g0.beta, g0.C, g0.ldc); break;
    case L_TASKLIST: gemm_tasklist_dev(ctx, dtasks.p, ntasks, maxM, maxN); break;
    case L_TASKLIST64: gemm_tasklist_dev(ctx, dtasks.p, ntasks, maxM, maxN, {GemmTile::T64}); break;
    case L_RECT: gemm_tasklist_dev(ctx, dtasks.p, ntasks, maxM, maxN, {GemmTile::T128x64}); break;
    case L_ACC: gemm_tasklist_dev(ctx, dtasks.p, ntasks, maxM, maxN, {flag != 0 ? GemmTile::T64 : GemmTile::T128, /*acc*/ true}); break;
    case L_MAP64: gemm_tasklist_dev(ctx, dtasks.p, ntasks, maxM, maxN, {GemmTile::T64, /*acc*/ false, /*split2*/ false, /*map*/ true}); break;
    case L_SPLIT2: gemm_tasklist_dev(ctx, dtasks.p, ntasks, maxM, maxN, {GemmTile::T128, /*acc*/ false, /*split2*/ true}); break;
    case L_SPLIT2_RECT: gemm_tasklist_dev(ctx, dtasks.p, ntasks, maxM, maxN, {GemmTile::T128x64, /*acc*/ false, /*split2*/ true}); break;
    case L_WL: gemm_worklist_dev(ctx, dtasks.p, dwl.p, nwg, wl_tile); break;
    case L_WL_SPLIT2_RECT: gemm_worklist_dev(ctx, dtasks.p, dwl.p, nwg, wl_tile, true); break;
    case L_MIRROR: gemm_mirror_lower_dev(ctx, dtasks.p, ntasks, maxN); break;
    default: throw std::logic_error("probe_gemm_launch: unknown launcher");
  }
  HFG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (nC > 0) HFG_HIP_CHECK(hipMemcpy(C, dC.p, sizeof(double) * nC, hipMemcpyDeviceToHost));
  HFG_CATCH
}

// gemm_worklist alone (host work): tasks of mn[2 t] rows and mn[2 t + 1] columns; tile 1: 64 x 64, 2: 128 x 128, 3: 128 x 64
// (the values of GemmTile); out receives the first `cap` (task, entry) pairs, *n_out the length of the list
int probe_gemm_worklist(int ntasks, const int *mn, int tile, int split2, int *out, int cap, int *n_out) {
  HFG_TRY
  std::vector<GemmTask> tasks(ntasks);
  for (int t = 0; t < ntasks; t++) {
    memset((void *)&tasks[t], 0, sizeof(GemmTask));
    tasks[t].M = mn[2 * t], tasks[t].N = mn[2 * t + 1];
  }
  std::vector<int2> wl;
  gemm_worklist(tasks, (GemmTile)tile, split2 != 0, wl);
  *n_out = (int)wl.size();
  for (int i = 0; i < std::min(cap, *n_out); i++) out[2 * i] = wl[i].x, out[2 * i + 1] = wl[i].y;
  HFG_CATCH
}
}
