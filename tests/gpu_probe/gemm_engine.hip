// Direct access to the launchers of the FP64 GEMM tile engine (helfem_amd/csrc/hip/gemm.hip) for
// tests/test_gpu_gemm_engine.py: one call uploads the operand buffers and a list of task descriptions, runs ONE named
// launcher once and copies the WHOLE C buffer back, padding included.  A probe library of its own
// (tests/gpu_probe/libgemm_engine_probe.so, linked against libhelfem_amd.so); the product library gains no entry point.
#include "../../helfem_amd/csrc/hip/common.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace hfg {
void gemm_dev(hfg_ctx *ctx, bool tA, bool tB, int M, int N, int K, double alpha, const double *A, int lda, const double *B, int ldb,
              double beta, double *C, int ldc);
void gemm_tasklist_dev(hfg_ctx *ctx, const GemmTask *dtasks, int ntasks, int maxM, int maxN);
void gemm_tasklist64_dev(hfg_ctx *ctx, const GemmTask *dtasks, int ntasks, int maxM, int maxN);
void gemm_tasklist_rect_dev(hfg_ctx *ctx, const GemmTask *dtasks, int ntasks, int maxM, int maxN);
void gemm_tasklist_acc_dev(hfg_ctx *ctx, const GemmTask *dtasks, int ntasks, int maxM, int maxN, bool tile64);
void gemm_tasklist64_map_dev(hfg_ctx *ctx, const GemmTask *dtasks, int ntasks, int maxM, int maxN);
void gemm_tasklist_split2_dev(hfg_ctx *ctx, const GemmTask *dtasks, int ntasks, int maxM, int maxN);
void gemm_tasklist_split2_rect_dev(hfg_ctx *ctx, const GemmTask *dtasks, int ntasks, int maxM, int maxN);
void gemm_tasklist_wl_dev(hfg_ctx *ctx, const GemmTask *dtasks, const int2 *dwl, int nwg, int tiles);
void gemm_tasklist_wl_split2_rect_dev(hfg_ctx *ctx, const GemmTask *dtasks, const int2 *dwl, int nwg);
void gemm_mirror_lower_dev(hfg_ctx *ctx, const GemmTask *dtasks, int ntasks, int maxN);
}  // namespace hfg

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
  L_TASKLIST = 1,     // gemm_tasklist_dev
  L_TASKLIST64 = 2,   // gemm_tasklist64_dev
  L_RECT = 3,         // gemm_tasklist_rect_dev
  L_ACC = 4,          // gemm_tasklist_acc_dev, flag != 0: 64 x 64 tiles
  L_MAP64 = 5,        // gemm_tasklist64_map_dev
  L_SPLIT2 = 6,       // gemm_tasklist_split2_dev
  L_SPLIT2_RECT = 7,  // gemm_tasklist_split2_rect_dev
  L_WL = 8,           // gemm_tasklist_wl_dev, flag = tiles (0: 128 x 128, 1: 128 x 64, 2: 64 x 64)
  L_WL_SPLIT2_RECT = 9,  // gemm_tasklist_wl_split2_rect_dev
  L_MIRROR = 10       // gemm_mirror_lower_dev (maxN)
};
constexpr int TI = 16;  // integers per task description
}  // namespace

extern "C" {
// ti[t * 16 + ...]: 0 offA, 1 offB, 2 offC (elements inside the buffers A, B, C), 3 M, 4 N, 5 K, 6 lda, 7 ldb, 8 ldc, 9 tA,
// 10 tB, 11 sym, 12 over, 13 / 14 offsets of amap / cmap inside `maps` (-1: none); td[t * 2 + ...]: alpha, beta.
// The work-list launchers get their list from here: (task, tile) for every tile tm + nbm * tn of every task in task order,
// (task, 2 tile + half) for split K -- as exchange_lr.hip enumerates them; *nwg_out receives its length.
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
  if (launcher == L_WL || launcher == L_WL_SPLIT2_RECT) {
    const bool split = launcher == L_WL_SPLIT2_RECT;
    const int BM = (!split && flag == 2) ? 64 : 128, BN = (!split && flag == 0) ? 128 : 64;
    std::vector<int2> wl;
    for (int t = 0; t < ntasks; t++) {
      if (tasks[t].M <= 0 || tasks[t].N <= 0) continue;
      const int nt = ((tasks[t].M + BM - 1) / BM) * ((tasks[t].N + BN - 1) / BN);
      for (int q = 0; q < (split ? 2 * nt : nt); q++) wl.push_back(make_int2(t, q));
    }
    nwg = (int)wl.size();
    dwl.resize(wl.size() ? wl.size() : 1);
    if (nwg) HFG_HIP_CHECK(hipMemcpy((void *)dwl.p, (const void *)wl.data(), sizeof(int2) * wl.size(), hipMemcpyHostToDevice));
  }
  if (nwg_out) *nwg_out = nwg;
  const GemmTask &g0 = tasks[0];
  switch (launcher) {
    case L_GEMM: gemm_dev(ctx, g0.tA != 0, g0.tB != 0, g0.M, g0.N, g0.K, g0.alpha, g0.A, g0.lda, g0.B, g0.ldb, g0.beta, g0.C, g0.ldc); break;
    case L_TASKLIST: gemm_tasklist_dev(ctx, dtasks.p, ntasks, maxM, maxN); break;
    case L_TASKLIST64: gemm_tasklist64_dev(ctx, dtasks.p, ntasks, maxM, maxN); break;
    case L_RECT: gemm_tasklist_rect_dev(ctx, dtasks.p, ntasks, maxM, maxN); break;
    case L_ACC: gemm_tasklist_acc_dev(ctx, dtasks.p, ntasks, maxM, maxN, flag != 0); break;
    case L_MAP64: gemm_tasklist64_map_dev(ctx, dtasks.p, ntasks, maxM, maxN); break;
    case L_SPLIT2: gemm_tasklist_split2_dev(ctx, dtasks.p, ntasks, maxM, maxN); break;
    case L_SPLIT2_RECT: gemm_tasklist_split2_rect_dev(ctx, dtasks.p, ntasks, maxM, maxN); break;
    case L_WL: gemm_tasklist_wl_dev(ctx, dtasks.p, dwl.p, nwg, flag); break;
    case L_WL_SPLIT2_RECT: gemm_tasklist_wl_split2_rect_dev(ctx, dtasks.p, dwl.p, nwg); break;
    case L_MIRROR: gemm_mirror_lower_dev(ctx, dtasks.p, ntasks, maxN); break;
    default: throw std::logic_error("probe_gemm_launch: unknown launcher");
  }
  HFG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (nC > 0) HFG_HIP_CHECK(hipMemcpy(C, dC.p, sizeof(double) * nC, hipMemcpyDeviceToHost));
  HFG_CATCH
}
}
