// Every hfg:: function that is defined in one translation unit of csrc/hip/ and called from another (or from a probe
// under tests/gpu_probe/), declared once, grouped by the file that defines it.  Default arguments live here and nowhere
// else.  The defining file includes this header too, so a definition that drifts from its declaration shows up as an
// ambiguous call or a missing-prototype warning (tests/test_internal_header_cpu.py).  Not a public header: the C ABI is
// include/helfem_gpu.h.  (set_error is declared in common.h; upload_basis_tables in tables.h.)
#pragma once
#include "common.h"
#include "tables.h"
#include "../host/scf.h"
#include "../host/eig_plan.h"

namespace hfg {

// gemm.hip: the FP64 tile engine.  One launcher for task lists, one for task lists with a work list.  GemmTile and GemmHow
// are plain data and live in host/eig_plan.h, beside the rules that choose them for the blocked eigensolve.
// kernel by (tile, variant); HELFEM_MFMA=4x4x4 reaches the plain, acc and map lists and gemm_dev:
//   {} / {T64} / {T128}           k_dgemm_tasklist<64, 64> or <128, 128>
//   {T128x64}                     k_dgemm_tasklist<128, 64>
//   {T64 or T128, acc}            k_dgemm_tasklist<.., true>      C = alpha A B + beta C, beta != 0 in every active task
//   {T64, map}                    k_dgemm_tasklist_map            GemmTask::amap and cmap set in every active task
//   {T128 or T128x64, split2}     k_dgemm_tasklist_split2<..>     beta == 0 tasks, C zeroed by the caller
//   {T64, T128 or T128x64, scatter}  k_dgemm_tasklist_scatter<..>  GemmTask::rmap and cmap set in every active task, beta == 0
//   {T128 or T128x64, split2, scatter}  k_dgemm_tasklist_split2_scatter<..>  likewise, the mapped elements of C zeroed by the caller
//   {T64, scatter, klist}         k_dgemm_tasklist_klist        the scatter list with the k loop over GemmTask::kstart, nk (no transposes)
// anything else throws std::logic_error
void gemm_tasklist_dev(hfg_ctx *ctx, const GemmTask *dtasks, int ntasks, int maxM, int maxN, GemmHow how = {});  // gemm.hip
// k_dgemm_tasklist_wl<tile>; T64, T128 or T128x64, split2 with T128x64 only
void gemm_worklist_dev(hfg_ctx *ctx, const GemmTask *dtasks, const int2 *dwl, int nwg, GemmTile tile, bool split2 = false);  // gemm.hip
// host: (task, tile) or, split2, (task, 2 tile + half) for every tile of every non-empty task, in task order
void gemm_worklist(const std::vector<GemmTask> &tasks, GemmTile tile, bool split2, std::vector<int2> &out);  // gemm.hip
void gemm_mirror_lower_dev(hfg_ctx *ctx, const GemmTask *dtasks, int ntasks, int maxN);  // gemm.hip
int gemm_tile_slots(hfg_ctx *ctx);  // gemm.hip; workgroup slots of the large tiles: 2 x CUs, taken once per process
bool gemm_prefers_128(hfg_ctx *ctx, long tiles128);  // gemm.hip; helfem::gemm_prefers_128 on this chip and HELFEM_GEMM_TILE
void gemm_dev(hfg_ctx *ctx, bool tA, bool tB, int M, int N, int K, double alpha, const double *A, int lda, const double *B, int ldb,
              double beta, double *C, int ldc);  // gemm.hip

// fock.hip
void coulomb_dev(hfg_ctx *ctx, hfg_basis *basis, const double *dP, double *dJ);  // fock.hip
// nP densities, N x N each and one after the other, in one pass over the in-element tables per chunk (hfg_coulomb_batch_devptr)
void coulomb_batch_dev(hfg_ctx *ctx, hfg_basis *basis, int64_t nP, const double *dP, double *dJ);  // fock.hip
void coulomb_energy_matrix_dev(hfg_ctx *ctx, hfg_basis *basis, int64_t nP, const double *dP, double *dW);  // fock.hip
void set_xc_params(hfg_ctx *ctx, int x_func, const double *x_pars, int nx, int c_func, const double *c_pars, int nc);  // fock.hip
void xc_eval_host(int id, int nspin, size_t np, const double *rho, const double *sigma, const double *lapl, const double *tau,
                  double *exc, double *vrho, double *vsigma, double *vlapl, double *vtau, double thr);  // fock.hip
void xc_eval_host_ext(int id, const double *pars, int npars, int nspin, size_t np, const double *rho, const double *sigma,
                      const double *lapl, const double *tau, double *exc, double *vrho, double *vsigma, double *vlapl, double *vtau,
                      double thr);  // fock.hip
void xc_fock_dev(hfg_ctx *ctx, hfg_basis *basis, int x_func, int c_func, const double *dP, double *dH, double *dScal,
                 double thr);  // fock.hip
void xc_fock_pol_dev(hfg_ctx *ctx, hfg_basis *basis, int x_func, int c_func, const double *dPa, const double *dPb, double *dHa,
                     double *dHb, double *dScal, double thr);  // fock.hip
void model_potential_dev(hfg_ctx *ctx, hfg_basis *basis, int kind1, int Z1, double d1, double H1, int kind2, int Z2, double d2,
                         double H2, double *dH);  // fock.hip
void set_fock_blocks(hfg_ctx *ctx, hfg_basis *basis, const int *dBlockId);  // fock.hip
size_t fock_compact_size(hfg_basis *basis);  // fock.hip
void fock_compact_dev(hfg_ctx *ctx, hfg_basis *basis, int x_func, int c_func, const double *dP, double *dFc, double *dScal,
                      double thr);  // fock.hip
void fock_finish_dev(hfg_ctx *ctx, hfg_basis *basis, const double *dFc, const double *dH0, const int *dBlockId,
                     double *dF);  // fock.hip
// the unrestricted fused build: two slabs of fock_compact_size() doubles, J[Pa + Pb] + XC_a then J[Pa + Pb] + XC_b
void fock_compact_pol_dev(hfg_ctx *ctx, hfg_basis *basis, int x_func, int c_func, const double *dPa, const double *dPb,
                          double *dFc, double *dScal, double thr);  // fock.hip
void fock_finish_pol_dev(hfg_ctx *ctx, hfg_basis *basis, const double *dFc, const double *dH0, const int *dBlockId,
                         double *dFa, double *dFb);  // fock.hip

// exchange.hip, exchange_lr.hip
// the table set an exchange build reads: basis->dev (1/r12), basis->dev_rs (the screened kernel of hfg_rs_exchange) or
// basis->dev_mix (alpha 1/r12 + beta screened, exchange_mix.hip)
enum class ExTables { coulomb, screened, mix };
hfg_dev_tables *exchange_tables(hfg_basis *basis, ExTables which);  // exchange.hip; throws when the set is not there
void exchange_dev(hfg_ctx *ctx, hfg_basis *basis, const double *dP, double *dK, ExTables which = ExTables::coulomb,
                  const double *Lknown = nullptr, int rknown = 0);  // exchange.hip
bool exchange_lowrank_dev(hfg_ctx *ctx, hfg_dev_tables *t, const double *dP, double *dK, const double *Lknown,
                          int rknown);  // exchange_lr.hip
// nP densities in one pass over the exchange-ordered tables per chunk (hfg_exchange_batch_devptr); dC / nocc (host array) / ldc:
// nP sets of occupied columns as exchange_dev's Lknown, or null
void exchange_batch_dev(hfg_ctx *ctx, hfg_basis *basis, int64_t nP, const double *dP, double *dK, ExTables which = ExTables::coulomb,
                        const double *dC = nullptr, const int64_t *nocc = nullptr, int64_t ldc = 0);  // exchange_lr.hip
// what the last single and batched low-rank builds on a table set took (host/exl_plan.h), as JSON; a set that is not there
// or has not built yet gives null records
std::string exl_last_plan_json(hfg_basis *basis, ExTables which);  // exchange_lr.hip

// exchange_mix.hip
constexpr double EXL_PAIR_MAX_BYTES = 32e9;  // largest pair table the low-rank path takes (exchange_lowrank_dev) and the mixed set builds
// fills basis->dev_mix for (alpha, beta) from dev and dev_rs; 0: built or already there, 4: beyond EXL_PAIR_MAX_BYTES (nothing allocated)
int mix_exchange_tables_dev(hfg_ctx *ctx, hfg_basis *basis, double alpha, double beta);  // exchange_mix.hip

// tei_dev.hip
void compute_tei_dev(hfg_ctx *ctx, hfg_basis *basis);  // tei_dev.hip

// rs_tei_dev.hip
void compute_rs_tei_dev(hfg_ctx *ctx, hfg_basis *basis, int rs_kind, double omega);  // rs_tei_dev.hip
void rs_special_dev(hfg_ctx *ctx, int which, int L, const double *a, const double *b, size_t n, double *out);  // rs_tei_dev.hip

// eig.hip
void eig_sym_dev(hfg_ctx *ctx, int n, const double *dA, double *dE, double *dC);  // eig.hip
void eig_gsym_dev(hfg_ctx *ctx, int N, int n, const double *dF, const double *dS, double *dE, double *dC);  // eig.hip
void eig_gsym_sub_dev(hfg_ctx *ctx, int N, const double *dF, const double *dS, int nblk, const int64_t *blk_ptr,
                      const int64_t *blk_idx, double *dE, double *dC);  // eig.hip
void eig_gsym_sub_pair_dev(hfg_ctx *ctx, int N, const double *dFa, const double *dFb, const double *dS, int nblk,
                           const int64_t *blk_ptr, const int64_t *blk_idx, double *dEa, double *dCa, double *dEb,
                           double *dCb);  // eig.hip
size_t eig_block_buf_size(int nblk, const int64_t *blk_ptr);  // eig.hip
void eig_blocks_dev(hfg_ctx *ctx, int N, const double *dF, const double *dS, int nblk, const int64_t *blk_ptr,
                    const int64_t *blk_idx, double *dBlockBuf);  // eig.hip
void eig_assemble_dev(hfg_ctx *ctx, int N, int nblk, const int64_t *blk_ptr, const int64_t *blk_idx, const double *dBlockBuf,
                      double *dE, double *dC);  // eig.hip
void eig_block_supports(hfg_ctx *ctx, int N, const double *dS, int nblk, const int64_t *blk_ptr, const int64_t *blk_idx,
                        std::vector<int64_t> &cols);  // eig.hip
// the lowest min(nev, n_b) eigenpairs of every block (hfg_eig_sym_sel, hfg_eig_gsym_sub_sel): E has K = eig_sel_count values, C K columns
int64_t eig_sel_count(int nblk, const int64_t *blk_ptr, int64_t nev);  // eig.hip
void eig_sym_sel_dev(hfg_ctx *ctx, int n, const double *dA, int nev, double *dE, double *dC);  // eig.hip
void eig_gsym_sub_sel_dev(hfg_ctx *ctx, int N, const double *dF, const double *dS, int nblk, const int64_t *blk_ptr,
                          const int64_t *blk_idx, int nev, double *dE, double *dC);  // eig.hip

// hfg_ctx_declare_fock_band: the radial-element pattern of F for the blocked eigensolves under the current hfg_ctx_fix_sinvh;
// returns hfg_ctx::band_state (1 declared, 2 refused: dH0 has a non-zero entry outside the pattern)
int eig_declare_band(hfg_ctx *ctx, int N, const int *node, int pm, int E, const double *dH0, const int *dBlockId);  // eig.hip

// dc.hip, stsel.hip, trd.hip, trdp.hip: the stages of the eigensolver
void tridiag_dc_batch(hfg_ctx *ctx, int nblk, const int *ns, double *const *d, double *const *e, double *const *Z);  // dc.hip
int dc_status(hfg_ctx *ctx);  // dc.hip
int *dc_status_word(hfg_ctx *ctx);  // dc.hip
void tridiag_sel_batch(hfg_ctx *ctx, int nblk, const int *ns, const int *nev, double *const *d, double *const *e, double *const *W,
                       double *const *Z);  // stsel.hip
void tridiagonalize_batch(hfg_ctx *ctx, int nblk, const int *ns, double *const *A, double *const *d, double *const *e,
                          double *const *tau);  // trd.hip
void trd_measure_gemv(hfg_ctx *ctx, double *ms, int64_t *launches);  // trd.hip
bool tridiagonalize_takes_chain(int nblk, const int *ns);  // trdp.hip
void tridiagonalize_persistent(hfg_ctx *ctx, int nblk, const int *ns, double *const *A, double *const *d, double *const *e,
                               double *const *tau, std::vector<char> &done);  // trdp.hip
void trdp_check_status(hfg_ctx *ctx);  // trdp.hip

// misc.hip
void form_sinvh_dev(hfg_ctx *ctx, int N, const double *dS, bool chol, int nblk, const int64_t *blk_ptr, const int64_t *blk_idx,
                    double *dSinvh);  // misc.hip
void form_density_dev(hfg_ctx *ctx, int N, int ncols, const double *dC, int nocc, double *dP);  // misc.hip

// diis_dev.hip: the launchers of the device-resident DIIS object (hfg_diis_*)
constexpr int DIIS_LR_MAXCOLS = 64;  // occupied columns the low-rank error kernel takes; more go through the dense products
constexpr int DIIS_HIST_CHUNK = 8;   // stored entries per history pass
// err = A B^T - B A^T of order n from two n x k factors (leading dimension ld), written to out (leading dimension ldo)
struct DiisErrTask {
  const double *A, *B;
  double *out;
  int n, k, ld, ldo;
};
// the stored entries of one history pass: error, density and Fock matrices, all spins of an entry back to back
struct DiisHistory {
  const double *E[DIIS_HIST_CHUNK], *P[DIIS_HIST_CHUNK], *F[DIIS_HIST_CHUNK];
  int n;
};
struct DiisComb {
  const double *F[16];
  double w[16];
  int n;
};
size_t diis_lowrank_partials(int ntasks, int nmax);  // diis_dev.hip
// every task's error matrix and *dMax = max |err| over all of them; dPartialMax: diis_lowrank_partials() doubles
void diis_lowrank_error_dev(hfg_ctx *ctx, const DiisErrTask *dtasks, int ntasks, int nmax, double *dPartialMax,
                            double *dMax);  // diis_dev.hip
// dRes[1 + j0 + k] = Enew . E_k, dRes[1 + nhtot + j0 + k] = P_k . Fnew, dRes[1 + 2 nhtot + j0 + k] = Pnew . F_k for the h.n
// entries of the pass; want_max: dRes[0] = max |Enew|.  dPartial: (3 DIIS_HIST_CHUNK + 1) x 1024 doubles
void diis_history_dev(hfg_ctx *ctx, const DiisHistory &h, int j0, int nhtot, const double *dEnew, size_t elen, const double *dPnew,
                      const double *dFnew, size_t flen, bool want_max, double *dPartial, double *dRes);  // diis_dev.hip
// dFa = sum_k w_k F_k[0 : NN], dFb = sum_k w_k F_k[NN : 2 NN] (nspin == 2)
void diis_extrapolate_dev(hfg_ctx *ctx, const DiisComb &c, size_t NN, int nspin, double *dFa, double *dFb);  // diis_dev.hip

// cuhf_dev.hip: the constrained-UHF form of ROHF (scf::ROHF_update) on device pointers
constexpr int CUHF_LR_MAXCOLS = 128;  // occupied columns of both spins together that the low-rank route takes
// Fa += lambda, Fb -= lambda from the occupied orbitals (N x nocca, N x noccb) and S: rank nocca + noccb work
void cuhf_lowrank_dev(hfg_ctx *ctx, int N, const double *dS, const double *dCa, int nocca, const double *dCb, int noccb, double *dFa,
                      double *dFb);  // cuhf_dev.hip
// the dense sequence of the SCF driver from P = Pa + Pb, Sh (N x n, Sh^T Sinvh = 1) and Sinvh (N x n)
void cuhf_dense_dev(hfg_ctx *ctx, int N, int n, const double *dP, const double *dSh, const double *dSinvh, int nocca, int noccb,
                    double *dFa, double *dFb);  // cuhf_dev.hip

// occupy.hip: fractional occupations by symmetry block (hfg_occupy_blocks_devptr)
void occupy_blocks_dev(hfg_ctx *ctx, int64_t N, int64_t ncols, const double *dE, const double *dC, const int *dBlockId, int nblk,
                       const int64_t *occ_ptr, const double *occ, double *dCocc, double *dEocc, double *dFocc);  // occupy.hip

// the next call counts the rows per block anew (hfg_occupy_forget_blocks)
void occupy_forget_blocks(hfg_ctx *ctx);  // occupy.hip

// scf_device.hip
helfem::scf::Result scf_device_loop(hfg_ctx *ctx, hfg_basis *hb, const helfem::scf::Options &opt, int nel, double Enucr, int symm,
                                    const std::vector<std::vector<size_t> > &dsym, int ldft, int mdft,
                                    const std::vector<std::vector<std::vector<size_t> > > &avg_idx =
                                        std::vector<std::vector<std::vector<size_t> > >());  // scf_device.hip

}  // namespace hfg
