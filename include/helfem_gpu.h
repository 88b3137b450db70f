/*
 * helfem_gpu.h — C ABI of the MI355X (gfx950) implementation of HelFEM's SCF hot path.
 *
 * The reference has no plugin/FFI layer: its hot path is a set of C++ member functions taking and
 * returning arma::mat (contiguous column-major double).  Each entry point below replaces one of
 * them; the C++ adapter with the reference's exact signatures is include/helfem_gpu_arma.hpp and
 * the binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - all matrices: column-major double, leading dimension = number of rows, caller-owned buffers;
 *   - matrices live in the *boundary-cleaned* N x N index space of the reference (Nbf), exactly
 *     what TwoDBasis::coulomb & friends take/return; the expansion to the Ndummy layout
 *     (basis.cpp:1754 expand_boundaries / :1735 remove_boundaries) happens inside the kernels;
 *   - "host" entry points take host pointers and copy through pinned staging; "_dev" entry points
 *     take pointers to HBM (e.g. torch tensors' data_ptr()) and enqueue on the context's stream
 *     without synchronising;
 *   - return value: 0 = success, non-zero = error, text via hfg_last_error() (thread-local).  The code is the class of
 *     the exception the reference throws in the same situation: 1 = std::logic_error (e.g. "Primitive teis have not
 *     been computed!" basis.cpp:1361), 2 = std::runtime_error (functional, shape and device errors, dftgrid.cpp:54),
 *     3 = any other; include/helfem_gpu_arma.hpp turns them back into those exceptions;
 *   - a context is bound to one device + one stream; one context per host thread.
 *   - there is NO CPU fallback: every compute entry point fails with an error when no gfx950
 *     device is usable.
 */
#ifndef HELFEM_GPU_H
#define HELFEM_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hfg_ctx hfg_ctx;
typedef struct hfg_basis hfg_basis;

/* ---- context ------------------------------------------------------------------------------ */
/* stream: a hipStream_t to enqueue on (e.g. torch.cuda.current_stream().cuda_stream), HFG_NULL_STREAM for the
 * device's default (null) stream -- which is what a framework's "current stream" handle 0 means: kernels must be
 * enqueued THERE to stay ordered with the framework's own operations and collectives -- or NULL to let the context
 * create its own non-blocking stream. */
#define HFG_NULL_STREAM ((void *)(intptr_t)-1)
int hfg_ctx_create(hfg_ctx **ctx, int device, void *stream);
int hfg_ctx_destroy(hfg_ctx *ctx);
int hfg_ctx_synchronize(hfg_ctx *ctx);
const char *hfg_last_error(void);
const char *hfg_version(void);
/* number of visible HIP devices (0 when there is none or the runtime is unusable) */
int hfg_device_count(void);

/* Multi-GPU sharding of the Fock build: this context computes only the contributions of its
 * shard (rank of nranks); the caller sums the partial matrices over ranks (one all-reduce over
 * RCCL).  Default (0,1) = everything. */
int hfg_ctx_set_shard(hfg_ctx *ctx, int rank, int nranks);

/* The caller's promise that the DEVICE matrix at dSinvh keeps its contents until the next call of this function
 * (NULL withdraws it): S^{-1/2} is fixed through an SCF run (diatomic/main.cpp:470-479 forms it once), so
 * hfg_eig_blocks_dev / hfg_eig_gsym_sub_dev derive the column supports of the symmetry blocks
 * (scf_helpers.cpp:150-157) from it once instead of in every iteration.  Without it every call re-derives them. */
int hfg_ctx_fix_sinvh(hfg_ctx *ctx, const double *dSinvh);

/* The caller's promise, beside hfg_ctx_fix_sinvh and until its next call, that every Fock matrix handed to the blocked
 * eigensolves with that Sinvh is local in the radial finite-element index: F(i, j) != 0 only where the radial functions of
 * i and j lie in a common element.  That holds for F = H0 + J + XC of every LDA / GGA / meta-GGA (and for DIIS
 * combinations of such matrices), not with exact or range-separated exchange and not under the CUHF constraint.  node[i]
 * (host, N values, 0 ... pm * E): radial node of basis function i; pm = nodes per element - 1; E elements.  The eigensolve
 * then takes the rows of every block of F radial-major and forms F X over the k steps that meet the non-zero columns of each
 * 64-row tile, columns and summation order as in the dense product: E and C are bit for bit those without the declaration
 * (HELFEM_EIG_BAND=0 ignores it).  dH0 (device, N x N, or
 * NULL): checked by one reduction, inside the blocks of dBlockId (device, N block ids, or NULL: everywhere); a non-zero
 * entry outside the pattern refuses the declaration without an error.  *state (may be NULL), and hfg_ctx_fock_band_state:
 * 0 no declaration, 1 declared, 2 refused.  hfg_ctx_declare_fock_band takes the pattern from the uploaded tables of basis. */
int hfg_ctx_declare_band(hfg_ctx *ctx, int64_t N, const int *node, int pm, int E, const double *dH0, const int *dBlockId, int *state);
int hfg_ctx_declare_fock_band(hfg_ctx *ctx, hfg_basis *basis, const double *dH0, const int *dBlockId, int *state);
int hfg_ctx_fock_band_state(hfg_ctx *ctx, int *state);
/* The plan behind it, no device needed: node[i] = radial node of position i of one block's index list (n values).  perm (n):
 * the positions radial-major, the ROW order of F in the product; tile t = rows perm[64 t ...] takes the k steps
 * kstart[toff[t] ... toff[t + 1]) (toff: (n + 63) / 64 + 1 values; kstart: cap values at most, ((n + 63) / 64) * ((n + 15) / 16)
 * always suffice): 16 columns each, in the caller's column order, ascending multiples of 4.  *banded: 0 when the block
 * keeps the dense product (every tile gets all steps). */
int hfg_eig_band_plan(int64_t n, const int *node, int pm, int E, int64_t *perm, int *toff, int *kstart, int64_t cap, int *banded);

/* ---- basis (host-side setup; no GPU needed) ------------------------------------------------
 * Constructor arguments of diatomic::basis::TwoDBasis (src/diatomic/basis.cpp:307):
 * Z1,Z2,Rhalf, primitive basis (only primbas 4 = LIP on Gauss-Lobatto nodes), n_quad, element
 * boundaries bval (mu values), angular shells (lval,mval), lpad. */
typedef struct {
  int Z1, Z2;
  double Rhalf;
  int primbas; /* must be 4 */
  int nnodes;
  int nquad;
  const double *bval;
  int nbval;
  const int *lval;
  const int *mval;
  int nang;
  int lpad;
} hfg_diatomic_desc;

int hfg_diatomic_basis_create(const hfg_diatomic_desc *desc, hfg_basis **basis);

/* Constructor arguments of helfem::atomic::basis::TwoDBasis (src/atomic/TwoDBasis.cpp:38-76) for the
 * point-nucleus case the atomic driver builds at src/atomic/main.cpp:268-273 (finitenuc = 0, no off-centre
 * charges, zeroder = 0; hfg_atomic_basis_create_ex takes the rest).  The handle is used with every hfg_basis_* / hfg_coulomb / hfg_exchange / hfg_xc_fock
 * entry below exactly like a diatomic one (replacing TwoDBasis::coulomb / exchange, TwoDBasis.cpp:817/957,
 * and atomic::dftgrid::DFTGrid::eval_Fxc, src/atomic/dftgrid.cpp:810). */
typedef struct {
  int Z;
  int primbas;   /* 4 = LIP on Gauss-Lobatto nodes (the default); others are rejected */
  int nnodes;
  int nquad;
  const double *bval; /* element boundaries in r, bval[0] = 0 */
  int nbval;
  const int *lval;
  const int *mval;
  int nang;
} hfg_atomic_desc;
int hfg_atomic_basis_create(const hfg_atomic_desc *desc, hfg_basis **basis);
/* The remaining constructor arguments of atomic::basis::TwoDBasis (TwoDBasis.cpp:38): finitenuc = nuclear model of the
 * central charge (modelpotential::nuclear_model_t: 0 point, 1 Gaussian, 2 uniformly charged sphere, 3 hollow sphere with
 * rms radius Rrms; 4 regularized nucleus with a = Rrms), zeroder = zero derivative instead of zero value at
 * the last grid point (the last radial function is kept: Nbf grows by Nang; host matrices only, hfg_basis_upload and the SCF
 * drivers refuse such a basis because the device tables have no slot for that function), and point charges Zl at z = -Rmid, Zr at
 * z = +Rmid, which must lie on an element boundary.  hfg_basis_nuclear then returns the full nuclear attraction matrix
 * (TwoDBasis::nuclear, TwoDBasis.cpp:378-456), which couples l for off-centre charges. */
typedef struct {
  hfg_atomic_desc base;
  int finitenuc;
  double Rrms;
  int zeroder;
  int Zl, Zr;
  double Rmid;
} hfg_atomic_desc_ex;
int hfg_atomic_basis_create_ex(const hfg_atomic_desc_ex *desc, hfg_basis **basis);
/* TwoDBasis::confinement(N, R, iconf, V, shift) (TwoDBasis.cpp:480, RadialBasis::confinement_potential,
 * RadialBasis.cpp:412-455): iconf 1 polynomial sign(R) ((r - shift)/|R|)^N, 2 exponential, 3 barrier of height V beyond
 * shift, 4 Junquera et al. with r_c = the last grid point; iconf 0 gives zeros.  Atomic bases only; out is Nbf x Nbf. */
int hfg_basis_confinement(const hfg_basis *basis, int iconf, int N, double R, double V, double shift, double *out);
/* atomic::basis::form_grid (src/atomic/basis.cpp:119-172): the element boundaries of the atomic program for a finite
 * nucleus (nelem0 elements up to the nuclear radius, twice, then nelem elements), for off-centre charges (a boundary at
 * Rmid with nelem0 elements inside it per segment) or neither (hfg_radial_grid), plus a boundary at shift_conf when add_conf
 * is set and none is there.  n in: capacity of bval, out: number of boundaries. */
int hfg_atomic_grid(int finitenuc, double Rrms, int nelem, double Rmax, int grid, double zexp, int nelem0, int grid0,
                    double zexp0, int Z, int Zl, int Zr, double Rmid, int add_conf, double shift_conf, double *bval, int *n);
/* atomic::basis::angular_basis (src/atomic/basis.cpp:174): shell list for --lmax/--mmax */
int hfg_angular_basis(int lmax, int mmax, int *lval, int *mval, int *nang /* in: capacity, out: count */);
int hfg_basis_destroy(hfg_basis *basis);
/* Nbf, Ndummy, Nrad, Nang, Nel (TwoDBasis::Nbf/Ndummy/Nrad/Nang, basis.cpp:457-480) */
int hfg_basis_dims(const hfg_basis *basis, int64_t *Nbf, int64_t *Ndummy, int64_t *Nrad, int64_t *Nang,
                   int64_t *Nel);
/* one-electron matrices, N x N  (TwoDBasis::overlap / kinetic / nuclear, basis.cpp:677/752/780) */
int hfg_basis_overlap(const hfg_basis *basis, double *S);
int hfg_basis_kinetic(const hfg_basis *basis, double *T);
int hfg_basis_nuclear(const hfg_basis *basis, double *V);
/* symmetry blocks (TwoDBasis::get_sym_idx, basis.cpp:561): blk_ptr has nblk+1 entries, blk_idx Nbf.
 * Pass blk_ptr = NULL to query nblk only. */
int hfg_basis_sym_blocks(const hfg_basis *basis, int symm, int *nblk, int64_t *blk_ptr, int64_t *blk_idx);
/* TwoDBasis::compute_tei (basis.cpp:1166): primitive two-electron integral tables (host, threaded) */
int hfg_compute_tei(hfg_basis *basis, int exchange);
/* Range-separated exchange tables of the atomic program: rs_kind 1 = TwoDBasis::compute_yukawa(omega)
 * (src/atomic/TwoDBasis.cpp:741), 2 = TwoDBasis::compute_erfc(omega) (:780).  Call before hfg_basis_upload, which
 * then also places the screened-kernel tables in HBM.  A diatomic basis fails like the reference driver
 * ("Range separated functionals are not supported.", src/diatomic/main.cpp:393). */
int hfg_compute_rs_tei(hfg_basis *basis, int rs_kind, double omega);
/* the same range-separated tables built on the GPU: the Bessel / Phi_L weights are evaluated and summed on the device and the
 * tables stay there in the layout hfg_basis_upload uses; the host keeps rs_kind and omega.  Follow with hfg_basis_upload.
 * hfg_basis_get_prim (12-15) reads them back through ctx.  Same refusal of a diatomic basis as hfg_compute_rs_tei. */
int hfg_compute_rs_tei_dev(hfg_ctx *ctx, hfg_basis *basis, int rs_kind, double omega);
/* the same tables built on the GPU (diatomic: host computes quadrature points and Legendre values, the
 * O(Nlm nq p^4) sums run on the device and the tables stay there); follow with hfg_basis_upload */
int hfg_compute_tei_dev(hfg_ctx *ctx, hfg_basis *basis, int exchange);
/* helpers of main.cpp:276-277: mu grid for --grid/--zexp, and (l,m) shell list for lmmax */
/* DIIS::get_w + solve_F (src/general/diis.cpp:214-290, 392-412): ADIIS + CDIIS weights of the Fock extrapolation from the
 * inner products of a history of n entries, oldest first: B[i*n+j] = err_i . err_j, T[i*n+j] = Tr(Pa_i Fa_j) + Tr(Pb_i Fb_j),
 * energies E[n], max |err| of the newest entry.  mode 0: mixed as the drivers run it (--diiseps / --diisthr), 1: CDIIS only,
 * 2: ADIIS only.  Host-side arithmetic (no GPU). */
int hfg_diis_weights(int n, const double *B, const double *T, const double *E, double maxerr, double diiseps, double diisthr,
                     int mode, double *w, int *dropped);

/* Device-resident DIIS accelerator: uDIIS::update / solve_F (src/general/diis.cpp:129-168, 392-412) on matrices that stay in
 * HBM.  The object keeps its own copies of F, P and the error Sinvh^T (F P S - S P F) Sinvh of up to `order` (<= 16) entries;
 * everything is queued on the context's stream, so the caller's buffers are free again when a call returns.  In steady
 * state update synchronises the stream once (the new row of B, row and column of T and max |err|: at most 3 order + 1
 * doubles); the first use of each ring slot, a change of nocc or of the route, and growth of a workspace add a
 * synchronisation for the upload of that slot's task list or an allocation.  solve does not synchronise.  An update that
 * fails empties the history.  All reductions run in a fixed order: two objects fed the same matrices give the same bits.
 * Matrices are column-major. */
typedef struct hfg_diis hfg_diis;
int hfg_diis_create(hfg_ctx *ctx, int64_t N, int nspin /*1|2*/, int order, double diiseps, double diisthr,
                    int mode /* as hfg_diis_weights: 0 mixed, 1 CDIIS, 2 ADIIS */, hfg_diis **d);
int hfg_diis_destroy(hfg_diis *d);
/* S (N x N) and Sinvh (N x n) in HBM; both are copied, so the caller may free them.  Empties the history and forgets the
 * blocks. */
int hfg_diis_set_metric_devptr(hfg_diis *d, const double *dS, const double *dSinvh, int64_t n);
/* optional symmetry blocks (host arrays as for hfg_eig_gsym_sub): the error is then formed per block.  Needs n = N, a
 * block-structured Sinvh and an empty history; F, P and S must be block diagonal.  nblk = 0 removes the blocks. */
int hfg_diis_set_blocks(hfg_diis *d, int nblk, const int64_t *blk_ptr, const int64_t *blk_idx);
/* new entry: energy E, Fock and density matrices of each spin (nspin = 1: dFb = dPb = NULL and the one spin counts twice,
 * as the restricted driver does); dC* / nocc*: the occupied orbitals P was formed from (P = C_o C_o^T, N x nocc), or NULL / 0.
 * With the orbitals of every spin that has electrons and at most 64 of them per spin the error comes from products with
 * nocc columns and the rank-nocc kernel; otherwise from the four dense products of the definition. */
int hfg_diis_update_devptr(hfg_diis *d, double E, const double *dFa, const double *dPa, const double *dCa, int64_t nocca,
                           const double *dFb, const double *dPb, const double *dCb, int64_t noccb, double *maxerr /* host */);
/* extrapolated Fock matrices into dFa / dFb (may alias the inputs of the last update); dropped: entries discarded */
int hfg_diis_solve_devptr(hfg_diis *d, double *dFa, double *dFb, int *dropped);
int hfg_diis_size(const hfg_diis *d);
/* test access: which 0 = B, 1 = T (size x size, row-major, oldest first), 2 = weights of the last solve (one per entry left),
 * 3 = error matrix of the newest entry (nspin x n x n, n the columns of Sinvh; N x N when Sinvh is square) */
int hfg_diis_get(hfg_diis *d, int which, double *out, int64_t cap);

/* Read-back of the setup tables (test and diagnostic access; basis.cpp:1166-1302 fills them):
 *   hfg_basis_lm_map: the sorted (L,|M|) channel list of the constructor (basis.cpp:333-375); n in: capacity, out: count
 *   hfg_basis_get_prim: which 0-3 prim_tei00/02/20/22, 4-7 prim_ktei00/02/20/22, 8-11 disjoint_P0/P2/Q0/Q2 of channel ilm and
 *   element iel, column-major in the reference's shape (rows/cols returned; out may be NULL to query the shape).  Tables built
 *   by hfg_compute_tei_dev are copied back from the device (ctx required).  Atomic handles: ilm = L; which 0 prim_tei[L],
 *   4 prim_ktei[L], 8 disjoint_L, 10 disjoint_m1L, and after hfg_compute_rs_tei 12 disjoint_iL, 13 disjoint_kL, 14 rs_tei,
 *   15 rs_ktei (erfc tables, one per element pair: iel * Nel + kel in place of iel); after hfg_compute_rs_tei_dev these four are
 *   copied back from the device (ctx required). */
/* arma::mat TwoDBasis::overlap(const TwoDBasis &rh)   basis.cpp:713 and atomic/TwoDBasis.cpp:330: interbasis overlap
 * <a|b>, Nbf(a) x Nbf(b), of two bases of the same program (the projection of a checkpoint's orbitals onto another
 * basis, --load) */
int hfg_basis_interbasis_overlap(const hfg_basis *a, const hfg_basis *b, double *S12);
int hfg_basis_lm_map(const hfg_basis *basis, int *L, int *M, int *n);
int hfg_basis_get_prim(hfg_ctx *ctx, const hfg_basis *basis, int which, int ilm, int iel, double *out, int64_t *rows,
                       int64_t *cols);
int hfg_radial_grid(double mumax, int nelem, int igrid, double zexp, double *bval /* nelem+1 */);
int hfg_lm_list(const int *lmmax, int nlm, int *lval, int *mval, int *nang /* in: capacity, out: count */);

/* host-side special functions (exposed for the parity tests against the reference's
 * gaunt_test / legendre_test / sphtest known answers) */
double hfg_gaunt_coefficient(int L, int M, int l, int m, int lp, int mp);          /* gaunt.cpp:35 */
double hfg_modified_gaunt_coefficient(int lj, int mj, int L, int M, int li, int mi); /* gaunt.cpp:55 */
void hfg_legendre_PQ(int Lmax, int Mmax, double xi, double *P, double *Q);           /* Legendre_Wrapper.f90:135,173 */
double hfg_theta_lm(int l, int m, double cth);                                       /* spherical_harmonics.cpp:25 */
double hfg_bessel_il(double x, int L);              /* utils::bessel_il, libhelfem/src/utils.cpp:47 */
double hfg_bessel_kl(double x, int L);              /* utils::bessel_kl, libhelfem/src/utils.cpp:59 */
double hfg_erfc_phi(int n, double Xi, double xi);   /* atomic::erfc_expn::Phi, libhelfem/src/erfc_expn.cpp:181 */
/* binomials of the short-range series of Phi: 0 exact (default), 1 the helper of erfc_expn.cpp:46-70 (the reference's
 * arithmetic); read by hfg_erfc_phi, hfg_compute_rs_tei and their device counterparts */
void hfg_set_erfc_binomial_mode(int mode);
/* the device versions of the three functions above (hip/special_dev.h), one launch: out[i] = i_L(a[i]) (which 0), k_L(a[i]) (1)
 * or Phi_L(a[i], b[i]) (2); a, b, out are host arrays of n entries (b is read for which 2 only) */
int hfg_rs_special_dev(hfg_ctx *ctx, int which, int L, const double *a, const double *b, int64_t n, double *out);
void hfg_chebyshev_rule(int n, double *x, double *w);                                /* chebyshev.cpp:22 */
void hfg_lobatto_nodes(int n, double *x);                                            /* lobatto.cpp:588 */

/* ---- tables -> HBM ------------------------------------------------------------------------- */
/* Uploads the Gaunt-coupling lists, disjoint/in-element integral tables and (ldft>0) the XC grid
 * tables (DFTGrid ctor, dftgrid.cpp:760) of this basis to the context's device. */
int hfg_basis_upload(hfg_ctx *ctx, hfg_basis *basis, int ldft, int mdft);

/* ---- per-iteration hot path, host-pointer API (drop-in for the arma::mat signatures) -------- */
/* arma::mat TwoDBasis::coulomb(const arma::mat & P) const            basis.h:247, basis.cpp:1359 */
int hfg_coulomb(hfg_ctx *ctx, hfg_basis *basis, const double *P, double *J);
/* J for nP densities in one pass over the in-element tables (per chunk of densities, DESIGN 3.1 "Batched J"): P and J
 * hold nP matrices of N x N, column-major, one after the other (density index last); J_b = hfg_coulomb(P_b), each P_b
 * symmetric.  nP = 0 does nothing and returns 0; nP < 0, a null pointer and a basis without uploaded tables are errors. */
int hfg_coulomb_batch(hfg_ctx *ctx, hfg_basis *basis, int64_t nP, const double *P, double *J);
/* W (nP x nP, column-major): W(a, b) = tr(P_a J[P_b]), summed on the device over the element-diagonal blocks, which are
 * all that J has and all of P that meets them.  Symmetric by the symmetry of the integrals; not symmetrised. */
int hfg_coulomb_energy_matrix(hfg_ctx *ctx, hfg_basis *basis, int64_t nP, const double *P, double *W);
/* arma::mat TwoDBasis::exchange(const arma::mat & P) const           basis.h:249, basis.cpp:1532 */
int hfg_exchange(hfg_ctx *ctx, hfg_basis *basis, const double *P, double *K);
/* arma::mat atomic::basis::TwoDBasis::rs_exchange(const arma::mat & P) const   TwoDBasis.h:184, TwoDBasis.cpp:1142 */
int hfg_rs_exchange(hfg_ctx *ctx, hfg_basis *basis, const double *P, double *K);
/* K for nP densities in one pass over the exchange-ordered element tables per chunk of densities (DESIGN 3.3 "Batched K"):
 * P and K hold nP matrices of N x N, column-major, one after the other; each P_b symmetric.  K_b is bitwise hfg_exchange(P_b)
 * (hfg_rs_exchange(P_b)): densities whose low-rank factors fit 64 columns together share a pass, a zero matrix gives an exact
 * zero, a density of more than 64 factors or of full rank takes the single build on its own, and so does every density of an
 * erfc basis.  nP = 0 does nothing and returns 0; nP < 0 and a null pointer are errors (status 1), as for hfg_coulomb_batch. */
int hfg_exchange_batch(hfg_ctx *ctx, hfg_basis *basis, int64_t nP, const double *P, double *K);
int hfg_rs_exchange_batch(hfg_ctx *ctx, hfg_basis *basis, int64_t nP, const double *P, double *K);
/* void DFTGrid::eval_Fxc(x_func,x_pars,c_func,c_pars,P,H,Exc,Nel,Ekin,thr)   dftgrid.h:179 (restricted).
 * Functional ids are libxc's; hfg_xc_func_table() lists the ones of this build, <= 0 is none.  Of a hybrid the DFT part is
 * evaluated: the caller adds alpha K + beta K_screened of hfg_xc_exact_exchange, the screened kernel being that of
 * hfg_xc_rs_kind.  The Laplacian-dependent functionals take atomic bases only (a diatomic basis fails with "Laplacian not
 * implemented!"); for the meta-GGAs Ekin returns the integral of tau.  The spin-polarised entry takes the same ids. */
int hfg_xc_fock(hfg_ctx *ctx, hfg_basis *basis, int x_func, int c_func, const double *P, double *H, double *Exc,
                double *Nel, double *Ekin, double dens_thr);
/* void DFTGrid::eval_Fxc(x_func,x_pars,c_func,c_pars,Pa,Pb,Ha,Hb,Exc,Nel,Ekin,beta,thr)   dftgrid.h:181,
 * dftgrid.cpp:812 (unrestricted; both spin matrices are always formed, i.e. beta = true) */
int hfg_xc_fock_pol(hfg_ctx *ctx, hfg_basis *basis, int x_func, int c_func, const double *Pa, const double *Pb,
                    double *Ha, double *Hb, double *Exc, double *Nel, double *Ekin, double dens_thr);
/* The same with the reference's full argument list (dftgrid.h:179/181): x_pars / c_pars are the external functional
 * parameters of --x_pars / --c_pars (xc_func_set_ext_params in the reference, dftgrid.cpp:405-410).  Supported: gga_x_pbe
 * (kappa, mu), gga_c_pbe (beta, gamma, B), lda_x (alpha), and (omega > 0) of gga_x_ityh, gga_x_sfat, gga_x_ityh_pbe,
 * gga_x_sfat_pbe; NULL / 0 keeps the functional's defaults; any other combination is refused with an error rather than
 * ignored. */
int hfg_xc_fock_ext(hfg_ctx *ctx, hfg_basis *basis, int x_func, const double *x_pars, int n_x_pars, int c_func,
                    const double *c_pars, int n_c_pars, const double *P, double *H, double *Exc, double *Nel, double *Ekin,
                    double dens_thr);
int hfg_xc_fock_pol_ext(hfg_ctx *ctx, hfg_basis *basis, int x_func, const double *x_pars, int n_x_pars, int c_func,
                        const double *c_pars, int n_c_pars, const double *Pa, const double *Pb, double *Ha, double *Hb,
                        double *Exc, double *Nel, double *Ekin, double dens_thr);
/* Point evaluation of one functional on host arrays in libxc's xc_mgga_exc_vxc layout (no context, no device): nspin 1:
 * rho, sigma, lapl, tau and exc, vrho, vsigma, vlapl, vtau one value per point; nspin 2: rho[2], sigma[3] (aa, ab, bb),
 * lapl[2], tau[2] per point, vrho, vsigma, vlapl, vtau likewise, exc per particle of the total density.  The same code as
 * the grid kernels, with their threshold rules (dens_thr; exchange channels below it are left out).  NULL inputs are
 * zero, NULL outputs are skipped; functionals without sigma / tau / lapl dependence return zero for those potentials. */
int hfg_xc_eval(int func_id, int nspin, int64_t np, const double *rho, const double *sigma, const double *lapl, const double *tau,
                double *exc, double *vrho, double *vsigma, double *vlapl, double *vtau, double dens_thr);
/* hfg_xc_eval with external parameters of the one functional for this call: pars / n_pars as hfg_xc_fock_ext takes them for
 * that id (lda_x, gga_x_pbe, gga_c_pbe, omega of the short-range GGA primitives); NULL / 0 is hfg_xc_eval. */
int hfg_xc_eval_ext(int func_id, const double *pars, int n_pars, int nspin, int64_t np, const double *rho, const double *sigma,
                    const double *lapl, const double *tau, double *exc, double *vrho, double *vsigma, double *vlapl, double *vtau,
                    double dens_thr);
/* --method parsing of the drivers (dftfuncs.cpp:64-118): "x-c" names or numeric ids -> libxc ids; and id -> name */
int hfg_xc_func_ids(const char *method, int *x_func, int *c_func);
const char *hfg_xc_func_name(int func_id);
/* Exact exchange the drivers add for an exchange id (range_separation, dftfuncs.cpp:505): K = alpha K[1/r12] + beta K[screened
 * kernel of range omega]; 1 for HF, 0.25 for hyb_gga_xc_pbeh and hyb_mgga_x_scan0, 0 for the pure functionals; for a CAM
 * hybrid with 1/r = [1 - a - b s(r)]/r + [a + b s(r)]/r: alpha = a + b, beta = -b (hyb_gga_xc_cam_b3lyp: 0.33, 0.65, -0.46) */
int hfg_xc_exact_exchange(int x_func, double *omega, double *alpha, double *beta);
/* The screened kernel of an exchange id (is_range_separated, dftfuncs.cpp:464): 0 none, 1 Yukawa exp(-omega r)/r, 2
 * erfc(omega r)/r -- the rs_kind hfg_compute_rs_tei needs for the beta term of hfg_xc_exact_exchange */
int hfg_xc_rs_kind(int x_func);
/* The functionals of this build (no context, no device), one line each, tab separated: id, name, role (x, c or xc), needs
 * the gradient, tau, the Laplacian (0 / 1 each), evaluated by the EXT instantiation of the grid kernels (0 no; 1 SCAN and the
 * PBE variants, 2 short-range GGA exchange primitive, 3 range-separated GGA hybrid), skipped as a whole where a spin channel
 * is below the density threshold, then kfrac, kshort, omega, rs_kind as hfg_xc_exact_exchange (alpha, beta) and hfg_xc_rs_kind
 * return them, the number of external parameters and the parameters they set, a remark.  buf / cap as hfg_tuning_table. */
int hfg_xc_func_table(char *buf, size_t cap);
/* Radial tables of an atomic basis at the quadrature points of element iel (nquad x Nprim(iel), column-major): which 0 =
 * B/r (RadialBasis::get_bf), 1 = d/dr (B/r) (get_df), 2 = d^2/dr^2 (B/r) (get_lf), 3 = the radial coordinates
 * (nquad x 1).  out = NULL returns the shape only. */
int hfg_basis_radial_table(const hfg_basis *basis, int which, int iel, double *out, int64_t *rows, int64_t *cols);
/* Initial-guess model potential: arma::mat TwoDGrid::model_potential(p1, p2) (src/diatomic/twodquadrature.cpp:351) on the
 * quadrature grid of hfg_basis_upload(ldft, mdft), or atomic::basis::TwoDBasis::model_potential(pot)
 * (src/atomic/TwoDBasis.cpp:458; the second centre is ignored).  kind: 0 point nucleus, 1 Green-Sellin-Zachor with the
 * screening length d (H = d (Z-1)^0.4 when H <= 0), 3 Thomas-Fermi (model_potential.cpp / gsz.cpp of the reference);
 * 2 (SAP) needs the reference's tabulation and fails with "Unsupported guess". */
typedef struct {
  int kind;
  int Z;
  double d, H;
} hfg_model_pot;
int hfg_model_potential(hfg_ctx *ctx, hfg_basis *basis, const hfg_model_pot *p1, const hfg_model_pot *p2, double *H);
/* --iguess of the drivers (0 core, 3 Thomas-Fermi) for the following hfg_scf_* calls of this thread */
int hfg_scf_set_iguess(int iguess);
/* void scf::eig_gsym(E,C,F,Sinvh): Sinvh is N x n                     scf_helpers.h:34, .cpp:131 */
int hfg_eig_gsym(hfg_ctx *ctx, int64_t N, int64_t n, const double *F, const double *Sinvh, double *E, double *C);
/* void scf::eig_gsym_sub(E,C,F,Sinvh,m_idx)                           scf_helpers.h:36, .cpp:142 */
int hfg_eig_gsym_sub(hfg_ctx *ctx, int64_t N, const double *F, const double *Sinvh, int nblk,
                     const int64_t *blk_ptr, const int64_t *blk_idx, double *E, double *C);
/* the two consecutive scf::eig_gsym_sub calls of an unrestricted iteration (diatomic/main.cpp:936-958: same Sinvh, same
 * blocks, Fa then Fb) as ONE batch: the blocks of both matrices share the tridiagonalisation's chain of launches */
int hfg_eig_gsym_sub_pair(hfg_ctx *ctx, int64_t N, const double *Fa, const double *Fb, const double *Sinvh, int nblk,
                          const int64_t *blk_ptr, const int64_t *blk_idx, double *Ea, double *Ca, double *Eb, double *Cb);
/* arma::eig_sym(E,C,A) as used by utils::invh                         libhelfem/src/utils.cpp:172 */
int hfg_eig_sym(hfg_ctx *ctx, int64_t n, const double *A, double *E, double *C);
/* Selected eigenpairs: from every symmetry block the lowest min(nev, n_b) eigenpairs (LAPACK users: dsyevx / dsygvx with
 * range = 'I'; the reference has no counterpart, it reaches LAPACK through arma::eig_sym on a submatrix only).
 * K = hfg_eig_sel_count() pairs come back: E ascending over all of them, ties between blocks ordered as hfg_eig_gsym_sub
 * orders them; column j of C (N x K, column-major) belongs to E[j], is S-orthonormal and zero outside its block's rows.
 * nev >= the largest block gives the eigenvalues of hfg_eig_gsym_sub; nev < 1 is an error (status 1).
 * Aufbau property, by construction: the globally lowest m <= nev values of the full spectrum are the first m returned (a
 * block holds at most m of them, and its lowest nev are all here), which is why an SCF caller may pass nev = nocc + nvirt.
 * HELFEM_EIGSEL = stein | dc forces the tridiagonal stage's path (multisection and inverse iteration | the full divide and
 * conquer followed by taking the lowest columns); unset, a crossover on the wanted fraction chooses per call. */
int64_t hfg_eig_sel_count(int nblk, const int64_t *blk_ptr, int64_t nev); /* K; needs no device */
/* one dense matrix: E (min(nev, n) values), C (n x min(nev, n)) */
int hfg_eig_sym_sel(hfg_ctx *ctx, int64_t n, const double *A, int64_t nev, double *E, double *C);
int hfg_eig_gsym_sub_sel(hfg_ctx *ctx, int64_t N, const double *F, const double *Sinvh, int nblk, const int64_t *blk_ptr,
                         const int64_t *blk_idx, int64_t nev, double *E /* K */, double *C /* N x K */);
/* arma::mat TwoDBasis::Sinvh(bool chol, int sym) -> block-structured S^{-1/2}   basis.cpp:627 */
int hfg_form_sinvh(hfg_ctx *ctx, int64_t N, const double *S, int chol, int nblk, const int64_t *blk_ptr,
                   const int64_t *blk_idx, double *Sinvh);
/* arma::mat scf::form_density(C, nocc): P = C(:,0:nocc) C(:,0:nocc)^T   scf_helpers.cpp:22 */
int hfg_form_density(hfg_ctx *ctx, int64_t N, int64_t ncols, const double *C, int64_t nocc, double *P);
/* C = op(A) op(B), FP64 MFMA (the dense products around the eigensolver and in DIIS) */
int hfg_gemm(hfg_ctx *ctx, int transA, int transB, int64_t m, int64_t n, int64_t k, const double *A, int64_t lda,
             const double *B, int64_t ldb, double *C, int64_t ldc);

/* ---- device-resident API (pointers into HBM, asynchronous on the context's stream) ---------- */
int hfg_coulomb_dev(hfg_ctx *ctx, hfg_basis *basis, const double *dP, double *dJ);
/* hfg_coulomb_batch on device pointers, honouring the context's shard like hfg_coulomb_dev (the partial J's of the ranks
 * sum to the whole).  Deliberately not named *_dev: the entries of that name are exactly the plan of
 * tests/stream_order_worker.py; this entry's stream ordering is tested in tests/test_gpu_coulomb_batch.py. */
int hfg_coulomb_batch_devptr(hfg_ctx *ctx, hfg_basis *basis, int64_t nP, const double *dP, double *dJ);
int hfg_exchange_dev(hfg_ctx *ctx, hfg_basis *basis, const double *dP, double *dK);
int hfg_rs_exchange_dev(hfg_ctx *ctx, hfg_basis *basis, const double *dP, double *dK);
/* TwoDBasis::exchange(Pa) as the SCF driver calls it (src/diatomic/main.cpp:822, src/atomic/main.cpp:767): the caller has
 * just formed dP = C_occ C_occ^T with scf::form_density from the nocc occupied orbitals dC (N x nocc, column-major, ld N)
 * and hands them over as the factors of dP, which saves the pivoted factorisation of dP and its verification. */
int hfg_exchange_occ_dev(hfg_ctx *ctx, hfg_basis *basis, const double *dP, const double *dC, int64_t nocc, double *dK);
/* hfg_exchange_batch / hfg_rs_exchange_batch on device pointers, honouring the context's shard like hfg_exchange_dev (the
 * partial K_b of the ranks sum to the whole); everything is queued on the context's stream and no argument is read after the
 * return.  hfg_exchange_occ_batch_devptr is hfg_exchange_occ_dev for nP densities: dC holds nP sets of occupied orbitals,
 * N x ldc_cols each (column-major, ld N), one after the other; the first nocc[b] columns of set b are the factors of P_b
 * (nocc: HOST array of nP counts, 0 <= nocc[b] <= ldc_cols; 0 gives K_b = 0).  Deliberately not named *_dev, like
 * hfg_coulomb_batch_devptr: the entries of that name are exactly the plan of tests/stream_order_worker.py; the stream ordering
 * of these is tested in tests/test_gpu_exchange_batch.py (the range-separated entry is the first one's code on the other
 * table set). */
int hfg_exchange_batch_devptr(hfg_ctx *ctx, hfg_basis *basis, int64_t nP, const double *dP, double *dK);
int hfg_rs_exchange_batch_devptr(hfg_ctx *ctx, hfg_basis *basis, int64_t nP, const double *dP, double *dK);
int hfg_exchange_occ_batch_devptr(hfg_ctx *ctx, hfg_basis *basis, int64_t nP, const double *dP, const double *dC,
                                  const int64_t *nocc, int64_t ldc_cols, double *dK);
/* The exact exchange of the range-separated hybrids, alpha K[1/r12] + beta K[screened kernel] (hfg_xc_exact_exchange), from
 * ONE build on a mixed-kernel table set (DESIGN 3.3a "Mixed-kernel set"; atomic handles only, a diatomic one gets "Range
 * separated functionals are not supported.").  hfg_mix_exchange_tables mixes the uploaded tables on the device, once: it
 * needs hfg_basis_upload with exchange tables and, for beta != 0, an uploaded range-separated set of either kind (status 1
 * with a text that names what is missing).  A second call with the same (alpha, beta) on unchanged tables does nothing;
 * hfg_basis_upload, hfg_compute_rs_tei and hfg_compute_rs_tei_dev drop the set, after which the exchange entries below fail
 * until it is rebuilt.  Status 4: the set would exceed the 32e9 bytes of the pair path, nothing was allocated and the caller
 * builds K from the two table sets.  The exchange entries are hfg_exchange_dev, hfg_exchange_occ_dev and
 * hfg_exchange_occ_batch_devptr (dC and nocc may both be NULL there) on that set: asynchronous on the context's stream,
 * honouring its shard, K_b of the batch bitwise that of the single entry.  Not named *_dev, like hfg_coulomb_batch_devptr;
 * their stream ordering is tested in tests/test_gpu_exchange_mix.py.  hfg_mix_exchange takes host pointers.
 * hfg_basis_get_prim with which = 16 reads one block of the set back: ilm = L, iel = e * Nel + f, the padded p^2 x p^2
 * block (rows: primitives of e, columns: primitives of f). */
int hfg_mix_exchange_tables(hfg_ctx *ctx, hfg_basis *basis, double alpha, double beta);
int hfg_mix_exchange(hfg_ctx *ctx, hfg_basis *basis, const double *P, double *K);
int hfg_mix_exchange_devptr(hfg_ctx *ctx, hfg_basis *basis, const double *dP, double *dK);
int hfg_mix_exchange_occ_devptr(hfg_ctx *ctx, hfg_basis *basis, const double *dP, const double *dC, int64_t nocc, double *dK);
int hfg_mix_exchange_occ_batch_devptr(hfg_ctx *ctx, hfg_basis *basis, int64_t nP, const double *dP, const double *dC,
                                      const int64_t *nocc, int64_t ldc_cols, double *dK);
/* The chunks of a batched exchange build, no device needed: ranks[b] factors of density b (0: the zero matrix, no chunk,
 * chunk_of[b] = -1; negative or above 64: routed alone), chunk_of[b] the chunk of density b, *nchunks their number.  Chunks
 * are runs of consecutive densities whose ranks sum to 64 at most, of max_members densities at most (0: the value of
 * HELFEM_EXCHANGE_BATCH_CHUNK, itself 0 for no limit). */
int hfg_exchange_batch_plan(int64_t nP, const int *ranks, int max_members, int *chunk_of, int *nchunks);
/* dScal: 3 doubles in HBM receiving Exc, Nel, Ekin */
int hfg_xc_fock_dev(hfg_ctx *ctx, hfg_basis *basis, int x_func, int c_func, const double *dP, double *dH,
                    double *dScal, double dens_thr);
int hfg_xc_fock_pol_dev(hfg_ctx *ctx, hfg_basis *basis, int x_func, int c_func, const double *dPa, const double *dPb,
                        double *dHa, double *dHb, double *dScal /* 3: Exc, Nel, Ekin */, double dens_thr);
/* Fused, shardable Fock build for the SCF loop (main.cpp:808-900): J and the XC matrix are block-banded in
 * the radial index, so each rank produces its shard's contribution in a compact layout of
 * hfg_fock_compact_size() doubles; the caller all-reduces that buffer (and dScal) over ranks and
 * hfg_fock_finish_dev() forms F = enforce_fock_symmetry(H0 + J + XC) (dBlockId: symmetry block of
 * every basis function, or NULL). */
int64_t hfg_fock_compact_size(hfg_basis *basis);
int hfg_fock_compact_dev(hfg_ctx *ctx, hfg_basis *basis, int x_func, int c_func, const double *dP, double *dFc,
                         double *dScal, double dens_thr);
int hfg_fock_finish_dev(hfg_ctx *ctx, hfg_basis *basis, const double *dFc, const double *dH0, const int *dBlockId,
                        double *dF);
/* The fused build of an unrestricted iteration (main.cpp:808-900, unrestricted branch).  dFc holds
 * hfg_fock_compact_pol_size() = 2 * hfg_fock_compact_size() doubles: this shard's J[Pa + Pb] + XC_a, then J[Pa + Pb] + XC_b,
 * each in the layout of hfg_fock_compact_dev; dScal its partial (Exc, Nel, Ekin).  x_func <= 0 and c_func <= 0 (Hartree-Fock):
 * both slabs are J and dScal is zero.  The shard, hfg_ctx_set_fock_blocks, HELFEM_FOCK_SKIP and HELFEM_FOCK_OVERLAP act as on
 * hfg_fock_compact_dev; a shell pair is skipped on the density side only if its block is zero in BOTH spins.  After the
 * all-reduce of dFc and dScal, hfg_fock_finish_pol_devptr forms Fa and Fb = enforce_fock_symmetry(H0 + slab) in one pass (dH0,
 * dBlockId may be NULL), each bitwise what hfg_fock_finish_dev gives on its slab.  External functional parameters: those of
 * the context, as for hfg_fock_compact_dev.  hfg_eig_gsym_sub_pair_devptr is hfg_eig_gsym_sub_pair on device pointers
 * (blk_ptr and blk_idx stay host pointers; one device, whatever the shard).  A null pointer is status 1.
 * Deliberately not named *_dev, like hfg_coulomb_batch_devptr: the entries of that name are exactly the plan of
 * tests/stream_order_worker.py; the stream ordering of these three is tested in tests/test_gpu_fock_pol.py. */
int64_t hfg_fock_compact_pol_size(hfg_basis *basis); /* needs no device */
int hfg_fock_compact_pol_devptr(hfg_ctx *ctx, hfg_basis *basis, int x_func, int c_func, const double *dPa, const double *dPb,
                                double *dFc, double *dScal /* 3 */, double dens_thr);
int hfg_fock_finish_pol_devptr(hfg_ctx *ctx, hfg_basis *basis, const double *dFc, const double *dH0, const int *dBlockId,
                               double *dFa, double *dFb);
int hfg_eig_gsym_sub_pair_devptr(hfg_ctx *ctx, int64_t N, const double *dFa, const double *dFb, const double *dSinvh, int nblk,
                                 const int64_t *blk_ptr, const int64_t *blk_idx, double *dEa, double *dCa, double *dEb,
                                 double *dCb);
/* The constrained-UHF form of ROHF, scf::ROHF_update (scf_helpers.cpp:470-523), on matrices in HBM (column-major): dFa += lambda,
 * dFb -= lambda in place, lambda the core-virtual coupling of (Fa - Fb) / 2 between the natural orbitals of Pa + Pb.  dS: the
 * overlap (N x N); dCa (N x nocca) and dCb (N x noccb): the occupied orbitals the densities were formed from, Pa = Ca Ca^T,
 * Pb = Cb Cb^T.  With nocca + noccb <= 128 the natural orbitals of non-zero occupation come from the eigenvectors of the
 * (nocca + noccb)-order matrix C^T S C and lambda from rank-(nocca + noccb) products: O(N^2 (nocca + noccb)) work, Fa and Fb
 * read twice and written once.  More columns, or HELFEM_CUHF_LOWRANK=0 (read at every call), take the dense sequence of the
 * SCF driver: S^{-1/2} and its partner from dS, P from the orbitals, an eigensolve of order N and eight N^3 products.  Both
 * need non-zero occupation gaps at the core / active and active / virtual boundaries.  nocca == noccb, or either zero, leaves
 * dFa and dFb untouched and launches nothing.  Everything is queued on the context's stream behind the caller's work there and
 * the outputs are ordered with what the caller queues next; the eigensolver's status read-back synchronises the stream once per
 * call (the dense route, which also forms S^{-1/2}: three times), growth of the context's workspace when a larger shape arrives once more.  Fixed summation
 * orders and no atomics: two contexts give equal bits, and on the low-rank route lambda is symmetric bit for bit.  Named
 * *_devptr, not *_dev, like hfg_coulomb_batch_devptr: the stream ordering is tested in tests/test_gpu_cuhf_stream_order.py.
 * hfg_rohf_update is the same update on host matrices as the reference states it, from P = Pa + Pb, Sh (N x n, the partner
 * of Sinvh: Sh^T Sinvh = 1) and Sinvh (N x n): the dense sequence, since it has no orbitals. */
int hfg_cuhf_update_devptr(hfg_ctx *ctx, int64_t N, const double *dS, const double *dCa, int64_t nocca, const double *dCb,
                           int64_t noccb, double *dFa, double *dFb);
int hfg_rohf_update(hfg_ctx *ctx, int64_t N, int64_t n, double *Fa, double *Fb, const double *P, const double *Sh,
                    const double *Sinvh, int64_t nocca, int64_t noccb);
/* Which entries of the compact buffer the caller reads.  blockid_dev: the device array hfg_fock_finish_dev takes as
 * dBlockId (symmetry block of every basis function), or NULL to clear.  A set-up call (it synchronises the device and
 * copies the array to the host): from it the context derives the shell pairs (x, y) in which some function of x and some
 * function of y share a block, and hfg_fock_compact_dev of THIS context and the tables the basis has now writes exact
 * zeros to every other pair instead of computing it -- what hfg_fock_finish_dev with the same block ids discards anyway.
 * With nothing set (the default) every pair is computed.  HELFEM_FOCK_SKIP=0 ignores the declaration. */
int hfg_ctx_set_fock_blocks(hfg_ctx *ctx, hfg_basis *basis, const int *blockid_dev);
/* the host derivation behind it, no device needed: nfunc[x] functions in shell x (shell after shell), blockid of every
 * function, need[x * nshell + y] = 1 if the pair is read, else 0 */
int hfg_fock_need_pairs(int nshell, const int *nfunc, const int *blockid, int *need);
int hfg_eig_gsym_sub_dev(hfg_ctx *ctx, int64_t N, const double *dF, const double *dSinvh, int nblk,
                         const int64_t *blk_ptr, const int64_t *blk_idx, double *dE, double *dC);
/* hfg_eig_gsym_sub_sel on device pointers (blk_ptr and blk_idx stay host pointers); one device, whatever the shard */
int hfg_eig_gsym_sub_sel_dev(hfg_ctx *ctx, int64_t N, const double *dF, const double *dSinvh, int nblk, const int64_t *blk_ptr,
                             const int64_t *blk_idx, int64_t nev, double *dE /* K */, double *dC /* N x K */);
/* Multi-GPU form of eig_gsym_sub: symmetry blocks are independent (scf_helpers.cpp:148-175), block ib is
 * solved by rank ib % nranks into a buffer of hfg_eig_block_buf_size() doubles (other slots zero); after a
 * sum all-reduce of that buffer every rank calls hfg_eig_assemble_dev() for the global sort (:183-185). */
int64_t hfg_eig_block_buf_size(int nblk, const int64_t *blk_ptr);
int hfg_eig_blocks_dev(hfg_ctx *ctx, int64_t N, const double *dF, const double *dSinvh, int nblk,
                       const int64_t *blk_ptr, const int64_t *blk_idx, double *dBlockBuf);
int hfg_eig_assemble_dev(hfg_ctx *ctx, int64_t N, int nblk, const int64_t *blk_ptr, const int64_t *blk_idx,
                         const double *dBlockBuf, double *dE, double *dC);
int hfg_form_density_dev(hfg_ctx *ctx, int64_t N, int64_t ncols, const double *dC, int64_t nocc, double *dP);
/* Fractional occupations by symmetry block, on device pointers.  dE (ncols) and dC (N x ncols, leading dimension N) as
 * hfg_eig_gsym_sub_dev and hfg_eig_assemble_dev leave them: ascending energies, the blocks' columns interleaved, every column
 * exactly zero outside its block.  dBlockId (device, N ints): the block of every row, as the step objects hold it.  occ_ptr
 * (host, nblk + 1, occ_ptr[0] = 0) and occ (host, nslots = occ_ptr[nblk] values in [0, 1]): the occupations of block b, lowest
 * level first, at occ[occ_ptr[b] .. occ_ptr[b + 1]).  Slot occ_ptr[b] + k receives the k-th column of block b in the order of
 * (E, column index) -- for sorted energies, the order of dC -- times sqrt(occ[occ_ptr[b] + k]) in dCocc (N x nslots), its energy
 * in dEocc and its occupation in dFocc; an occupation of 0 gives a zero column.  A column belongs to the block of the row of
 * its entry of largest magnitude (the lowest such row).  dCocc dCocc^T is then the density sum_i f_i c_i c_i^T, and the panel
 * serves wherever the occupied orbitals do as the factors of a density (hfg_form_density_dev, hfg_exchange_occ_dev, the
 * low-rank error of hfg_diis_update_devptr, none of which assumes orthonormal columns).
 * Three launches on the context's stream, ordered behind the caller's work there; every output has one writer at a fixed place
 * (no atomics: bitwise repeatable); dE and dC are only read.  No argument is read after the return.  The host synchronises
 * only when something is new: the first call with a block-id array (address, N, nblk) reads it back once to count the rows of
 * every block -- the array at an address is taken to keep its contents until hfg_occupy_forget_blocks -- and a call whose
 * occupation lists differ from the previous call's drains the stream before staging them; an SCF run does neither after
 * its first iteration.  Refused before any launch (status 1, hfg_last_error): nblk < 1, ncols < N, an occupation outside
 * [0, 1] -- these before the context is touched -- and more occupations for a block than it has rows.
 * Profile scope: "occupy". */
int hfg_occupy_blocks_devptr(hfg_ctx *ctx, int64_t N, int64_t ncols, const double *dE, const double *dC,
                             const int *dBlockId /* device, N */, int nblk, const int64_t *occ_ptr /* host, nblk + 1 */,
                             const double *occ /* host, nslots */, double *dCocc /* N x nslots */, double *dEocc /* nslots */,
                             double *dFocc /* nslots */);
/* The rows per block that hfg_occupy_blocks_devptr counted for the block-id array it saw last are dropped: the next call reads
 * the array back again.  For a caller that rewrites a block-id array in place, or whose allocator hands a new array the address
 * of an old one with the same N and nblk. */
int hfg_occupy_forget_blocks(hfg_ctx *ctx);
int hfg_gemm_dev(hfg_ctx *ctx, int transA, int transB, int64_t m, int64_t n, int64_t k, const double *dA,
                 int64_t lda, const double *dB, int64_t ldb, double *dC, int64_t ldc);

/* ---- SCF driver, the loop of src/diatomic/main.cpp:780-995: restricted closed shell (multiplicity 1) or
 * unrestricted (multiplicity = 2S+1 > 1: nela - nelb = multiplicity - 1, --M of main.cpp:100); a NEGATIVE
 * multiplicity selects the restricted open-shell run of `--restricted 1` (scf::ROHF_update, main.cpp:903) --------- */
/* out[0..7] = Etot, Ekin, Epot, Ecoul, Exx, Exc, Enucr, iterations(+0.5 if converged); out[8..11] =
 * seconds of the last iteration's J, K, XC and diagonalisation steps (the reference's Timer prints). */
int hfg_scf_diatomic(hfg_ctx *ctx, int Z1, int Z2, double Rbond, const int *lmmax, int nlm, int nelem, int nnodes,
                     int nquad, double Rmax, int igrid, double zexp, int lpad, const char *method, int ldft, int mdft,
                     int symmetry, int multiplicity, int maxit, double convthr, int verbose, double *out /* 12 */);

/* ---- complete runs: what `diatomic` (src/diatomic/main.cpp) and `atomic` (src/atomic/main.cpp) do between parsing their
 * command line and printing the energy table.  Field names are the reference's flag names (main.cpp:89-133 /
 * atomic/main.cpp:63-119); hfg_scf_options_default() fills in the reference's defaults.  Flags of features outside the
 * hot-path scope (external fields, finite nuclei, confinement, non-LIP primitive bases) are carried so
 * that the drivers can reject non-default values with the reference's wording instead of ignoring them. -------------- */
#define HFG_MAX_LMMAX 16
typedef struct hfg_scf_options {
  int program;               /* 0: diatomic, 1: atomic */
  int Z1, Z2;                /* diatomic: --Z1 --Z2; atomic: --Z in Z1 (Z2 unused) */
  double Rbond;              /* --Rbond in bohr (the drivers convert --angstrom input) */
  int nela, nelb, Q, M;      /* --nela --nelb --Q --M (scf::parse_nela_nelb); M = 0 means "not given": 1 */
  int lmmax[HFG_MAX_LMMAX];  /* diatomic: l_max for |m| = 0 .. nlm-1 (--lmax list, or --lmax with --mmax) */
  int nlm;
  int lmax, mmax;            /* atomic: --lmax --mmax */
  int lpad;                  /* --lpad = 10 */
  double Rmax;               /* --Rmax = 40 */
  int grid;                  /* --grid = 4 */
  double zexp;               /* --zexp = 1 (diatomic), 2 (atomic) */
  int nelem, nnodes, nquad;  /* --nelem, --nnodes = 15, --nquad = 0 (5 per primitive) */
  int maxit;                 /* --maxit = 50 */
  double convthr;            /* --convthr = 1e-7 */
  int diag;                  /* --diag = 1: S^-1/2 by diagonalisation, 0: Cholesky */
  char method[128];          /* --method = HF */
  int ldft, mdft;            /* --ldft --mdft = 0 (automatic) */
  double dftthr;             /* --dftthr = 1e-12 */
  int restricted;            /* --restricted = -1 (restricted iff nela == nelb) */
  int symmetry;              /* --symmetry = 1 */
  int primbas;               /* --primbas = 4 (LIP); anything else is rejected */
  double diiseps, diisthr;   /* --diiseps = 1e-2, --diisthr = 1e-3 */
  int diisorder;             /* --diisorder = 5 */
  int iguess;                /* --iguess = 2 in the reference (SAP, a data table that is out of scope): 0 core, 3 Thomas-Fermi */
  const double *x_pars;      /* --x_pars / --c_pars: external functional parameters (scf::parse_xc_params), or NULL */
  int n_x_pars;
  const double *c_pars;
  int n_c_pars;
  int maverage;              /* --maverage = false */
  double dampfock, dampthr;  /* atomic: --dampfock = 0.7, --dampthr = 0.1 (damping of the occupied-virtual Fock blocks,
                                atomic/main.cpp:917-936); 1.0 switches it off */
  char save[512];            /* --save = helfem.chk ("" to skip); HDF5, src/general/checkpoint.cpp */
  char load[512];            /* --load = "" */
  /* out of scope, must keep their defaults: */
  double Ez, Qzz, Bz;        /* external fields */
  int finitenuc;             /* finite nuclear model */
  int readocc;               /* --readocc = 0: forced occupations from occs (the drivers read occs.dat), enforced after the
                                guess and after the eigensolves of the iterations i < readocc; negative: always */
  const int *occs;           /* occ_rows x occ_cols, row-major: nalpha, nbeta, m [, parity +-1 | atomic --symmetry 2: l, m] */
  int occ_rows, occ_cols;
  double perturb;            /* random perturbation of the guess */
  int iconf;                 /* atomic: confinement potential */
  int zeroder;               /* atomic: zero derivative at Rmax */
  int verbose;               /* print the reference's per-iteration lines to stdout */
} hfg_scf_options;

typedef struct hfg_scf_result {
  double Etot, Ekin, Epot, Enucr, Ecoul, Exx, Exc;
  int iterations, converged;
  int nela, nelb;
  int64_t Nbf;
  double tJ, tK, tXC, tdiag; /* seconds of the last iteration's steps (the reference's Timer prints) */
} hfg_scf_result;

int hfg_scf_options_default(hfg_scf_options *opt, int program);
/* --readocc for the following hfg_scf_diatomic / hfg_scf_atomic calls of this thread (the short entry points have no
 * options structure); readocc = 0 switches it off */
int hfg_scf_set_occupations(int readocc, int nrows, int ncols, const int *rows);
/* the validation hfg_scf_run performs before it touches the device (no GPU needed): 0 = acceptable */
int hfg_scf_options_check(const hfg_scf_options *opt);
/* runs the calculation on ctx's device; E / C (alpha orbital energies Nbf, orbitals Nbf x Nbf) may be NULL */
int hfg_scf_run(hfg_ctx *ctx, const hfg_scf_options *opt, hfg_scf_result *res, double *E, double *C);
/* The atomic program's flags that hfg_scf_options carries no value for (atomic/main.cpp:64-66, 104, 113-118, 160-194).
 * With them hfg_scf_options::finitenuc and iconf take effect (zeroder is refused with a text that says why); Rmid is in bohr.  Econf is an output: tr(P Vconf),
 * the "Confinement potential" line of the energy table, which is part of Etot (atomic/main.cpp:748, 858). */
typedef struct hfg_scf_atomic_extras {
  double Rrms;               /* --Rrms */
  int conf_N;                /* --conf_N */
  double conf_R;             /* --conf_R */
  double conf_barrier;       /* --conf_barrier */
  double shift_conf;         /* --shift_conf */
  int add_conf;              /* --add_conf = 1 */
  int Zl, Zr;                /* --Zl --Zr */
  double Rmid;               /* --Rmid */
  int nelem0;                /* --nelem0 */
  int grid0;                 /* --grid0 = 4 */
  double zexp0;              /* --zexp0 = 2 */
  double Econf;              /* out */
} hfg_scf_atomic_extras;
int hfg_scf_atomic_extras_default(hfg_scf_atomic_extras *extras);
/* hfg_scf_options_check for an atomic run with extras (NULL: exactly hfg_scf_options_check): the combination, the grid and
 * the one-electron matrices are formed on the host, so every refusal of the run short of the device comes out here */
int hfg_scf_options_check_ex(const hfg_scf_options *opt, const hfg_scf_atomic_extras *extras);
/* hfg_scf_run with the extras (NULL: exactly hfg_scf_run, with its refusals); opt->program must be 1 when extras is given */
int hfg_scf_run_ex(hfg_ctx *ctx, const hfg_scf_options *opt, hfg_scf_atomic_extras *extras, hfg_scf_result *res, double *E,
                   double *C);
/* scf::parse_xc_params (src/general/scf_helpers.cpp): one number per line of a text file; n in: capacity, out: count */
int hfg_parse_xc_params(const char *path, double *pars, int *n);
/* element symbol or number -> nuclear charge (get_Z of src/general/elements.h as the drivers use it); < 0: unknown */
int hfg_get_Z(const char *symbol_or_number);

/* ---- checkpoint files in the reference's HDF5 layout (src/general/checkpoint.cpp: matrices as 2-D datasets with swapped
 * dimensions :117-144, integer vectors :220-257, scalars :627/:701, the basis as its constructor arguments :477-507,
 * :560-584).  libhdf5 is loaded at run time ($HELFEM_HDF5_LIB, libhdf5.so, ...); every call fails with an error text
 * when none can be loaded.  hfg_scf_run writes one when hfg_scf_options::save is set. -------------------------------- */
typedef struct hfg_chk hfg_chk;
int hfg_chk_available(void);                                    /* 1 when a libhdf5 could be loaded */
int hfg_chk_open(const char *path, int write, hfg_chk **chk);   /* write != 0 truncates / creates */
int hfg_chk_close(hfg_chk *chk);
int hfg_chk_exist(hfg_chk *chk, const char *name);              /* 1 / 0 */
int hfg_chk_write_mat(hfg_chk *chk, const char *name, const double *m, int64_t rows, int64_t cols); /* arma::mat / arma::vec */
int hfg_chk_write_ivec(hfg_chk *chk, const char *name, const int *v, int64_t n);                    /* arma::ivec */
int hfg_chk_write_double(hfg_chk *chk, const char *name, double v);
int hfg_chk_write_int(hfg_chk *chk, const char *name, int v);
int hfg_chk_write_basis(hfg_chk *chk, const hfg_basis *basis);  /* Checkpoint::write(basis) */
/* m == NULL queries the shape */
int hfg_chk_read_mat(hfg_chk *chk, const char *name, double *m, int64_t *rows, int64_t *cols);
int hfg_chk_read_ivec(hfg_chk *chk, const char *name, int *v, int64_t *n);
int hfg_chk_read_double(hfg_chk *chk, const char *name, double *v);
int hfg_chk_read_int(hfg_chk *chk, const char *name, int *v);
/* Checkpoint::read(diatomic::basis::TwoDBasis &): a basis object from the stored constructor arguments */
int hfg_chk_read_diatomic_basis(hfg_chk *chk, int lpad, hfg_basis **basis);

/* ---- measurement --------------------------------------------------------------------------- */
/* When enabled, every kernel family is bracketed by hipEvents on the context's stream; the
 * accumulated device time (ms) and launch count per family can be read back after a synchronize.
 * names: "coulomb", "coulomb_batch" (the batched build; "coulomb_batch_tei": its pass over the tables), "xc", "exchange" (the full-range build; "exchange_yukawa" / "exchange_erfc": the screened build of
 * hfg_rs_exchange and of the range-separated hybrids; "exchange_mix": the build on the mixed-kernel set, "exchange_mix_tables":
 * its mixing, once), "eig_reduce", "eig_tridiag", "eig_tridiag_solve",
 * "eig_backtransform", "gemm", "density", "scatter", "occupy" (hfg_occupy_blocks_devptr). */
int hfg_profile_enable(hfg_ctx *ctx, int on);
int hfg_profile_reset(hfg_ctx *ctx);
int hfg_profile_get(hfg_ctx *ctx, const char *name, double *ms, int64_t *launches);
/* the names seen since the last reset, separated by '\n' (besides the families above: one name per tile shape of the
 * persistent tridiagonalisation, "k_trdp<R, U>", and "k_trdp" for all its launches) */
int hfg_profile_names(hfg_ctx *ctx, char *buf, size_t cap);
/* the HELFEM_* environment switches of the library, one line per switch, fields separated by '\t': name, kind, default,
 * current value in this process, "once" (read when the process first uses a switch) or "live" (read at every use),
 * meaning.  Needs no device. */
int hfg_tuning_table(char *buf, size_t cap);
/* What the last low-rank exchange builds on a table set of the basis took ("coulomb": the set of hfg_exchange, "screened":
 * of hfg_rs_exchange, "mix": of hfg_mix_exchange), as JSON text: {"single": record, "batch": record}, the record of
 * hfg_exchange and its kin and of the last chunk of the batched entries; null for a build that has not run.  A record
 * holds NLM, A, Ntab, E, p, the shells per run of equal m, the ranks of the factor groups (or of the chunk's members), per
 * group or member whether its cross-element products were split over K, the kernels ("alpha", "rb"), whether the cross
 * products go by blocks of equal m, the tiles and launchers of the cross products and of the element GEMM, the task
 * counts, the largest M and N of a cross task, the longest pair list, and "declined" when the build handed the density to
 * the general kernels.  The host fills it while it builds its task lists; nothing is read from the device.  Tests only. */
int hfg_exl_last_plan(hfg_basis *basis, const char *which, char *buf, size_t cap);

/* Atomic SCF, restricted closed shell or unrestricted (driver loop of src/atomic/main.cpp:760-1005); out as for hfg_scf_diatomic */
int hfg_scf_atomic(hfg_ctx *ctx, int Z, int Q, int lmax, int mmax, int nelem, int nnodes, int nquad, double Rmax,
                   int igrid, double zexp, const char *method, int ldft, int mdft, int symmetry, int multiplicity,
                   int maverage /* --maverage: scf::fock_symmetry_average over m */, int maxit, double convthr,
                   int verbose, double *out /* 12 */);

/* Replays every launch of the named kernel of the last eigensolve back to back between two HIP events on the
 * context's stream (the roofline leg of bench.py).  Supported: "k_trdf" (the tridiagonalisation sweep of the default
 * path; "k_trdb_gemv" is accepted as an alias and replays the same launches -- with HELFEM_TRD=twokernel those are the
 * launches of k_trdb_gemv).  Any other name: status 1. */
int hfg_measure_kernel(hfg_ctx *ctx, const char *name, double *ms, int64_t *launches);

/* pinned host memory for arma-owned buffers ("Armadillo matrices pinned and mirrored to HBM") */
int hfg_pin(void *host_ptr, size_t bytes);
int hfg_unpin(void *host_ptr);

#ifdef __cplusplus
}
#endif
#endif /* HELFEM_GPU_H */
