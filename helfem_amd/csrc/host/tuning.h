// The HELFEM_* run-time switches of the library: one list, from which the Tuning struct, its parse function and the table that
// hfg_tuning_table() prints are generated (DESIGN.md's table is written from that output).  A switch is read ONCE per process, when
// tuning() is first called; the LIVE rows are read at every use through tuning_live(): tests and drivers change them in-process.
#pragma once
#include <string>

namespace helfem {
constexpr int EXL_GMAX = 16;  // factor groups (residual factorisations) of the low-rank exchange at most
enum class TrdMode { persistent, chain, twokernel, unblocked };
enum class EigSel { crossover, stein, dc };
enum class RsTei { host, dev };
// X(field, type, default, variable, LIVE, kind, value from the variable's text e, meaning)
// kinds: "off if 0" = on unless atoi gives 0 (so empty or a word is off); "=w" = on when the text is exactly w; "int" = atoi
// of the text; "present" = on when set to anything, the empty string included; "path" = the text (empty: unset)
#define HELFEM_TUNING(X) \
  X(scf_host, bool, false, "HELFEM_SCF", true, "=host", !strcmp(e, "host"), "SCF loop driven from the host through the per-stage entry points (checker of the device-resident loop)") \
  X(tei_host, bool, false, "HELFEM_TEI", false, "=host", !strcmp(e, "host"), "in-element tables built by the threaded host code and uploaded (checker of tei_dev.hip)") \
  X(rs_tei, RsTei, RsTei::host, "HELFEM_RS_TEI", false, "word", !strcmp(e, "dev") ? RsTei::dev : RsTei::host, "range-separated exchange tables of the SCF drivers: dev = built on the device (rs_tei_dev.hip); unset or any other word = built by the threaded host code and uploaded") \
  X(exchange_general, bool, false, "HELFEM_EXCHANGE", true, "=general", !strcmp(e, "general"), "general exchange kernels always, not only where the low-rank fast path declines") \
  X(exl_rb, int, 0, "HELFEM_EXL_RB", false, "int", atoi(e), "RB kernel of the low-rank exchange: 4 the 4 x 4 vector kernel, 1 the one-pair vector kernel (checkers), else the matrix-core kernel k_exl_RBm") \
  X(exl_mgroups, bool, true, "HELFEM_EXL_MGROUPS", false, "off if 0", atoi(e) != 0, "cross-element products by blocks of equal m; off: the full products") \
  X(exl_rect, int, -1, "HELFEM_EXL_RECT", false, "int", atoi(e), "tiles of the element GEMM: 0 / 1 / 2 = 128 x 128 / 128 x 64 / 64 x 64 always; negative: 64 x 64 when the tasks average fewer than 1500 pairs, else 128 x 128") \
  X(exl_wl, bool, true, "HELFEM_EXL_WL", false, "off if 0", atoi(e) != 0, "XCD-contiguous workgroup lists for the element GEMM and the cross products; off: plain task-list grids") \
  X(exl_splitk, bool, true, "HELFEM_EXL_SPLITK", false, "off if 0", atoi(e) != 0, "two half-K workgroups per tile for the cross products; off: one workgroup per tile") \
  X(exl_crect, bool, true, "HELFEM_EXL_CRECT", false, "off if 0", atoi(e) != 0, "128 x 64 tiles for the split cross products; off: 128 x 128") \
  X(exl_groups, int, 4, "HELFEM_EXL_GROUPS", false, "int", std::max(1, std::min(EXL_GMAX, atoi(e))), "groups of 64 factors tried before the general kernels take over, clamped to 1 ... 16") \
  X(exl_hint, bool, true, "HELFEM_EXL_HINT", false, "off if 0", atoi(e) != 0, "the SCF loop's occupied orbitals taken as the factors of P; off: always factorise and verify P (checker)") \
  X(exl_pair, bool, true, "HELFEM_EXL_PAIR", false, "off if 0", atoi(e) != 0, "low-rank fast path for the pair (erfc) tables; off: general kernels") \
  X(exl_mix, int, -1, "HELFEM_EXL_MIX", true, "int", atoi(e), "range-separated hybrids in the step objects: 0 = K from two builds, hfg_exchange_occ_dev and hfg_rs_exchange_dev, added on the device (checker); other non-negative = one build on the mixed-kernel table set (hfg_mix_exchange_tables); negative: by kernel kind as measured, the mixed set for both Yukawa and erfc") \
  X(fock_overlap, bool, true, "HELFEM_FOCK_OVERLAP", false, "off if 0", atoi(e) != 0, "Coulomb kernels on the side stream beside the XC kernels; off: one after the other on the main stream") \
  X(fock_skip, bool, true, "HELFEM_FOCK_SKIP", true, "off if 0", atoi(e) != 0, "Fock build skips shell pairs whose density block is zero and, after hfg_ctx_set_fock_blocks, pairs the caller does not read; off: every pair is computed (checker)") \
  X(xc_lds_limit, size_t, 150 * 1024, "HELFEM_XC_LDS_LIMIT", false, "int", (size_t)atol(e), "bytes of LDS the angular XC kernels plan with; smaller forces the chunked kernels (tests)") \
  X(coulomb_batch_chunk, int, 0, "HELFEM_COULOMB_BATCH_CHUNK", true, "int", std::max(0, atoi(e)), "densities per pass over the tables of the batched Coulomb build forced smaller than the LDS rule allows (tests; 0: the rule's own)") \
  X(exchange_batch_chunk, int, 0, "HELFEM_EXCHANGE_BATCH_CHUNK", true, "int", std::max(0, atoi(e)), "densities per pass over the tables of the batched exchange build at most (tests; 0: as many as fit the 64 factor columns of a pass)") \
  X(uscf_kbatch, bool, false, "HELFEM_USCF_KBATCH", true, "=1", atoi(e) == 1, "DeviceUSCFStep: K[Pa] and K[Pb] through one call of hfg_exchange_occ_batch_devptr; off: one call per spin") \
  X(diis_blocks, bool, true, "HELFEM_DIIS_BLOCKS", false, "off if 0", atoi(e) != 0, "DIIS error per symmetry block; off: the four dense N^3 products (checker)") \
  X(diis_lowrank, bool, true, "HELFEM_DIIS_LOWRANK", false, "off if 0", atoi(e) != 0, "blocked DIIS error from the occupied orbitals; off: per-block n^3 products from F and P (checker)") \
  X(cuhf_lowrank, bool, true, "HELFEM_CUHF_LOWRANK", true, "off if 0", atoi(e) != 0, "hfg_cuhf_update_devptr: the constraint from the occupied orbitals (rank na + nb, up to 128 columns); off: the dense natural-orbital sequence always (checker)") \
  X(eig_pair, bool, true, "HELFEM_EIG_PAIR", false, "off if 0", atoi(e) != 0, "both spins' Fock matrices in one batched eigensolve; off: two calls") \
  X(eig_direct, bool, true, "HELFEM_EIG_DIRECT", true, "off if 0", atoi(e) != 0, "one-call blocked eigensolve (hfg_eig_gsym_sub_dev, _sel_dev, _pair_devptr) ranks before its last product and stores that product straight into C; off: block slots, then hfg_eig_assemble_dev (checker)") \
  X(eig_band, bool, true, "HELFEM_EIG_BAND", true, "off if 0", atoi(e) != 0, "blocked eigensolve under a declared radial-element pattern of F (hfg_ctx_declare_fock_band): rows of F radial-major, F X as row-tile tasks over the k steps that meet their non-zero columns, bit for bit the dense product; off: the declaration is ignored (checker)") \
  X(trd_mode, TrdMode, TrdMode::persistent, "HELFEM_TRD", false, "word", !strcmp(e, "persistent") ? TrdMode::persistent : !strcmp(e, "twokernel") ? TrdMode::twokernel : !strcmp(e, "unblocked") ? TrdMode::unblocked : TrdMode::chain, "tridiagonalisation: persistent = k_trdp where the batch fits, else the chain; chain (and any unknown word) = one k_trdf launch per column always (checker); twokernel = k_trdb_gemv + k_trdb_w; unblocked = the first-generation kernels") \
  X(trdp_min, int, 256, "HELFEM_TRDP_MIN", false, "int", atoi(e), "smallest order the persistent kernel takes") \
  X(trdp_r, int, 0, "HELFEM_TRDP_R", false, "int", atoi(e), "rows per thread of the persistent kernel forced (0: the first that fits)") \
  X(trdp_u, int, 0, "HELFEM_TRDP_U", false, "int", atoi(e), "column chunks per thread of the persistent kernel forced wider than needed (measurement; 0: narrowest)") \
  X(trdp_limit_ms, long long, 200, "HELFEM_TRDP_LIMIT_MS", false, "int", atoll(e), "wall-clock bound of every spin of the persistent kernel, ms") \
  X(trdp_phases, bool, true, "HELFEM_TRDP_PHASES", false, "off if 0", atoi(e) != 0, "one cooperative launch per phase; off: the whole matrix in one launch (checker)") \
  X(trdp_step, int, 96, "HELFEM_TRDP_STEP", false, "int", std::max(1, atoi(e)), "fewest columns of a phase (at least 1)") \
  X(trdp_coop, bool, true, "HELFEM_TRDP_COOP", false, "off if 0", atoi(e) != 0, "hipLaunchCooperativeKernel for the phases; off: plain launches (A/B of the launch overhead)") \
  X(trdp_stamps, int, 0, "HELFEM_TRDP_STAMPS", false, "int", atoi(e), "non-zero: the stamping kernels, one launch per eigensolve, phase summary on stderr; 2 and more: also per-column stamps of one workgroup") \
  X(trdp_stamps_file, std::string, "", "HELFEM_TRDP_STAMPS_FILE", false, "path", e, "with stamps: file for the stamps of every workgroup over 64 columns (tools/trdp_window.py)") \
  X(trd_tail, int, 2, "HELFEM_TRD_TAIL", false, "int", atoi(e), "last columns of the chain in one launch: 0 none, 1 the LDS-resident kernel (order 128), else the register-resident kernel (order 192)") \
  X(trdf_sym, int, -1, "HELFEM_TRDF_SYM", false, "int", atoi(e), "symmetric sweep of k_trdf: 0 never, other non-negative always, negative by HELFEM_TRDF_SYM_MIN") \
  X(trdf_sym_min, int, 0, "HELFEM_TRDF_SYM_MIN", false, "int", atoi(e), "panels whose full grid has more tiles than this sweep one triangle only") \
  X(trd_band_update, bool, true, "HELFEM_TRD_BAND_UPDATE", false, "off if 0", atoi(e) != 0, "band-limited trailing updates when every sweep is symmetric; off: full updates") \
  X(trdf_nth, int, 0, "HELFEM_TRDF_NTH", false, "int", atoi(e), "512: k_trdf with 512 threads; anything else 1024 (A/B runs)") \
  X(acc_tile, int, 0, "HELFEM_ACC_TILE", false, "int", atoi(e), "128: 128 x 128 tiles for the accumulating updates (and full, not band-limited ones); anything else 64 x 64") \
  X(trdf_dbg, int, 0, "HELFEM_TRDF_DBG", false, "int", atoi(e), "measurement replay of k_trdf only: bits 0-2 go to the kernel's debug field, bit 2 also prints the per-wave stamps (tools/trdf_probe.py)") \
  X(trdf_c, int, -1, "HELFEM_TRDF_C", false, "int", atoi(e), "measurement replay of k_trdf only: column-in-panel index forced for every launch (negative: each launch's own)") \
  X(tridiag_ql, bool, false, "HELFEM_TRIDIAG", false, "=ql", !strcmp(e, "ql"), "one-lane implicit QL for the tridiagonal problem instead of divide and conquer (checker)") \
  X(dc_gemm_small, bool, false, "HELFEM_DC_GEMM", false, "=small", !strcmp(e, "small"), "Q U of the divide-and-conquer merges by the first 64 x 64 kernel instead of the tile engine (checker)") \
  X(dc_levels, bool, false, "HELFEM_DC", false, "=levels", !strcmp(e, "levels"), "divide-and-conquer merges with the gather, scatter and copy-back passes over Q and ten launches per level (checker of the column-mapped product)") \
  X(eigsel, EigSel, EigSel::crossover, "HELFEM_EIGSEL", false, "word", !strcmp(e, "stein") ? EigSel::stein : !strcmp(e, "dc") ? EigSel::dc : EigSel::crossover, "selected eigenpairs (hfg_eig_*_sel): stein = multisection and inverse iteration always; dc = the full divide and conquer, then the lowest columns (checker); unset or any other word = the crossover, which sends every wanted fraction to dc (measured: stein is slower down to 1/64 of the columns)") \
  X(dc_dbg, bool, false, "HELFEM_DC_DBG", false, "present", true, "merge statistics of divide and conquer on stderr") \
  X(bt_column, bool, false, "HELFEM_BT", false, "=column", !strcmp(e, "column"), "back-transformation reflector by reflector instead of compact WY (checker)") \
  X(bt_fold, bool, true, "HELFEM_BT_FOLD", false, "off if 0", atoi(e) != 0, "X Q formed on the side stream beside divide and conquer; off: Z <- Q Z on the main stream behind it") \
  X(bt_side, bool, false, "HELFEM_BT_SIDE", false, "=1", atoi(e) == 1, "without the fold: the compact-WY set-up on the side stream") \
  X(gemm_tile, int, 0, "HELFEM_GEMM_TILE", false, "int", atoi(e), "128: 128 x 128 tiles always; other non-zero: 64 x 64 always; 0: the large tiles where they fill whole rounds of the chip") \
  X(gemm_splitk, int, -1, "HELFEM_GEMM_SPLITK", false, "int", atoi(e), "eigensolve's products: 0 / other non-negative = large tiles without / with two half-K workgroups each; negative: chosen by tile count") \
  X(gemm_rect, bool, false, "HELFEM_GEMM_RECT", false, "on if not 0", atoi(e) != 0, "128 x 64 tiles for the eigensolve's large-tile products") \
  X(mfma_4x4x4, bool, false, "HELFEM_MFMA", false, "=4x4x4", !strcmp(e, "4x4x4"), "v_mfma_f64_4x4x4_4b_f64 in the tile engine instead of v_mfma_f64_16x16x4_f64 (A/B runs)") \
  X(num_threads, int, 0, "HELFEM_NUM_THREADS", true, "int", std::max(0, atoi(e)), "host threads of the set-up code (0: one per core, 64 at most)") \
  X(hdf5_lib, std::string, "", "HELFEM_HDF5_LIB", true, "path", e, "HDF5 library tried before the usual names")

struct Tuning {
#define X(field, type, def, ...) type field = def;
  HELFEM_TUNING(X)
#undef X
};
const Tuning &tuning();  // the process-wide snapshot, taken on first use
Tuning tuning_live();    // the snapshot with the LIVE rows read again now
/// one line per switch: name, kind, default, current value in this process, "live" or "once", meaning (tab separated)
std::string tuning_table();
}  // namespace helfem
