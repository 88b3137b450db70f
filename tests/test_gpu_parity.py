"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle on the same seeded inputs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    if helfem_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the hot path has no CPU fallback")
    return helfem_amd


def test_gemm_all_transposes(hf):
    rng = np.random.RandomState(0)
    for (m, n, k) in [(5, 7, 3), (64, 64, 16), (130, 67, 45), (200, 300, 129)]:
        for tA in (False, True):
            for tB in (False, True):
                A = rng.uniform(-1, 1, size=(k, m) if tA else (m, k))
                B = rng.uniform(-1, 1, size=(n, k) if tB else (k, n))
                C = hf.scf.gemm(A, B, tA, tB)
                ref = (A.T if tA else A) @ (B.T if tB else B)
                assert np.max(np.abs(C - ref)) < 1e-12 * k, (m, n, k, tA, tB)


def test_gemm_large_product(hf):
    """3000 x 200 x 2900 through hfg_gemm.  Written for the 128 x 128 kernel, which it no longer reaches: 24 x 23 = 552 large
    tiles fill two rounds of the 512 slots of a 256-CU part to 54 % only, so gemm_prefers_128 sends the product to
    k_dgemm<64, 64> (47 x 46 tiles).  The large-tile kernels are tested in tests/test_gpu_gemm_engine.py."""
    rng = np.random.RandomState(1)
    A = rng.uniform(-1, 1, size=(3000, 200))
    B = rng.uniform(-1, 1, size=(200, 2900))
    C = hf.scf.gemm(A, B)
    assert np.max(np.abs(C - A @ B)) < 1e-11


@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 130, 257, 333, 400, 1025])
def test_eig_sym_vs_lapack(hf, n):
    rng = np.random.RandomState(n)
    A = rng.uniform(-1, 1, size=(n, n))
    A = A + A.T + np.diag(np.linspace(0, 50.0, n))
    E, C = hf.scf.eig_sym(A)
    Eref = np.linalg.eigvalsh(A)
    scale = max(1.0, np.max(np.abs(Eref)))
    assert np.max(np.abs(E - Eref)) < 1e-12 * scale * max(n, 10)
    assert np.max(np.abs(C.T @ C - np.eye(n))) < 1e-12 * max(n, 10)
    assert np.max(np.abs(A @ C - C * E)) < 1e-11 * scale * max(n, 10)


def test_eig_sym_degenerate_and_diagonal(hf):
    A = np.diag([3.0, 1.0, 1.0, 2.0, 1.0])
    E, C = hf.scf.eig_sym(A)
    assert np.allclose(E, [1, 1, 1, 2, 3], atol=1e-14)
    assert np.max(np.abs(A @ C - C * E)) < 1e-13


# ---------------------------------------------------------------------------------------------------
# Fock build parity: diatomic J, XC, K against the oracle
# ---------------------------------------------------------------------------------------------------
CASES = {
    # name: (Z1, Z2, Rbond, lmmax, nelem, nnodes)
    "sigma_only": (1, 1, 1.4, (4,), 2, 6),
    "sigma_pi": (7, 7, 2.068, (3, 2), 2, 5),
    "hetero_sigma_pi_delta": (3, 9, 2.955, (3, 3, 2), 3, 4),
}


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request, hf):
    import common
    Z1, Z2, R, lmmax, nelem, nnodes = CASES[request.param]
    gb, ob = common.make_bases(Z1, Z2, R, lmmax, nelem, nnodes)
    gb.compute_tei(True)
    ob.compute_tei(True)
    lmax = max(lmmax)
    ldft, mdft = 4 * lmax + 12, 4 * len(lmmax) + 5
    gb.upload(ldft, mdft)
    return request.param, gb, ob, ldft, mdft


def _densities(gb):
    import common
    N = gb.Nbf()
    yield "general", common.random_density(N, 3, seed=11)
    yield "m_blocked", common.random_density(N, 2, seed=12, blocks=gb.get_sym_idx(1))


def test_coulomb_parity(case):
    import common
    name, gb, ob, _, _ = case
    for tag, P in _densities(gb):
        J = gb.coulomb(P)
        Jo = ob.coulomb(P)
        assert common.relerr(J, Jo) < 1e-12, (name, tag, common.relerr(J, Jo))


def test_exchange_parity(case):
    import common
    name, gb, ob, _, _ = case
    for tag, P in _densities(gb):
        K = gb.exchange(P)
        Ko = ob.exchange(P)
        assert common.relerr(K, Ko) < 1e-12, (name, tag, common.relerr(K, Ko))


def test_exchange_general_kernels_parity(case, monkeypatch):
    """HELFEM_EXCHANGE=general: the kernels that take any symmetric P (the fallback of the low-rank fast path)"""
    import common
    name, gb, ob, _, _ = case
    monkeypatch.setenv("HELFEM_EXCHANGE", "general")
    tag, P = list(_densities(gb))[1]
    K = gb.exchange(P)
    assert common.relerr(K, ob.exchange(P)) < 1e-12, name


def test_exchange_indefinite_and_full_rank_inputs(case):
    """a difference density (indefinite, low rank: signed factors) and a full-rank symmetric matrix (falls back)"""
    import common
    name, gb, ob, _, _ = case
    N = gb.Nbf()
    P1 = common.random_density(N, 3, seed=31) - common.random_density(N, 2, seed=32)
    K = gb.exchange(P1)
    assert common.relerr(K, ob.exchange(P1)) < 1e-11, (name, "indefinite")
    rng = np.random.RandomState(5)
    P2 = rng.uniform(-1, 1, size=(N, N))
    P2 = np.asfortranarray(P2 + P2.T)
    K = gb.exchange(P2)
    assert common.relerr(K, ob.exchange(P2)) < 1e-12, (name, "full rank")
    K0 = gb.exchange(np.zeros((N, N), order="F"))
    assert np.all(K0 == 0.0)


def test_xc_kernels_with_chunked_angular_tables(hf):
    """angular bases beyond lmax ~ 33 (restricted) / 26 (unrestricted) do not fit the XC kernels' Theta tables and potential
    planes into one CU's LDS: the theta points then go through LDS in chunks.  HELFEM_XC_LDS_LIMIT (read once per process)
    forces those paths on a small basis in ONE child process (tests/xc_chunk_worker.py), against the oracle"""
    import os
    import subprocess
    import sys
    env = dict(os.environ, HELFEM_XC_LDS_LIMIT="2500")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "xc_chunk_worker.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    assert "worst relative deviation" in p.stdout.decode()


@pytest.mark.parametrize("rb", ["", "1", "4", "mgroups0"])
def test_exchange_rb_kernels_at_large_element_order(hf, rb):
    """exact exchange against the oracle at 15, 16 and 17 nodes per element (tests/exl_worker.py, one child process per
    setting because HELFEM_EXL_RB is read once): the matrix-core RB kernel with and without a padding row in its 16 x 16
    tiles and the one-pair kernel beyond 16 nodes; HELFEM_EXL_RB = 1 / 4 run the two vector kernels (the checkers of the
    matrix-core one) on the padded element tables"""
    import os
    import subprocess
    import sys
    env = dict(os.environ)
    env.pop("HELFEM_EXL_RB", None)
    env.pop("HELFEM_EXL_MGROUPS", None)
    if rb == "mgroups0":
        env["HELFEM_EXL_MGROUPS"] = "0"  # the cross-element products as ten full ones instead of blocks of equal m
    elif rb:
        env["HELFEM_EXL_RB"] = rb
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "exl_worker.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    assert "worst relative deviation" in p.stdout.decode()


def test_exchange_of_a_density_with_more_than_64_factors(case, monkeypatch):
    """rank 70 ... 150: the fast path factorises the residual matrix again (groups of 64 factors, K is linear in P) instead
    of handing the density to the general kernels; HELFEM_EXL_GROUPS=1 restores the single-group behaviour (fallback)"""
    import common
    name, gb, ob, _, _ = case
    N = gb.Nbf()
    for ncol, seed in ((70, 41), (150, 42)):
        if ncol >= N:
            continue
        P = common.random_density(N, ncol, seed=seed) - 0.5 * common.random_density(N, 5, seed=seed + 7)
        Ko = ob.exchange(P)
        K = gb.exchange(P)
        assert common.relerr(K, Ko) < 1e-11, (name, ncol, common.relerr(K, Ko))


@pytest.mark.parametrize("nranks", [2, 3])
def test_exchange_shards_sum_to_full(case, hf, nranks):
    """the shards of hfg_exchange_dev (device-pointer entry point: partial results) sum to the full matrix, and the
    host-pointer entry point returns the FULL matrix whatever shard the context carries"""
    import common
    import ctypes
    import torch
    name, gb, ob, _, _ = case
    tag, P = list(_densities(gb))[1]
    ctx = gb.ctx
    full = gb.exchange(P)
    N = gb.Nbf()
    dP = torch.from_numpy(np.ascontiguousarray(P.T)).cuda()  # symmetric: layout does not matter
    dK = torch.zeros((N, N), dtype=torch.float64, device="cuda")
    acc = np.zeros_like(full)
    try:
        for rk in range(nranks):
            ctx.set_shard(rk, nranks)
            rc = hf.lib().hfg_exchange_dev(ctx.h, gb.h, ctypes.c_void_p(dP.data_ptr()), ctypes.c_void_p(dK.data_ptr()))
            assert rc == 0
            torch.cuda.synchronize()
            part = dK.cpu().numpy().T
            assert common.relerr(part, full) > 1e-3  # a shard is not the whole
            acc += part
            assert common.relerr(gb.exchange(P), full) < 1e-13  # host-pointer call: complete, shard restored afterwards
            assert common.relerr(gb.coulomb(P), ob.coulomb(P)) < 1e-11
    finally:
        ctx.set_shard(0, 1)
    assert common.relerr(acc, full) < 1e-12, name


@pytest.mark.parametrize("funcs", [(1, 7), (1, 0), (101, 130), (101, 0), (0, 130), (1, 12), (406, 0), (202, 231), (202, 0),
                                   (0, 231), (202, 130), (106, 131), (106, 0), (0, 131), (402, 0), (1, 8)])
def test_xc_parity(case, hf, funcs):
    import common
    name, gb, ob, ldft, mdft = case
    grid = hf.DFTGrid(gb, ldft, mdft)
    x, c = funcs
    for tag, P in _densities(gb):
        if tag == "general":
            # a general random P is not positive on the grid: scale it down onto a positive block-diagonal part
            P = 0.05 * P + list(_densities(gb))[1][1]
        H, Exc, Nel, Ekin = grid.eval_Fxc(x, c, P)
        Ho, Exco, Nelo, Ekino = ob.eval_Fxc(ldft, mdft, x, c, P)
        assert abs(Nel - Nelo) < 1e-11 * max(1.0, abs(Nelo)), (name, tag, Nel, Nelo)
        assert abs(Exc - Exco) < 1e-11 * max(1.0, abs(Exco)), (name, tag, Exc, Exco)
        assert common.relerr(H, Ho) < 1e-10, (name, tag, funcs, common.relerr(H, Ho))
        # meta-GGAs also integrate the kinetic energy density (DFTGrid::eval_Fxc returns it as Ekin)
        assert abs(Ekin - Ekino) < 1e-10 * max(1.0, abs(Ekino)), (name, tag, Ekin, Ekino)
        if x in (202,) or c in (231,):
            assert Ekino > 0.0


def test_eig_gsym_sub_parity(case, hf):
    import common
    import oracle_lib as orc
    name, gb, ob, _, _ = case
    S = gb.overlap()
    F = gb.kinetic() + gb.nuclear()
    for symm in (1, 0):
        blocks = gb.get_sym_idx(symm)
        X = hf.scf.form_Sinvh(S, False, blocks)
        Xo = orc.form_Sinvh(S, False, blocks)
        # S^{-1/2} is unique: compare directly
        assert common.relerr(X, Xo) < 1e-9, (name, symm, common.relerr(X, Xo))
        assert np.max(np.abs(X.T @ S @ X - np.eye(S.shape[0]))) < 1e-10
        Fs = np.zeros_like(F)
        for b in blocks:
            Fs[np.ix_(b, b)] = F[np.ix_(b, b)]
        E, C = hf.scf.eig_gsym_sub(Fs, Xo, blocks)
        Eo, Co = orc.eig_gsym_sub(Fs, Xo, blocks)
        scale = max(1.0, np.max(np.abs(Eo)))
        assert np.max(np.abs(E - Eo)) < 1e-10 * scale, (name, symm, np.max(np.abs(E - Eo)))
        assert np.all(np.diff(E) >= 0)
        assert np.max(np.abs(C.T @ S @ C - np.eye(len(E)))) < 1e-9
        assert np.max(np.abs(Fs @ C - S @ C * E)) < 1e-9 * scale
    # eig_gsym on the full problem
    X = orc.form_Sinvh(S, False, gb.get_sym_idx(0))
    E, C = hf.scf.eig_gsym(F, X)
    Eo, _ = orc.eig_gsym(F, X)
    assert np.max(np.abs(E - Eo)) < 1e-10 * max(1.0, np.max(np.abs(Eo)))


def test_form_density_parity(case, hf):
    import oracle_lib as orc
    name, gb, ob, _, _ = case
    rng = np.random.RandomState(5)
    C = rng.uniform(-1, 1, size=(gb.Nbf(), 9))
    assert np.max(np.abs(hf.scf.form_density(C, 4) - orc.form_density(C, 4))) < 1e-13
    assert np.max(np.abs(hf.scf.form_density(C, 0))) == 0.0


def test_tei_tables_built_on_device_match_host_tables(hf):
    """hfg_compute_tei_dev (in-element integrals summed on the GPU) against the host tables: J, K and a full SCF"""
    import common
    for kw in (dict(Z1=7, Z2=7, Rbond=2.068, lmmax=(3, 2), nelem=2, nnodes=5),
               dict(Z1=3, Z2=9, Rbond=2.955, lmmax=(3, 3, 2), nelem=3, nnodes=4)):
        gb, ob = common.make_bases(**kw)
        gd, _ = common.make_bases(oracle=False, **kw)
        gb.compute_tei(True)
        gd.compute_tei(True, device=True)
        gb.upload()
        gd.upload()
        for tag, P in _densities(gb):
            Jh, Jd = gb.coulomb(P), gd.coulomb(P)
            Kh, Kd = gb.exchange(P), gd.exchange(P)
            assert common.relerr(Jd, Jh) < 1e-13 and common.relerr(Kd, Kh) < 1e-12, (kw, tag)


def test_atomic_tei_tables_built_on_device(hf):
    """hfg_compute_tei_dev for the atomic basis (one operand type, kernel r_<^L / r_>^{L+1}, prefix form of the inner
    integral): every in-element table against the host tables (quadrature::twoe_integral in its carried-ratio form, pinned
    by the Maple rationals of src/atomic/inttest.cpp in tests/test_golden_cpu.py), then J and K against the oracle"""
    import common
    for kw in (dict(Z=10, lmax=2, mmax=2, nelem=4, nnodes=7), dict(Z=4, lmax=1, mmax=0, nelem=6, nnodes=5, igrid=1)):
        gh, ob = common.make_atomic_bases(**kw)
        gd, _ = common.make_atomic_bases(oracle=False, **kw)
        gh.compute_tei(True)
        gd.compute_tei(True, device=True)
        NL = 2 * kw["lmax"] + 1
        worst = 0.0
        for L in range(NL):
            for iel in range(kw["nelem"]):
                th, td = gh.prim_table("tei00", L, iel), gd.prim_table("tei00", L, iel)
                assert th.shape == td.shape
                worst = max(worst, np.max(np.abs(th - td)) / np.max(np.abs(th)))
                for name in ("P0", "Q0"):
                    assert np.array_equal(gh.prim_table(name, L, iel), gd.prim_table(name, L, iel))
        assert worst < 1e-12, (kw, worst)
        ob.compute_tei(True)
        gh.upload()
        gd.upload()
        N = gh.Nbf()
        P = common.random_density(N, 3, seed=77)
        Jo, Ko = ob.coulomb(P), ob.exchange(P)
        assert common.relerr(gd.coulomb(P), Jo) < 1e-12 and common.relerr(gd.exchange(P), Ko) < 1e-12, kw
        assert common.relerr(gd.coulomb(P), gh.coulomb(P)) < 1e-13


def test_tei_tables_against_the_independent_fixture(hf):
    """hfg_compute_tei_dev and the host tables against tests/golden/diatomic_tei.npz: tables of the NumPy restatement
    oracle/diatomic_tei.py of quadrature.cpp:22-123 / basis.cpp:1166-1302, which shares no code with the product (the
    'exact' set uses 40-digit Legendre functions, the 'ref' set the reference's own Fortran library)"""
    import os
    import test_tei_golden_cpu as tg
    gold = np.load(tg.GOLD)
    names = ["tei00", "tei02", "tei20", "tei22"]
    gd = tg.golden_basis(hf, gold)
    gd.compute_tei(True, device=True)
    dev = tg.table_errors(gd.prim_table, gold, "exact", names + ["P0", "P2", "Q0", "Q2"])
    assert tg.tight(dev) < 5e-12 and max(dev.values()) < 1e-8, dev
    ref = tg.table_errors(gd.prim_table, gold, "ref", names)
    assert max(ref.values()) < tg.REF_TEI_TOL, ref
    gh = tg.golden_basis(hf, gold)
    gh.compute_tei(True)
    host = tg.table_errors(gh.prim_table, gold, "exact", list(hf.TwoDBasis.PRIM_TABLES))
    assert tg.tight(host) < 5e-12 and max(host.values()) < 1e-8, host
    # and the Coulomb / exchange matrices built from the device tables equal those from the host tables
    gd.upload()
    gh.upload()
    P = __import__("common").random_density(gh.Nbf(), 2, seed=11, blocks=gh.get_sym_idx(1))
    assert __import__("common").relerr(gd.coulomb(P), gh.coulomb(P)) < 1e-13
    assert __import__("common").relerr(gd.exchange(P), gh.exchange(P)) < 1e-12


def test_atomic_device_tei_tables_against_the_independent_fixture(hf):
    """hfg_compute_tei_dev on an ATOMIC basis (in-element tables of compute_tei built on the device, read back) against
    tests/golden/atomic_tei.npz, the tables of the NumPy restatement oracle/atomic_tei.py (no product code)"""
    import test_tei_golden_cpu as tg
    g, ab, NL = tg._atomic_case(hf)
    E = len(g["bval"]) - 1
    ab.compute_tei(True, device=True)
    le = [(L, e) for L in range(NL) for e in range(E)]
    err = tg._worst(lambda L, e: ab.atomic_table("prim_tei", L, e), g, "prim_tei", le)
    assert err < 1e-12, err
    for name in ("disjoint_L",):
        assert tg._worst(lambda L, e, n=name: ab.atomic_table(n, L, e), g, name, le) < 1e-12


def test_device_tei_tables_at_the_bench_element_order(hf):
    """hfg_compute_tei_dev at the headline workload's element order (15-node LIPs, 75-point quadrature, channels up to
    L = 40) against tests/golden/diatomic_tei_p15.npz: seeded samples of the independent NumPy / mpmath restatement"""
    import test_tei_golden_cpu as tg
    g = np.load(tg.P15)
    gd = tg.p15_basis(hf, g)
    gd.compute_tei(False, device=True)
    dev = tg.p15_errors(gd.prim_table, g, "exact")
    assert max(v for k, v in dev.items() if not k.endswith("[0]")) < 2e-11, dev


@pytest.mark.parametrize("env", [dict(HELFEM_TRD="twokernel"), dict(HELFEM_BT="column"),
                                 dict(HELFEM_TRD="unblocked", HELFEM_BT="column"), dict(HELFEM_TRDF_SYM="1"),
                                 dict(HELFEM_TRDF_SYM="0"), dict(HELFEM_TRDF_NTH="512", HELFEM_TRDF_SYM="1"),
                                 dict(HELFEM_BT_SIDE="1", HELFEM_BT_FOLD="0"), dict(HELFEM_TRD_TAIL="0"), dict(HELFEM_TRD_TAIL="1"),
                                 dict(HELFEM_TRD="chain"), dict(HELFEM_TRD="chain", HELFEM_TRDF_SYM="0"),
                                 dict(HELFEM_TRDP_PHASES="0"), dict(HELFEM_TRDP_STEP="1000"), dict(HELFEM_BT_FOLD="0"),
                                 dict(HELFEM_DC_GEMM="small"), dict(HELFEM_GEMM_TILE="128"), dict(HELFEM_GEMM_TILE="64"),
                                 dict(HELFEM_GEMM_SPLITK="1")],
                         ids=["two_launches_per_column", "column_backtransform", "unblocked_tridiagonalisation",
                              "symmetric_sweep_everywhere", "full_sweep_everywhere", "symmetric_sweep_512_threads",
                              "wy_setup_on_side_stream", "no_tail_kernel", "lds_tail_kernel", "launch_chain",
                              "launch_chain_full_sweep", "persistent_one_launch", "persistent_long_phases",
                              "backtransform_on_Z", "small_dc_gemm", "tiles_128", "tiles_64", "split_k_products"])
def test_fallback_variants(native_libs, env):
    """the earlier kernel variants stay selectable (environment, read once per process: helfem_amd.tuning_table() says which) and stay correct"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    e.update(env)
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "fallback_worker.py")], env=e, cwd=root, timeout=300,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0 and b"ok" in out.stdout, out.stdout.decode()[-2000:]


def test_form_sinvh_cholesky_variant(case, hf):
    """TwoDBasis::Sinvh(chol=true) -> utils::invh: Sinvh = D inv(chol(D S D)) per symmetry block (--diag 0)"""
    import oracle_lib as orc
    name, gb, ob, _, _ = case
    S = gb.overlap()
    blocks = gb.get_sym_idx(1)
    X = hf.scf.form_Sinvh(S, True, blocks)
    Xo = orc.form_Sinvh(S, True, blocks)
    assert np.max(np.abs(X - Xo)) < 1e-9 * np.max(np.abs(Xo)), name
    assert np.max(np.abs(X.T @ S @ X - np.eye(S.shape[0]))) < 1e-9
    # the generalized eigenproblem does not care which half-inverse it gets
    F = gb.kinetic() + gb.nuclear()
    E1, _ = hf.scf.eig_gsym_sub(F, X, blocks)
    E2, _ = hf.scf.eig_gsym_sub(F, hf.scf.form_Sinvh(S, False, blocks), blocks)
    assert np.max(np.abs(E1 - E2)) < 1e-8 * max(1.0, np.max(np.abs(E2)))


def test_form_sinvh_cholesky_large_block(hf):
    rng = np.random.RandomState(4)
    n = 333
    A = rng.uniform(-1, 1, (n, n))
    S = A @ A.T + 0.5 * n * np.eye(n)
    X = hf.scf.form_Sinvh(S, True, [np.arange(n)])
    assert np.max(np.abs(X.T @ S @ X - np.eye(n))) < 1e-10
    assert np.max(np.abs(np.tril(X, -1))) == 0.0
    with pytest.raises(RuntimeError):
        hf.scf.form_Sinvh(-S, True, [np.arange(n)])


def test_edge_case_bases(hf):
    """smallest shapes the reference accepts: one radial element, one angular shell, sigma-only with lmax 0"""
    import common
    for kw in (dict(Z1=1, Z2=1, Rbond=1.4, lmmax=(0,), nelem=1, nnodes=4),
               dict(Z1=2, Z2=1, Rbond=1.5, lmmax=(2, 0), nelem=1, nnodes=5),
               dict(Z1=1, Z2=1, Rbond=1.4, lmmax=(1,), nelem=4, nnodes=3)):
        gb, ob = common.make_bases(**kw)
        gb.compute_tei(True)
        ob.compute_tei(True)
        lmax = max(kw["lmmax"])
        ldft, mdft = 4 * lmax + 12, 4 * len(kw["lmmax"]) + 5
        gb.upload(ldft, mdft)
        P = common.random_density(gb.Nbf(), 1, seed=7, blocks=gb.get_sym_idx(1))
        assert common.relerr(gb.coulomb(P), ob.coulomb(P)) < 1e-12, kw
        assert common.relerr(gb.exchange(P), ob.exchange(P)) < 1e-12, kw
        H, Exc, Nel, _ = hf.DFTGrid(gb, ldft, mdft).eval_Fxc(101, 130, P)
        Ho, Exco, Nelo, _ = ob.eval_Fxc(ldft, mdft, 101, 130, P)
        assert common.relerr(H, Ho) < 1e-10 and abs(Exc - Exco) < 1e-11 * max(1.0, abs(Exco)), kw


def test_eig_gsym_sub_pair_equals_two_calls(hf):
    """hfg_eig_gsym_sub_pair (both spins of an unrestricted iteration in one batch) against two eig_gsym_sub calls and the
    oracle; eleven ragged blocks per matrix, so the batch is cut into groups of eight across the two matrices"""
    import oracle_lib as orc
    rng = np.random.RandomState(17)
    sizes = [40, 1, 65, 2, 130, 7, 33, 5, 64, 3, 17]
    N = sum(sizes)
    perm = rng.permutation(N)
    blocks, o = [], 0
    for sz in sizes:
        blocks.append(np.sort(perm[o:o + sz]))
        o += sz
    A = rng.standard_normal((N, N))
    S = A @ A.T + N * np.eye(N)
    Sb = np.zeros_like(S)
    for b in blocks:
        Sb[np.ix_(b, b)] = S[np.ix_(b, b)]
    X = orc.form_Sinvh(Sb, False, blocks)
    Fs = []
    for k in range(2):
        F = rng.standard_normal((N, N))
        F = F + F.T
        Fm = np.zeros_like(F)
        for b in blocks:
            Fm[np.ix_(b, b)] = F[np.ix_(b, b)]
        Fs.append(Fm)
    Ea, Ca, Eb, Cb = hf.scf.eig_gsym_sub_pair(Fs[0], Fs[1], X, blocks)
    for F, E, C in ((Fs[0], Ea, Ca), (Fs[1], Eb, Cb)):
        E1, C1 = hf.scf.eig_gsym_sub(F, X, blocks)
        Eo, _ = orc.eig_gsym_sub(F, X, blocks)
        assert np.max(np.abs(E - E1)) < 1e-12 * N and np.max(np.abs(E - Eo)) < 1e-10 * max(1.0, np.max(np.abs(Eo)))
        assert np.max(np.abs(C.T @ Sb @ C - np.eye(N))) < 1e-9
        assert np.max(np.abs(F @ C - Sb @ C * E)) < 1e-8 * max(1.0, np.max(np.abs(E)))


def test_eig_gsym_sub_many_small_and_odd_blocks(hf):
    """ragged symmetry blocks (sizes 1, 2, odd; more than 8 blocks go through the batch in groups of 8) through eig_gsym_sub"""
    import oracle_lib as orc
    rng = np.random.RandomState(3)
    sizes = [1, 2, 7, 33, 129, 5]
    N = sum(sizes)
    perm = rng.permutation(N)
    blocks, o = [], 0
    for sz in sizes:
        blocks.append(np.sort(perm[o:o + sz]))
        o += sz
    F = rng.uniform(-1, 1, (N, N))
    F = F + F.T
    A = rng.uniform(-1, 1, (N, N))
    S = A @ A.T + N * np.eye(N)
    for i, bi in enumerate(blocks):
        for j, bj in enumerate(blocks):
            if i != j:
                S[np.ix_(bi, bj)] = 0.0
                F[np.ix_(bi, bj)] = 0.0
    X = hf.scf.form_Sinvh(S, False, blocks)
    assert np.max(np.abs(X - orc.form_Sinvh(S, False, blocks))) < 1e-10
    E, C = hf.scf.eig_gsym_sub(F, X, blocks)
    Eo, _ = orc.eig_gsym_sub(F, X, blocks)
    assert np.max(np.abs(E - Eo)) < 1e-10
    assert np.max(np.abs(C.T @ S @ C - np.eye(N))) < 1e-10
    assert np.max(np.abs(F @ C - S @ C * E)) < 1e-9


@pytest.mark.parametrize("sizes", [[769, 513, 300], [1025], [257, 256, 255], [897, 896, 641, 640, 385], [1793, 3]])
def test_persistent_tridiagonalisation_phase_boundaries(hf, sizes):
    """block sets whose orders sit on and next to the tile widths of hip/trdp.hip (multiples of 128 / 256: where a phase
    ends, where a matrix changes tile shape, where a block finishes inside a phase of the others; 255 and 3 take the
    launch chain) through eig_gsym_sub with X = 1, against LAPACK; twice, bitwise the same"""
    rng = np.random.RandomState(sum(sizes))
    N = sum(sizes)
    F = np.zeros((N, N), order="F")
    blocks, off = [], 0
    for n in sizes:
        B = rng.standard_normal((n, n))
        F[off:off + n, off:off + n] = B + B.T
        blocks.append(np.arange(off, off + n))
        off += n
    X = np.asfortranarray(np.eye(N))
    E, C = hf.scf.eig_gsym_sub(F, X, blocks)
    Er = np.sort(np.concatenate([np.linalg.eigvalsh(F[np.ix_(b, b)]) for b in blocks]))
    sc = np.max(np.abs(Er))
    assert np.max(np.abs(E - Er)) < 1e-12 * sc
    assert np.max(np.abs(F @ C - C * E)) < 1e-11 * sc
    assert np.max(np.abs(C.T @ C - np.eye(N))) < 1e-11
    E2, C2 = hf.scf.eig_gsym_sub(F, X, blocks)
    assert np.array_equal(E, E2) and np.array_equal(C, C2)


# ---------------------------------------------------------------------------------------------------
# Fock build parity: atomic J, K, XC against the oracle (BASELINE configs 1 and 2 run on this path)
# ---------------------------------------------------------------------------------------------------
ATOMIC_CASES = {
    # name: (Z, lmax, mmax, nelem, nnodes)
    "s_only": (2, 0, 0, 3, 6),
    "sp": (10, 1, 1, 3, 5),
    "spd_m1": (18, 2, 1, 2, 6),
    "spdf_full": (4, 3, 3, 1, 5),
}


@pytest.fixture(scope="module", params=sorted(ATOMIC_CASES))
def acase(request, hf):
    import common
    Z, lmax, mmax, nelem, nnodes = ATOMIC_CASES[request.param]
    gb, ob = common.make_atomic_bases(Z, lmax, mmax, nelem, nnodes)
    gb.compute_tei(True)
    ob.compute_tei(True)
    ldft, mdft = 4 * lmax + 10, 4 * mmax + 5
    gb.upload(ldft, mdft)
    return request.param, gb, ob, ldft, mdft


def test_atomic_one_electron_matrices(acase):
    import common
    name, gb, ob, _, _ = acase
    assert gb.Nbf() == ob.Nbf
    for which, M in (("overlap", gb.overlap()), ("kinetic", gb.kinetic()), ("nuclear", gb.nuclear())):
        assert common.relerr(M, ob.onebody(which)) < 1e-14, (name, which)


def test_atomic_coulomb_parity(acase):
    import common
    name, gb, ob, _, _ = acase
    for tag, P in _densities(gb):
        J = gb.coulomb(P)
        Jo = ob.coulomb(P)
        assert common.relerr(J, Jo) < 1e-12, (name, tag, common.relerr(J, Jo))


def test_atomic_exchange_parity(acase):
    import common
    name, gb, ob, _, _ = acase
    for tag, P in _densities(gb):
        K = gb.exchange(P)
        Ko = ob.exchange(P)
        assert common.relerr(K, Ko) < 1e-12, (name, tag, common.relerr(K, Ko))


@pytest.mark.parametrize("funcs", [(1, 7), (101, 130), (101, 0), (0, 130), (1, 12), (202, 231), (106, 131), (402, 0)])
def test_atomic_xc_parity(acase, hf, funcs):
    import common
    name, gb, ob, ldft, mdft = acase
    grid = hf.DFTGrid(gb, ldft, mdft)
    x, c = funcs
    for tag, P in _densities(gb):
        if tag == "general":
            P = 0.05 * P + list(_densities(gb))[1][1]
        H, Exc, Nel, _ = grid.eval_Fxc(x, c, P)
        Ho, Exco, Nelo, _ = ob.eval_Fxc(ldft, mdft, x, c, P)
        assert abs(Nel - Nelo) < 1e-11 * max(1.0, abs(Nelo)), (name, tag, Nel, Nelo)
        assert abs(Exc - Exco) < 1e-11 * max(1.0, abs(Exco)), (name, tag, Exc, Exco)
        assert common.relerr(H, Ho) < 1e-10, (name, tag, funcs, common.relerr(H, Ho))


def _spin_densities(gb):
    """two different positive block-diagonal spin densities"""
    import common
    N = gb.Nbf()
    blocks = gb.get_sym_idx(1)
    Pa = common.random_density(N, 2, seed=21, blocks=blocks) + 0.03 * common.random_density(N, 3, seed=23)
    Pb = common.random_density(N, 1, seed=22, blocks=blocks)
    return Pa, Pb


def _orbital_spin_densities(gb, na=3, nb=2):
    """spin densities of the lowest core-Hamiltonian orbitals: smooth, with the tails real densities have.  The
    polarised meta-GGA potentials are ill-conditioned on random matrices: where rho_b sinks under the threshold while its
    gradient stays finite (a node of a random density), d e_c/d sigma_bb ~ (1 - zeta)^{-4/3} reaches 1e11 and more, and
    two arithmetic routes then differ in the leading digits.  Physical densities have the gradient vanish with the
    density."""
    import scipy.linalg as sl
    E, C = sl.eigh(gb.kinetic() + gb.nuclear(), gb.overlap())
    return np.asfortranarray(C[:, :na] @ C[:, :na].T), np.asfortranarray(C[:, :nb] @ C[:, :nb].T)


@pytest.mark.parametrize("funcs", [(202, 231), (202, 0), (0, 231), (202, 130)])
def test_xc_polarized_mgga_parity(case, hf, funcs):
    """DFTGridWorker::update_density(Pa,Pb) with tau, compute_xc and eval_Fxc(Ha,Hb) for a tau-dependent functional
    (src/diatomic/dftgrid.cpp:119-200, 343-458, 547-640)"""
    import common
    name, gb, ob, ldft, mdft = case
    grid = hf.DFTGrid(gb, ldft, mdft)
    x, c = funcs
    for Pa, Pb in (_orbital_spin_densities(gb, 3, 2), _orbital_spin_densities(gb, 2, 0)):
        Ha, Hb, Exc, Nel, Ekin = grid.eval_Fxc_pol(x, c, Pa, Pb)
        Hao, Hbo, Exco, Nelo, Ekino = ob.eval_Fxc_pol(ldft, mdft, x, c, Pa, Pb)
        assert np.all(np.isfinite(Ha)) and np.all(np.isfinite(Hb))
        assert abs(Nel - Nelo) < 1e-11 * max(1.0, abs(Nelo)), (name, Nel, Nelo)
        assert abs(Exc - Exco) < 1e-10 * max(1.0, abs(Exco)), (name, funcs, Exc, Exco)
        assert abs(Ekin - Ekino) < 1e-10 * max(1.0, abs(Ekino)), (name, funcs, Ekin, Ekino)
        assert common.relerr(Ha, Hao) < 1e-8, (name, funcs, common.relerr(Ha, Hao))
        if np.max(np.abs(Pb)) > 0:
            assert common.relerr(Hb, Hbo) < 1e-8, (name, funcs, common.relerr(Hb, Hbo))
        else:  # empty channel: potential evaluated at rho_b = threshold, see test_xc_polarized_parity
            assert common.relerr(Hb, Hbo) < 1e-4, (name, funcs, common.relerr(Hb, Hbo))


@pytest.mark.parametrize("funcs", [(1, 7), (101, 130), (1, 12), (101, 0), (0, 130), (406, 0), (106, 131), (0, 131), (402, 0), (1, 8)])
def test_xc_polarized_parity(case, hf, funcs):
    import common
    name, gb, ob, ldft, mdft = case
    grid = hf.DFTGrid(gb, ldft, mdft)
    x, c = funcs
    Pa, Pb = _spin_densities(gb)
    Ha, Hb, Exc, Nel, _ = grid.eval_Fxc_pol(x, c, Pa, Pb)
    Hao, Hbo, Exco, Nelo, _ = ob.eval_Fxc_pol(ldft, mdft, x, c, Pa, Pb)
    assert abs(Nel - Nelo) < 1e-11 * max(1.0, abs(Nelo)), (name, Nel, Nelo)
    assert abs(Exc - Exco) < 1e-11 * max(1.0, abs(Exco)), (name, Exc, Exco)
    assert common.relerr(Ha, Hao) < 1e-10, (name, funcs, common.relerr(Ha, Hao))
    assert common.relerr(Hb, Hbo) < 1e-10, (name, funcs, common.relerr(Hb, Hbo))
    # a fully polarised density (Pb = 0, the hydrogen-like case) must stay finite and agree too
    Ha, Hb, Exc, Nel, _ = grid.eval_Fxc_pol(x, c, Pa, 0.0 * Pb)
    Hao, Hbo, Exco, Nelo, _ = ob.eval_Fxc_pol(ldft, mdft, x, c, Pa, 0.0 * Pb)
    assert np.all(np.isfinite(Ha)) and np.all(np.isfinite(Hb))
    assert abs(Exc - Exco) < 1e-11 * max(1.0, abs(Exco))
    # the empty channel's potential is evaluated at rho_b = threshold where d/d rho_b of (1 - zeta)^{2/3, 4/3} is
    # huge: two arithmetic routes agree to ~1e-7 there, not to rounding
    # (gga_c_lyp alone: the checker sums the gradient terms of the published formula as printed, which cancel to 1e-8 of
    # their size where one spin density dominates; the kernels use the collapsed form, see xc_device.h)
    tola = 1e-7 if funcs == (0, 131) else 1e-10
    assert common.relerr(Ha, Hao) < tola and common.relerr(Hb, Hbo) < 1e-5, (name, funcs)


def test_xc_polarized_equals_restricted_for_equal_spins(case, hf):
    import common
    name, gb, ob, ldft, mdft = case
    grid = hf.DFTGrid(gb, ldft, mdft)
    Pa, _ = _spin_densities(gb)
    Ha, Hb, Exc, Nel, _ = grid.eval_Fxc_pol(101, 130, Pa, Pa)
    H, Exc0, Nel0, _ = grid.eval_Fxc(101, 130, 2.0 * Pa)
    assert abs(Exc - Exc0) < 1e-11 * abs(Exc0) and abs(Nel - Nel0) < 1e-11 * Nel0
    assert common.relerr(Ha, H) < 1e-10 and common.relerr(Hb, H) < 1e-10


@pytest.mark.parametrize("funcs", [(1, 7), (101, 130)])
def test_atomic_xc_polarized_parity(acase, hf, funcs):
    import common
    name, gb, ob, ldft, mdft = acase
    grid = hf.DFTGrid(gb, ldft, mdft)
    x, c = funcs
    Pa, Pb = _spin_densities(gb)
    Ha, Hb, Exc, Nel, _ = grid.eval_Fxc_pol(x, c, Pa, Pb)
    Hao, Hbo, Exco, Nelo, _ = ob.eval_Fxc_pol(ldft, mdft, x, c, Pa, Pb)
    assert abs(Nel - Nelo) < 1e-11 * max(1.0, abs(Nelo)), (name, Nel, Nelo)
    assert abs(Exc - Exco) < 1e-11 * max(1.0, abs(Exco)), (name, Exc, Exco)
    assert common.relerr(Ha, Hao) < 1e-10 and common.relerr(Hb, Hbo) < 1e-10, (name, funcs)


OPEN_SHELL_CASES = [
    # unrestricted runs: NIST LSD (VWN) atomic reference data, numerical UHF limits, H/PBE
    ("H_LSD", "atomic", dict(Z=1, lmax=0, mmax=0, nelem=5, nnodes=15, method="lda_x-lda_c_vwn", M=2), -0.478671, 2e-6),
    ("H_PBE", "atomic", dict(Z=1, lmax=0, mmax=0, nelem=5, nnodes=15, method="gga_x_pbe-gga_c_pbe", M=2), -0.499990, 2e-6),
    ("Li_UHF", "atomic", dict(Z=3, lmax=0, mmax=0, nelem=5, nnodes=15, method="HF", M=2), -7.432751, 2e-6),
    ("N_LSD", "atomic", dict(Z=7, lmax=1, mmax=1, nelem=5, nnodes=12, method="lda_x-lda_c_vwn", M=4), -54.136799, 5e-6),
    # spin-polarised B-LYP / B3LYP: hydrogen (LYP has no self-correlation: E = T + V + J + E_x^B88) and nitrogen 4S against the checker
    ("H_BLYP", "atomic", dict(Z=1, lmax=0, mmax=0, nelem=5, nnodes=12, method="gga_x_b88-gga_c_lyp", M=2), None, None),
    ("N_B3LYP", "atomic", dict(Z=7, lmax=1, mmax=1, nelem=5, nnodes=12, method="hyb_gga_xc_b3lyp", M=4), None, None),
    # restricted open shell (constrained-UHF form of ROHF, scf::ROHF_update): M < 0 selects it; ROHF limits
    ("Li_ROHF", "atomic", dict(Z=3, lmax=0, mmax=0, nelem=5, nnodes=15, method="HF", M=-2), -7.4327269, 1e-6),
    ("N_ROHF", "atomic", dict(Z=7, lmax=1, mmax=1, nelem=5, nnodes=12, method="HF", M=-4), -54.400934, 2e-6),
    # --maverage (scf::fock_symmetry_average): boron 2P with spherically averaged Fock matrices
    ("B_UHF_maverage", "atomic", dict(Z=5, lmax=1, mmax=1, nelem=4, nnodes=10, method="HF", M=2, maverage=True), None, None),
    # (a DFT run of boron would depend on WHICH of the degenerate p orbitals the aufbau picks: |Y10|^2 and |Y11|^2 are
    # different densities for a density functional; nitrogen 4S fills all three)
    # the same with the open p shell FORCED into m = 0 / m = +1 on both sides (--readocc, scf::enforce_occupations): no
    # degeneracy left to rounding noise, so every energy component is compared
    ("B_UHF_maverage_forced_m0", "atomic", dict(Z=5, lmax=1, mmax=1, nelem=4, nnodes=10, method="HF", M=2, maverage=True,
                                                occs=[[3, 2, 0], [0, 0, 1], [0, 0, -1]]), None, None),
    ("B_UHF_maverage_forced_m1", "atomic", dict(Z=5, lmax=1, mmax=1, nelem=4, nnodes=10, method="HF", M=2, maverage=True,
                                                occs=[[2, 2, 0], [1, 0, 1], [0, 0, -1]]), None, None),
    # forced occupations reach excited states: Li 1s2 2p (numerical HF -7.365070), and a pi state of HeH
    ("Li_2P_forced", "atomic", dict(Z=3, lmax=1, mmax=1, nelem=4, nnodes=10, method="HF", M=2, occs=[[1, 1, 0], [0, 0, 1], [1, 0, -1]]),
     -7.365070, 5e-5),
    ("Li_2P_forced_lm_blocks", "atomic", dict(Z=3, lmax=1, mmax=1, nelem=4, nnodes=10, method="HF", M=2, symmetry=2,
                                              occs=[[1, 1, 0, 0], [1, 0, 1, 1], [0, 0, 1, 0], [0, 0, 1, -1]]), -7.365070, 5e-5),
    ("HeH_pi_forced", "diatomic", dict(Z1=2, Z2=1, Rbond=1.5, lmmax=[4, 3], nelem=2, nnodes=8, method="HF", M=2,
                                       occs=[[1, 1, 0], [1, 0, 1], [0, 0, -1]]), None, None),
    # homonuclear molecule with --symmetry 2: occupations by m AND parity (fourth column +-1, main.cpp:352-365): the
    # 1 sigma_g 2 sigma_g triplet of H2 (not the Aufbau state, which is sigma_g sigma_u)
    ("H2_triplet_forced_parity", "diatomic", dict(Z1=1, Z2=1, Rbond=2.0, lmmax=[6], nelem=3, nnodes=10, method="HF", M=3, symmetry=2,
                                                  occs=[[2, 0, 0, 1], [0, 0, 0, -1]]), None, None),
    ("N_LSD_maverage", "atomic", dict(Z=7, lmax=1, mmax=1, nelem=4, nnodes=10, method="lda_x-lda_c_vwn", M=4, maverage=True),
     None, None),
    ("H_PBE0", "atomic", dict(Z=1, lmax=0, mmax=0, nelem=5, nnodes=15, method="hyb_gga_xc_pbeh", M=2), None, None),
    # unrestricted meta-GGA: TPSS, Staroverov et al., PRB 69, 075102 (4 decimals)
    ("H_TPSS", "atomic", dict(Z=1, lmax=0, mmax=0, nelem=5, nnodes=12, method="mgga_x_tpss-mgga_c_tpss", M=2), -0.5002, 1e-4),
    ("Li_TPSS", "atomic", dict(Z=3, lmax=0, mmax=0, nelem=5, nnodes=12, method="mgga_x_tpss-mgga_c_tpss", M=2), -7.4891, 1e-4),
    ("N_TPSS", "atomic", dict(Z=7, lmax=1, mmax=1, nelem=5, nnodes=12, method="mgga_x_tpss-mgga_c_tpss", M=4), None, None),
    ("HeH_TPSS_diatomic", "diatomic", dict(Z1=2, Z2=1, Rbond=1.5, lmmax=[3, 1], nelem=2, nnodes=8,
                                           method="mgga_x_tpss-mgga_c_tpss", M=2), None, None),
    ("H2+_like_HeH2+", "diatomic", dict(Z1=1, Z2=1, Rbond=2.0, lmmax=[6], nelem=3, nnodes=10, method="HF", M=3), None, None),
    ("OH_like_LiH+_PBE", "diatomic", dict(Z1=3, Z2=0, Rbond=3.0, lmmax=[4, 2], nelem=3, nnodes=8,
                                          method="gga_x_pbe-gga_c_pbe", M=2), None, None),
]


@pytest.mark.parametrize("name,prog,kw,lit,littol", OPEN_SHELL_CASES, ids=[c[0] for c in OPEN_SHELL_CASES])
def test_unrestricted_scf_energy_parity(hf, name, prog, kw, lit, littol):
    import oracle_lib as orc
    gfn, ofn = (hf.scf_atomic, orc.scf_atomic) if prog == "atomic" else (hf.scf_diatomic, orc.scf_diatomic)
    g = gfn(convthr=1e-9, maxit=80, **kw)
    o = ofn(convthr=1e-9, maxit=80, **kw)
    assert g["converged"] and o["converged"]
    assert abs(g["Etot"] - o["Etot"]) < 1e-8 * max(1.0, abs(o["Etot"]) / 10), (name, g["Etot"], o["Etot"])
    # degenerate open shell under --maverage: only boron's single p electron (nitrogen 4S fills m = -1, 0, 1: no choice)
    if name == "B_UHF_maverage":
        # The averaged Fock operator leaves the open p shell exactly degenerate in m: which member the Aufbau rule
        # occupies (the torus of m = +-1 or the dumbbell of m = 0) is decided by rounding noise in the eigenvalue order.
        # The members share the radial functions, hence Etot, Ekin, Epot and the SUM of the two-electron terms; the
        # split between Coulomb and exchange energy differs between them (observed: 8.6e-3 Eh for boron).
        g2, o2 = (g["Ecoul"] + g["Exx"] + g["Exc"]), (o["Ecoul"] + o["Exx"] + o["Exc"])
        assert abs(g2 - o2) < 1e-6 * max(1.0, abs(o2) / 10), (name, "two-electron", g2, o2)
        for k in ("Ekin", "Epot"):
            assert abs(g[k] - o[k]) < 1e-6 * max(1.0, abs(o[k]) / 10), (name, k, g[k], o[k])
    else:
        for k in ("Ekin", "Epot", "Ecoul", "Exx", "Exc"):
            assert abs(g[k] - o[k]) < 1e-6 * max(1.0, abs(o[k]) / 10), (name, k, g[k], o[k])
    if lit is not None:
        assert abs(g["Etot"] - lit) < littol, (name, g["Etot"], lit)


ATOMIC_SCF_CASES = [
    # BASELINE config 1: He, LDA (NIST reference-data total energy) ; config 2-like: Ne / Be with l up to 1
    ("He_LDA", dict(Z=2, lmax=0, mmax=0, nelem=5, nnodes=15, method="lda_x-lda_c_vwn"), -2.834836, 2e-6),
    ("He_PBE", dict(Z=2, lmax=0, mmax=0, nelem=5, nnodes=15, method="gga_x_pbe-gga_c_pbe"), -2.892935, 2e-6),
    ("He_HF", dict(Z=2, lmax=0, mmax=0, nelem=5, nnodes=15, method="HF"), -2.8616799956, 1e-8),
    ("Be_HF", dict(Z=4, lmax=0, mmax=0, nelem=5, nnodes=15, method="HF"), -14.573023168, 1e-7),
    ("Ne_HF", dict(Z=10, lmax=1, mmax=1, nelem=5, nnodes=15, method="HF"), -128.54709811, 1e-7),
    ("Ne_LDA", dict(Z=10, lmax=1, mmax=1, nelem=5, nnodes=15, method="lda_x-lda_c_vwn"), -128.233481, 2e-6),
    # global hybrid: J + 0.25 K + XC in one Fock build (hyb_gga_xc_pbeh = PBE0)
    ("He_PBE0", dict(Z=2, lmax=0, mmax=0, nelem=5, nnodes=15, method="hyb_gga_xc_pbeh"), -2.895178, 2e-6),
    # B-LYP and B3LYP (0.20 exact exchange; libxc's definition with the VWN RPA fit): literature totals to four decimals
    ("He_BLYP", dict(Z=2, lmax=0, mmax=0, nelem=5, nnodes=12, method="gga_x_b88-gga_c_lyp"), -2.9071, 1e-4),
    ("He_B3LYP", dict(Z=2, lmax=0, mmax=0, nelem=5, nnodes=12, method="hyb_gga_xc_b3lyp"), -2.9152, 1e-4),
    ("Ne_B3LYP", dict(Z=10, lmax=1, mmax=1, nelem=5, nnodes=12, method="hyb_gga_xc_b3lyp"), -128.9810, 3e-4),
    # meta-GGA (tau): TPSS, total energies of Staroverov et al., PRB 69, 075102, Table (4 decimals)
    ("He_TPSS", dict(Z=2, lmax=0, mmax=0, nelem=5, nnodes=15, method="mgga_x_tpss-mgga_c_tpss"), -2.9097, 1e-4),
    ("Ne_TPSS", dict(Z=10, lmax=1, mmax=1, nelem=4, nnodes=12, method="mgga_x_tpss-mgga_c_tpss"), -128.9811, 2e-4),
    # BASELINE config 2 itself: Ar, PBE, 20 radial elements x 15 nodes, lmax = mmax = 1 (Nbf = 1116, (l,m) blocks of 279);
    # the same basis with LDA against the NIST reference-data total energy
    ("Ar_PBE_config2", dict(Z=18, lmax=1, mmax=1, nelem=20, nnodes=15, method="gga_x_pbe-gga_c_pbe", symmetry=2), None, None),
    ("Ar_LDA_config2_basis", dict(Z=18, lmax=1, mmax=1, nelem=20, nnodes=15, method="lda_x-lda_c_vwn", symmetry=2),
     -525.946195, 2e-6),
]


@pytest.mark.parametrize("name,kw,lit,littol", ATOMIC_SCF_CASES, ids=[c[0] for c in ATOMIC_SCF_CASES])
def test_atomic_scf_energy_parity(hf, name, kw, lit, littol):
    import oracle_lib as orc
    g = hf.scf_atomic(convthr=1e-9, maxit=60, **kw)
    o = orc.scf_atomic(convthr=1e-9, maxit=60, **kw)
    assert g["converged"] and o["converged"]
    assert abs(g["Etot"] - o["Etot"]) < 1e-8 * max(1.0, abs(o["Etot"]) / 10), (name, g["Etot"], o["Etot"])
    for k in ("Ekin", "Epot", "Ecoul", "Exx", "Exc"):
        assert abs(g[k] - o[k]) < 1e-6 * max(1.0, abs(o[k]) / 10), (name, k, g[k], o[k])
    if lit is not None:
        assert abs(g["Etot"] - lit) < littol, (name, g["Etot"], lit)


# ---------------------------------------------------------------------------------------------------
# end-to-end SCF: converged total energies, GPU vs oracle on identical grids (north-star bar: 1e-8 Eh)
# ---------------------------------------------------------------------------------------------------
SCF_CASES = [
    ("N2_TPSS_small", dict(Z1=7, Z2=7, Rbond=2.068, lmmax=[4, 3], nelem=3, nnodes=8, method="mgga_x_tpss-mgga_c_tpss"), None, None),
    ("N2_PBE0_small", dict(Z1=7, Z2=7, Rbond=2.068, lmmax=[4, 3], nelem=3, nnodes=8, method="hyb_gga_xc_pbeh"), None, None),
    # BASELINE config 3: diatomic H2 at R=1.4, HF, small (mu,nu) grid
    ("H2_HF", dict(Z1=1, Z2=1, Rbond=1.4, lmmax=[6], nelem=3, nnodes=10, method="HF"), -1.13362957, 2e-7),
    ("H2_LDA", dict(Z1=1, Z2=1, Rbond=1.4, lmmax=[4], nelem=2, nnodes=8, method="lda_x-lda_c_vwn"), None, None),
    ("HeH+like_PBE", dict(Z1=2, Z2=0, Rbond=2.0, lmmax=[5], nelem=3, nnodes=8, method="gga_x_pbe-gga_c_pbe"), None, None),
]


@pytest.mark.parametrize("name,kw,lit,littol", SCF_CASES)
def test_scf_energy_parity(hf, name, kw, lit, littol):
    import oracle_lib as orc
    g = hf.scf_diatomic(convthr=1e-9, maxit=60, **kw)
    o = orc.scf_diatomic(convthr=1e-9, maxit=60, **kw)
    assert g["converged"] and o["converged"]
    assert abs(g["Etot"] - o["Etot"]) < 1e-8, (name, g["Etot"], o["Etot"])
    for k in ("Ekin", "Epot", "Ecoul", "Exx", "Exc"):
        assert abs(g[k] - o[k]) < 1e-6, (name, k, g[k], o[k])
    if lit is not None:
        assert abs(g["Etot"] - lit) < littol, (name, g["Etot"], lit)


def test_scf_device_resident_driver_matches_host_pointer_driver(hf, monkeypatch):
    """hfg_scf_* keeps every matrix in HBM (DIIS included); HELFEM_SCF=host runs the same loop through the
    host-pointer entry points -- both must give the same energies and iteration counts"""
    kw = dict(Z1=7, Z2=7, Rbond=2.068, lmmax=[4, 3], nelem=3, nnodes=8, method="gga_x_pbe-gga_c_pbe")
    dev = hf.scf_diatomic(convthr=1e-8, maxit=60, **kw)
    monkeypatch.setenv("HELFEM_SCF", "host")
    host = hf.scf_diatomic(convthr=1e-8, maxit=60, **kw)
    assert dev["converged"] and host["converged"] and dev["iterations"] == host["iterations"]
    for k in ("Etot", "Ekin", "Epot", "Ecoul", "Exc"):
        assert abs(dev[k] - host[k]) < 1e-8 * max(1.0, abs(host[k])), (k, dev[k], host[k])
    kw = dict(Z=7, lmax=1, mmax=1, nelem=4, nnodes=10, method="HF", M=4)
    monkeypatch.delenv("HELFEM_SCF")
    dev = hf.scf_atomic(convthr=1e-8, maxit=60, **kw)
    monkeypatch.setenv("HELFEM_SCF", "host")
    host = hf.scf_atomic(convthr=1e-8, maxit=60, **kw)
    assert dev["converged"] and host["converged"]
    assert abs(dev["Etot"] - host["Etot"]) < 1e-8 and abs(dev["Exx"] - host["Exx"]) < 1e-7


# ---------------------------------------------------------------------------------------------------
# divide-and-conquer tridiagonal stage: hard spectra (through eig_sym on tridiagonal input)
# ---------------------------------------------------------------------------------------------------
def _tridiag(d, e):
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def _hard_cases():
    rng = np.random.RandomState(42)
    n = 300
    yield "near_identity", _tridiag(np.ones(n), np.full(n - 1, 1e-9))
    yield "graded", _tridiag(np.arange(n, dtype=float) ** 3, rng.uniform(0, 1, n - 1))
    yield "wilkinson", _tridiag(np.abs(np.arange(n) - n // 2).astype(float), np.ones(n - 1))
    yield "toeplitz", _tridiag(np.zeros(n), np.ones(n - 1))
    yield "decoupled", _tridiag(rng.uniform(-1, 1, n), np.where(rng.rand(n - 1) < 0.3, 0.0, rng.uniform(-1, 1, n - 1)))
    dd = rng.uniform(-1, 1, n)
    dd[100:140] = 0.5
    yield "clustered", _tridiag(dd, rng.uniform(-1, 1, n - 1) * 1e-8)
    yield "dynamic_range", _tridiag(np.exp(rng.uniform(-20, 15, n)), np.exp(rng.uniform(-20, 10, n - 1)))
    for m in (33, 65, 97, 129, 513, 1000):
        yield "random_%d" % m, _tridiag(rng.uniform(-1, 1, m), rng.uniform(-1, 1, m - 1))
    # exactly degenerate blocks (the +m / -m degeneracy of the diatomic problem when symmetry is off)
    A = rng.uniform(-1, 1, (40, 40))
    A = A + A.T
    Z = np.zeros_like(A)
    yield "degenerate_pairs", np.block([[A, Z], [Z, A]])


@pytest.mark.parametrize("name,A", list(_hard_cases()), ids=[c[0] for c in _hard_cases()])
def test_eig_sym_hard_spectra(hf, name, A):
    n = A.shape[0]
    E, C = hf.scf.eig_sym(A)
    Eref = np.linalg.eigvalsh(A)
    scale = max(np.max(np.abs(Eref)), 1e-300)
    assert np.max(np.abs(E - Eref)) < 5e-14 * scale * max(np.sqrt(n), 10), (name, np.max(np.abs(E - Eref)) / scale)
    assert np.max(np.abs(C.T @ C - np.eye(n))) < 1e-12, name
    assert np.max(np.abs(A @ C - C * E)) < 1e-12 * scale * max(np.sqrt(n), 10), name


def test_eig_sym_2305_more_than_twelve_slabs(hf):
    """n > 1536: the sweep's partial-slab sums leave their unrolled part (rolled tail loops), 19 x 19 tiles"""
    rng = np.random.RandomState(8)
    n = 2305
    A = rng.uniform(-1, 1, (n, n))
    A = A + A.T
    E, C = hf.scf.eig_sym(A)
    Eref = np.linalg.eigvalsh(A)
    assert np.max(np.abs(E - Eref)) < 1e-10 * n
    assert np.max(np.abs(C.T @ C - np.eye(n))) < 1e-10
    assert np.max(np.abs(A @ C - C * E)) < 1e-9 * n


def test_eig_sym_1400_dense(hf):
    rng = np.random.RandomState(7)
    n = 1400
    A = rng.uniform(-1, 1, (n, n))
    A = A + A.T + np.diag(np.linspace(0, 2000.0, n))
    E, C = hf.scf.eig_sym(A)
    Eref = np.linalg.eigvalsh(A)
    assert np.max(np.abs(E - Eref)) < 1e-10
    assert np.max(np.abs(C.T @ C - np.eye(n))) < 1e-11
    assert np.max(np.abs(A @ C - C * E)) < 1e-9


# ---------------------------------------------------------------------------------------------------
# multi-GPU sharding rules, exercised on one device: shards (rank r of n) must sum to the unsharded result
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_sharded_step_sums_to_unsharded(hf, nranks):
    import common
    import ctypes
    import torch
    gb, _ = common.make_bases(7, 7, 2.068, (3, 2), 2, 5, oracle=False)
    gb.compute_tei(False)
    ldft, mdft = 24, 13
    N = gb.Nbf()
    blocks = gb.get_sym_idx(1)
    P = common.random_density(N, 2, seed=33, blocks=blocks)
    S = gb.overlap()
    H0 = gb.kinetic() + gb.nuclear()
    full = hf.DeviceSCFStep(gb, 101, 130, ldft, mdft, 3, symmetry=1, device=0, rank=0, nranks=1)
    X = hf.scf.form_Sinvh(S, False, blocks, ctx=full.ctx)
    full.set_matrices(H0, X)
    full.set_density(P)
    full.step(None)
    torch.cuda.synchronize()
    Fc_ref = full.Fc.clone()
    scal_ref = full.scal.clone()
    E_ref, C_ref, P_ref = full.E.clone(), full.C.clone(), full.P.clone()
    Fc_sum = torch.zeros_like(Fc_ref)
    scal_sum = torch.zeros_like(scal_ref)
    bb_sum = torch.zeros_like(full.blockbuf)
    for r in range(nranks):
        full.ctx.set_shard(r, nranks)
        full.set_density(P)
        full.fock_partial()
        torch.cuda.synchronize()
        Fc_sum += full.Fc
        scal_sum += full.scal
    assert float((Fc_sum - Fc_ref).abs().max()) < 1e-11 * float(Fc_ref.abs().max())
    assert float((scal_sum - scal_ref).abs().max()) < 1e-11 * float(scal_ref.abs().max())
    # eigensolve: each rank's owned blocks, summed buffer, then assemble
    full.Fc.copy_(Fc_sum)
    full.fock_finish()
    for r in range(nranks):
        full.ctx.set_shard(r, nranks)
        full.eig_partial()
        torch.cuda.synchronize()
        bb_sum += full.blockbuf
    full.blockbuf.copy_(bb_sum)
    full.ctx.set_shard(0, 1)
    full.eig_finish()
    full.density()
    torch.cuda.synchronize()
    assert float((full.E - E_ref).abs().max()) < 1e-10 * max(1.0, float(E_ref.abs().max()))
    assert float((full.P - P_ref).abs().max()) < 1e-9 * max(1.0, float(P_ref.abs().max()))


def test_fixed_sinvh_declaration_caches_block_supports_only_for_that_matrix(hf):
    """hfg_ctx_fix_sinvh: the column supports of the blocks are derived once per declaration; a different matrix, a new
    declaration of a matrix at the same address or other blocks are derived afresh"""
    import torch
    import oracle_lib as orc
    rng = np.random.RandomState(8)
    sizes = [40, 25, 35]
    N = sum(sizes)

    def problem(seed, perm):
        r = np.random.RandomState(seed)
        blocks, o = [], 0
        for sz in sizes:
            blocks.append(np.sort(perm[o:o + sz]))
            o += sz
        F = r.uniform(-1, 1, (N, N))
        F = F + F.T
        A = r.uniform(-1, 1, (N, N))
        S = A @ A.T + N * np.eye(N)
        for i, bi in enumerate(blocks):
            for j, bj in enumerate(blocks):
                if i != j:
                    S[np.ix_(bi, bj)] = 0.0
                    F[np.ix_(bi, bj)] = 0.0
        return F, S, blocks

    import ctypes
    ctx = hf.default_context()
    dev = torch.device("cuda", 0)
    perm1, perm2 = rng.permutation(N), rng.permutation(N)
    F1, S1, b1 = problem(1, perm1)
    F2, S2, b2 = problem(2, perm2)
    X1, X2 = orc.form_Sinvh(S1, False, b1), orc.form_Sinvh(S2, False, b2)

    def up(M):
        return torch.from_numpy(np.asfortranarray(M).ravel(order="F").copy()).to(dev)

    def solve(Fd, Xd, blocks):
        ptr, idx = hf.scf._blocks(blocks)
        Ed, Cd = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(N * N, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        i64p = ctypes.POINTER(ctypes.c_int64)
        rc = hf.lib().hfg_eig_gsym_sub_dev(ctx.h, ctypes.c_int64(N), ctypes.c_void_p(Fd.data_ptr()), ctypes.c_void_p(Xd.data_ptr()),
                                           len(blocks), ptr.ctypes.data_as(i64p), idx.ctypes.data_as(i64p),
                                           ctypes.c_void_p(Ed.data_ptr()), ctypes.c_void_p(Cd.data_ptr()))
        assert rc == 0, hf.lib().hfg_last_error(ctx.h)
        ctx.synchronize()
        return Ed.cpu().numpy(), Cd.cpu().numpy().reshape((N, N), order="F")

    Xd = up(X1)
    try:
        ctx.fix_sinvh(Xd.data_ptr())
        for rep in range(2):  # second call: cached supports
            E, C = solve(up(F1), Xd, b1)
            assert np.max(np.abs(E - orc.eig_gsym_sub(F1, X1, b1)[0])) < 1e-10
        # same address, new contents and blocks, declared again: nothing stale may be used
        Xd.copy_(up(X2))
        ctx.fix_sinvh(Xd.data_ptr())
        E, C = solve(up(F2), Xd, b2)
        assert np.max(np.abs(E - orc.eig_gsym_sub(F2, X2, b2)[0])) < 1e-10
        assert np.max(np.abs(C.T @ S2 @ C - np.eye(N))) < 1e-10
        # declared matrix, other blocks of the same sizes: the key holds the index lists
        ctx.fix_sinvh(Xd.data_ptr())
        E, C = solve(up(F2), Xd, b2)
        Xd.copy_(up(X1))
        ctx.fix_sinvh(Xd.data_ptr())
        E, C = solve(up(F1), Xd, b1)
        assert np.max(np.abs(E - orc.eig_gsym_sub(F1, X1, b1)[0])) < 1e-10
    finally:
        ctx.fix_sinvh(None)
