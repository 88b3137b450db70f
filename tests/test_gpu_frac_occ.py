"""Fractional occupations by symmetry block on the device: hfg_occupy_blocks_devptr (Context.occupy_blocks) alone against a
NumPy restatement written here, and DeviceFracSCFStep on the basis of the Ne pin (lmax = 1, mmax = 1, 5 elements of 15
nodes, symmetry 2).

The stage.  Five blocks of 1, 63, 64, 65 and 257 rows (N = 450: a block on each side of a wave and of a 256-thread
workgroup), the rows of the blocks interleaved, block-sparse random C whose columns are interleaved by a random ascending E
with two pairs of exactly equal energies (one inside the 257 block, one across the 65 and the 257 block); occupation lists
of length 0, 1, the full block (64), one with zeros in the middle, and 24 values that reach past both ties.  Cocc, Eocc and
Focc are compared with == : the square root comes from the host's correctly rounded sqrt on both sides and one IEEE
multiplication is all that follows.  The same for columns handed over in no order at all (the rank is by (E, column
index)), a second call bit for bit, E and C untouched, one call queued directly behind a device copy into C on the same
stream, and the one refusal that needs the device (more occupations than a block has rows), with the row counts it keeps
per block-id array and Context.forget_block_ids.

Longer columns.  Up to 512 rows a wave of k_occ_argmax takes a column; beyond, a workgroup of four waves strides over it and
hands the waves' maxima on through LDS.  Blocks of 70 and 513 rows (N = 583: two strides of 256 and a tail of 71) go through
the same exact comparison, with columns whose largest magnitude stands twice, in rows of different blocks: in the same
thread (256 rows apart), in two lanes of one wave, in two waves, and in the tail.  The lowest row decides the block.

The step.  (1) Ne with every occupation 1.0 against DeviceSCFStep.run, both at convthr = 1e-8: |dEtot| < 1e-8 and the same
number of iterations.  (2) Carbon, LDA, occupations from spherical_occupations, run(convthr = 1e-7): P to the host, F
rebuilt from it through the host-pointer entries only, Sinvh^T (F P S - S P F) Sinvh below 2 convthr with the total density
P (twice the P/2 that run() tests against convthr: the stricter reading), tr(P S) = 6 to 1e-10, and the three (1, m) diagonal
blocks of P equal to within ten times the largest difference that the density SciPy occupies from the same F shows.  (3) the
same self-consistency for boron with exact exchange (kfrac = 1, K rebuilt with basis.exchange(P / 2)): the low-rank exchange
on scaled factors.  (4) NIST atomic reference data, LDA: H (occupation 0.5), C, N and O to the 2e-6 of the He, Ne and Rn pins.

Measured on the MI355X: see DESIGN.md section 3.5b."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (1, 63, 64, 65, 257)
N = sum(SIZES)


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    return helfem_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ---- the stage alone --------------------------------------------------------------------------------------------------
def problem(sort=True):
    """blockid (N), E (N), C (N x N, column-major) and the occupation lists; built once per variant and never changed"""
    rng = np.random.RandomState(20260 + int(sort))
    blockid = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int32)
    rng.shuffle(blockid)
    colblk = np.repeat(np.arange(len(SIZES)), SIZES)
    rng.shuffle(colblk)

    def put(pos, b):  # column pos belongs to block b: swap with a later column of that block
        if colblk[pos] != b:
            other = [j for j in range(40, N) if colblk[j] == b][0]
            colblk[other], colblk[pos] = colblk[pos], b
    put(10, 4)
    put(11, 4)
    put(20, 3)
    put(21, 4)
    E = np.sort(rng.uniform(-5.0, 5.0, N))
    E[11] = E[10]  # a tie inside block 4
    E[21] = E[20]  # a tie across blocks 3 and 4
    assert np.all(np.diff(E) >= 0)
    C = np.zeros((N, N), order="F")
    for j in range(N):
        rows = np.nonzero(blockid == colblk[j])[0]
        C[rows, j] = rng.uniform(-1.0, 1.0, len(rows))
    if not sort:
        perm = rng.permutation(N)
        E, C = E[perm].copy(), np.asfortranarray(C[:, perm])
    occ = [[], [0.37], list(rng.uniform(0.0, 1.0, 64)), [1.0, 0.5, 0.0, 0.0, 0.25], list(rng.uniform(0.05, 1.0, 24))]
    occ[2][5] = 0.0
    occ[2][63] = 1.0
    return blockid, E, C, occ


def restate(blockid, E, C, occ):
    """the stage in NumPy: (Cocc, Eocc, Focc)"""
    colblk = blockid[np.argmax(np.abs(C), axis=0)]  # the first row of largest magnitude
    order = np.lexsort((np.arange(len(E)), E))  # ascending E, ties by column index
    nslots = sum(len(o) for o in occ)
    Cocc, Eocc, Focc = np.zeros((C.shape[0], nslots), order="F"), np.zeros(nslots), np.zeros(nslots)
    s = 0
    for b, fs in enumerate(occ):
        cols = [j for j in order if colblk[j] == b]
        for k, f in enumerate(fs):
            Cocc[:, s] = np.sqrt(np.float64(f)) * C[:, cols[k]]
            Eocc[s], Focc[s] = E[cols[k]], f
            s += 1
    return Cocc, Eocc, Focc


SIZES_LONG = (70, 513)
N_LONG = sum(SIZES_LONG)
# (lower row, higher row) of the doubled maxima; a row r is searched by thread r % 256, wave (r % 256) // 64
TIES = ((3, 259), (70, 101), (10, 200), (130, 540), (300, 577))


def problem_long():
    """blocks of 70 and 513 rows: as problem(), with five columns whose largest magnitude stands in two rows of different
    blocks, so that the block of the column hangs on which of the two rows the search keeps"""
    rng = np.random.RandomState(583)
    n = N_LONG
    blockid = np.repeat(np.arange(2), SIZES_LONG).astype(np.int32)
    rng.shuffle(blockid)
    for lo, hi in TIES:  # the two rows lie in different blocks: swap the higher row's id with a row outside all pairs
        if blockid[lo] == blockid[hi]:
            used = {r for pair in TIES for r in pair}
            other = [r for r in range(n) if r not in used and blockid[r] != blockid[hi]][0]
            blockid[other], blockid[hi] = blockid[hi], blockid[other]
    assert [int((blockid == b).sum()) for b in range(2)] == list(SIZES_LONG)
    colblk = np.repeat(np.arange(2), SIZES_LONG)
    rng.shuffle(colblk)
    E = np.sort(rng.uniform(-5.0, 5.0, n))
    C = np.zeros((n, n), order="F")
    for j in range(n):
        rows = np.nonzero(blockid == colblk[j])[0]
        C[rows, j] = rng.uniform(-1.0, 1.0, len(rows))
    tie_cols = []
    for q, (lo, hi) in enumerate(TIES):
        j = [c for c in range(n) if colblk[c] == blockid[lo]][q]  # among the lowest levels of the lower row's block
        C[lo, j], C[hi, j] = 1.5, -1.5  # above every other magnitude; the column now reaches into the other block
        tie_cols.append(j)
    occ = [list(rng.uniform(0.05, 1.0, 70)), list(rng.uniform(0.05, 1.0, 40))]
    return blockid, E, C, occ, tie_cols


@pytest.fixture(scope="module")
def stage_long(hf, torch):
    blockid, E, C, occ, _ = problem_long()
    ctx = hf.Context(0)
    dB, dE, dC = torch.from_numpy(blockid).cuda(), dev(torch, E), dev(torch, C)
    torch.cuda.synchronize()
    calls = []
    for _ in range(2):
        Cocc, Eocc, Focc = ctx.occupy_blocks(dE, dC, dB, occ)
        ctx.synchronize()
        calls.append((Cocc.cpu().numpy().reshape((N_LONG, -1), order="F"), Eocc.cpu().numpy(), Focc.cpu().numpy()))
    return dict(calls=calls, E=dE.cpu().numpy(), C=dC.cpu().numpy().reshape((N_LONG, N_LONG), order="F"))


def test_long_columns_equal_the_restatement_exactly(stage_long):
    blockid, E, C, occ, tie_cols = problem_long()
    assert N_LONG > 512 and N_LONG % 256 not in (0, 255)
    Cref, Eref, Fref = restate(blockid, E, C, occ)
    Cocc, Eocc, Focc = stage_long["calls"][0]
    assert Cocc.shape == Cref.shape == (N_LONG, 110)
    assert np.all(Eocc == Eref) and np.all(Focc == Fref)
    wrong = np.nonzero(~np.all(Cocc == Cref, axis=0))[0]
    assert len(wrong) == 0, "slots that differ: %r" % list(wrong)
    # the doubled maxima are there, in rows of different blocks and of the threads and waves meant, and every such column is
    # occupied: keeping the higher row would have moved it to the other block's slots
    where = [((lo % 256, (lo % 256) // 64), (hi % 256, (hi % 256) // 64)) for lo, hi in TIES]
    assert where[0][0][0] == where[0][1][0]                                   # one thread, 256 rows apart
    assert where[1][0][1] == where[1][1][1] and where[1][0][0] != where[1][1][0]  # two lanes of one wave
    assert where[2][0][1] != where[2][1][1] and where[3][0][1] != where[3][1][1]  # two waves
    assert TIES[4][1] >= 512 and TIES[3][1] >= 512                            # the higher row in the tail
    for (lo, hi), j in zip(TIES, tie_cols):
        assert blockid[lo] != blockid[hi] and abs(C[lo, j]) == abs(C[hi, j]) == np.abs(C[:, j]).max()
        s = [q for q in range(110) if Eocc[q] == E[j]]
        assert len(s) == 1 and np.array_equal(Cocc[:, s[0]], np.sqrt(Focc[s[0]]) * C[:, j])
        assert (s[0] < 70) == (blockid[lo] == 0)


def test_long_columns_second_call_is_bitwise_the_first_and_inputs_are_untouched(stage_long):
    first, second = stage_long["calls"]
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    _, E, C, _, _ = problem_long()
    assert np.array_equal(stage_long["E"], E) and np.array_equal(stage_long["C"], C)


def dev(torch, a):
    return torch.from_numpy(np.asfortranarray(a).ravel(order="F").copy()).cuda()


@pytest.fixture(scope="module")
def stage(hf, torch):
    """both variants through the device once: outputs of two calls each, and the inputs read back afterwards"""
    ctx = hf.Context(0)
    out = {}
    for sort in (True, False):
        blockid, E, C, occ = problem(sort)
        dB, dE, dC = torch.from_numpy(blockid).cuda(), dev(torch, E), dev(torch, C)
        torch.cuda.synchronize()
        calls = []
        for _ in range(2):
            Cocc, Eocc, Focc = ctx.occupy_blocks(dE, dC, dB, occ)
            ctx.synchronize()
            calls.append((Cocc.cpu().numpy().reshape((N, -1), order="F"), Eocc.cpu().numpy(), Focc.cpu().numpy()))
        out[sort] = dict(calls=calls, E=dE.cpu().numpy(), C=dC.cpu().numpy().reshape((N, N), order="F"), keep=(dB, dE, dC))
    out["ctx"] = ctx
    return out


@pytest.mark.parametrize("sort", [True, False], ids=["as-the-eigensolve-leaves-them", "columns-in-no-order"])
def test_stage_equals_the_restatement_exactly(stage, sort):
    blockid, E, C, occ = problem(sort)
    Cref, Eref, Fref = restate(blockid, E, C, occ)
    Cocc, Eocc, Focc = stage[sort]["calls"][0]
    assert Cocc.shape == Cref.shape == (N, 94)
    assert np.all(Eocc == Eref) and np.all(Focc == Fref)
    wrong = np.nonzero(~np.all(Cocc == Cref, axis=0))[0]
    assert len(wrong) == 0, "slots that differ: %r" % list(wrong)
    # the cases the inputs were built for are really there
    if sort:
        assert E[10] == E[11] and E[20] == E[21]
        s4 = 1 + 64 + 5
        inside = [s for s in range(s4, 94) if Eocc[s] == E[10]]
        assert len(inside) == 2 and inside[1] == inside[0] + 1 and Focc[inside[0]] != Focc[inside[1]]
        assert np.array_equal(Cocc[:, inside[0]], np.sqrt(Focc[inside[0]]) * C[:, 10])
        assert sum(1 for s in range(94) if Eocc[s] == E[20]) >= 1


def test_zero_occupations_give_zero_columns_and_keep_their_energy(stage):
    Cocc, Eocc, Focc = stage[True]["calls"][0]
    zeros = np.nonzero(Focc == 0.0)[0]
    assert len(zeros) == 3
    assert not Cocc[:, zeros].any() and np.all(Eocc[zeros] != 0.0)
    assert np.all(np.abs(Cocc[:, Focc > 0.0]).max(axis=0) > 0.0)


@pytest.mark.parametrize("sort", [True, False], ids=["sorted", "unsorted"])
def test_second_call_is_bitwise_the_first_and_inputs_are_untouched(stage, sort):
    first, second = stage[sort]["calls"]
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    _, E, C, _ = problem(sort)
    assert np.array_equal(stage[sort]["E"], E) and np.array_equal(stage[sort]["C"], C)


def test_queued_behind_a_write_of_C_on_the_same_stream(hf, torch):
    """the stream-order contract of the _devptr entries: a device copy into C, queued behind a few milliseconds of other work
    on the context's stream, and the stage directly behind it with no synchronisation in between.  The first call is the
    warm-up that reads the block ids back and stages the occupation lists; the second call has nothing left to wait for."""
    blockid, E, C, occ = problem(True)
    # other values in the same block pattern
    C2 = np.asfortranarray(np.where(C != 0.0, 1.0, 0.0) * np.random.RandomState(5).uniform(-1.0, 1.0, C.shape))
    want = restate(blockid, E, C2, occ)
    s = torch.cuda.Stream()
    ctx = hf.Context(0, stream=s.cuda_stream)
    with torch.cuda.stream(s):
        dB, dE, dC, dC2 = torch.from_numpy(blockid).cuda(), dev(torch, E), dev(torch, C), dev(torch, C2)
        busy = torch.rand(1024, 1024, dtype=torch.float64, device="cuda")
        out = ctx.occupy_blocks(dE, dC, dB, occ)
        torch.cuda.synchronize()
        for _ in range(8):
            busy = busy @ busy * 1e-3
        dC.copy_(dC2)
        out = ctx.occupy_blocks(dE, dC, dB, occ, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy().reshape((N, -1), order="F"), want[0])
    assert np.array_equal(out[1].cpu().numpy(), want[1]) and np.array_equal(out[2].cpu().numpy(), want[2])


def test_more_occupations_than_rows_is_refused(hf, torch, stage):
    blockid, _, _, occ = problem(True)
    dB, dE, dC = stage[True]["keep"]
    for b, n in ((0, 2), (1, 64)):
        too_many = [list(o) for o in occ]
        too_many[b] = [0.5] * n
        with pytest.raises(RuntimeError, match="block %d has %d rows and %d occupations" % (b, SIZES[b], n)):
            stage["ctx"].occupy_blocks(dE, dC, dB, too_many)


def test_row_counts_are_kept_per_block_id_array_until_forgotten(hf, torch):
    """a block-id tensor rewritten in place keeps its address: the counts of the old layout hold until forget_block_ids"""
    blockid, E, C, occ = problem(True)
    ctx = hf.Context(0)
    dB, dE, dC = torch.from_numpy(blockid).cuda(), dev(torch, E), dev(torch, C)
    ctx.occupy_blocks(dE, dC, dB, occ)
    swapped = blockid.copy()  # blocks 1 (63 rows) and 3 (65 rows) change names
    swapped[blockid == 1], swapped[blockid == 3] = 3, 1
    dB.copy_(torch.from_numpy(swapped))
    torch.cuda.synchronize()
    more = [list(o) for o in occ]
    more[1] = [0.5] * 65  # fits the new block 1 and not the old one
    with pytest.raises(RuntimeError, match="block 1 has 63 rows and 65 occupations"):
        ctx.occupy_blocks(dE, dC, dB, more)
    ctx.forget_block_ids()
    out = ctx.occupy_blocks(dE, dC, dB, more)
    ctx.synchronize()
    want = restate(swapped, E, C, more)
    assert np.array_equal(out[0].cpu().numpy().reshape((N, -1), order="F"), want[0])
    assert np.array_equal(out[1].cpu().numpy(), want[1]) and np.array_equal(out[2].cpu().numpy(), want[2])


# ---- the step ---------------------------------------------------------------------------------------------------------
BASIS = dict(lmax=1, mmax=1, nelem=5, nnodes=15)
LDFT, MDFT = 4 * BASIS["lmax"] + 10, 4 * BASIS["mmax"] + 5  # the atomic driver's defaults
SHELLS = {1: {0: [1]}, 5: {0: [2, 2], 1: [1]}, 6: {0: [2, 2], 1: [2]}, 7: {0: [2, 2], 1: [3]}, 8: {0: [2, 2], 1: [4]},
          10: {0: [2, 2], 1: [6]}}


def atom(hf, Z, exchange=False):
    lval, mval = hf.angular_basis(BASIS["lmax"], BASIS["mmax"])
    basis = hf.AtomicTwoDBasis(Z, BASIS["nnodes"], 5 * BASIS["nnodes"], hf.atomic_grid(BASIS["nelem"], Rmax=40.0, igrid=4, zexp=2.0),
                               lval, mval)
    basis.compute_tei(exchange)
    return basis


def prepared(hf, step, basis):
    S = basis.overlap()
    H0 = basis.kinetic() + basis.nuclear()
    X = hf.scf.form_Sinvh(S, False, step.blocks, ctx=step.ctx)
    step.set_matrices(H0, X)
    return S, H0, X


def frac_run(hf, Z, method, convthr, kfrac=0.0):
    basis = atom(hf, Z, exchange=kfrac != 0.0)
    x, c = (0, 0) if method == "HF" else hf.xc_func_ids(method)
    ldft, mdft = (0, 0) if method == "HF" else (LDFT, MDFT)
    occ = hf.spherical_occupations(basis, SHELLS[Z])
    step = hf.DeviceFracSCFStep(basis, x, c, ldft, mdft, occ, symmetry=2, kfrac=kfrac)
    S, H0, X = prepared(hf, step, basis)
    res = step.run(S, maxit=60, convthr=convthr)
    return dict(basis=basis, step=step, S=S, H0=H0, X=X, res=res, occ=occ, x=x, c=c, ldft=ldft, mdft=mdft)


def test_neon_with_whole_occupations_is_the_restricted_step(hf):
    convthr = 1e-8
    f = frac_run(hf, 10, "lda_x-lda_c_vwn", convthr)
    basis = atom(hf, 10)
    ref = hf.DeviceSCFStep(basis, f["x"], f["c"], LDFT, MDFT, 5, symmetry=2)
    S, _, _ = prepared(hf, ref, basis)
    r = ref.run(S, maxit=60, convthr=convthr)
    print("Ne: fractional step %d iterations Etot % .12f, restricted step %d iterations % .12f, difference %.2e" %
          (f["res"]["iterations"], f["res"]["Etot"], r["iterations"], r["Etot"], f["res"]["Etot"] - r["Etot"]))
    assert f["res"]["converged"] and r["converged"]
    assert abs(f["res"]["Etot"] - r["Etot"]) < 1e-8
    assert f["res"]["iterations"] == r["iterations"]
    E, occ = f["step"].occupied()
    assert np.all(occ == 1.0) and len(E) == 5 and np.all(np.isfinite(E))


def self_consistency(hf, run, convthr, nel):
    """the figures of checks 2 and 3 from an independent route: host-pointer Fock build, SciPy eigensolve"""
    import scipy.linalg
    basis, step, S, H0, X = run["basis"], run["step"], run["S"], run["H0"], run["X"]
    n = step.N
    P = step.numpy(step.P, (n, n)).copy()
    F = H0 + basis.coulomb(P)
    if run["ldft"]:
        F = F + hf.DFTGrid(basis, run["ldft"], run["mdft"]).eval_Fxc(run["x"], run["c"], P)[0]
    if step.anyK:
        F = F + step.kscale * basis.exchange(0.5 * P)
    comm = X.T @ (F @ P @ S - S @ P @ F) @ X
    Psci = np.zeros_like(P)
    for idx, fs in zip(step.blocks, run["occ"]):
        if not len(fs):
            continue
        ix = np.ix_(idx, idx)
        _, v = scipy.linalg.eigh(F[ix], S[ix])
        Cb = v[:, :len(fs)] * np.sqrt(np.asarray(fs))
        Psci[ix] = 2.0 * Cb @ Cb.T
    pblocks = [i for i, (l, m) in enumerate(zip(basis.lval, basis.mval)) if l == 1]
    assert len(pblocks) == 3

    def spread(M):
        d = [M[np.ix_(step.blocks[i], step.blocks[i])] for i in pblocks]
        return max(float(np.abs(d[0] - d[1]).max()), float(np.abs(d[0] - d[2]).max()), float(np.abs(d[1] - d[2]).max()))
    fig = dict(comm=float(np.abs(comm).max()), trace=float(np.trace(P @ S)), spread=spread(P), spread_scipy=spread(Psci),
               dP=float(np.abs(P - Psci).max()))
    print("Z = %d: %d iterations, Etot % .10f; max |X^T (F P S - S P F) X| = %.3e (total P; %.3e with P/2; bound %.1e); "
          "tr(P S) - %d = %.2e; p blocks differ by %.3e on the device, %.3e from SciPy's occupation of the same F; "
          "max |P - P_scipy| = %.3e" % (nel, run["res"]["iterations"], run["res"]["Etot"], fig["comm"], 0.5 * fig["comm"],
                                        2 * convthr, nel, fig["trace"] - nel, fig["spread"], fig["spread_scipy"], fig["dP"]))
    return fig


def test_carbon_lda_is_self_consistent_and_spherical(hf):
    convthr = 1e-7
    run = frac_run(hf, 6, "lda_x-lda_c_vwn", convthr)
    assert run["res"]["converged"]
    fig = self_consistency(hf, run, convthr, 6)
    assert fig["comm"] < 2 * convthr
    assert abs(fig["trace"] - 6.0) < 1e-10
    assert fig["spread"] <= 10.0 * fig["spread_scipy"]
    E, occ = run["step"].occupied()
    assert sorted(occ) == [2.0 / 6.0, 2.0 / 6.0, 2.0 / 6.0, 1.0, 1.0] and np.all(np.isfinite(E))


def test_boron_with_exact_exchange_is_self_consistent(hf):
    convthr = 1e-7
    run = frac_run(hf, 5, "HF", convthr, kfrac=1.0)
    assert run["res"]["converged"] and abs(run["res"]["Exx"]) > 1.0
    plan = run["basis"].exchange_last_plan()
    print("exchange plan of the last build:", plan)
    # the build took the scaled columns as the factors of P / 2: the low-rank route, one density of rank nslots = 5
    assert run["step"].have_C and run["step"].nocc == 5
    assert plan["single"] is not None and not plan["single"]["declined"] and plan["single"]["ranks"] == [5]
    fig = self_consistency(hf, run, convthr, 5)
    assert fig["comm"] < 2 * convthr
    assert abs(fig["trace"] - 5.0) < 1e-10
    assert fig["spread"] <= 10.0 * fig["spread_scipy"]


@pytest.mark.parametrize("Z,nist", [(1, -0.445671), (6, -37.425749), (7, -54.025016), (8, -74.473077)], ids=["H", "C", "N", "O"])
def test_nist_lda_total_energies(hf, Z, nist):
    """NIST Atomic Reference Data for Electronic Structure Calculations, LDA (VWN) total energies: spherical atoms with
    fractional occupations, the table the He, Ne and Rn pins come from"""
    run = frac_run(hf, Z, "lda_x-lda_c_vwn", 1e-7)
    print("Z = %d: Etot % .8f after %d iterations, NIST % .6f, difference %.2e" %
          (Z, run["res"]["Etot"], run["res"]["iterations"], nist, run["res"]["Etot"] - nist))
    assert run["res"]["converged"]
    assert abs(run["res"]["Etot"] - nist) < 2e-6
