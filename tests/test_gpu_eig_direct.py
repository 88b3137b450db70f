"""The one-call blocked eigensolve without block slots (HELFEM_EIG_DIRECT, the default): eigenvalues ranked as soon as they are
final, the last product stored straight into C through the row and column maps of the GEMM task, X = Sinvh(rows, cols) gathered
once while hfg_ctx_fix_sinvh holds.

1, 2. hfg_eig_gsym_sub_dev and hfg_eig_gsym_sub_sel_dev (nev = 1, 3, 200) with the switch on against the switch off (the two
   phases through block slots): E and the WHOLE of C, zeros outside the blocks included, equal with maximum difference 0 --
   the same tiles and k order form every stored value -- on outputs pre-filled with NaN; and against numpy.linalg.eigh per
   block at the bounds of test_gpu_eigsel.py (1e-10 on E, scaled, and on C^T S C - I; 1e-9 on the scaled residual).  One worker
   process per kernel the last product can be (tests/eig_direct_worker.py): the GEMM switches are read once per process.
3. The X cache: a declared Sinvh overwritten in place and declared again, an undeclared one overwritten in place, other block
   lists under the same declaration -- the result follows the matrix and the lists of the call (bound on E as above).
4. DeviceSCFStep at bench.py's n2_pbe_small: two steps from the core guess with the switch on and off, E, C, P, F and scal
   equal with maximum difference 0.
5. Stream order (the protocol of test_gpu_stream_order.py): the entry queued on a non-default stream behind a delayed producer
   of F, decoys over inputs and outputs afterwards, no host synchronisation in between, gives what it gives after one."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import eig_direct_worker as wk  # noqa: E402

FAULT_LIKE = (134, 139, -6, -11)
WORKER_TIMEOUT_S = 300
# the kernel of the last product: 64 x 64 tiles (these sizes' default), 128 x 128 tiles in two half-K workgroups that add into
# the zeroed C, 128 x 128 and 128 x 64 tiles
SETTINGS = (("default", {}), ("splitk", {"HELFEM_GEMM_SPLITK": "1"}), ("tile128", {"HELFEM_GEMM_SPLITK": "0", "HELFEM_GEMM_TILE": "128"}),
            ("rect", {"HELFEM_GEMM_SPLITK": "0", "HELFEM_GEMM_RECT": "1"}))
PLAN = [(s, c[0], nev) for s, _ in SETTINGS for c in wk.CASES for nev in (None,) + wk.NEVS]


@pytest.fixture(scope="module")
def runs(native_libs, tmp_path_factory):
    """one GPU process per setting, one after the other; after a fault-like end nothing more is started"""
    d = tmp_path_factory.mktemp("eig_direct")
    res, stopped = {}, None
    for setting, env in SETTINGS:
        if stopped:
            res[setting] = dict(error="not run: %s" % stopped)
            continue
        e = {k: v for k, v in os.environ.items() if k not in wk.GEMM_SWITCHES and k != wk.SWITCH}
        e.update(env)
        path = str(d / (setting + ".json"))
        try:
            out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "eig_direct_worker.py"), path], env=e, cwd=ROOT,
                                 timeout=WORKER_TIMEOUT_S, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        except subprocess.TimeoutExpired as x:
            stopped = "the worker of '%s' ran into its time limit" % setting
            res[setting] = dict(error=stopped + "\n" + (x.stdout or b"").decode(errors="replace")[-3000:])
            continue
        text = out.stdout.decode(errors="replace")[-3000:]
        if out.returncode in FAULT_LIKE:
            stopped = "the worker of '%s' ended with status %d" % (setting, out.returncode)
        if out.returncode != 0 or "ok" not in text.split():
            res[setting] = dict(error="status %d\n%s" % (out.returncode, text))
            continue
        res[setting] = json.load(open(path))
    return res


@pytest.mark.parametrize("setting,case,nev", PLAN, ids=["%s-%s-%s" % (s, c, "all" if n is None else "nev%d" % n) for s, c, n in PLAN])
def test_direct_equals_the_slot_path_and_eigh(runs, setting, case, nev):
    r = runs[setting]
    if "error" in r:
        pytest.fail("worker of '%s': %s" % (setting, r["error"]))
    rec = [x for x in r["records"] if x["case"] == case and x["nev"] == nev]
    assert len(rec) == 1
    rec = rec[0]
    print(setting, r["tuning"], rec)
    assert rec["dE"] == 0.0 and rec["dC"] == 0.0  # bit for bit the checker's, every word written
    assert rec["outside"] == 0.0 and rec["ascending"]
    assert rec["E"] < 1e-10 and rec["orth"] < 1e-10 and rec["resid"] < 1e-9


@pytest.fixture(scope="module")
def gpu(native_libs):
    import torch
    import helfem_amd as hf
    return hf, torch, torch.device("cuda", 0)


def _close(E, Eref):
    return wk.maxdiff(E, Eref) / max(1.0, float(np.max(np.abs(Eref)))) < 1e-10


def test_x_cache_follows_declaration_matrix_and_blocks(gpu):
    hf, torch, dev = gpu
    ctx = hf.default_context()
    sizes = [5, 70, 64]
    F1, S1, X1, b1 = wk.problem(sizes, 21)
    _, S2, X2, _ = wk.problem(sizes, 21)  # same index lists ...
    r = np.random.RandomState(22)
    for b in b1:  # ... another overlap on them
        B = r.uniform(-1, 1, (len(b), len(b)))
        S2[np.ix_(b, b)] = B @ B.T + len(b) * np.eye(len(b))
        w, V = np.linalg.eigh(S2[np.ix_(b, b)])
        X2[np.ix_(b, b)] = (V / np.sqrt(w)) @ V.T
    N = F1.shape[0]
    E_x1, E_x2 = wk.reference(F1, X1, b1), wk.reference(F1, X2, b1)
    assert not _close(E_x1, E_x2)  # the two matrices can be told apart
    # other lists under the same matrix: the first two blocks joined, F coupling them
    b2 = [np.sort(np.concatenate(b1[:2])), b1[2]]
    F2 = F1.copy()
    A = r.uniform(-1, 1, (len(b1[0]), len(b1[1])))
    F2[np.ix_(b1[0], b1[1])], F2[np.ix_(b1[1], b1[0])] = A, A.T
    E_b2 = wk.reference(F2, X1, b2)
    assert not _close(E_b2, E_x1)
    Fd, F2d, Xd = wk.up(torch, F1, dev), wk.up(torch, F2, dev), wk.up(torch, X1, dev)

    def solve(Fdev, blocks):
        return wk.solve(hf, torch, ctx, Fdev, Xd, N, blocks)

    try:
        # declared pointer: gathered at the first call, reused at the second
        ctx.fix_sinvh(Xd.data_ptr())
        E, C = solve(Fd, b1)
        Eh, Ch = solve(Fd, b1)
        assert _close(E, E_x1) and np.array_equal(E, Eh) and np.array_equal(C, Ch)
        assert wk.maxdiff(C.T @ S1 @ C, np.eye(N)) < 1e-10
        # changed block lists under the same declaration, and back
        E, C = solve(F2d, b2)
        assert _close(E, E_b2)
        assert wk.maxdiff(C.T @ S1 @ C, np.eye(N)) < 1e-10
        E, _ = solve(Fd, b1)
        assert np.array_equal(E, Eh)
        # overwritten in place, withdrawn and declared again: the result follows the new matrix
        Xd.copy_(wk.up(torch, X2, dev))
        ctx.fix_sinvh(None)
        ctx.fix_sinvh(Xd.data_ptr())
        E, C = solve(Fd, b1)
        assert _close(E, E_x2)
        assert wk.maxdiff(C.T @ S2 @ C, np.eye(N)) < 1e-10
        # undeclared pointer overwritten in place: nothing is cached
        ctx.fix_sinvh(None)
        E, _ = solve(Fd, b1)
        assert _close(E, E_x2)
        Xd.copy_(wk.up(torch, X1, dev))
        E, C = solve(Fd, b1)
        assert _close(E, E_x1)
        assert wk.maxdiff(C.T @ S1 @ C, np.eye(N)) < 1e-10
    finally:
        ctx.fix_sinvh(None)


def test_scf_step_is_the_same_with_the_switch_on_and_off(gpu):
    hf, torch, dev = gpu
    import bench
    w = bench.WORKLOADS["n2_pbe_small"]
    basis, bval, lval, mval, ldft, mdft = bench.build_basis(hf, w)
    basis.compute_tei(False)
    step = hf.DeviceSCFStep(basis, w["x"], w["c"], ldft, mdft, w["nocc"], symmetry=1, device=0)
    S = basis.overlap()
    H0 = basis.kinetic() + basis.nuclear()
    Sinvh = hf.scf.form_Sinvh(S, False, step.blocks, ctx=step.ctx)
    step.set_matrices(H0, Sinvh)
    E0, C0 = hf.scf.eig_gsym_sub(H0, Sinvh, step.blocks, ctx=step.ctx)
    P0 = 2.0 * hf.scf.form_density(C0, w["nocc"], ctx=step.ctx)

    def two_steps(direct):
        os.environ[wk.SWITCH] = "1" if direct else "0"
        try:
            step.set_density(P0, C0)
            for t in (step.E, step.C, step.F):
                t.fill_(float("nan"))
            for _ in range(2):
                step.step()
                step.P.mul_(2.0)  # closed shell: P = Pa + Pb
            torch.cuda.synchronize()
        finally:
            os.environ.pop(wk.SWITCH, None)
        return {k: getattr(step, k).cpu().numpy().copy() for k in ("E", "C", "P", "F", "scal")}

    on, off = two_steps(True), two_steps(False)
    for k in on:
        d = wk.maxdiff(on[k], off[k])
        print(k, d)
        assert d == 0.0, k
    assert np.all(np.diff(on["E"]) >= 0)


def test_entry_keeps_the_stream_order(gpu):
    hf, torch, dev = gpu
    sizes = [65, 1, 129]
    F, S, X, blocks = wk.problem(sizes, 31)
    Fdecoy = wk.problem(sizes, 32)[0]
    Fdecoy_on_blocks = np.zeros_like(F)
    for b in blocks:  # a valid input of the same kind: another F on the same blocks
        n = len(b)
        Fdecoy_on_blocks[np.ix_(b, b)] = Fdecoy[:n, :n] + Fdecoy[:n, :n].T
    N = F.shape[0]
    stream = torch.cuda.Stream(device=dev)
    ctx = hf.Context(0, stream=stream.cuda_stream)
    ptr, idx = hf.scf._blocks(blocks)
    import ctypes
    with torch.cuda.stream(stream):
        Ftrue, Fdec, Xd = wk.up(torch, F, dev), wk.up(torch, Fdecoy_on_blocks, dev), wk.up(torch, X, dev)
        Fin = torch.empty_like(Ftrue)
        Ed, Cd = torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N * N, dtype=torch.float64, device=dev)

        def call():
            rc = hf.lib().hfg_eig_gsym_sub_dev(ctx.h, ctypes.c_int64(N), ctypes.c_void_p(Fin.data_ptr()), ctypes.c_void_p(Xd.data_ptr()),
                                               len(blocks), ptr.ctypes.data_as(wk.I64P), idx.ctypes.data_as(wk.I64P),
                                               ctypes.c_void_p(Ed.data_ptr()), ctypes.c_void_p(Cd.data_ptr()))
            assert rc == 0, hf.lib().hfg_last_error(ctx.h)

        def baseline(src):
            Fin.copy_(src)
            Ed.fill_(-7.0)
            Cd.fill_(-7.0)
            torch.cuda.synchronize()
            call()
            torch.cuda.synchronize()
            return Ed.cpu().numpy().copy(), Cd.cpu().numpy().copy()

        Eb, Cb = baseline(Ftrue)
        Eb2, Cb2 = baseline(Ftrue)
        assert np.array_equal(Eb, Eb2) and np.array_equal(Cb, Cb2)  # the entry repeats bitwise: so must the ordered run
        Edec, _ = baseline(Fdec)
        assert not np.array_equal(Edec, Eb)
        # ordered run: decoy in place, a delay, the true F copied in behind it, the call, the outputs copied out, decoys again
        sleep = getattr(torch.cuda, "_sleep", None)
        Fin.copy_(Fdec)
        Eres, Cres = torch.empty_like(Ed), torch.empty_like(Cd)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if sleep:
            sleep(40000000)
        else:
            a = torch.rand(2048, 2048, dtype=torch.float64, device=dev)
            for _ in range(8):
                a = (a @ a) * 1e-3
        e1.record()
        Fin.copy_(Ftrue)
        call()
        Eres.copy_(Ed)
        Cres.copy_(Cd)
        Fin.copy_(Fdec)
        Ed.fill_(-7.0)
        Cd.fill_(-7.0)
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        print("delay %.1f ms" % ms)
        assert ms >= 5.0, "the delay is too short for the run to mean anything"
        assert np.array_equal(Eres.cpu().numpy(), Eb) and np.array_equal(Cres.cpu().numpy(), Cb)
    del ctx
