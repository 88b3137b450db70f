"""K for a batch of densities in one pass over the exchange-ordered tables per chunk: hfg_exchange_batch,
hfg_rs_exchange_batch, their device-pointer forms and hfg_exchange_occ_batch_devptr (hip/exchange_lr.hip, DESIGN 3.3
"Batched K").

Bases, the smallest the parity suites use: the diatomic sigma + pi basis "sigma_pi" of tests/test_gpu_parity.py (N2, lmmax
(3, 2), 2 elements of 5 nodes) and the atomic basis "sp" of tests/test_gpu_rs.py (Z = 10, lmax = mmax = 1, 3 elements of 5
nodes).

Bounds.  Against the oracle: 1e-12 max|K_b|, the bound of test_exchange_parity (tests/test_gpu_parity.py:105), of
test_atomic_exchange_parity (:589) and of test_rs_exchange_parity (tests/test_gpu_rs.py:63) on these bases.  Against the
single build: bitwise -- every stage of the batched build sums in the single build's order with the single build's tiles.
Shards: 1e-12 max|K_b|, the bound of test_exchange_shards_sum_to_full (tests/test_gpu_parity.py:216).  The step with
HELFEM_USCF_KBATCH=1 against the step without: bitwise, what test_two_whole_steps (tests/test_gpu_fock_pol.py:538) asks of
the step's two build paths."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exchange_batch_worker as wk  # noqa: E402

ATOMIC_SP = (10, 1, 1, 3, 5)  # "sp" of tests/test_gpu_rs.py
V = ctypes.c_void_p


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    if helfem_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the hot path has no CPU fallback")
    return helfem_amd


class Dia(object):
    """the sigma + pi basis, the batch of ranks (2, 5, 1) and its single builds, computed once and left unchanged"""

    def __init__(self):
        self.gb, self.ob = common.make_bases(*wk.SIGMA_PI)
        self.gb.compute_tei(True)
        self.gb.upload()
        self.N = self.gb.Nbf()
        self.P = np.array(wk.batch(self.N, wk.RANKS_1, 100))
        self.K1 = np.array([self.gb.exchange(P) for P in self.P])
        self.Kb = self.gb.exchange_batch(self.P)
        for a in (self.P, self.K1, self.Kb):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def dia(hf):
    return Dia()


def singles(gb, Ps, rs=False):
    return np.array([(gb.rs_exchange if rs else gb.exchange)(np.asfortranarray(P)) for P in Ps])


def report(what, got, ref):
    err = max(common.relerr(g, r) for g, r in zip(got, ref))
    print("%s: %.3e" % (what, err))
    return err


def test_diatomic_batch_against_the_oracle_and_the_single_build(dia):
    d = dia
    assert [np.linalg.matrix_rank(P) for P in d.P] == list(wk.RANKS_1)
    assert all(np.any(np.linalg.eigvalsh(P) < -0.1) for P in d.P[:2])  # S has both signs
    d.ob.compute_tei(True)
    Ko = [d.ob.exchange(np.asfortranarray(P)) for P in d.P]
    assert report("batch of ranks (2, 5, 1) against the oracle", d.Kb, Ko) < 1e-12
    print("against hfg_exchange: max difference %.3e" % max(np.max(np.abs(a - b)) for a, b in zip(d.Kb, d.K1)))
    assert np.array_equal(d.Kb, d.K1)
    assert np.array_equal(d.gb.exchange_batch(d.P), d.Kb)  # repeats bitwise
    assert np.array_equal(d.gb.exchange_batch(d.P[:1]), d.K1[:1])  # nP = 1: the single build


def test_one_pass_over_the_tables_per_chunk(dia):
    """the profile counts the element GEMM's launches: one for the batch of ranks (2, 5, 1), none of the single build's;
    (30, 30, 10) is one shared pass and one single build; a zero matrix takes part in neither"""
    d = dia
    ctx = d.gb.ctx

    def launches(Ps):
        ctx.profile(True)
        ctx.profile_reset()
        try:
            d.gb.exchange_batch(Ps)
            ctx.synchronize()
            names = ctx.profile_names()
            return tuple(ctx.profile_get(n)[1] if n in names else 0 for n in ("exl_batch_element_gemm", "exl_element_gemm"))
        finally:
            ctx.profile(False)
    assert launches(d.P) == (1, 0)
    assert launches(wk.batch(d.N, wk.RANKS_SPLIT, 200)) == (1, 1)
    assert launches([d.P[0], np.zeros((d.N, d.N)), d.P[2]]) == (1, 0)  # the zero matrix does not end the run
    assert launches([d.P[0], np.zeros((d.N, d.N))]) == (0, 1)  # a chunk of one: the single build


@pytest.mark.parametrize("kind", ["coulomb", "yukawa", "erfc"])
def test_atomic_batch(hf, kind):
    gb, ob = common.make_atomic_bases(*ATOMIC_SP)
    gb.compute_tei(True)
    ob.compute_tei(True)
    rs = kind != "coulomb"
    if rs:
        getattr(gb, "compute_" + kind)(0.4)
        getattr(ob, "compute_" + kind)(0.4)
    Ps = wk.batch(gb.Nbf(), wk.RANKS_1, 400)
    K = gb.rs_exchange_batch(Ps) if rs else gb.exchange_batch(Ps)
    Ko = [(ob.rs_exchange if rs else ob.exchange)(P) for P in Ps]
    assert report("atomic %s batch against the oracle" % kind, K, Ko) < 1e-12
    assert np.array_equal(K, singles(gb, Ps, rs))


def _child(mode, path, env=None, limit=240):
    e = dict(os.environ)
    for k in ("HELFEM_EXCHANGE_BATCH_CHUNK", "HELFEM_USCF_KBATCH"):
        e.pop(k, None)
    e.update(env or {})
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "exchange_batch_worker.py"), mode, path], cwd=ROOT, env=e, timeout=limit,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    # a child that ends with a signal (negative return code) or an error ends the test here: nothing else is started
    assert out.returncode == 0 and "ok" in out.stdout.decode().split(), (out.returncode, out.stdout.decode()[-3000:])


def test_chunked_batches_equal_the_unchunked_ones(dia, tmp_path):
    d = dia
    Ps = wk.batch(d.N, wk.RANKS_SPLIT, 200)
    K2 = d.gb.exchange_batch(Ps)  # 70 factors: two chunks, (30, 30) and (10): the last one through the single build
    assert np.array_equal(K2, singles(d.gb, Ps))
    for chunk in ("1", "2"):
        path = str(tmp_path / ("chunk%s.npz" % chunk))
        _child("chunk", path, {"HELFEM_EXCHANGE_BATCH_CHUNK": chunk})
        r = np.load(path)
        assert r["chunk"][0] == chunk
        assert np.array_equal(r["K1"], d.Kb) and np.array_equal(r["K2"], K2), chunk


def test_members_that_leave_the_fast_path(hf):
    """a low-rank density, the zero matrix, a full-rank symmetric matrix (the general kernels), a density of 70 factors (the
    construction of test_exchange_of_a_density_with_more_than_64_factors: the single build's residual groups) and two
    more low-rank ones that stay batched behind them.  The basis is the small N2 basis of tests/test_gpu_fock_pol.py: with
    HELFEM_EXL_GROUPS = 4 groups of 64 factors, only a matrix of more than 256 functions reaches the general kernels."""
    gb, _ = common.make_bases(7, 7, 2.068, (6, 6), 3, 8, oracle=False)
    gb.compute_tei(True)
    gb.upload()
    N = gb.Nbf()
    assert N > 4 * 64
    rng = np.random.RandomState(5)
    full = rng.uniform(-1, 1, size=(N, N))
    P70 = common.random_density(N, 70, seed=41) - 0.5 * common.random_density(N, 5, seed=48)
    lo = wk.batch(N, wk.RANKS_1, 500)
    Ps = [lo[0], np.zeros((N, N)), full + full.T, P70, lo[1], lo[2]]
    K = gb.exchange_batch(Ps)
    K1 = singles(gb, Ps)
    assert np.all(K[1] == 0.0) and all(np.any(K[b] != 0.0) for b in (0, 2, 3, 4, 5))
    for b in range(len(Ps)):
        assert np.array_equal(K[b], K1[b]), b


def test_known_factors(dia, hf):
    import torch
    d = dia
    L, N, ctx = hf.lib(), d.N, d.gb.ctx
    C = np.random.RandomState(8).uniform(-1, 1, (2, N, N))
    occ = hf.lib().hfg_exchange_occ_dev
    occ.argtypes = [V, V, V, V, ctypes.c_int64, V]
    for nocc in ((5, 3), (4, 0)):
        Ps = [c[:, :n] @ c[:, :n].T for c, n in zip(C, nocc)]
        dP, dC = torch.from_numpy(wk.flat(Ps)).cuda(), torch.from_numpy(wk.flat(C)).cuda()
        dK, dK1 = torch.full((2 * N * N,), -7.0, dtype=torch.float64, device="cuda"), torch.zeros(2 * N * N, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        n64 = np.array(nocc, dtype=np.int64)
        assert L.hfg_exchange_occ_batch_devptr(ctx.h, d.gb.h, 2, V(dP.data_ptr()), V(dC.data_ptr()), n64.ctypes.data_as(hf.c_i64_p), N,
                                               V(dK.data_ptr())) == 0, L.hfg_last_error()
        for b, n in enumerate(nocc):
            if n:
                off = b * N * N * 8
                assert occ(ctx.h, d.gb.h, V(dP.data_ptr() + off), V(dC.data_ptr() + off), n, V(dK1.data_ptr() + off)) == 0
        ctx.synchronize()
        assert np.array_equal(dK.cpu().numpy(), dK1.cpu().numpy()), nocc
    assert np.all(dK.cpu().numpy()[N * N:] == 0.0) and np.any(dK.cpu().numpy()[:N * N] != 0.0)  # nelb = 0: a zero Kb


def test_devptr_entries_keep_the_stream_order(hf, tmp_path):
    """the protocol of tests/stream_order_worker.py on a non-default torch stream: inputs written by copies enqueued just
    before the call and overwritten right after it, output read by a copy enqueued just after, no host synchronisation"""
    import stream_order_worker as sow
    path = str(tmp_path / "stream.json")
    _child("stream", path)
    recs = json.load(open(path))
    assert [r["entry"] for r in recs] == ["hfg_exchange_batch_devptr", "hfg_exchange_occ_batch_devptr"]
    for rec in recs:
        print(rec)
        assert rec["decoy_differs"] and rec["repeat"]["ok"] and rec["twin"]["ok"]
        assert rec["baselines_bitwise"], "results repeat bitwise from call to call"
        assert rec["delay_ms"] >= sow.DELAY_MIN_MS, "the delay is too short for the run to mean anything"
        assert not rec["ordered_is_decoy"], "the call read its inputs before the copy enqueued ahead of it"
        assert rec["ordered"]["ok"] and rec["ordered"]["bitwise"]


def test_shards_sum_to_the_unsharded_batch(dia):
    import torch
    d = dia
    ctx = d.gb.ctx
    dP = torch.from_numpy(wk.flat(d.P)).cuda()
    torch.cuda.synchronize()

    def run():
        out = d.gb.exchange_batch_torch(dP)
        ctx.synchronize()
        return out.cpu().numpy().reshape(len(d.P), d.N, d.N).transpose(0, 2, 1)
    whole = run()
    assert np.array_equal(whole, d.Kb)
    acc = np.zeros_like(whole)
    try:
        for rk in range(2):
            ctx.set_shard(rk, 2)
            part = run()
            assert all(common.relerr(p, w) > 1e-3 for p, w in zip(part, whole))  # a shard is not the whole
            acc += part
            assert np.array_equal(d.gb.exchange_batch(d.P), d.Kb)  # host-pointer entry: complete whatever the shard
    finally:
        ctx.set_shard(0, 1)
    assert report("shards (0,2) + (1,2)", acc, whole) < 1e-12


def test_opt_in_step_equals_the_step_without(hf, tmp_path):
    res = {}
    for tag, env in (("off", {}), ("on", {"HELFEM_USCF_KBATCH": "1"})):
        path = str(tmp_path / ("step_%s.npz" % tag))
        _child("step", path, env)
        res[tag] = np.load(path)
    for how in "CP":
        assert not res["off"]["kbatch" + how][0] and res["on"]["kbatch" + how][0]
        for name in ("Ka", "Kb", "Fa", "Fb", "Ea", "Eb"):
            a, b = res["off"][name + how], res["on"][name + how]
            print("%s%s: max difference %.3e" % (name, how, np.max(np.abs(a - b))))
            assert np.array_equal(a, b), (name, how)
        assert np.any(res["on"]["Ka" + how] != 0.0) and np.any(res["on"]["Ka" + how] != res["on"]["Kb" + how])


def test_refusals(dia, hf):
    d = dia
    L = hf.lib()
    buf = np.zeros(d.N * d.N)
    p = buf.ctypes.data_as(hf.c_double_p)
    assert L.hfg_exchange_batch(d.gb.ctx.h, d.gb.h, 0, None, None) == 0  # nothing to do
    assert L.hfg_exchange_batch(d.gb.ctx.h, d.gb.h, -1, p, p) == 1 and b"negative" in L.hfg_last_error()
    assert L.hfg_exchange_batch(d.gb.ctx.h, d.gb.h, 1, None, p) == 1 and b"null" in L.hfg_last_error()
    assert L.hfg_rs_exchange_batch(d.gb.ctx.h, d.gb.h, 1, p, p) == 1 and b"Primitive teis have not been computed" in L.hfg_last_error()
    assert L.hfg_exchange_batch_devptr(d.gb.ctx.h, d.gb.h, 2, None, None) == 1 and b"null" in L.hfg_last_error()
    with pytest.raises(ValueError):
        d.gb.exchange_batch([np.zeros((d.N + 1, d.N + 1))])
