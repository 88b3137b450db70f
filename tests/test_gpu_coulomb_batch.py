"""J for a batch of densities in one pass over the in-element tables: hfg_coulomb_batch, hfg_coulomb_batch_devptr and
hfg_coulomb_energy_matrix (hip/fock.hip, DESIGN 3.1 "Batched J").

Shapes, the smallest at which each mechanism can still go wrong:
  diatomic lmmax (2, 1), 3 elements of 6 nodes     the base shape: +-M partner channels, p^2 = 36 (2.25 row tiles of 16)
  diatomic lmmax (2, 1), 17 elements of 4 nodes    4 E = 68 > 64 threads of the radial stage (strided scalars, per density)
  atomic lmax 2, mmax 1, 4 elements of 6 nodes     the atomic layout: one table type, tables by L only
Batch sizes 1 (the single build's kernels), 3 (register-blocked kernel), 8 (n = 16 columns: one matrix-core tile exactly),
17 (two tiles and a remainder inside a tile).  The LDS rule gives passes of 32 densities at these orders, so the chunked
path is forced through HELFEM_COULOMB_BATCH_CHUNK (a live switch): 8 with nP = 9 and 17 (8 + 1, 8 + 8 + 1: the matrix-core
kernel and the single-density remainder), 3 with nP = 4 and 5 (3 + 1, 3 + 2).

Bounds.  J_b against hfg_coulomb(P_b) and against the oracle: 1e-12 max|J_b|, the bound J is held to everywhere
(test_gpu_parity.py).  Linearity: both sides carry that error, the right-hand side once per term, so
1e-12 (max|J[Q_a]| + sum_b |A_ab| max|J[P_b]|).  W_ab against trace(P_a J_b) on the host with the batch's own J_b: an entry
of J_b is good to 1e-12 max|J_b| and meets every entry of P_a once, so 1e-12 max|J_b| sum|P_a|.  |W - W^T| <= 1e-11 max|W|.
Repeated calls: bitwise.  Shards (0,2) + (1,2) against the whole: 1e-13 max|J_b|.

Known answer: (1s1s|1s1s) = 5 Z / 8 for the hydrogenic 1s orbital.  Basis lmax = 0, 5 elements of 10 nodes, Rmax = 40: the
oracle's J with the lowest eigenvector of T + V (S-normalised) gives W - 5Z/8 = +5.29e-9 at Z = 1 and -3.52e-9 at Z = 2 on
the CPU (the basis-set error of the orbital); the bound is ten times that, 5.29e-8 and 3.52e-8, both below 1e-6."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coulomb_batch_worker as wk  # noqa: E402

SHAPES = [("diatomic", (2, 1), 3, 6), ("diatomic", (2, 1), 17, 4), ("atomic", (2, 1), 4, 6)]
BATCHES = [1, 3, 8, 17]
NMAX = max(BATCHES)
KNOWN = {1: 5.29e-9, 2: 3.52e-9}  # the oracle's own distance from 5 Z / 8 in the basis of the known-answer test


def _id(s):
    return "%s-ang%s-E%d-p%d" % (s[0], "_".join(str(a) for a in s[1]), s[2], s[3])


@pytest.fixture(scope="module")
def hf(native_libs):
    import helfem_amd
    if helfem_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the hot path has no CPU fallback")
    return helfem_amd


class Shape(object):
    """product and oracle basis of one shape; NMAX random symmetric densities and NMAX rank-one ones; hfg_coulomb of each,
    computed once and left unchanged"""

    def __init__(self, prog, ang, E, p):
        self.key = (prog, ang, E, p)
        if prog == "diatomic":
            self.gb, self.ob = common.make_bases(1, 1, 1.4, ang, E, p)
        else:
            self.gb, self.ob = common.make_atomic_bases(2, ang[0], ang[1], E, p)
        self.gb.compute_tei(False)
        self.gb.upload()
        N = self.gb.Nbf()
        self.P = wk.symmetric_batch(N, NMAX, 5)
        rng = np.random.RandomState(6)
        self.R = np.array([np.outer(c, c) for c in rng.uniform(-1, 1, (NMAX, N))])
        self.J = np.array([self.gb.coulomb(P) for P in self.P])
        self.JR = np.array([self.gb.coulomb(P) for P in self.R])
        for a in (self.P, self.R, self.J, self.JR):
            a.setflags(write=False)
        self._oracle = None

    def oracle(self):
        if self._oracle is None:
            self.ob.compute_tei(False)
            self._oracle = np.array([self.ob.coulomb(np.asfortranarray(P)) for P in self.P])
            self._oracle.setflags(write=False)
        return self._oracle


@pytest.fixture(scope="module", params=SHAPES, ids=[_id(s) for s in SHAPES])
def shape(request, hf):
    return Shape(*request.param)


def _worst(s, what, got, ref):
    """largest |got_b - ref_b| / max|ref_b| over the batch, printed"""
    err = max(float(np.max(np.abs(g - r)) / np.max(np.abs(r))) for g, r in zip(got, ref))
    print("%s %s: %.3e" % (_id(s.key), what, err))
    return err


@pytest.mark.parametrize("nP", BATCHES)
def test_batch_equals_single_calls(shape, nP):
    s = shape
    J = s.gb.coulomb_batch(s.P[:nP])
    assert J.shape == (nP,) + s.P[0].shape
    assert _worst(s, "random symmetric nP=%d" % nP, J, s.J[:nP]) < 1e-12


@pytest.mark.parametrize("nP", [3, 17])
def test_rank_one_batch(shape, nP):
    s = shape
    assert _worst(s, "rank one nP=%d" % nP, s.gb.coulomb_batch(s.R[:nP]), s.JR[:nP]) < 1e-12


def test_batch_against_the_oracle(shape):
    s = shape
    assert _worst(s, "nP=%d against the oracle" % NMAX, s.gb.coulomb_batch(s.P), s.oracle()) < 1e-12


@pytest.mark.parametrize("chunk,nP", [(8, 9), (8, 17), (3, 4), (3, 5)])
def test_chunked_batches(shape, hf, monkeypatch, chunk, nP):
    s = shape
    monkeypatch.setenv("HELFEM_COULOMB_BATCH_CHUNK", str(chunk))
    assert {r["name"]: r["value"] for r in hf.tuning_table()}["HELFEM_COULOMB_BATCH_CHUNK"] == str(chunk)
    J = s.gb.coulomb_batch(s.P[:nP])
    assert _worst(s, "chunk %d nP=%d" % (chunk, nP), J, s.J[:nP]) < 1e-12
    W = s.gb.coulomb_energy_matrix(s.P[:nP])
    monkeypatch.delenv("HELFEM_COULOMB_BATCH_CHUNK")
    W1 = s.gb.coulomb_energy_matrix(s.P[:nP])
    bound = 1e-12 * np.array([[np.max(np.abs(s.J[b])) * np.sum(np.abs(s.P[a])) for b in range(nP)] for a in range(nP)])
    assert np.all(np.abs(W - W1) <= 2 * bound)  # each within the bound of test_energy_matrix of the exact traces


def test_linearity(shape):
    s = shape
    nP = 8
    A = np.random.RandomState(9).uniform(-1, 1, (nP, nP))
    Q = np.einsum("ab,bij->aij", A, s.P[:nP])
    JQ = s.gb.coulomb_batch(Q)
    want = np.einsum("ab,bij->aij", A, s.gb.coulomb_batch(s.P[:nP]))
    big = np.array([np.max(np.abs(J)) for J in s.J[:nP]])
    for a in range(nP):
        err, bound = np.max(np.abs(JQ[a] - want[a])), 1e-12 * (np.max(np.abs(JQ[a])) + np.abs(A[a]) @ big)
        print("%s linearity row %d: %.3e (bound %.3e)" % (_id(s.key), a, err, bound))
        assert err <= bound


@pytest.mark.parametrize("nP", [3, 17])
def test_energy_matrix(shape, nP):
    s = shape
    W = s.gb.coulomb_energy_matrix(s.P[:nP])
    J = s.gb.coulomb_batch(s.P[:nP])
    assert W.shape == (nP, nP)
    worst = 0.0
    for a in range(nP):
        for b in range(nP):
            err, bound = abs(W[a, b] - np.trace(s.P[a] @ J[b])), 1e-12 * np.max(np.abs(J[b])) * np.sum(np.abs(s.P[a]))
            worst = max(worst, err / bound)
            assert err <= bound, (a, b, err, bound)
    asym = np.max(np.abs(W - W.T)) / np.max(np.abs(W))
    print("%s W nP=%d: worst error / bound %.3e, |W - W^T| / max|W| %.3e" % (_id(s.key), nP, worst, asym))
    assert asym <= 1e-11
    assert nP < 17 or np.max(np.abs(W - W.T)) > 0.0  # formed entry by entry, not symmetrised


def test_repeated_calls_are_bitwise_equal(shape):
    s = shape
    assert np.array_equal(s.gb.coulomb_batch(s.P), s.gb.coulomb_batch(s.P))
    assert np.array_equal(s.gb.coulomb_batch(s.P[:3]), s.gb.coulomb_batch(s.P[:3]))
    assert np.array_equal(s.gb.coulomb_energy_matrix(s.P), s.gb.coulomb_energy_matrix(s.P))


@pytest.mark.parametrize("nP", [3, 17])
def test_shards_sum_to_the_unsharded_result(shape, nP):
    """the device-pointer entry honours hfg_ctx_set_shard (the host-pointer ones return whole matrices)"""
    import torch
    s = shape
    ctx = s.gb.ctx
    dP = torch.from_numpy(wk.flat(s.P[:nP])).to("cuda")
    torch.cuda.synchronize()

    def run():
        out = s.gb.coulomb_batch_torch(dP)
        ctx.synchronize()
        return out.cpu().numpy().reshape(nP, -1)
    whole = run()
    acc = np.zeros_like(whole)
    try:
        for rk in range(2):
            ctx.set_shard(rk, 2)
            part = run()
            assert np.max(np.abs(part)) > 0.0 and not np.array_equal(part, whole)
            acc += part
    finally:
        ctx.set_shard(0, 1)
    assert _worst(s, "torch entry nP=%d against single calls" % nP, whole, [wk.flat([J]) for J in s.J[:nP]]) < 1e-12
    assert _worst(s, "shards (0,2) + (1,2) nP=%d" % nP, acc, whole) <= 1e-13
    # the host-pointer entry ignores a shard left on the context
    try:
        ctx.set_shard(1, 2)
        J = s.gb.coulomb_batch(s.P[:nP])
    finally:
        ctx.set_shard(0, 1)
    assert _worst(s, "host entry under a shard", J, s.J[:nP]) < 1e-12


@pytest.mark.parametrize("Z", [1, 2])
def test_hydrogenic_self_repulsion(hf, Z):
    """W = tr(P J[P]), P = c c^T with the 1s orbital of T + V: (1s1s|1s1s) = 5 Z / 8"""
    gb, _ = common.make_atomic_bases(Z, 0, 0, 5, 10, oracle=False)
    gb.compute_tei(False)
    gb.upload()
    S, H0 = gb.overlap(), gb.kinetic() + gb.nuclear()
    Sinvh = hf.scf.form_Sinvh(S, False, gb.get_sym_idx(0))
    E, C = hf.scf.eig_gsym(H0, Sinvh)
    c = C[:, 0] / np.sqrt(C[:, 0] @ S @ C[:, 0])
    W = gb.coulomb_energy_matrix([np.outer(c, c), np.outer(c, c)])
    print("Z = %d: E0 %.12f, W %.12f, W - 5Z/8 %+.3e (bound %.3e)" % (Z, E[0], W[0, 0], W[0, 0] - 0.625 * Z, 10 * KNOWN[Z]))
    assert abs(E[0] + 0.5 * Z * Z) < 1e-7
    assert np.all(np.abs(W - 0.625 * Z) <= 10 * KNOWN[Z])


def _worker(mode, path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "coulomb_batch_worker.py"), mode, path], cwd=ROOT, timeout=300,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0 and "ok" in out.stdout.decode().split(), out.stdout.decode()[-3000:]


def test_devptr_entry_keeps_the_stream_order(hf, tmp_path):
    """the protocol of tests/stream_order_worker.py on a non-default torch stream: input written by a copy enqueued just
    before the call, output read by a copy enqueued just after, decoys before and after, no host synchronisation"""
    import stream_order_worker as sow
    path = str(tmp_path / "stream.json")
    _worker("stream", path)
    rec = json.load(open(path))
    print(rec)
    assert rec["decoy_differs"] and rec["repeat"]["ok"] and rec["twin"]["ok"]
    assert rec["baselines_bitwise"], "results repeat bitwise from call to call"
    assert rec["delay_ms"] >= sow.DELAY_MIN_MS, "the delay is too short for the run to mean anything"
    assert not rec["ordered_is_decoy"], "the call read its inputs before the copy enqueued ahead of it"
    assert rec["ordered"]["ok"] and rec["ordered"]["bitwise"]


def test_workspace_dies_with_its_table_set(hf, tmp_path):
    """a batched call, the basis destroyed, a basis of another size: the second call is right (against single calls in the
    worker and against the oracle here)"""
    path = str(tmp_path / "own.npz")
    _worker("ownership", path)
    r = np.load(path)
    assert r["J1"].shape[1:] != r["J2"].shape[1:]
    for tag, nP in zip("12", wk.NP_OWN):
        J, S, W = r["J" + tag], r["S" + tag], r["W" + tag]
        assert J.shape[0] == nP and W.shape == (nP, nP)
        assert max(np.max(np.abs(j - s)) / np.max(np.abs(s)) for j, s in zip(J, S)) < 1e-12
    gb, ob = common.make_bases(*wk.DIATOMIC_2, product=False)
    ob.compute_tei(False)
    N = r["J2"].shape[1]
    Ps = wk.symmetric_batch(N, wk.NP_OWN[1], 31)
    for b, P in enumerate(Ps):
        assert common.relerr(r["J2"][b], ob.coulomb(np.asfortranarray(P))) < 1e-12


def test_refusals(shape, hf):
    import ctypes
    s = shape
    L = hf.lib()
    N = s.gb.Nbf()
    buf = np.zeros(N * N)
    p = buf.ctypes.data_as(hf.c_double_p)
    assert L.hfg_coulomb_batch(s.gb.ctx.h, s.gb.h, 0, None, None) == 0  # nothing to do
    assert L.hfg_coulomb_batch(s.gb.ctx.h, s.gb.h, -1, p, p) == 1 and b"negative" in L.hfg_last_error()
    assert L.hfg_coulomb_batch(s.gb.ctx.h, s.gb.h, 1, None, p) == 1 and b"null" in L.hfg_last_error()
    assert L.hfg_coulomb_energy_matrix(s.gb.ctx.h, s.gb.h, 1, p, None) == 1 and b"null" in L.hfg_last_error()
    assert L.hfg_coulomb_batch_devptr(s.gb.ctx.h, s.gb.h, 2, None, None) == 1 and b"null" in L.hfg_last_error()
    fresh, _ = common.make_bases(1, 1, 1.4, (0,), 2, 4, oracle=False)  # tables neither computed nor uploaded
    n = fresh.Nbf()
    z = np.zeros(2 * n * n)
    zp = z.ctypes.data_as(hf.c_double_p)
    assert L.hfg_coulomb_batch(s.gb.ctx.h, fresh.h, 2, zp, zp) == 1 and b"Primitive teis have not been computed" in L.hfg_last_error()
    with pytest.raises(ValueError):
        s.gb.coulomb_batch([np.zeros((N + 1, N + 1))])


def test_cpp_adapter_overload(native_libs):
    exe = os.path.join(ROOT, "tests", "cpp", "coulomb_batch_adapter_test")
    p = subprocess.run([exe, "run"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0 and "adapter ok" in out, out
    assert "logic_error_before_compute_tei 1" in out and "empty_batch 0" in out
    for prog in ("diatomic", "atomic"):
        assert float(re.search(r"^%s Nbf \d+ worst (\S+)$" % prog, out, flags=re.M).group(1)) < 1e-12, out
