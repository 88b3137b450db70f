"""Worker of tests/test_gpu_gemm_engine.py: every launcher of the FP64 GEMM tile engine (hip/gemm.hip) through the probe
library tests/gpu_probe/libgemm_engine_probe.so, in ONE process (HELFEM_GEMM_TILE and HELFEM_MFMA are read once per
process; the test starts this file once per setting).

    python tests/gemm_engine_worker.py OUT.npz [--big]

Two host references per group of tasks:
  exact    operands are integers in [-8, 8], alpha in {1, -1, 2}, beta in {0, 1, -1}: every partial sum is an integer far
           below 2^53, so the result does not depend on the order of summation, on the matrix instruction or on the
           order of the split-K atomic additions.  Reference: NumPy int64.  Criterion: np.array_equal.
  rounded  uniform(-1, 1) data, row i of op(A) scaled by 2^e_i and column j of op(B) by 2^f_j (e, f seeded integers in
           [-30, 30]); reference and |op A| |op B| in np.longdouble; componentwise
               |C - ref| <= (K + 4) 2^-53 (|alpha| |op A| |op B| + |beta| |C0|),
           the bound of a length-K dot product summed in any order, one scaling and one addition.
Every C buffer is filled with a finite sentinel first: the rows M..ldc-1, the gaps between the tasks, the columns outside
cmap and the tiles sym = 2 skips must hold it (or C0) bit for bit afterwards.  The operand buffers hold NaN wherever a
task has no element, so a NaN in the stored part of C means that something outside M x K or K x N was used.

The result file holds one record per (group, reference): name, value_ok, sentinel_ok, ratio (largest error / bound of
the rounded reference, 0 for the exact one) and a line of detail for the first task that failed."""
import ctypes
import os
import sys

import numpy as np

try:  # one HIP runtime per process: torch's must be loaded first
    import torch
except Exception:  # pragma: no cover
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import helfem_amd as hf  # noqa: E402

SENT = -12345.0625
U = np.longdouble(2.0) ** -53
LD = np.longdouble
(L_GEMM, L_TASKLIST, L_TASKLIST64, L_RECT, L_ACC, L_MAP64, L_SPLIT2, L_SPLIT2_RECT, L_WL, L_WL_SPLIT2_RECT, L_MIRROR) = range(11)
MN_EDGES = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 193]
K_EDGES = [0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 100]
ALPHAS = [1.0, -1.0, 2.0]
BETAS = [0.0, 1.0, -1.0]

# (name, launcher, flag, tile (BM, BN) for the work lists, traits)
#   beta: the launcher honours beta; acc: beta != 0 required; zero: C zeroed beforehand (split K); over: honours `over`
VARIANTS = [
    ("tasklist", L_TASKLIST, 0, None, dict(beta=True, over=True)),
    ("tasklist64", L_TASKLIST64, 0, None, dict(beta=True, over=True)),
    ("rect", L_RECT, 0, None, dict(beta=True, over=True)),
    ("acc64", L_ACC, 1, None, dict(acc=True, over=True)),
    ("acc128", L_ACC, 0, None, dict(acc=True, over=True)),
    ("split2", L_SPLIT2, 0, None, dict(zero=True)),
    ("split2_rect", L_SPLIT2_RECT, 0, None, dict(zero=True)),
    ("wl128", L_WL, 0, (128, 128), dict(over=True)),
    ("wl128x64", L_WL, 1, (128, 64), dict(over=True)),
    ("wl64", L_WL, 2, (64, 64), dict(over=True)),
    ("wl_split2_rect", L_WL_SPLIT2_RECT, 0, (128, 64), dict(zero=True)),
]


class Task(object):
    """one product; ld*: None -> rows + pad with the parity asked for; share: tasks with the same key get the same data"""

    def __init__(self, M, N, K, tA=0, tB=0, alpha=1.0, beta=0.0, sym=0, over=0, odd_ld=False, odd_off=False, lda=None, ldb=None,
                 ldc_pad=3, zero_c=False, share=None, gen=None, amap=None, wa=0, cmap=None, wc=0, band=None):
        self.__dict__.update(locals())
        del self.__dict__["self"]

    def __repr__(self):
        return "Task(M=%d N=%d K=%d tA=%d tB=%d alpha=%g beta=%g sym=%d over=%d odd_ld=%s odd_off=%s)" % (
            self.M, self.N, self.K, self.tA, self.tB, self.alpha, self.beta, self.sym, self.over, self.odd_ld, self.odd_off)


def _data(t, rng, mode):
    """op(A) (M x K), op(B) (K x N), C0 (M x N)"""
    if t.gen is not None:
        return t.gen(rng, mode)
    M, N, K = t.M, t.N, t.K
    if mode == "exact":
        return (rng.randint(-8, 9, size=(M, K)).astype(np.float64), rng.randint(-8, 9, size=(K, N)).astype(np.float64),
                rng.randint(-8, 9, size=(M, N)).astype(np.float64))
    e = np.ldexp(1.0, rng.randint(-30, 31, size=(M, 1)))
    f = np.ldexp(1.0, rng.randint(-30, 31, size=(1, N)))
    return rng.uniform(-1, 1, size=(M, K)) * e, rng.uniform(-1, 1, size=(K, N)) * f, rng.uniform(-1, 1, size=(M, N)) * e * f


def _ld(rows, given, odd, pad=2):
    if given is not None:
        return given
    ld = max(rows, 1) + pad
    return ld + 1 if (ld & 1) != int(odd) else ld


def _view(arena, off, rows, cols, ld):
    return np.lib.stride_tricks.as_strided(arena[off:], shape=(rows, cols), strides=(arena.itemsize, arena.itemsize * ld))


class Packed(object):
    pass


def pack(tasks, mode, seed):
    """operand buffers (NaN where no task has an element), the C buffer (sentinel, C0 in the stored parts), the task table
    and the reference: `owned` marks the elements the launch must write, `ref` / `bnd` their values and bounds"""
    rng = np.random.RandomState(seed)
    shared = {}
    p = Packed()
    p.tasks, p.mode = tasks, mode
    lay = []
    cur = [0, 0, 0]
    maps = []

    def place(which, size, odd):
        off = (cur[which] + 1) & ~1
        off += 2 if not odd else 1  # (even offsets are not zero either: an element offset inside the buffer)
        cur[which] = off + size
        return off

    for t in tasks:
        if t.share is not None and (t.share, mode) in shared:
            opA, opB, C0 = shared[(t.share, mode)]
        else:
            opA, opB, C0 = _data(t, rng, mode)
            if t.share is not None:
                shared[(t.share, mode)] = (opA, opB, C0)
        if t.zero_c:
            C0 = np.zeros((t.M, t.N))
        if t.amap is not None:  # op(A) = A[:, amap] of a wider A whose other columns hold NaN
            sa = np.full((t.M, t.wa), np.nan)
            sa[:, t.amap] = opA
        else:
            sa = opA.T if t.tA else opA
        sb = opB.T if t.tB else opB
        lda, ldb = _ld(sa.shape[0], t.lda, t.odd_ld), _ld(sb.shape[0], t.ldb, t.odd_ld)
        ldc = max(t.M, 1) + t.ldc_pad
        ccols = t.wc if t.cmap is not None else t.N
        offA = place(0, lda * sa.shape[1] + 16 + (128 * lda if t.over & 1 else 0), t.odd_off)
        offB = place(1, ldb * sb.shape[1] + 16 + (128 * ldb if t.over & 2 else 0), t.odd_off)
        offC = place(2, ldc * ccols + 8, False)
        am = cm = -1
        if t.amap is not None:
            am = len(maps)
            maps += list(t.amap)
            cm = len(maps)
            maps += list(t.cmap)
        lay.append(dict(sa=sa, sb=sb, C0=C0, opA=opA, opB=opB, lda=lda, ldb=ldb, ldc=ldc, offA=offA, offB=offB, offC=offC, am=am, cm=cm,
                        ccols=ccols))
    p.A = np.full(cur[0] + 16, np.nan)
    p.B = np.full(cur[1] + 16, np.nan)
    p.C0 = np.full(cur[2] + 16, SENT)
    p.owned = np.zeros(p.C0.size, dtype=bool)
    p.ref = np.zeros(p.C0.size, dtype=np.float64 if mode == "exact" else LD)
    p.bnd = np.zeros(p.C0.size, dtype=LD) if mode != "exact" else None
    p.ti = np.zeros((len(tasks), 16), dtype=np.int64)
    p.td = np.zeros((len(tasks), 2))
    p.maps = np.asarray(maps if maps else [0], dtype=np.int32)
    p.lay = lay
    for i, (t, l) in enumerate(zip(tasks, lay)):
        if l["sa"].size:
            _view(p.A, l["offA"], l["sa"].shape[0], l["sa"].shape[1], l["lda"])[...] = l["sa"]
        if l["sb"].size:
            _view(p.B, l["offB"], l["sb"].shape[0], l["sb"].shape[1], l["ldb"])[...] = l["sb"]
        p.ti[i] = [l["offA"], l["offB"], l["offC"], t.M, t.N, t.K, l["lda"], l["ldb"], l["ldc"], t.tA, t.tB, t.sym, t.over, l["am"], l["cm"], 0]
        p.td[i] = [t.alpha, t.beta]
        if t.M <= 0 or t.N <= 0:
            continue
        cols = np.asarray(t.cmap) if t.cmap is not None else np.arange(t.N)
        cv = _view(p.C0, l["offC"], t.M, l["ccols"], l["ldc"])
        beta = 1.0 if t.zero_c else t.beta
        if t.cmap is None:
            cv[...] = l["C0"]
        own = np.ones((t.M, t.N), dtype=bool)
        if t.band is not None:  # sym = 2: tiles with bm / BM + 3 < bn / BN keep C0
            BM = t.band
            own = ~((np.arange(t.M)[:, None] // BM + 3) < (np.arange(t.N)[None, :] // BM))
        if mode == "exact":
            ref = t.alpha * (l["opA"].astype(np.int64) @ l["opB"].astype(np.int64))
            if beta != 0.0 and t.cmap is None:
                ref = ref + beta * l["C0"].astype(np.int64)
            ref = ref.astype(np.float64)
        else:
            a, b = l["opA"].astype(LD), l["opB"].astype(LD)
            ref = LD(t.alpha) * (a @ b)
            bnd = abs(LD(t.alpha)) * (np.abs(a) @ np.abs(b))
            if beta != 0.0 and t.cmap is None:
                ref = ref + LD(beta) * l["C0"].astype(LD)
                bnd = bnd + abs(LD(beta)) * np.abs(l["C0"]).astype(LD)
            bnd = bnd * (LD(t.K + 4) * U)
            bv = _view(p.bnd, l["offC"], t.M, l["ccols"], l["ldc"])
            bv[:, cols] = np.where(own, bnd, bv[:, cols])
        ov = _view(p.owned, l["offC"], t.M, l["ccols"], l["ldc"])
        ov[:, cols] = own
        rv = _view(p.ref, l["offC"], t.M, l["ccols"], l["ldc"])
        rv[:, cols] = np.where(own, ref, rv[:, cols])
    return p


_probe = None


def probe():
    global _probe
    if _probe is None:
        path = os.path.join(ROOT, "tests", "gpu_probe", "libgemm_engine_probe.so")
        if not os.path.exists(path):
            from helfem_amd import build
            build.build_gemm_probe(verbose=False)
        _probe = ctypes.CDLL(path)
        dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)
        _probe.probe_gemm_launch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, lp, dp, dp, ctypes.c_int64, dp,
                                             ctypes.c_int64, dp, ctypes.c_int64, ip, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ip]
        _probe.probe_gemm_worklist.argtypes = [ctypes.c_int, ip, ctypes.c_int, ctypes.c_int, ip, ctypes.c_int, ip]
    return _probe


def launch(p, launcher, flag=0, Cin=None, maxM=None, maxN=None):
    """one launcher, once, on the packed tasks; returns the whole C buffer and the length of the work list"""
    dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)
    C = (p.C0 if Cin is None else Cin).copy()
    maxM = max(t.M for t in p.tasks) if maxM is None else maxM
    maxN = max(t.N for t in p.tasks) if maxN is None else maxN
    nwg = ctypes.c_int(0)
    rc = probe().probe_gemm_launch(hf.default_context().h, launcher, flag, len(p.tasks), p.ti.ctypes.data_as(lp), p.td.ctypes.data_as(dp),
                                   p.A.ctypes.data_as(dp), p.A.size, p.B.ctypes.data_as(dp), p.B.size, C.ctypes.data_as(dp), C.size,
                                   p.maps.ctypes.data_as(ip), p.maps.size, maxM, maxN, ctypes.byref(nwg))
    if rc != 0:
        raise RuntimeError(hf.lib().hfg_last_error().decode())
    return C, nwg.value


RESULTS = []


def record(name, value_ok, sentinel_ok, ratio, detail):
    RESULTS.append((name, bool(value_ok), bool(sentinel_ok), float(ratio), detail))
    print("%-58s value %-5s sentinel %-5s ratio %.3f %s" % (name, bool(value_ok), bool(sentinel_ok), ratio, detail), flush=True)


def check(name, p, C, extra_ok=True, extra_detail=""):
    """the stored parts against the reference, everything else against what was there before, bit for bit"""
    name = "%s[%s]" % (name, p.mode)
    own = p.owned
    sentinel_ok = np.array_equal(C[~own].view(np.int64), p.C0[~own].view(np.int64))
    ratio = 0.0
    if p.mode == "exact":
        value_ok = np.array_equal(C[own], p.ref[own])
        bad = own & (C != p.ref)
    else:
        err = np.abs(C.astype(LD) - p.ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, LD(0), err / p.bnd)  # (no error: 0 whatever the bound; NaN or error at bound 0: not <= 1)
        r = np.where(np.isfinite(r), r, LD(np.inf))
        bad = own & ~(r <= 1)
        ratio = float(np.max(r[own])) if own.any() else 0.0
        value_ok = not bad.any()
    detail = extra_detail
    if not (value_ok and sentinel_ok):
        wrong = bad | (~own & (C.view(np.int64) != p.C0.view(np.int64)))
        for i, (t, l) in enumerate(zip(p.tasks, p.lay)):
            lo, hi = l["offC"], l["offC"] + l["ldc"] * l["ccols"]
            if wrong[lo:hi].any():
                k = int(np.flatnonzero(wrong[lo:hi])[0])
                detail += " first failure: task %d %r at (row %d, column %d): got %r want %r" % (
                    i, t, k % l["ldc"], k // l["ldc"], C[lo + k], float(p.ref[lo + k]) if own[lo + k] else p.C0[lo + k])
                break
        else:
            detail += " failure outside every task's C"
    record(name, value_ok and extra_ok, sentinel_ok, ratio, detail.strip())
    return C


def stored(p, C, i):
    t, l = p.tasks[i], p.lay[i]
    return _view(C, l["offC"], t.M, l["ccols"], l["ldc"]).copy()


def run_variant(group, var, tasks, seed, modes=("exact", "rounded")):
    """the task list through one launcher variant with both references; the flags a variant does not take are normalised"""
    name, launcher, flag, tile, traits = var
    out = {}
    for mode in modes:
        ts = []
        for t in tasks:
            kw = dict(t.__dict__)
            if traits.get("zero"):
                kw.update(beta=0.0, zero_c=True)
            elif traits.get("acc"):
                kw.update(beta=t.beta if t.beta != 0.0 else 1.0)
            elif not traits.get("beta"):
                kw.update(beta=0.0)
            if not traits.get("over"):
                kw.update(over=0)
            ts.append(Task(**kw))
        p = pack(ts, mode, seed)
        C, nwg = launch(p, launcher, flag)
        out[mode] = (p, check("%s/%s" % (group, name), p, C), nwg)
    return out


def edge_triples(seed, count=44):
    """the eight corner triples of the edge sets and a seeded sample of the rest of the cross product"""
    tri = [(m, n, k) for m in (MN_EDGES[0], MN_EDGES[-1]) for n in (MN_EDGES[0], MN_EDGES[-1]) for k in (K_EDGES[0], K_EDGES[-1])]
    rng = np.random.RandomState(seed)
    while len(tri) < count:
        c = (MN_EDGES[rng.randint(11)], MN_EDGES[rng.randint(11)], K_EDGES[rng.randint(11)])
        if c not in tri:
            tri.append(c)
    return tri


def edge_tasks(seed):
    ts = []
    for i, (m, n, k) in enumerate(edge_triples(seed)):
        ts.append(Task(m, n, k, tA=i & 1, tB=(i >> 1) & 1, alpha=ALPHAS[i % 3], beta=BETAS[(i // 3) % 3], odd_ld=(i % 5 == 2),
                       odd_off=(i % 7 == 3), ldc_pad=1 + i % 4))
    return ts


def transpose_tasks():
    """every tA/tB combination on the 16-byte path and on the element-wise path for each reason it is taken"""
    ts = []
    for tA in (0, 1):
        for tB in (0, 1):
            ts += [Task(128, 128, 32, tA, tB),  # even ld, aligned base, interior tiles, whole k steps
                   Task(128, 128, 32, tA, tB, odd_ld=True), Task(128, 128, 32, tA, tB, odd_off=True),
                   Task(130, 131, 32, tA, tB),  # partial edge tiles
                   Task(128, 128, 40, tA, tB, alpha=2.0, beta=-1.0)]  # K tail
    return ts


def over_tasks():
    """the exchange's shape class scaled down: M = 225 of 256 readable rows, N no multiple of a tile, K = 48; the four
    values of `over` on the same data"""
    ts = []
    for g, (tA, tB) in enumerate([(0, 0), (0, 1), (1, 0)]):
        for over in (0, 1, 2, 3):
            ts.append(Task(225, 100, 48, tA, tB, alpha=ALPHAS[g], beta=BETAS[g], over=over, lda=(48 if tA else 256), ldb=(128 if tB else 48),
                           share="over%d" % g))
    return ts


def sym1_tasks():
    def gen(n, K):
        def g(rng, mode):
            Y = rng.randint(-8, 9, size=(K, n))
            S = rng.randint(-8, 9, size=(K, K))
            S = np.tril(S) + np.tril(S, -1).T
            return Y.T.astype(np.float64), (S @ Y).astype(np.float64), np.zeros((n, n))
        return g
    ts = [Task(n, n, 40, tA=1, tB=0, sym=1, gen=gen(n, 40)) for n in (64, 65, 129, 200, 321)]
    ts.insert(2, Task(70, 45, 40, tA=1, tB=0, sym=0))
    return ts


def map_tasks(seed):
    rng = np.random.RandomState(seed)
    ts = []
    i = 0
    for K in (1, 16, 17, 47):
        for M in (33, 64, 97, 345):
            N = (20, 64, 70, 130)[(i + i // 4) % 4]
            wa, wc = K + 9, N + 7
            amap = np.sort(rng.permutation(wa)[:K]) if i % 2 == 0 else rng.permutation(wa)[:K]
            cmap = rng.permutation(wc)[:N]
            # offset of A: even (16-byte lookups) or odd (element-wise lookups) number of rows
            ts.append(Task(M, N, K, alpha=ALPHAS[i % 3], amap=[int(x) for x in amap], wa=wa, cmap=[int(x) for x in cmap], wc=wc,
                           odd_off=(i % 3 == 1)))
            i += 1
    return ts


def wl_tasks(tile, target, split):
    """three tasks of different shapes whose work list has a length of `target` modulo 8"""
    BM, BN = tile
    nt = lambda m, n: ((m + BM - 1) // BM) * ((n + BN - 1) // BN) * (2 if split else 1)
    base = [(200, 150), (70, 300)]
    for m3 in range(1, 700, 37):
        for n3 in range(1, 500, 41):
            if (sum(nt(m, n) for m, n in base) + nt(m3, n3)) % 8 == target:
                return [Task(200, 150, 40, 0, 0, alpha=2.0), Task(70, 300, 33, 1, 0), Task(m3, n3, 17, 0, 1, alpha=-1.0, odd_ld=True)]
    raise RuntimeError("no third task gives a work list of length %d mod 8" % target)


WL_EDGES = [1, 64, 65, 128, 129]
WL_TILES = [("64", 1, (64, 64)), ("128", 2, (128, 128)), ("128x64", 3, (128, 64))]  # (name, GemmTile, (BM, BN))


def worklist_cases():
    """the list gemm_worklist builds (host work) against its enumeration written out here: (task, tile), or for split K
    (task, 2 tile + half), for every tile of every non-empty task in task order; two tasks around an empty one"""
    ip = ctypes.POINTER(ctypes.c_int)
    for tname, tile, (BM, BN) in WL_TILES:
        for split in (0, 1):
            ok, detail, count = True, "", 0
            for i, m in enumerate(WL_EDGES):
                for j, n in enumerate(WL_EDGES):
                    shapes = [(m, n), ((0, 50), (50, 0))[(i + j) % 2], (WL_EDGES[(j + 2) % 5], WL_EDGES[(i + 1) % 5])]
                    want = [(t, q) for t, (M, N) in enumerate(shapes) if M > 0 and N > 0
                            for q in range(-(-M // BM) * -(-N // BN) * (2 if split else 1))]
                    mn = np.asarray(shapes, dtype=np.int32).ravel()
                    out = np.full(2 * len(want) + 8, -7, dtype=np.int32)
                    n_out = ctypes.c_int(-1)
                    rc = probe().probe_gemm_worklist(len(shapes), mn.ctypes.data_as(ip), tile, split, out.ctypes.data_as(ip), out.size // 2,
                                                     ctypes.byref(n_out))
                    got = [tuple(int(x) for x in out[2 * k:2 * k + 2]) for k in range(max(0, min(n_out.value, out.size // 2)))]
                    count += len(want)
                    if ok and (rc != 0 or n_out.value != len(want) or got != want):
                        ok, detail = False, "tasks %r: %d entries %r..., want %d %r..." % (shapes, n_out.value, got[:6], len(want), want[:6])
            record("worklist-host/%s%s" % (tname, "-split2" if split else ""), ok, True, 0.0, detail or "%d entries" % count)


def bitwise_equal(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


def engine_cases():
    by_name = dict((v[0], v) for v in VARIANTS)
    # ---- shapes around the tile edges: every launcher, >= 40 triples each with the corners ----
    for vi, var in enumerate(VARIANTS):
        run_variant("edges", var, edge_tasks(100 + vi), 200 + vi)
    for mode in ("exact", "rounded"):  # gemm_dev takes one product per call
        n0 = len(RESULTS)
        for i, t in enumerate(edge_tasks(150)):
            p = pack([t], mode, 1000 + i)
            check("edges/gemm_dev#%d" % i, p, launch(p, L_GEMM)[0])
        _fold("edges/gemm_dev[%s]" % mode, n0)
    # ---- transposes x load paths ----
    for var in VARIANTS:
        run_variant("transposes", var, transpose_tasks(), 300)
    for mode in ("exact", "rounded"):
        n0 = len(RESULTS)
        for i, t in enumerate(transpose_tasks()):
            p = pack([t], mode, 1100 + i)
            check("transposes/gemm_dev#%d" % i, p, launch(p, L_GEMM)[0])
        _fold("transposes/gemm_dev[%s]" % mode, n0)
    # ---- over = 1, 2, 3 give what over = 0 gives, bit for bit ----
    for var in VARIANTS:
        if not var[4].get("over"):
            continue
        out = run_variant("over", var, over_tasks(), 400)
        for mode, (p, C, _) in out.items():
            same = all(bitwise_equal(stored(p, C, 4 * g), stored(p, C, 4 * g + o)) for g in range(3) for o in (1, 2, 3))
            record("over-equals-plain/%s[%s]" % (var[0], mode), same, True, 0.0, "")
    # ---- sym = 1: lower tiles, then the mirror; the full square is the host's product ----
    for name in ("tasklist64", "tasklist", "split2"):
        var = by_name[name]
        ts = [Task(**dict(t.__dict__, zero_c=bool(var[4].get("zero")))) for t in sym1_tasks()]
        p = pack(ts, "exact", 500)
        C1, _ = launch(p, var[1], var[2])
        C2, _ = launch(p, L_MIRROR, 0, Cin=C1)
        check("sym1/%s+mirror" % name, p, C2)
    # ---- sym = 2 with the accumulating epilogue: the tridiagonalisation's trailing update ----
    for name, BM, ns in (("acc64", 64, (321, 385)), ("acc128", 128, (641,))):
        var = by_name[name]
        ts = []
        for n in ns:
            ts.append(Task(n, n, 32, 0, 1, alpha=-1.0, beta=1.0, sym=2, band=BM, share="trd%d" % n, ldc_pad=5))
            ts.append(Task(n, n, 32, 0, 1, alpha=-1.0, beta=1.0, sym=0, share="trd%d" % n, ldc_pad=5))
        for mode in ("exact", "rounded"):
            p = pack(ts, mode, 600)
            C, _ = launch(p, var[1], var[2])
            check("sym2/%s" % name, p, C)
    # ---- the accumulating epilogues without sym: PRE (64) and batched (128), ragged shapes ----
    acc = [Task(m, n, k, tA=i & 1, tB=(i >> 1) & 1, alpha=ALPHAS[i % 3], beta=(1.0, -1.0)[i % 2], ldc_pad=2 + i)
           for i, (m, n, k) in enumerate([(150, 70, 32), (97, 201, 64), (130, 129, 33), (257, 65, 64), (63, 130, 33), (129, 257, 32)])]
    for name in ("acc64", "acc128"):
        run_variant("acc", by_name[name], acc, 700)
    # ---- column maps ----
    mv = ("map64", L_MAP64, 0, None, dict())
    run_variant("map", mv, map_tasks(800), 801)
    # ---- split K: the second half is empty for K <= 16 ----
    shapes = [(130, 70), (128, 128), (65, 193)]
    sk = [Task(shapes[i % 3][0], shapes[i % 3][1], K, tA=i & 1, tB=(i >> 1) & 1, alpha=ALPHAS[i % 3])
          for i, K in enumerate((1, 16, 17, 31, 32, 33, 100))]
    for name in ("split2", "split2_rect", "wl_split2_rect"):
        run_variant("splitk", by_name[name], sk, 900)
    # ---- work lists: three tasks, nwg % 8 = 0, 1, 7 (the dealing over the XCDs has a remainder branch) ----
    for name in ("wl128", "wl128x64", "wl64", "wl_split2_rect"):
        var = by_name[name]
        split = name == "wl_split2_rect"
        for target in ((0, 2, 6) if split else (0, 1, 7)):  # (two entries per tile: a split list has an even length)
            out = run_variant("worklist%d" % target, var, wl_tasks(var[3], target, split), 1000 + target)
            nwg = out["exact"][2]
            record("worklist%d/%s/length" % (target, name), nwg % 8 == target and nwg >= 8, True, 0.0, "nwg = %d" % nwg)
    worklist_cases()
    # ---- empty tasks and a task far smaller than maxM x maxN ----
    empty = [Task(200, 200, 24), Task(0, 50, 24), Task(5, 3, 24, alpha=-1.0), Task(50, 0, 24), Task(190, 70, 24, 1, 1, beta=1.0)]
    for var in VARIANTS:
        run_variant("empty", var, empty, 1200)
    em = [Task(t.M, t.N, t.K, amap=list(range(t.K)), wa=t.K, cmap=list(range(t.N))[::-1], wc=t.N + 2) for t in empty]
    run_variant("empty", mv, em, 1201)


def public_cases(big):
    """hfg_gemm and hfg_gemm_dev, the two public doors to gemm_dev (alpha = 1, beta = 0)"""
    dp = ctypes.POINTER(ctypes.c_double)
    i64 = ctypes.c_int64
    lib, ctx = hf.lib(), hf.default_context()
    specs = [Task(70, 45, 33, tA, tB, odd_ld=odd, odd_off=True) for tA in (0, 1) for tB in (0, 1) for odd in (False, True)]
    specs += [Task(70, 45, 0, tA, tB, odd_off=True) for tA in (0, 1) for tB in (0, 1)]
    for mode in ("exact", "rounded"):
        # host pointers, lda > m (or k) and ldc > m: the call may write the m x n part of the caller's C only
        n0 = len(RESULTS)
        for i, t in enumerate(specs):
            p = pack([t], mode, 1300 + i)
            l = p.lay[0]
            C = p.C0.copy()
            rc = lib.hfg_gemm(ctx.h, t.tA, t.tB, i64(t.M), i64(t.N), i64(t.K), p.A[l["offA"]:].ctypes.data_as(dp), i64(l["lda"]),
                              p.B[l["offB"]:].ctypes.data_as(dp), i64(l["ldb"]), C[l["offC"]:].ctypes.data_as(dp), i64(l["ldc"]))
            if rc != 0:
                record("public/hfg_gemm#%d[%s]" % (i, mode), False, False, 0.0, repr(t) + ": " + lib.hfg_last_error().decode())
                continue
            check("public/hfg_gemm#%d" % i, p, C)
        _fold("public/hfg_gemm[%s]" % mode, n0)
        # device pointers: torch buffers, data_ptr() advanced by 8 bytes, odd lda, k = 0
        n0 = len(RESULTS)
        for i, t in enumerate(specs):
            p = pack([t], mode, 1400 + i)
            l = p.lay[0]
            dA, dB, dC = (torch.from_numpy(x).cuda() for x in (p.A, p.B, p.C0))
            torch.cuda.synchronize()
            # (pack places an odd_off operand at an odd element: an even element plus 8 bytes)
            ptr = [ctypes.c_void_p(d.data_ptr() + 8 * (l[k] - 1) + 8) for d, k in ((dA, "offA"), (dB, "offB"))]
            rc = lib.hfg_gemm_dev(ctx.h, t.tA, t.tB, i64(t.M), i64(t.N), i64(t.K), ptr[0], i64(l["lda"]), ptr[1], i64(l["ldb"]),
                                  ctypes.c_void_p(dC.data_ptr() + 8 * l["offC"]), i64(l["ldc"]))
            if rc != 0:
                record("public/hfg_gemm_dev#%d[%s]" % (i, mode), False, False, 0.0, repr(t) + ": " + lib.hfg_last_error().decode())
                continue
            ctx.synchronize()
            check("public/hfg_gemm_dev#%d" % i, p, dC.cpu().numpy())
        _fold("public/hfg_gemm_dev[%s]" % mode, n0)
    if big:
        # 2688 x 40 x 2688: 441 tiles of 128 x 128, which the default rule (gemm_prefers_128) sends to the large tiles on a
        # part with 256 CUs -- 441 >= 0.85 * 512; on another CU count it may not.  HELFEM_GEMM_TILE=128 is the guarantee.
        rng = np.random.RandomState(7)
        A, B = rng.randint(-8, 9, size=(2688, 40)), rng.randint(-8, 9, size=(40, 2688))
        C = hf.scf.gemm(A.astype(np.float64), B.astype(np.float64))
        record("public/hfg_gemm-2688x40x2688[exact]", np.array_equal(C, (A @ B).astype(np.float64)), True, 0.0, "")


def _fold(name, n0):
    sub = RESULTS[n0:]
    del RESULTS[n0:]
    bad = [r for r in sub if not (r[1] and r[2])]
    record(name, not any(not r[1] for r in sub), not any(not r[2] for r in sub), max([r[3] for r in sub] + [0.0]),
           bad[0][0] + ": " + bad[0][4] if bad else "%d products" % len(sub))


def main():
    out = sys.argv[1]
    big = "--big" in sys.argv[2:]
    if hf.device_count() < 1:
        raise RuntimeError("no HIP device visible")
    tab = dict((r["name"], r["value"]) for r in hf.tuning_table())
    print("HELFEM_GEMM_TILE=%s HELFEM_MFMA=%s" % (tab.get("HELFEM_GEMM_TILE"), tab.get("HELFEM_MFMA")), flush=True)
    engine_cases()
    public_cases(big)
    np.savez(out, name=np.array([r[0] for r in RESULTS]), value_ok=np.array([r[1] for r in RESULTS]),
             sentinel_ok=np.array([r[2] for r in RESULTS]), ratio=np.array([r[3] for r in RESULTS]), detail=np.array([r[4] for r in RESULTS]),
             gemm_tile=np.array(str(tab.get("HELFEM_GEMM_TILE"))), mfma=np.array(str(tab.get("HELFEM_MFMA"))))
    print("gemm engine worker: %d records, %d failed" % (len(RESULTS), sum(1 for r in RESULTS if not (r[1] and r[2]))))


if __name__ == "__main__":
    main()
