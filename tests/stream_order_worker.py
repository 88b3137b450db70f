"""Worker of test_gpu_stream_order.py: the stream-ordering contract of the device-pointer entry points, in a process of its
own (the HELFEM_* switches are read once per process).

Usage: stream_order_worker.py --plan               the cases, one per line, without touching the GPU
       stream_order_worker.py SETTING OUT.json     every entry of the plan on every stream kind under SETTING's switches

The contract ("Stream ordering"): a call on a context reads its inputs after everything enqueued earlier on
the context's stream, writes its outputs before anything enqueued later, and is finished with its inputs by then.  Per entry
(protocol()): two synchronised baselines, the host-pointer twin, then with NO host synchronisation a delay, device-to-device
copies of the true inputs over decoys, the call, a copy of the outputs, and the decoys and a fill value written back over
inputs and outputs.  The copied outputs must be the baseline.  Decoys are valid inputs of the same kind (never NaN).

The process exits non-zero at the first error of the library and does nothing on the GPU after it."""
import contextlib
import ctypes
import json
import os
import re
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "helfem_gpu.h")

STREAM_KINDS = ("null", "torch", "own")
# name -> environment of the child process (the switches of these names are removed from it first)
SETTINGS = (
    ("defaults", {}),
    ("fock_overlap0", {"HELFEM_FOCK_OVERLAP": "0"}),
    ("bt_side", {"HELFEM_BT_FOLD": "0", "HELFEM_BT_SIDE": "1"}),
    ("trd_chain", {"HELFEM_TRD": "chain"}),
    ("profile", {}),
)
SWITCHES = ("HELFEM_FOCK_OVERLAP", "HELFEM_BT_FOLD", "HELFEM_BT_SIDE", "HELFEM_TRD", "HELFEM_BT", "HELFEM_TRDP_MIN", "HELFEM_EIGSEL",
            "HELFEM_EXCHANGE", "HELFEM_FOCK_SHARD")
# hfg_*_dev symbols of the header that take no device pointer: they build tables on the device from the host-side basis
# or evaluate host arrays, and synchronise before they return
EXCLUDED = {
    "hfg_compute_tei_dev": "takes no device pointer: set-up of the basis' tables on the device, complete when it returns",
    "hfg_compute_rs_tei_dev": "takes no device pointer: set-up of the basis' tables on the device, complete when it returns",
    "hfg_rs_special_dev": "takes host arrays (a, b, out): copies in, evaluates, copies out and synchronises",
}
# eigensolver: one block just above HELFEM_TRDP_MIN (256) and 4 * BT_KB (eig.hip: BT_KB = 64), an odd and a tiny one
EIG_SIZES = (257, 130, 3)
# a batch with a block of 1024 and more that goes through the chain of launches makes the context give its side stream up
# (tridiagonalize_takes_chain, trdp.hip): the smallest such block, for the trd_chain setting
GIVEUP_SIZES = (1024, 130, 3)
AFTER_GIVEUP = ("hfg_fock_compact_dev", "hfg_eig_gsym_sub_dev")
GEMM_MNK = (200, 300, 129)
FILL = -7.25
DELAY_TARGET_MS = 50.0
DELAY_MIN_MS = 10.0


def header_dev_symbols():
    """every hfg_*_dev function the header declares, in its order"""
    text = open(HEADER).read()
    seen = []
    for m in re.finditer(r"^\s*(?:int|int64_t)\s+(hfg_\w+_dev)\s*\(", text, re.M):
        if m.group(1) not in seen:
            seen.append(m.group(1))
    return seen


def entries():
    """the entries under test: what the header declares minus the documented exclusions"""
    return [s for s in header_dev_symbols() if s not in EXCLUDED]


def plan():
    """(setting, stream kind, case) of every run; a header symbol without a builder shows up as 'UNCOVERED'"""
    out = []
    for setting, _ in SETTINGS:
        for kind in STREAM_KINDS:
            for e in entries():
                out.append((setting, kind, e if e in BUILDERS else "UNCOVERED:" + e))
            if setting == "trd_chain":
                out.append((setting, kind, "hfg_eig_gsym_sub_dev@giveup"))
                for e in AFTER_GIVEUP:
                    out.append((setting, kind, e + "@after_giveup"))
    return out


# ---- figures: (label, value, bound) triples at the parity bounds of test_gpu_parity.py -----------------------------------
def _relerr(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _scal_figs(a, b):
    """Exc and Nel at 1e-11, Ekin at 1e-10, relative to max(1, |ref|) (test_xc_parity)"""
    d = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    return [("Exc,Nel", float(np.max(d[:2])), 1e-11), ("Ekin", float(d[2]), 1e-10)]


def rel_cmp(*tols):
    """one relative bound per output; an output with the bound 'scal' is the (Exc, Nel, Ekin) triple"""
    def cmp(outs, ref, data):
        figs = []
        for i, tol in enumerate(tols):
            figs += _scal_figs(outs[i], ref[i]) if tol == "scal" else [("relerr[%d]" % i, _relerr(outs[i], ref[i]), tol)]
        return figs
    return cmp


def abs_cmp(tol):
    return lambda outs, ref, data: [("abserr", float(np.max(np.abs(outs[0] - ref[0]))), tol)]


def _eig_figs(E, C, Eref, F):
    """test_gpu_eigsel.py::test_generalized_blocked with S = 1: eigenvalues, orthonormality and residual against the TRUE F"""
    scale = max(1.0, float(np.max(np.abs(Eref))))
    K = len(E)
    return [("|E - Eref| / scale", float(np.max(np.abs(E - Eref))) / scale, 1e-10),
            ("|C^T C - 1|", float(np.max(np.abs(C.T @ C - np.eye(K)))), 1e-10),
            ("|F C - C E| / scale", float(np.max(np.abs(F @ C - C * E))) / scale, 1e-9)]


def eig_cmp(outs, ref, data):
    N = data["F"].shape[0]
    return _eig_figs(outs[0], outs[1].reshape((N, -1), order="F"), ref[0], data["F"])


def blockbuf_cmp(outs, ref, data):
    """slot ib = [C block (n x n, ld n) | pad | eigenvalues (n) at offset nmax^2]: every block's pairs as in eig_cmp"""
    blocks, F = data["blocks"], data["F"]
    nmax = max(len(b) for b in blocks)
    slot = nmax * nmax + nmax
    worst = {}
    for ib, b in enumerate(blocks):
        n = len(b)
        s, r = outs[0][ib * slot:(ib + 1) * slot], ref[0][ib * slot:(ib + 1) * slot]
        for lab, v, bound in _eig_figs(s[nmax * nmax:nmax * nmax + n], s[:n * n].reshape((n, n), order="F"), r[nmax * nmax:nmax * nmax + n],
                                       F[np.ix_(b, b)]):
            worst[lab] = (max(v, worst.get(lab, (0.0, bound))[0]), bound)
    return [(lab, v, bound) for lab, (v, bound) in worst.items()]


# ---- cases ---------------------------------------------------------------------------------------------------------------
class Case(object):
    """ins: [buffer, true, decoy] device tensors per input; outs: output buffers; call(): the entry on the buffers;
    twin(): the host-pointer twin's outputs in the layout of outs, or None; cmp: the figures at the entry's parity bound"""

    def __init__(self, name, ins, outs, call, cmp, twin=None, data=None):
        self.name, self.ins, self.outs, self.call, self.cmp, self.twin, self.data = name, ins, outs, call, cmp, twin, data or {}


class Env(object):
    """what the builders share: torch, the library, the context, helpers for buffers and calls"""

    def __init__(self, torch, hf, ctx):
        self.torch, self.hf, self.ctx = torch, hf, ctx
        self.dev = torch.device("cuda", 0)
        self.keep = []

    def up(self, a):
        a = np.asarray(a)
        t = self.torch.from_numpy(np.ascontiguousarray(a.ravel(order="F"))).to(self.dev)
        self.keep.append(t)
        return t

    def inp(self, true, decoy):
        t, d = self.up(true), self.up(decoy)
        return [self.torch.empty_like(t), t, d]

    def out(self, n):
        t = self.torch.full((int(n),), FILL, dtype=self.torch.float64, device=self.dev)
        self.keep.append(t)
        return t

    def fn(self, name, argtypes, restype=ctypes.c_int):
        f = getattr(self.hf.lib(), name)
        f.argtypes, f.restype = argtypes, restype
        return f

    def check(self, rc):
        if rc != 0:
            raise RuntimeError("library error: " + self.hf.lib().hfg_last_error().decode())


V, I, L64, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
P64 = ctypes.POINTER(ctypes.c_int64)


def _blocked_orbitals(N, blocks, nocc, seed):
    rng = np.random.RandomState(seed)
    C = np.zeros((N, nocc * len(blocks)))
    for ib, idx in enumerate(blocks):
        C[np.ix_(idx, range(ib * nocc, (ib + 1) * nocc))] = rng.uniform(-1, 1, size=(len(idx), nocc))
    return np.asfortranarray(C)


def build_fock(env):
    """the Fock-side entries on the sigma_pi basis of test_gpu_parity.py, functional 101/130"""
    import common
    hf, ctx = env.hf, env.ctx
    gb, _ = common.make_bases(7, 7, 2.068, (3, 2), 2, 5, oracle=False)
    gb.compute_tei(True)
    ldft, mdft = 4 * 3 + 12, 4 * 2 + 5
    gb.upload(ldft, mdft, ctx=ctx)
    env.keep.append(gb)
    grid = hf.DFTGrid(gb, ldft, mdft)
    N, blocks = gb.Nbf(), gb.get_sym_idx(1)
    Ct, Cd = _blocked_orbitals(N, blocks, 2, 12), _blocked_orbitals(N, blocks, 2, 77)
    Pt, Pd = np.asfortranarray(Ct @ Ct.T), np.asfortranarray(Cd @ Cd.T)
    nocc = Ct.shape[1]
    x, c, thr = 101, 130, 1e-12
    flat = lambda M: np.asarray(M).ravel(order="F")
    cases = {}

    def simple(name, twin):
        f = env.fn(name, [V, V, V, V])
        P, K = env.inp(Pt, Pd), env.out(N * N)
        cases[name] = Case(name, [P], [K], lambda: env.check(f(ctx.h, gb.h, P[0].data_ptr(), K.data_ptr())), rel_cmp(1e-12),
                           lambda: [flat(twin(Pt))])
    simple("hfg_coulomb_dev", gb.coulomb)
    simple("hfg_exchange_dev", gb.exchange)

    f_occ = env.fn("hfg_exchange_occ_dev", [V, V, V, V, L64, V])
    P, C, K = env.inp(Pt, Pd), env.inp(Ct, Cd), env.out(N * N)
    cases["hfg_exchange_occ_dev"] = Case(
        "hfg_exchange_occ_dev", [P, C], [K], lambda: env.check(f_occ(ctx.h, gb.h, P[0].data_ptr(), C[0].data_ptr(), nocc, K.data_ptr())),
        rel_cmp(1e-12), lambda: [flat(gb.exchange(Pt))])

    f_xc = env.fn("hfg_xc_fock_dev", [V, V, I, I, V, V, V, D])
    P1, H1, S1 = env.inp(Pt, Pd), env.out(N * N), env.out(3)

    def xc_twin():
        H, Exc, Nel, Ekin = grid.eval_Fxc(x, c, Pt, thr)
        return [flat(H), np.array([Exc, Nel, Ekin])]
    cases["hfg_xc_fock_dev"] = Case(
        "hfg_xc_fock_dev", [P1], [H1, S1], lambda: env.check(f_xc(ctx.h, gb.h, x, c, P1[0].data_ptr(), H1.data_ptr(), S1.data_ptr(), thr)),
        rel_cmp(1e-10, "scal"), xc_twin)

    f_pol = env.fn("hfg_xc_fock_pol_dev", [V, V, I, I, V, V, V, V, V, D])
    Pa, Pb = env.inp(0.6 * Pt, 0.6 * Pd), env.inp(0.4 * Pt, 0.4 * Pd)
    Ha, Hb, S2 = env.out(N * N), env.out(N * N), env.out(3)

    def pol_twin():
        A, B, Exc, Nel, Ekin = grid.eval_Fxc_pol(x, c, 0.6 * Pt, 0.4 * Pt, thr)
        return [flat(A), flat(B), np.array([Exc, Nel, Ekin])]
    cases["hfg_xc_fock_pol_dev"] = Case(
        "hfg_xc_fock_pol_dev", [Pa, Pb], [Ha, Hb, S2],
        lambda: env.check(f_pol(ctx.h, gb.h, x, c, Pa[0].data_ptr(), Pb[0].data_ptr(), Ha.data_ptr(), Hb.data_ptr(), S2.data_ptr(), thr)),
        rel_cmp(1e-10, 1e-10, "scal"), pol_twin)

    # no host-pointer twins: the sharded step's bound, 1e-11 of the largest element (test_sharded_step_sums_to_unsharded)
    nc = int(env.fn("hfg_fock_compact_size", [V], L64)(gb.h))
    f_cmp = env.fn("hfg_fock_compact_dev", [V, V, I, I, V, V, V, D])
    P3, Fc, S3 = env.inp(Pt, Pd), env.out(nc), env.out(3)
    cases["hfg_fock_compact_dev"] = Case(
        "hfg_fock_compact_dev", [P3], [Fc, S3],
        lambda: env.check(f_cmp(ctx.h, gb.h, x, c, P3[0].data_ptr(), Fc.data_ptr(), S3.data_ptr(), thr)), rel_cmp(1e-11, 1e-11))

    rng = np.random.RandomState(5)
    H0t = gb.kinetic() + gb.nuclear()
    H0d = rng.uniform(-1, 1, (N, N))
    H0d = H0d + H0d.T
    bid = np.zeros(N, dtype=np.int32)
    for ib, b in enumerate(blocks):
        bid[b] = ib
    f_fin = env.fn("hfg_fock_finish_dev", [V, V, V, V, V, V])
    Fci, H0, Bid, F = env.inp(rng.uniform(-1, 1, nc), rng.uniform(-1, 1, nc)), env.inp(H0t, H0d), env.inp(bid, np.zeros(N, dtype=np.int32)), env.out(N * N)
    cases["hfg_fock_finish_dev"] = Case(
        "hfg_fock_finish_dev", [Fci, H0, Bid], [F],
        lambda: env.check(f_fin(ctx.h, gb.h, Fci[0].data_ptr(), H0[0].data_ptr(), Bid[0].data_ptr(), F.data_ptr())), rel_cmp(1e-11))
    return cases


def build_rs(env):
    """hfg_rs_exchange_dev on the smallest atomic basis of test_gpu_rs.py (s_only), Yukawa kernel"""
    import common
    ctx = env.ctx
    gb, _ = common.make_atomic_bases(2, 0, 0, 3, 6, oracle=False)
    gb.compute_tei(True)
    gb.compute_yukawa(0.4)
    gb.upload(ctx=ctx)
    env.keep.append(gb)
    N = gb.Nbf()
    Pt, Pd = common.random_density(N, 3, seed=11), common.random_density(N, 3, seed=78)
    f = env.fn("hfg_rs_exchange_dev", [V, V, V, V])
    P, K = env.inp(Pt, Pd), env.out(N * N)
    return {"hfg_rs_exchange_dev": Case("hfg_rs_exchange_dev", [P], [K], lambda: env.check(f(ctx.h, gb.h, P[0].data_ptr(), K.data_ptr())),
                                        rel_cmp(1e-12), lambda: [gb.rs_exchange(Pt).ravel(order="F")])}


def eig_problem(sizes):
    """blocks over a permutation of the indices; F random symmetric, well conditioned, zero between the blocks; a decoy F"""
    N = sum(sizes)
    rng = np.random.RandomState(N)
    perm = rng.permutation(N)
    blocks, o = [], 0
    for sz in sizes:
        blocks.append(np.sort(perm[o:o + sz]))
        o += sz
    mask = np.zeros((N, N), dtype=bool)
    for b in blocks:
        mask[np.ix_(b, b)] = True

    def sym(shift):
        A = rng.uniform(-1, 1, (N, N))
        return np.where(mask, A + A.T + np.diag(np.linspace(shift, shift + 50.0, N)), 0.0)
    return blocks, sym(0.0), sym(3.0)


def build_eig(env, sizes=EIG_SIZES, only=None):
    hf, ctx = env.hf, env.ctx
    blocks, Ft, Fd = eig_problem(sizes)
    N, nblk = Ft.shape[0], len(blocks)
    Xt, Xd = np.eye(N), 0.5 * np.eye(N)  # the identity restricted to the blocks; the decoy scales every level by 1/4
    ptr, idx = hf.scf._blocks(blocks)
    env.keep += [ptr, idx]
    pp, ip = ptr.ctypes.data_as(P64), idx.ctypes.data_as(P64)
    data = dict(F=Ft, blocks=blocks)
    cases = {}

    def want(name):
        return only is None or name in only

    if want("hfg_eig_gsym_sub_dev"):
        f = env.fn("hfg_eig_gsym_sub_dev", [V, L64, V, V, I, P64, P64, V, V])
        F, X, E, C = env.inp(Ft, Fd), env.inp(Xt, Xd), env.out(N), env.out(N * N)

        def twin():
            Eh, Ch = hf.scf.eig_gsym_sub(Ft, Xt, blocks, ctx=ctx)
            return [Eh, Ch.ravel(order="F")]
        cases["hfg_eig_gsym_sub_dev"] = Case(
            "hfg_eig_gsym_sub_dev", [F, X], [E, C], lambda: env.check(f(ctx.h, N, F[0].data_ptr(), X[0].data_ptr(), nblk, pp, ip, E.data_ptr(), C.data_ptr())),
            eig_cmp, twin, data)
    if want("hfg_eig_gsym_sub_sel_dev"):
        nev = 3
        K = hf.scf.eig_sel_count(blocks, nev)
        fs = env.fn("hfg_eig_gsym_sub_sel_dev", [V, L64, V, V, I, P64, P64, L64, V, V])
        F2, X2, E2, C2 = env.inp(Ft, Fd), env.inp(Xt, Xd), env.out(K), env.out(N * K)

        def sel_twin():
            Eh, Ch = hf.scf.eig_gsym_sub_sel(Ft, Xt, blocks, nev, ctx=ctx)
            return [Eh, Ch.ravel(order="F")]
        cases["hfg_eig_gsym_sub_sel_dev"] = Case(
            "hfg_eig_gsym_sub_sel_dev", [F2, X2], [E2, C2],
            lambda: env.check(fs(ctx.h, N, F2[0].data_ptr(), X2[0].data_ptr(), nblk, pp, ip, nev, E2.data_ptr(), C2.data_ptr())), eig_cmp, sel_twin, data)
    if want("hfg_eig_blocks_dev") or want("hfg_eig_assemble_dev"):
        nb = int(env.fn("hfg_eig_block_buf_size", [I, P64], L64)(nblk, pp))
        fb = env.fn("hfg_eig_blocks_dev", [V, L64, V, V, I, P64, P64, V])
        F3, X3, B3 = env.inp(Ft, Fd), env.inp(Xt, Xd), env.out(nb)
        blocks_call = lambda: env.check(fb(ctx.h, N, F3[0].data_ptr(), X3[0].data_ptr(), nblk, pp, ip, B3.data_ptr()))
        cases["hfg_eig_blocks_dev"] = Case("hfg_eig_blocks_dev", [F3, X3], [B3], blocks_call, blockbuf_cmp, None, data)
        # the assembly's inputs: the block buffers of the true and of the decoy problem
        bufs = []
        for k in (1, 2):
            F3[0].copy_(F3[k])
            X3[0].copy_(X3[k])
            env.torch.cuda.synchronize()
            blocks_call()
            ctx.synchronize()
            bufs.append(B3.clone())
        env.keep += bufs
        fa = env.fn("hfg_eig_assemble_dev", [V, L64, I, P64, P64, V, V, V])
        B4, E4, C4 = [env.torch.empty_like(bufs[0]), bufs[0], bufs[1]], env.out(N), env.out(N * N)
        cases["hfg_eig_assemble_dev"] = Case(
            "hfg_eig_assemble_dev", [B4], [E4, C4], lambda: env.check(fa(ctx.h, N, nblk, pp, ip, B4[0].data_ptr(), E4.data_ptr(), C4.data_ptr())),
            eig_cmp, None, data)
    return cases


def build_dense(env):
    """hfg_form_density_dev (order of the eigensolver's problem, four occupied) and hfg_gemm_dev (200 x 300 x 129)"""
    hf, ctx = env.hf, env.ctx
    N, nocc = sum(EIG_SIZES), 4
    rng = np.random.RandomState(9)
    Ct, Cd = rng.uniform(-1, 1, (N, N)), rng.uniform(-1, 1, (N, N))
    fd = env.fn("hfg_form_density_dev", [V, L64, L64, V, L64, V])
    C, P = env.inp(Ct, Cd), env.out(N * N)
    cases = {"hfg_form_density_dev": Case(
        "hfg_form_density_dev", [C], [P], lambda: env.check(fd(ctx.h, N, N, C[0].data_ptr(), nocc, P.data_ptr())), abs_cmp(1e-13),
        lambda: [hf.scf.form_density(Ct, nocc, ctx=ctx).ravel(order="F")])}
    m, n, k = GEMM_MNK
    At, Ad, Bt, Bd = (rng.uniform(-1, 1, s) for s in ((m, k), (m, k), (k, n), (k, n)))
    fg = env.fn("hfg_gemm_dev", [V, I, I, L64, L64, L64, V, L64, V, L64, V, L64])
    A, B, Cm = env.inp(At, Ad), env.inp(Bt, Bd), env.out(m * n)
    cases["hfg_gemm_dev"] = Case(
        "hfg_gemm_dev", [A, B], [Cm], lambda: env.check(fg(ctx.h, 0, 0, m, n, k, A[0].data_ptr(), m, B[0].data_ptr(), k, Cm.data_ptr(), m)),
        abs_cmp(1e-12 * k), lambda: [hf.scf.gemm(At, Bt, ctx=ctx).ravel(order="F")])
    return cases


# entry -> the builder that makes its case
BUILDERS = {}
for _names, _b in ((("hfg_coulomb_dev", "hfg_exchange_dev", "hfg_exchange_occ_dev", "hfg_xc_fock_dev", "hfg_xc_fock_pol_dev",
                     "hfg_fock_compact_dev", "hfg_fock_finish_dev"), build_fock),
                   (("hfg_rs_exchange_dev",), build_rs),
                   (("hfg_eig_gsym_sub_dev", "hfg_eig_gsym_sub_sel_dev", "hfg_eig_blocks_dev", "hfg_eig_assemble_dev"), build_eig),
                   (("hfg_form_density_dev", "hfg_gemm_dev"), build_dense)):
    for _n in _names:
        BUILDERS[_n] = _b


# ---- the protocol --------------------------------------------------------------------------------------------------------
class Delay(object):
    """about DELAY_TARGET_MS of device time on the current stream: torch.cuda._sleep where the installed torch has it, a chain
    of fp64 matmuls on throwaway tensors otherwise; calibrated once with events"""

    def __init__(self, torch):
        self.torch = torch
        self.sleep = getattr(torch.cuda, "_sleep", None)
        self.a = None if self.sleep else torch.rand(1024, 1024, dtype=torch.float64, device="cuda")
        self.units = 20000000 if self.sleep else 8
        self.run()  # warm-up
        ms = self.timed()
        self.units = max(1, int(self.units * DELAY_TARGET_MS / max(ms, 1e-3)))

    def run(self):
        if self.sleep:
            self.sleep(self.units)
        else:
            b = self.a
            for _ in range(self.units):
                b = (self.a @ b) * 1e-3
            del b

    def timed(self):
        t = self.torch
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        t.cuda.synchronize()
        e0.record()
        self.run()
        e1.record()
        t.cuda.synchronize()
        return e0.elapsed_time(e1)


def _host(case):
    return [o.cpu().numpy().copy() for o in case.outs]


def _set(case, which):
    """inputs <- true (1) or decoy (2), outputs <- the fill value; enqueued on the current stream"""
    for buf in case.ins:
        buf[0].copy_(buf[which])
    for o in case.outs:
        o.fill_(FILL)


def baseline(env, case, which=1):
    _set(case, which)
    env.torch.cuda.synchronize()
    case.call()
    env.ctx.synchronize()
    return _host(case)


def _verdict(case, got, ref, bitwise):
    """bitwise where the baselines repeat bitwise, else the entry's parity bound"""
    same = all(np.array_equal(a, b) for a, b in zip(got, ref))
    figs = case.cmp(got, ref, case.data)
    return dict(bitwise=same, figs=figs, ok=bool(same if bitwise else all(v < b for _, v, b in figs)))


def ordered(env, case, delay):
    """steps 2 and 3: no host synchronisation between the first decoy and the last"""
    t = env.torch
    res = [t.empty_like(o) for o in case.outs]
    _set(case, 2)
    t.cuda.synchronize()
    e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    e0.record()
    delay.run()
    e1.record()
    for buf in case.ins:
        buf[0].copy_(buf[1])
    case.call()
    for r, o in zip(res, case.outs):
        r.copy_(o)
    _set(case, 2)
    t.cuda.synchronize()
    return [r.cpu().numpy() for r in res], float(e0.elapsed_time(e1))


def protocol(env, case, kind, delay, reference=None):
    """reference: the baseline of the same case on the null-stream context (for the context that owns its stream)"""
    b1, b2 = baseline(env, case), baseline(env, case)
    bitwise = all(np.array_equal(a, b) for a, b in zip(b1, b2))
    rec = dict(entry=case.name, kind=kind, baselines_bitwise=bitwise, repeat=_verdict(case, b2, b1, bitwise))
    decoy = baseline(env, case, 2)
    rec["decoy_differs"] = not all(np.array_equal(a, b) for a, b in zip(decoy, b1))
    if case.twin is not None:
        rec["twin"] = _verdict(case, b1, case.twin(), False)
    if kind == "own":
        # the contract of a context that owns its stream is hfg_ctx_synchronize alone: after it the outputs are complete,
        # side-stream work included, to a plain copy
        if reference is not None:
            rec["own_vs_null"] = _verdict(case, b1, reference, bitwise)
    else:
        got, ms = ordered(env, case, delay)
        rec["ordered"] = _verdict(case, got, b1, bitwise)
        rec["ordered_is_decoy"] = all(np.array_equal(a, b) for a, b in zip(got, decoy))
        rec["delay_ms"] = ms
    return rec, b1


def control(env, case, delay):
    """the method has teeth: the same delay and copy-in on a SECOND stream, no event between it and the context's stream --
    the call must then see the decoys.  hfg_gemm_dev only: no iteration, nothing can spin."""
    t = env.torch
    true = baseline(env, case, 1)
    decoy = baseline(env, case, 2)
    _set(case, 2)
    t.cuda.synchronize()
    res = [t.empty_like(o) for o in case.outs]
    s2 = t.cuda.Stream()
    e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    with t.cuda.stream(s2):
        e0.record()
        delay.run()
        e1.record()
        for buf in case.ins:
            buf[0].copy_(buf[1])
    case.call()
    for r, o in zip(res, case.outs):
        r.copy_(o)
    t.cuda.synchronize()
    got = [r.cpu().numpy() for r in res]
    return dict(got_decoy=all(np.array_equal(a, b) for a, b in zip(got, decoy)),
                got_true=all(np.array_equal(a, b) for a, b in zip(got, true)), delay_ms=float(e0.elapsed_time(e1)))


def run_kind(torch, hf, setting, kind, delay, null_baselines, out):
    if kind == "torch":
        s = torch.cuda.Stream()
        cm, handle = torch.cuda.stream(s), s.cuda_stream
        assert handle != 0
    else:
        cm, handle = contextlib.nullcontext(), (0 if kind == "null" else None)
    with cm:
        ctx = hf.Context(0, stream=handle)
        if setting == "profile":
            ctx.profile(True)
        env = Env(torch, hf, ctx)
        cases = {}
        for b in (build_fock, build_rs, build_eig, build_dense):
            cases.update(b(env))
        torch.cuda.synchronize()
        ctx.synchronize()
        first = {}
        for name in entries():
            rec, first[name] = protocol(env, cases[name], kind, delay, null_baselines.get(name))
            out["records"].append(rec)
            if kind == "null":
                null_baselines[name] = first[name]
        if kind == "torch":
            out["control"] = control(env, cases["hfg_gemm_dev"], delay)
        if setting == "trd_chain":
            # a batch with a block of 1024 goes through the chain: the context gives its side stream up for good.  Then the two
            # entries that used it, again, against what this context returned while it still had it (bitwise is not asked across
            # the two code paths: the parity bound)
            giveup = build_eig(env, GIVEUP_SIZES, only=("hfg_eig_gsym_sub_dev",))["hfg_eig_gsym_sub_dev"]
            extra = [(giveup, "@giveup")] + [(cases[name], "@after_giveup") for name in AFTER_GIVEUP]
            for case, tag in extra:
                rec, b = protocol(env, case, kind, delay, null_baselines.get(case.name + tag))
                if kind == "null":
                    null_baselines[case.name + tag] = b
                rec["entry"] += tag
                if tag == "@after_giveup":
                    rec["vs_fresh"] = _verdict(case, b, first[case.name], False)
                out["records"].append(rec)
        if setting == "profile":
            ctx.synchronize()
            out["profile"][kind] = {n: list(ctx.profile_get(n)) for n in ("coulomb", "xc", "exchange", "eig_tridiag", "eig_backtransform",
                                                                         "gemm", "density", "scatter")}
        torch.cuda.synchronize()
        ctx.synchronize()
        return env, cases  # kept alive by the caller: nothing is freed while another context works


def main(setting, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import helfem_amd as hf
    out = dict(setting=setting, records=[], control=None, profile={}, tuning={r["name"]: r["value"] for r in hf.tuning_table()
                                                                              if r["name"] in SWITCHES})
    delay = Delay(torch)
    out["delay_units"] = [("torch.cuda._sleep" if delay.sleep else "fp64 matmul chain"), delay.units]
    null_baselines, alive = {}, []
    for kind in STREAM_KINDS:
        alive.append(run_kind(torch, hf, setting, kind, delay, null_baselines, out))
    json.dump(out, open(out_path, "w"))
    print("ok")


if __name__ == "__main__":
    if sys.argv[1:] == ["--plan"]:
        for sym, why in EXCLUDED.items():
            print("excluded\t%s\t%s" % (sym, why))
        for row in plan():
            print("case\t%s\t%s\t%s" % row)
        sys.exit(0)
    if len(sys.argv) != 3 or sys.argv[1] not in dict(SETTINGS):
        sys.exit("usage: stream_order_worker.py --plan | SETTING OUT.json   (SETTING: %s)" % ", ".join(n for n, _ in SETTINGS))
    try:
        main(sys.argv[1], sys.argv[2])
    except BaseException:  # the first error ends the process: nothing more is enqueued, no destructor runs on the GPU
        traceback.print_exc()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(1)
