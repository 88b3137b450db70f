"""Worker of test_gpu_fock_pol.py, in a process of its own.

Usage: fock_pol_worker.py stream OUT.json    the stream-ordering protocol of tests/stream_order_worker.py (imported as it is)
                                             for hfg_fock_compact_pol_devptr, hfg_fock_finish_pol_devptr and
                                             hfg_eig_gsym_sub_pair_devptr, on a context of the null stream, of a non-default
                                             torch stream and of a stream of its own
       fock_pol_worker.py repeat OUT.npz     two builds in a row at shape (a) of the test module, in the settings of this
                                             process (HELFEM_FOCK_OVERLAP is read once)

The process exits non-zero at the first error and does nothing on the GPU after it."""
import contextlib
import ctypes
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("hfg_fock_compact_pol_devptr", "hfg_fock_finish_pol_devptr", "hfg_eig_gsym_sub_pair_devptr")
EIG_SIZES = (130, 65, 3)
W = dict(Z1=7, Z2=7, Rbond=2.068, lmmax=(6, 6), nelem=3, nnodes=8)  # shape (a): the basis of tests/test_gpu_fock_skip.py


def mixed_pair(gb):
    """the polarised pair of test_gpu_fock_shapes.py::test_xc_polarised: no zero anywhere"""
    import common
    N = gb.Nbf()
    blocked = common.random_density(N, 2, seed=12, blocks=gb.get_sym_idx(1))
    Pa = np.asfortranarray(0.05 * common.random_density(N, 3, seed=11) + blocked)
    return Pa, np.asfortranarray(0.5 * Pa + 0.25 * blocked)


def build_cases(env, sow):
    """the Fock-side entries on the basis and functional of stream_order_worker.build_fock, the pair solve on its kind of
    eigenproblem with S = 1"""
    import common
    hf, ctx = env.hf, env.ctx
    V, I, L64, D, P64 = sow.V, sow.I, sow.L64, sow.D, sow.P64
    gb, _ = common.make_bases(7, 7, 2.068, (3, 2), 2, 5, oracle=False)
    gb.compute_tei(True)
    gb.upload(4 * 3 + 12, 4 * 2 + 5, ctx=ctx)
    env.keep.append(gb)
    N, blocks = gb.Nbf(), gb.get_sym_idx(1)
    Ct, Cd = sow._blocked_orbitals(N, blocks, 2, 12), sow._blocked_orbitals(N, blocks, 2, 77)
    Pt, Pd = np.asfortranarray(Ct @ Ct.T), np.asfortranarray(Cd @ Cd.T)
    x, c, thr = 101, 130, 1e-12
    cases = {}

    # no host-pointer twins: the sharded step's bound, as for hfg_fock_compact_dev and hfg_fock_finish_dev
    nc2 = int(env.fn("hfg_fock_compact_pol_size", [V], L64)(gb.h))
    f_cmp = env.fn(ENTRIES[0], [V, V, I, I, V, V, V, V, D])
    Pa, Pb, Fc, S = env.inp(0.6 * Pt, 0.6 * Pd), env.inp(0.4 * Pt, 0.4 * Pd), env.out(nc2), env.out(3)
    cases[ENTRIES[0]] = sow.Case(
        ENTRIES[0], [Pa, Pb], [Fc, S],
        lambda: env.check(f_cmp(ctx.h, gb.h, x, c, Pa[0].data_ptr(), Pb[0].data_ptr(), Fc.data_ptr(), S.data_ptr(), thr)),
        sow.rel_cmp(1e-11, 1e-11))

    rng = np.random.RandomState(5)
    H0d = rng.uniform(-1, 1, (N, N))
    bid = np.zeros(N, dtype=np.int32)
    for ib, b in enumerate(blocks):
        bid[b] = ib
    f_fin = env.fn(ENTRIES[1], [V, V, V, V, V, V, V])
    Fci, H0 = env.inp(rng.uniform(-1, 1, nc2), rng.uniform(-1, 1, nc2)), env.inp(gb.kinetic() + gb.nuclear(), H0d + H0d.T)
    Bid, Fa, Fb = env.inp(bid, np.zeros(N, dtype=np.int32)), env.out(N * N), env.out(N * N)
    cases[ENTRIES[1]] = sow.Case(
        ENTRIES[1], [Fci, H0, Bid], [Fa, Fb],
        lambda: env.check(f_fin(ctx.h, gb.h, Fci[0].data_ptr(), H0[0].data_ptr(), Bid[0].data_ptr(), Fa.data_ptr(), Fb.data_ptr())),
        sow.rel_cmp(1e-11, 1e-11))

    eblocks, Fta, Fda = sow.eig_problem(EIG_SIZES)
    Ftb, Fdb = np.where(Fta != 0.0, 0.5 * Fta + 0.25 * Fda, 0.0), np.where(Fda != 0.0, Fda - 0.5 * Fta, 0.0)
    n, nblk = Fta.shape[0], len(eblocks)
    Xt, Xd = np.eye(n), 0.5 * np.eye(n)
    ptr, idx = hf.scf._blocks(eblocks)
    env.keep += [ptr, idx]
    pp, ip = ptr.ctypes.data_as(P64), idx.ctypes.data_as(P64)
    f_eig = env.fn(ENTRIES[2], [V, L64, V, V, V, I, P64, P64, V, V, V, V])
    FA, FB, X = env.inp(Fta, Fda), env.inp(Ftb, Fdb), env.inp(Xt, Xd)
    Ea, Ca, Eb, Cb = env.out(n), env.out(n * n), env.out(n), env.out(n * n)

    def eig_twin():
        r = hf.scf.eig_gsym_sub_pair(Fta, Ftb, Xt, eblocks, ctx=ctx)
        return [r[0], r[1].ravel(order="F"), r[2], r[3].ravel(order="F")]

    def eig_cmp(outs, ref, data):
        figs = []
        for s, F in enumerate((Fta, Ftb)):
            figs += [("spin %d " % s + lab, v, b)
                     for lab, v, b in sow._eig_figs(outs[2 * s], outs[2 * s + 1].reshape((n, -1), order="F"), ref[2 * s], F)]
        return figs
    cases[ENTRIES[2]] = sow.Case(
        ENTRIES[2], [FA, FB, X], [Ea, Ca, Eb, Cb],
        lambda: env.check(f_eig(ctx.h, n, FA[0].data_ptr(), FB[0].data_ptr(), X[0].data_ptr(), nblk, pp, ip, Ea.data_ptr(),
                                Ca.data_ptr(), Eb.data_ptr(), Cb.data_ptr())), eig_cmp, eig_twin)
    return cases


def stream(out_path):
    import torch
    import helfem_amd as hf
    import stream_order_worker as sow
    delay = sow.Delay(torch)
    out, null_baselines, alive = dict(records=[]), {}, []
    for kind in sow.STREAM_KINDS:  # null, torch, own
        if kind == "torch":
            s = torch.cuda.Stream()
            cm, handle = torch.cuda.stream(s), s.cuda_stream
            assert handle != 0
        else:
            cm, handle = contextlib.nullcontext(), (0 if kind == "null" else None)
        with cm:
            ctx = hf.Context(0, stream=handle)
            env = sow.Env(torch, hf, ctx)
            cases = build_cases(env, sow)
            torch.cuda.synchronize()
            ctx.synchronize()
            for name in ENTRIES:
                rec, first = sow.protocol(env, cases[name], kind, delay, null_baselines.get(name))
                out["records"].append(rec)
                if kind == "null":
                    null_baselines[name] = first
            torch.cuda.synchronize()
            ctx.synchronize()
            alive.append((env, cases))  # nothing is freed while another context works
    json.dump(out, open(out_path, "w"))


def repeat(out_path):
    import torch
    import helfem_amd as hf
    import common
    gb, _ = common.make_bases(W["Z1"], W["Z2"], W["Rbond"], W["lmmax"], W["nelem"], W["nnodes"], oracle=False)
    gb.compute_tei(False)
    gb.upload(4 * max(W["lmmax"]) + 12, 4 * len(W["lmmax"]) + 5)
    L, V = hf.lib(), ctypes.c_void_p
    dev = lambda M: torch.from_numpy(np.asfortranarray(M).ravel(order="F").copy()).cuda()
    Pa, Pb = (dev(M) for M in mixed_pair(gb))
    Fc = torch.zeros(int(L.hfg_fock_compact_pol_size(gb.h)), dtype=torch.float64, device="cuda")
    scal = torch.zeros(3, dtype=torch.float64, device="cuda")
    res = {}
    for k in "12":
        torch.cuda.synchronize()
        rc = L.hfg_fock_compact_pol_devptr(gb.ctx.h, gb.h, 101, 130, V(Pa.data_ptr()), V(Pb.data_ptr()), V(Fc.data_ptr()), V(scal.data_ptr()), 1e-12)
        if rc != 0:
            raise RuntimeError(L.hfg_last_error().decode())
        gb.ctx.synchronize()
        res["Fc" + k], res["scal" + k] = Fc.cpu().numpy().copy(), scal.cpu().numpy().copy()
    np.savez(out_path, **res)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        {"stream": stream, "repeat": repeat}[sys.argv[1]](sys.argv[2])
        print("ok")
    except BaseException:  # the first error ends the process: nothing more is enqueued, no destructor runs on the GPU
        traceback.print_exc()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(1)
