"""Worker of test_gpu_exchange_mix.py, in a process of its own.

Usage: exchange_mix_worker.py figures OUT.json   every shape x kernel kind x (alpha, beta): the mixed table against its NumPy
                                                 restatement, padding, rebuild, repeated call; K against the two builds and
                                                 the oracle; batch against single; invalidation; shards
       exchange_mix_worker.py stream OUT.json    the stream-ordering protocol of tests/stream_order_worker.py (imported as it
                                                 is) for the three device-pointer entries on a non-default torch stream

The process exits non-zero at the first error and does nothing on the GPU after it."""
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
# (elements, nodes, lmax, mmax)
SHAPES = [(1, 4, 1, 1), (2, 5, 1, 1), (3, 4, 1, 1), (3, 15, 2, 1)]
WEIGHTS = [(0.19, 0.46), (0.25, -0.25), (0.3, 0.0)]  # CAM-B3LYP-like, CAM-LDA0, no screened term
RANKS = (1, 3, 5)
OMEGA = 0.33


def orthonormal(N, rank, seed):
    Q, _ = np.linalg.qr(np.random.RandomState(seed).uniform(-1, 1, (N, rank)))
    return np.asfortranarray(Q)


def flat(Ms):
    return np.concatenate([np.asarray(M).ravel(order="F") for M in Ms])


def table_figures(gb, t, alpha, beta):
    """largest deviation of the device table from the restatement in units of 4 eps (|alpha coulomb| + |beta ratio screened|)
    (one rounding each for the outer products, the scalings and the sum, fused or not), and whether every entry that the
    restatement has exactly zero -- the padding -- is exactly zero on the device"""
    want, mag = t.mixed_blocks(alpha, beta), t.magnitude_blocks(alpha, beta)
    worst, zeros_ok, nz = 0.0, True, 0
    dev = {}
    for L in range(t.NL):
        for e in range(t.E):
            for f in range(t.E):
                d = gb.mixed_table(L, e, f)
                dev[(L, e, f)] = d
                m = mag[L][e][f]
                pad = m == 0.0
                zeros_ok = zeros_ok and bool(np.all(d[pad] == 0.0))
                nz += int(np.count_nonzero(pad))
                if np.any(~pad):
                    worst = max(worst, float(np.max(np.abs(d - want[L][e][f])[~pad] / (4 * EPS * m[~pad]))))
    return worst, zeros_ok, nz, dev


def figures(out_path):
    import torch
    import helfem_amd as hf
    import common
    import exchange_mix_restatement as xr
    ctx = hf.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    res = []
    for E, p, lmax, mmax in SHAPES:
        for kind in (1, 2):
            gb, t = xr.make(hf, 4, lmax, mmax, E, p, kind, OMEGA)
            _, ob = common.make_atomic_bases(Z=4, lmax=lmax, mmax=mmax, nelem=E, nnodes=p, product=False)
            ob.compute_tei(True)
            (ob.compute_yukawa if kind == 1 else ob.compute_erfc)(OMEGA)
            gb.upload(ctx=ctx)
            N = gb.Nbf()
            Cs = [orthonormal(N, r, 10 * r + E) for r in RANKS]
            Ps = [np.asfortranarray(C @ C.T) for C in Cs]
            Kc, Ks = [gb.exchange(P) for P in Ps], [gb.rs_exchange(P) for P in Ps]
            Koc, Kos = [ob.exchange(P) for P in Ps], [ob.rs_exchange(P) for P in Ps]
            for alpha, beta in WEIGHTS:
                rec = dict(shape=[E, p, lmax, mmax], kind=kind, alpha=alpha, beta=beta, N=N)
                ctx.profile(True)
                ctx.profile_reset()
                assert gb.mix_exchange_tables(alpha, beta, ctx=ctx)
                # every block of every slot, at every shape: 3 x 15 is the one whose blocks (50625 entries, an odd number) are
                # written in more than one slice and start at addresses that are not 16-byte aligned
                worst, zeros_ok, nz, dev = table_figures(gb, t, alpha, beta)
                assert len(dev) == t.NL * E * E
                rec.update(table_units=worst, padding_zero=zeros_ok, padding_entries=nz)
                assert gb.mix_exchange_tables(alpha, beta, ctx=ctx)  # same values: nothing to do
                ctx.synchronize()
                rec["builds_after_repeat"] = ctx.profile_get("exchange_mix_tables")[1]
                rec["repeat_unchanged"] = all(np.array_equal(gb.mixed_table(*k), v) for k, v in dev.items())
                ctx.profile(False)
                # K: with and without the orbitals, against the two builds and the oracle
                rec["K"] = []
                singles, singles_p = [], []
                for r, C, P, kc, ks, koc, kos in zip(RANKS, Cs, Ps, Kc, Ks, Koc, Kos):
                    oracle = alpha * koc + beta * kos
                    two = alpha * kc + beta * ks
                    dP, dC = torch.from_numpy(flat([P])).cuda(), torch.from_numpy(flat([np.hstack([C, np.zeros((N, N - r))])])).cuda()
                    k_p = gb.mix_exchange_torch(dP, ctx=ctx).cpu().numpy().reshape(N, N).T
                    k_c = gb.mix_exchange_torch(dP, dC, r, ctx=ctx).cpu().numpy().reshape(N, N).T
                    singles.append(k_c)
                    singles_p.append(k_p)
                    rec["K"].append(dict(rank=r, scale=float(np.max(np.abs(oracle))), two=float(np.max(np.abs(two - oracle))),
                                         mix_P=float(np.max(np.abs(k_p - oracle))), mix_C=float(np.max(np.abs(k_c - oracle))),
                                         mix_vs_two=float(np.max(np.abs(k_c - two))), host=bool(np.array_equal(gb.mix_exchange(P), k_p))))
                # the batch entry: bitwise the single entry, per density
                dPs = torch.from_numpy(flat(Ps)).cuda()
                dCs = torch.from_numpy(flat([np.hstack([C, np.zeros((N, N - r))]) for C, r in zip(Cs, RANKS)])).cuda()
                kb = gb.mix_exchange_torch(dPs, dCs, list(RANKS), ctx=ctx).cpu().numpy().reshape(len(RANKS), N, N).transpose(0, 2, 1)
                rec["batch_bitwise"] = all(np.array_equal(kb[i], singles[i]) for i in range(len(RANKS)))
                kb2 = gb.mix_exchange_torch(dPs, ctx=ctx).cpu().numpy().reshape(len(RANKS), N, N).transpose(0, 2, 1)
                rec["batch_without_orbitals_bitwise"] = all(np.array_equal(kb2[i], singles_p[i]) for i in range(len(RANKS)))
                # a second build from scratch: bitwise the first
                gb.upload(ctx=ctx)
                try:
                    gb.mix_exchange(Ps[0])
                    rec["gone_after_upload"] = False
                except RuntimeError as err:
                    rec["gone_after_upload"] = "have not been built" in str(err)
                assert gb.mix_exchange_tables(alpha, beta, ctx=ctx)
                rec["rebuild_bitwise"] = all(np.array_equal(gb.mixed_table(*k), v) for k, v in dev.items())
                res.append(rec)
            if (E, p) == (2, 5):
                # shards: the partial matrices of two ranks sum to the whole (the pair path deals the table slots out)
                dP = torch.from_numpy(flat([Ps[1]])).cuda()
                whole = gb.mix_exchange_torch(dP, ctx=ctx).cpu().numpy()
                acc = np.zeros_like(whole)
                for rk in range(2):
                    ctx.set_shard(rk, 2)
                    acc += gb.mix_exchange_torch(dP, ctx=ctx).cpu().numpy()
                ctx.set_shard(0, 1)
                res.append(dict(shards=True, kind=kind, err=float(np.max(np.abs(acc - whole))), scale=float(np.max(np.abs(whole))), N=N))
                # new screened tables: the mixed set goes with the old ones, before and after the upload that follows
                stale = gb.mix_exchange(Ps[0])
                getattr(gb, "compute_yukawa" if kind == 1 else "compute_erfc")(2 * OMEGA)
                outcome = []
                for again in (False, True):
                    if again:
                        gb.upload(ctx=ctx)
                    try:
                        gb.mix_exchange(Ps[0])
                        outcome.append("numbers")
                    except RuntimeError as err:
                        outcome.append("refused" if "have not been built" in str(err) else str(err))
                assert gb.mix_exchange_tables(*WEIGHTS[0], ctx=ctx)
                fresh = gb.mix_exchange(Ps[0])
                res.append(dict(invalidation=True, kind=kind, outcome=outcome, changed=float(np.max(np.abs(fresh - stale)))))
    json.dump(res, open(out_path, "w"))


def stream(out_path):
    import torch
    import helfem_amd as hf
    import exchange_mix_restatement as xr
    import stream_order_worker as sow
    delay = sow.Delay(torch)
    st = torch.cuda.Stream()
    assert st.cuda_stream != 0
    recs = []
    alpha, beta = WEIGHTS[0]
    with torch.cuda.stream(st):
        ctx = hf.Context(0, stream=st.cuda_stream)
        env = sow.Env(torch, hf, ctx)
        gb, _ = xr.make(hf, 4, 1, 1, 3, 6, 2, OMEGA)
        gb.upload(ctx=ctx)
        assert gb.mix_exchange_tables(alpha, beta, ctx=ctx)
        N = gb.Nbf()
        nocc = np.array([3, 2], dtype=np.int64)

        def dens(Cs):
            return [np.asfortranarray(C[:, :n] @ C[:, :n].T) for C, n in zip(Cs, nocc)]
        Ct = [np.hstack([orthonormal(N, n, 3 + n), np.zeros((N, N - n))]) for n in nocc]
        Cd = [np.hstack([orthonormal(N, n, 30 + n), np.zeros((N, N - n))]) for n in nocc]
        want1 = lambda: [flat([gb.mix_exchange(dens(Ct)[0])])]
        want2 = lambda: [flat([gb.mix_exchange(P) for P in dens(Ct)])]
        f1 = env.fn("hfg_mix_exchange_devptr", [sow.V, sow.V, sow.V, sow.V])
        f2 = env.fn("hfg_mix_exchange_occ_devptr", [sow.V, sow.V, sow.V, sow.V, sow.L64, sow.V])
        f3 = env.fn("hfg_mix_exchange_occ_batch_devptr", [sow.V, sow.V, sow.L64, sow.V, sow.V, sow.P64, sow.L64, sow.V])
        P1, K1 = env.inp(flat(dens(Ct)[:1]), flat(dens(Cd)[:1])), env.out(N * N)
        P2, C2, K2 = env.inp(flat(dens(Ct)[:1]), flat(dens(Cd)[:1])), env.inp(flat(Ct[:1]), flat(Cd[:1])), env.out(N * N)
        P3, C3, K3 = env.inp(flat(dens(Ct)), flat(dens(Cd))), env.inp(flat(Ct), flat(Cd)), env.out(2 * N * N)
        cases = [
            sow.Case("hfg_mix_exchange_devptr", [P1], [K1], lambda: env.check(f1(ctx.h, gb.h, P1[0].data_ptr(), K1.data_ptr())),
                     sow.rel_cmp(1e-12), want1),
            sow.Case("hfg_mix_exchange_occ_devptr", [P2, C2], [K2],
                     lambda: env.check(f2(ctx.h, gb.h, P2[0].data_ptr(), C2[0].data_ptr(), int(nocc[0]), K2.data_ptr())), sow.rel_cmp(1e-12), want1),
            sow.Case("hfg_mix_exchange_occ_batch_devptr", [P3, C3], [K3],
                     lambda: env.check(f3(ctx.h, gb.h, 2, P3[0].data_ptr(), C3[0].data_ptr(), nocc.ctypes.data_as(sow.P64), N, K3.data_ptr())),
                     sow.rel_cmp(1e-12), want2),
        ]
        torch.cuda.synchronize()
        ctx.synchronize()
        for case in cases:
            rec, _ = sow.protocol(env, case, "torch", delay)
            recs.append(rec)
            torch.cuda.synchronize()
            ctx.synchronize()
    json.dump(recs, open(out_path, "w"))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        {"figures": figures, "stream": stream}[sys.argv[1]](sys.argv[2])
        print("ok")
    except BaseException:  # the first error ends the process: nothing more is enqueued, no destructor runs on the GPU
        traceback.print_exc()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(1)
