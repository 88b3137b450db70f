"""Worker of test_gpu_exchange_batch.py, in a process of its own (the switches it is started under are read at start-up).

Usage: exchange_batch_worker.py chunk OUT.npz     the batches of ranks (2, 5, 1) and (30, 30, 10) on the sigma + pi basis
                                                  through hfg_exchange_batch, under whatever HELFEM_EXCHANGE_BATCH_CHUNK says
       exchange_batch_worker.py step OUT.npz      one DeviceUSCFStep step with a quarter of exact exchange, under whatever
                                                  HELFEM_USCF_KBATCH says
       exchange_batch_worker.py stream OUT.json   the stream-ordering protocol of tests/stream_order_worker.py (imported as
                                                  it is) for the three device-pointer entries on a non-default torch stream

The process exits non-zero at the first error and does nothing on the GPU after it."""
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA_PI = (7, 7, 2.068, (3, 2), 2, 5)  # "sigma_pi" of tests/test_gpu_parity.py
RANKS_1 = (2, 5, 1)
RANKS_SPLIT = (30, 30, 10)
NOCC = (8, 6)


def signed_density(N, rank, seed):
    """P = Q diag(s) Q^T: `rank` random orthonormal columns, signs of both kinds (all +1 only for rank 1)"""
    rng = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rng.uniform(-1, 1, (N, rank)))
    s = np.where(np.arange(rank) % 2 == 0, 1.0, -1.0) * rng.uniform(0.5, 1.5, rank)
    return np.asfortranarray((Q * s) @ Q.T)


def batch(N, ranks, seed):
    return [signed_density(N, r, seed + 10 * i) for i, r in enumerate(ranks)]


def flat(Ms):
    return np.concatenate([np.asarray(M).ravel(order="F") for M in Ms])


def sigma_pi(hf, common, ctx=None):
    gb, _ = common.make_bases(*SIGMA_PI, oracle=False)
    gb.compute_tei(True)
    gb.upload(ctx=ctx) if ctx is not None else gb.upload()
    return gb


def chunk(out_path):
    import helfem_amd as hf
    import common
    gb = sigma_pi(hf, common)
    N = gb.Nbf()
    np.savez(out_path, K1=gb.exchange_batch(batch(N, RANKS_1, 100)), K2=gb.exchange_batch(batch(N, RANKS_SPLIT, 200)),
             chunk=np.array([{r["name"]: r["value"] for r in hf.tuning_table()}["HELFEM_EXCHANGE_BATCH_CHUNK"]]))


def step(out_path):
    import torch
    import helfem_amd as hf
    import common
    gb, _ = common.make_bases(*SIGMA_PI, oracle=False)
    gb.compute_tei(True)
    ldft, mdft = 4 * 3 + 12, 4 * 2 + 5
    gb.upload(ldft, mdft)
    blocks = gb.get_sym_idx(1)
    H0, Sinvh = gb.kinetic() + gb.nuclear(), hf.scf.form_Sinvh(gb.overlap(), False, blocks)
    _, C0 = hf.scf.eig_gsym_sub(H0, Sinvh, blocks)
    res = {}
    for tag, with_C in (("C", True), ("P", False)):  # the orbitals handed over as factors, and the densities alone
        s = hf.DeviceUSCFStep(gb, 101, 130, ldft, mdft, NOCC, symmetry=1, device=0, kfrac=0.25)
        s.set_matrices(H0, Sinvh)
        Pa, Pb = hf.scf.form_density(C0, NOCC[0]), hf.scf.form_density(C0, NOCC[1])
        s.set_density(Pa, Pb, C0, C0) if with_C else s.set_density(Pa, Pb)
        s.step(None)
        torch.cuda.synchronize()
        for name in ("Fa", "Fb", "Ea", "Eb", "Ka", "Kb"):
            res[name + tag] = getattr(s, name).cpu().numpy().copy()
        res["kbatch" + tag] = np.array([s.kbatch])
    np.savez(out_path, **res)


def stream(out_path):
    import torch
    import helfem_amd as hf
    import common
    import stream_order_worker as sow
    delay = sow.Delay(torch)
    st = torch.cuda.Stream()
    assert st.cuda_stream != 0
    recs = []
    with torch.cuda.stream(st):
        ctx = hf.Context(0, stream=st.cuda_stream)
        env = sow.Env(torch, hf, ctx)
        gb = sigma_pi(hf, common, ctx)
        N = gb.Nbf()
        Pt, Pd = batch(N, RANKS_1, 100), batch(N, RANKS_1, 300)
        nP = len(RANKS_1)
        f = env.fn("hfg_exchange_batch_devptr", [sow.V, sow.V, sow.L64, sow.V, sow.V])
        P, K = env.inp(flat(Pt), flat(Pd)), env.out(nP * N * N)
        cases = [sow.Case("hfg_exchange_batch_devptr", [P], [K], lambda: env.check(f(ctx.h, gb.h, nP, P[0].data_ptr(), K.data_ptr())),
                          sow.rel_cmp(1e-12), lambda: [flat(gb.exchange_batch(Pt, ctx=ctx))])]
        # the known-factor form: two spins of different occupation
        rng = np.random.RandomState(7)
        Ct, Cd = rng.uniform(-1, 1, (2, N, N)), rng.uniform(-1, 1, (2, N, N))
        nocc = np.array(NOCC, dtype=np.int64)
        dens = lambda Cs: flat([C[:, :n] @ C[:, :n].T for C, n in zip(Cs, NOCC)])
        g = env.fn("hfg_exchange_occ_batch_devptr", [sow.V, sow.V, sow.L64, sow.V, sow.V, sow.P64, sow.L64, sow.V])
        P2, C2, K2 = env.inp(dens(Ct), dens(Cd)), env.inp(flat(Ct), flat(Cd)), env.out(2 * N * N)
        cases.append(sow.Case("hfg_exchange_occ_batch_devptr", [P2, C2], [K2],
                              lambda: env.check(g(ctx.h, gb.h, 2, P2[0].data_ptr(), C2[0].data_ptr(), nocc.ctypes.data_as(sow.P64), N,
                                                  K2.data_ptr())),
                              sow.rel_cmp(1e-12), lambda: [flat(gb.exchange_batch([M.reshape(N, N).T for M in dens(Ct).reshape(2, -1)], ctx=ctx))]))
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
        {"chunk": chunk, "step": step, "stream": stream}[sys.argv[1]](sys.argv[2])
        print("ok")
    except BaseException:  # the first error ends the process: nothing more is enqueued, no destructor runs on the GPU
        traceback.print_exc()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(1)
