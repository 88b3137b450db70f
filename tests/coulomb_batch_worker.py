"""Worker of test_gpu_coulomb_batch.py, in a process of its own.

Usage: coulomb_batch_worker.py stream OUT.json       the stream-ordering protocol of tests/stream_order_worker.py (imported
                                                     as it is) for hfg_coulomb_batch_devptr on a non-default torch stream
       coulomb_batch_worker.py ownership OUT.npz     a batched call, the basis destroyed, another basis of a different
                                                     size, a batched call on it

The process exits non-zero at the first error and does nothing on the GPU after it."""
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_STREAM = 17  # one full column tile of the matrix-core kernel and a remainder
DIATOMIC_1 = (1, 1, 1.4, (2, 1), 3, 6)
DIATOMIC_2 = (1, 1, 1.4, (1,), 2, 5)
NP_OWN = (9, 5)


def symmetric_batch(N, nP, seed):
    rng = np.random.RandomState(seed)
    A = rng.uniform(-1, 1, (nP, N, N))
    return A + A.transpose(0, 2, 1)


def flat(Ms):
    """the layout of hfg_coulomb_batch: one matrix after the other, each column by column"""
    return np.concatenate([np.asarray(M).ravel(order="F") for M in Ms])


def stream(out_path):
    import torch
    import helfem_amd as hf
    import common
    import stream_order_worker as sow
    delay = sow.Delay(torch)
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    with torch.cuda.stream(s):
        ctx = hf.Context(0, stream=s.cuda_stream)
        env = sow.Env(torch, hf, ctx)
        gb, _ = common.make_bases(*DIATOMIC_1, oracle=False)
        gb.compute_tei(True)
        gb.upload(ctx=ctx)
        N = gb.Nbf()
        Pt, Pd = symmetric_batch(N, NP_STREAM, 21), symmetric_batch(N, NP_STREAM, 22)
        f = env.fn("hfg_coulomb_batch_devptr", [sow.V, sow.V, sow.L64, sow.V, sow.V])
        P, J = env.inp(flat(Pt), flat(Pd)), env.out(NP_STREAM * N * N)
        case = sow.Case("hfg_coulomb_batch_devptr", [P], [J], lambda: env.check(f(ctx.h, gb.h, NP_STREAM, P[0].data_ptr(), J.data_ptr())),
                        sow.rel_cmp(1e-12), lambda: [flat(gb.coulomb_batch(Pt, ctx=ctx))])
        torch.cuda.synchronize()
        ctx.synchronize()
        rec, _ = sow.protocol(env, case, "torch", delay)
        torch.cuda.synchronize()
        ctx.synchronize()
    json.dump(rec, open(out_path, "w"))


def ownership(out_path):
    import helfem_amd as hf
    import common
    res = {}
    ctx = hf.default_context()
    for tag, shape, nP in (("1", DIATOMIC_1, NP_OWN[0]), ("2", DIATOMIC_2, NP_OWN[1])):
        gb, _ = common.make_bases(*shape, oracle=False)
        gb.compute_tei(True)
        gb.upload(ctx=ctx)
        Ps = symmetric_batch(gb.Nbf(), nP, 31)
        res["J" + tag] = gb.coulomb_batch(Ps)
        res["W" + tag] = gb.coulomb_energy_matrix(Ps)
        res["S" + tag] = np.array([gb.coulomb(P) for P in Ps])
        del gb  # hfg_basis_destroy: the table set and its workspaces go
    np.savez(out_path, **res)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        {"stream": stream, "ownership": ownership}[sys.argv[1]](sys.argv[2])
        print("ok")
    except BaseException:  # the first error ends the process: nothing more is enqueued, no destructor runs on the GPU
        traceback.print_exc()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(1)
