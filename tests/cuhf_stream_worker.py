"""Worker of tests/test_gpu_cuhf_stream_order.py: the protocol of tests/test_gpu_stream_order.py for the one entry
hfg_cuhf_update_devptr (Context.cuhf_update) on the three stream kinds -- the null stream, a non-default torch stream, a context
that owns its stream.  Per kind: two synchronised baselines and one with the decoy inputs; then, on the first two kinds and
with no host synchronisation in between, a delay, device-to-device copies of the true inputs over decoys, the call, a copy of
the outputs, and decoys over inputs and outputs.  Fa and Fb are inputs and outputs at once.  A decoy is a valid input of the
same kind (another seeded problem of the same shape)."""
import contextlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, NA, NB = 257, 4, 1
STREAM_KINDS = ["null", "torch", "own"]
NAMES = ("S", "Ca", "Cb", "Fa", "Fb")


def main(out_path):
    import torch
    import helfem_amd as hf
    import rohf_restatement as rr
    import stream_order_worker as sow
    dev = lambda M: torch.from_numpy(np.asfortranarray(M).ravel(order="F").copy()).cuda()
    pbs = [rr.problem(N, NA, NB, seed) for seed in (11, 12)]  # true, decoy
    delay = sow.Delay(torch)
    out = dict(records=[], delay_min_ms=sow.DELAY_MIN_MS)
    null_baseline, alive = None, []
    for kind in STREAM_KINDS:
        if kind == "torch":
            s = torch.cuda.Stream()
            cm, handle = torch.cuda.stream(s), s.cuda_stream
        else:
            cm, handle = contextlib.nullcontext(), (0 if kind == "null" else None)
        with cm:
            ctx = hf.Context(0, stream=handle)
            src = [[dev(pb[k]) for k in NAMES] for pb in pbs]
            work = [torch.empty_like(t) for t in src[0]]
            call = lambda: ctx.cuhf_update(work[0], work[1], NA, work[2], NB, work[3], work[4])

            def baseline(which):
                for w, t in zip(work, src[which]):
                    w.copy_(t)
                torch.cuda.synchronize()
                call()
                ctx.synchronize()
                return [work[3].cpu().numpy().copy(), work[4].cpu().numpy().copy()]

            same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
            b1, b2, decoy = baseline(0), baseline(0), baseline(1)
            rec = dict(kind=kind, baselines_bitwise=same(b1, b2), decoy_differs=not same(b1, decoy),
                       changed=not same(b1, [src[0][3].cpu().numpy(), src[0][4].cpu().numpy()]))
            if kind == "null":
                null_baseline = b1
            if kind == "own":
                rec["own_vs_null"] = same(b1, null_baseline)
            else:
                res = [torch.empty_like(work[3]), torch.empty_like(work[4])]
                for w, t in zip(work, src[1]):
                    w.copy_(t)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                delay.run()
                e1.record()
                for w, t in zip(work, src[0]):
                    w.copy_(t)
                call()
                res[0].copy_(work[3])
                res[1].copy_(work[4])
                for w, t in zip(work, src[1]):
                    w.copy_(t)
                torch.cuda.synchronize()
                got = [r.cpu().numpy() for r in res]
                rec.update(ordered_bitwise=same(got, b1), ordered_is_decoy=same(got, decoy), delay_ms=float(e0.elapsed_time(e1)))
            out["records"].append(rec)
            alive.append((ctx, src, work))  # nothing is freed while another context works
            torch.cuda.synchronize()
            ctx.synchronize()
    json.dump(out, open(out_path, "w"))
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
