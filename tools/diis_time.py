"""Times of the device-resident DIIS object and of the step objects' run() at a bench workload:
one DeviceDIIS update + solve with a full ring (low-rank blocked route) from the context's profile scopes "diis_update" and
"diis_solve" (hfg_profile_get: events on the context's stream), and energy(), the Fock build, one iteration of run() and
one step() from events recorded on the same stream.  One warm-up round with the ring full and REPEATS timed ones; prints
one JSON line.  The same stage of the driver is read from a verbose scf_diatomic run ("DIIS error ... update done in",
"DIIS solution done in").

  python tools/diis_time.py [workload]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS = 5


def timed(torch, fn):
    """device time of fn() between two events on the current stream, which is the context's"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main(workload):
    import torch
    import helfem_amd as hf
    import bench
    w = bench.WORKLOADS[workload]
    basis, bval, lval, mval, ldft, mdft = bench.build_basis(hf, w)
    kfrac = float(w.get("kfrac", 0.0))
    if kfrac == 0.0:
        basis.compute_tei(False)
    step = hf.DeviceSCFStep(basis, w["x"], w["c"], ldft, mdft, w["nocc"], symmetry=1, device=0, kfrac=kfrac, device_tei=(kfrac != 0.0))
    S = basis.overlap()
    step.set_matrices(basis.kinetic() + basis.nuclear(), hf.scf.form_Sinvh(S, False, step.blocks, ctx=step.ctx))
    diis = hf.DeviceDIIS(step.ctx, step.N, 1, order=5)
    diis.set_metric(torch.from_numpy(np.asfortranarray(S).ravel(order="F").copy()).to(step.dev), step.Sinvh)
    diis.set_blocks(step.blocks)
    step._core_guess(None, None)
    out = dict(workload=workload, Nbf=step.N, blocks=[len(b) for b in step.blocks], order=5, repeats=REPEATS)
    t = dict(update=[], solve=[], energy=[], iteration=[], fock=[])
    ctx = step.ctx

    def scope(name, fn):
        """fn() with the profile on; the time of the scope `name` it opened"""
        ctx.profile(True)
        ctx.profile_reset()
        fn()
        torch.cuda.synchronize()
        ms, calls = ctx.profile_get(name)
        ctx.profile(False)
        assert calls == 1, (name, calls)
        return ms

    def iteration(record):
        res = {}
        t0 = timed(torch, lambda: step._fock_stage(None))
        t1 = timed(torch, lambda: res.update(step.energy(0.0)))
        t2 = scope("diis_update", lambda: step._diis_update(diis, res["Etot"]))
        t3 = scope("diis_solve", lambda: step._diis_solve(diis))
        step._eig_stage(None, None)
        step._density_stage()
        if record:
            for k, v in zip(("fock", "energy", "update", "solve"), (t0, t1, t2, t3)):
                t[k].append(v)

    def whole():
        """one iteration as run() executes it, nothing between the stages"""
        step._fock_stage(None)
        res = step.energy(0.0)
        step._diis_update(diis, res["Etot"])
        step._diis_solve(diis)
        step._eig_stage(None, None)
        step._density_stage()

    for it in range(5 + 1 + REPEATS):  # five iterations fill the ring, one warms the full-ring path up
        iteration(it >= 6)
    whole()
    t["iteration"] = [timed(torch, whole) for _ in range(REPEATS)]
    out["diis_ring_size"] = diis.size
    P = step.P.clone()

    def bare():
        step.P.copy_(P)
        step.step()
    bare()
    t["step"] = [timed(torch, bare) for _ in range(REPEATS)]
    out["ms"] = {k: stats(v) for k, v in t.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "n2_pbe_nbf4230")
