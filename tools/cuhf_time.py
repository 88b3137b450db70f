"""Times of the CUHF constraint (hfg_cuhf_update_devptr) at an N2+-like shape on the bench basis:
Nbf = 4230, (na, nb) = (7, 6), the basis' own overlap matrix, seeded S-orthonormal orbitals (the beta set a perturbed rotation
of six alpha orbitals) and seeded symmetric Fock matrices.  The low-rank and the dense route alternate in one process
(HELFEM_CUHF_LOWRANK is read per call): WARMUP warm-up and ROUNDS timed rounds, device events around each call.  The dense
route of the entry also forms S^(-1/2), its partner and P, which a driver keeps from its set-up; three more rounds with the
context's profile on split it into the scopes "cuhf_dense_metric" and "cuhf_dense" (the sequence of the SCF driver proper) and
time the apply kernel ("cuhf_apply"), whose traffic is 4 N^2 doubles.  With --run: also one iteration of DeviceROHFStep.run
beside one of DeviceUSCFStep.run at the same occupations (PBE, as the bench workload).  Prints one JSON line.

  python tools/cuhf_time.py [--run] [workload]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, ROUNDS = 3, 10
NA, NB = 7, 6


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def s_orthonormal(S, V):
    """V (V^T S V)^(-1/2 by Cholesky): columns orthonormal in the metric S"""
    L = np.linalg.cholesky(V.T @ (S @ V))
    return np.linalg.solve(L, V.T).T


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main(workload, with_run):
    import torch
    import helfem_amd as hf
    import bench
    w = bench.WORKLOADS[workload]
    basis, _, _, _, ldft, mdft = bench.build_basis(hf, w)
    S = basis.overlap()
    N = S.shape[0]
    rng = np.random.RandomState(4230)
    Ca = s_orthonormal(S, rng.randn(N, NA))
    rot = np.linalg.qr(rng.randn(NB, NB))[0]
    Cb = s_orthonormal(S, Ca[:, :NB] @ rot + 0.3 * s_orthonormal(S, rng.randn(N, NB)))
    C = np.hstack([Ca, Cb])
    occ = np.linalg.eigvalsh(C.T @ S @ C)[::-1]
    dev = lambda M: torch.from_numpy(np.asfortranarray(M).ravel(order="F").copy()).cuda()
    dS, dCa, dCb = dev(S), dev(Ca), dev(Cb)
    g = torch.Generator(device="cuda").manual_seed(7)
    F0 = []
    for _ in range(2):
        A = torch.randn(N, N, dtype=torch.float64, device="cuda", generator=g)
        F0.append((0.5 * (A + A.T)).contiguous().view(-1))
    Fa, Fb = torch.empty_like(F0[0]), torch.empty_like(F0[1])
    ctx = hf.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    out = dict(workload=workload, Nbf=N, na=NA, nb=NB, warmup=WARMUP, rounds=ROUNDS, occupations=[float(x) for x in occ])

    def call(lowrank):
        os.environ["HELFEM_CUHF_LOWRANK"] = "1" if lowrank else "0"
        Fa.copy_(F0[0])
        Fb.copy_(F0[1])
        return timed(torch, lambda: ctx.cuhf_update(dS, dCa, NA, dCb, NB, Fa, Fb))

    t = dict(lowrank=[], dense=[])
    lam = {}
    for it in range(WARMUP + ROUNDS):
        for name in ("lowrank", "dense"):
            ms = call(name == "lowrank")
            if it >= WARMUP:
                t[name].append(ms)
            lam[name] = (Fa - F0[0]).cpu().numpy()
    out["routes_differ_by"] = float(np.max(np.abs(lam["lowrank"] - lam["dense"])))
    out["max_lambda"] = float(np.max(np.abs(lam["dense"])))
    scopes = {"cuhf_lowrank": [], "cuhf_apply": [], "cuhf_dense_metric": [], "cuhf_dense": []}
    ctx.profile(True)
    for _ in range(3):
        for lowrank in (True, False):
            ctx.profile_reset()
            call(lowrank)
            for name in (("cuhf_lowrank", "cuhf_apply") if lowrank else ("cuhf_dense_metric", "cuhf_dense")):
                scopes[name].append(ctx.profile_get(name)[0])
    ctx.profile(False)
    os.environ.pop("HELFEM_CUHF_LOWRANK", None)  # the step objects below run the default route
    out["ms"] = {k: stats(v) for k, v in list(t.items()) + list(scopes.items())}
    out["apply_GBps"] = 4.0 * N * N * 8 / (out["ms"]["cuhf_apply"]["median"] * 1e-3) / 1e9
    out["lowrank_faster_beyond_spread"] = out["ms"]["lowrank"]["max"] < out["ms"]["dense"]["min"]
    out["lowrank_faster_than_dense_sequence_alone"] = out["ms"]["lowrank"]["max"] < out["ms"]["cuhf_dense"]["min"]
    if with_run:
        basis.compute_tei(False)
        H0 = basis.kinetic() + basis.nuclear()
        for cls in (hf.DeviceUSCFStep, hf.DeviceROHFStep):
            step = cls(basis, w["x"], w["c"], ldft, mdft, (NA, NB), symmetry=1, device=0)
            step.set_matrices(H0, hf.scf.form_Sinvh(S, False, step.blocks, ctx=step.ctx))
            diis = hf.DeviceDIIS(step.ctx, N, 2, order=5)
            diis.set_metric(dS, step.Sinvh)
            diis.set_blocks(step.blocks)
            step._constraint_begin(S)
            step._core_guess(None, None)

            def whole():
                step._fock_stage(None)
                res = step.energy(0.0)
                step._constrain()
                step._diis_update(diis, res["Etot"])
                step._diis_solve(diis)
                step._eig_stage(None, None)
                step._density_stage()
            for _ in range(6):
                whole()
            out["ms"]["iteration_" + cls.__name__] = stats([timed(torch, whole) for _ in range(5)])
    print(json.dumps(out))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--run"]
    main(args[0] if args else "n2_pbe_nbf4230", "--run" in sys.argv[1:])
