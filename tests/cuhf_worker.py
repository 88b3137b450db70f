"""Worker of tests/test_gpu_cuhf.py: hfg_cuhf_update_devptr (Context.cuhf_update) on every shape of
tests/rohf_restatement.py under the switches of this process's environment (HELFEM_CUHF_LOWRANK is read per call; the
child process keeps the parent's setting out of the picture).  Writes one .npz: per shape the two differences Fa_out - Fa_in
and Fb_in - Fb_out, whether a second context gave the same bits, whether the outputs are bitwise the inputs, and the update
with Ca_o replaced by Ca_o U."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def dev(torch, M):
    return torch.from_numpy(np.asfortranarray(M).ravel(order="F").copy()).cuda()


def host(t, N):
    return t.cpu().numpy().reshape((N, N), order="F")


def update(torch, ctx, pb, Ca=None):
    """(Fa_out, Fb_out) as numpy matrices"""
    N = pb["N"]
    S, Fa, Fb = dev(torch, pb["S"]), dev(torch, pb["Fa"]), dev(torch, pb["Fb"])
    dCa, dCb = dev(torch, pb["Ca"] if Ca is None else Ca), dev(torch, pb["Cb"])
    torch.cuda.synchronize()
    ctx.cuhf_update(S, dCa, pb["na"], dCb, pb["nb"], Fa, Fb)
    ctx.synchronize()
    torch.cuda.synchronize()
    return host(Fa, N), host(Fb, N)


def main(out_path):
    import torch
    import helfem_amd as hf
    import rohf_restatement as rr
    out = {"switch": np.array([{r["name"]: r["value"] for r in hf.tuning_table()}["HELFEM_CUHF_LOWRANK"] == "on"])}
    first, second = hf.Context(0), hf.Context(0)  # each with a stream of its own
    for N, (na, nb) in rr.SHAPES:
        pb = rr.case(N, na, nb)["pb"]
        key = "%d_%d_%d" % (N, na, nb)
        Fa, Fb = update(torch, first, pb)
        Fa2, Fb2 = update(torch, second, pb)
        out[key + "_lamA"] = Fa - pb["Fa"]
        out[key + "_lamB"] = pb["Fb"] - Fb
        out[key + "_untouched"] = np.array([np.array_equal(Fa, pb["Fa"]) and np.array_equal(Fb, pb["Fb"])])
        out[key + "_same_bits"] = np.array([np.array_equal(Fa, Fa2) and np.array_equal(Fb, Fb2)])
        if na > 1:
            U = np.linalg.qr(np.random.RandomState(7 + N + na).randn(na, na))[0]
            Fr, _ = update(torch, first, pb, Ca=pb["Ca"] @ U)
            out[key + "_lamA_rotated"] = Fr - pb["Fa"]
    np.savez(out_path, **out)
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
