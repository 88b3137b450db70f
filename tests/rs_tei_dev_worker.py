"""Worker of test_gpu_rs_tei_dev.py, for what depends on switches that are read once per process (HELFEM_EXL_PAIR,
HELFEM_RS_TEI).  Usage: rs_tei_dev_worker.py exchange|scf OUT.npz
  exchange: hfg_rs_exchange of a random symmetric density with host-built and with device-built tables, both kinds
  scf:      He CAM-LDA0 and He LCY-PBE through both SCF drivers; Etot of each"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import helfem_amd as hf  # noqa: E402

SCF_METHODS = ("hyb_lda_xc_cam_lda0", "hyb_gga_xc_lcy_pbe")


def small_basis():
    g = np.load(os.path.join(ROOT, "tests", "golden", "atomic_tei.npz"))
    lmax = (int(g["case_NL"]) - 1) // 2
    lval = list(range(lmax + 1))
    return g, hf.AtomicTwoDBasis(2, int(g["case_nnodes"]), int(g["case_nquad"]), g["bval"], lval, [0] * len(lval))


def exchange(out):
    ctx = hf.default_context()
    g, _ = small_basis()
    for kind, omega in (("yukawa", float(g["case_lam"])), ("erfc", float(g["case_mu"]))):
        for where in ("host", "dev"):
            _, ab = small_basis()
            ab.ctx = ctx
            ab.compute_tei(True)
            getattr(ab, "compute_" + kind)(omega, device=(where == "dev"))
            N = ab.Nbf()
            rng = np.random.RandomState(7)
            P = rng.uniform(-1, 1, (N, N))
            out["K_%s_%s" % (kind, where)] = ab.rs_exchange(P + P.T)


def scf(out):
    for method in SCF_METHODS:
        for driver in ("device", "host"):
            if driver == "host":
                os.environ["HELFEM_SCF"] = "host"  # a live switch
            else:
                os.environ.pop("HELFEM_SCF", None)
            r = hf.scf_atomic(Z=2, lmax=0, mmax=0, nelem=5, nnodes=10, method=method, convthr=1e-9, maxit=80)
            assert r["converged"], (method, driver, r)
            out["E_%s_%s" % (method, driver)] = np.array([r["Etot"]])


if __name__ == "__main__":
    out = {}
    {"exchange": exchange, "scf": scf}[sys.argv[1]](out)
    out["rs_tei"] = np.array([{r["name"]: r["value"] for r in hf.tuning_table()}["HELFEM_RS_TEI"]])
    np.savez(sys.argv[2], **out)
    print("ok")
