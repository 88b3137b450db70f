"""Set-up shared by tests/test_gpu_scf_run.py and its worker: a step object prepared the way the diatomic driver prepares
its run (src/diatomic/main.cpp:245-430 as helfem_amd/csrc/hip/scf_gpu.cpp restates it), so that run() and scf_diatomic
solve the same problem."""
import numpy as np

# the smallest bases of the SCF cases of tests/test_gpu_parity.py (H2_LDA and HeH_TPSS_diatomic)
H2 = dict(Z1=1, Z2=1, Rbond=1.4, lmmax=[4], nelem=2, nnodes=8)
HEH = dict(Z1=2, Z2=1, Rbond=1.5, lmmax=[3, 1], nelem=2, nnodes=8, M=2)
CASES = {
    "H2_HF": dict(H2, method="HF"),
    "H2_PBE": dict(H2, method="gga_x_pbe-gga_c_pbe"),
    "H2_PBE0": dict(H2, method="hyb_gga_xc_pbeh"),
    "HeH_HF": dict(HEH, method="HF"),
    "HeH_PBE": dict(HEH, method="gga_x_pbe-gga_c_pbe"),
}


def make_step(hf, kw, rank=0, nranks=1):
    """(step, S, Enucr) with the matrices set and no density: run() starts from the core guess"""
    Rh = 0.5 * kw["Rbond"]
    lval, mval = hf.lm_to_l_m(kw["lmmax"])
    bval = hf.get_grid(float(np.arccosh(40.0 / Rh)), kw["nelem"], 4, 1.0)
    basis = hf.TwoDBasis(kw["Z1"], kw["Z2"], Rh, kw["nnodes"], 5 * kw["nnodes"], bval, lval, mval, 10)
    if kw["method"] == "HF":
        x, c, kfrac, ldft, mdft = 0, 0, 1.0, 0, 0
    else:
        x, c = hf.xc_func_ids(kw["method"])
        kfrac = hf.xc_exact_exchange(x)[1]
        ldft, mdft = 4 * max(kw["lmmax"]) + 12, 4 * len(kw["lmmax"]) + 5
    basis.compute_tei(kfrac != 0.0)
    nel, M = kw["Z1"] + kw["Z2"], kw.get("M", 1)
    nela, nelb = (nel + M - 1) // 2, (nel - M + 1) // 2
    if M == 1:
        step = hf.DeviceSCFStep(basis, x, c, ldft, mdft, nela, symmetry=1, device=0, rank=rank, nranks=nranks, kfrac=kfrac)
    else:
        step = hf.DeviceUSCFStep(basis, x, c, ldft, mdft, (nela, nelb), symmetry=1, device=0, rank=rank, nranks=nranks, kfrac=kfrac)
    S = basis.overlap()
    step.set_matrices(basis.kinetic() + basis.nuclear(), hf.scf.form_Sinvh(S, False, step.blocks, ctx=step.ctx))
    return step, S, kw["Z1"] * kw["Z2"] / kw["Rbond"]
