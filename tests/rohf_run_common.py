"""Set-up shared by tests/test_gpu_rohf_run.py and its worker: step objects prepared the way the drivers prepare their runs,
so that DeviceROHFStep.run and scf_atomic / scf_diatomic with M < 0 solve the same problem.  Bases: Li_ROHF and N_ROHF of
tests/test_gpu_parity.py and the HeH doublet of tests/scf_run_common.py."""
import numpy as np

import scf_run_common as diatomic

# name: (program, driver keywords with M > 0, literature ROHF energy and its tolerance or None)
CASES = {
    "Li": ("atomic", dict(Z=3, lmax=0, mmax=0, nelem=5, nnodes=15, method="HF", M=2), -7.4327269, 1e-6),
    "N": ("atomic", dict(Z=7, lmax=1, mmax=1, nelem=5, nnodes=12, method="HF", M=4), -54.400934, 2e-6),
    "HeH": ("diatomic", dict(diatomic.HEH, method="HF"), None, None),
}


def make_step(hf, name, cls=None, rank=0, nranks=1):
    """(step, S, Enucr) with the matrices set and no density: run() starts from the core guess.  cls: the step class
    (default DeviceROHFStep)"""
    program, kw = CASES[name][:2]
    cls = cls or hf.DeviceROHFStep
    if program == "atomic":
        grid = hf.atomic_grid(kw["nelem"], Rmax=40.0, igrid=4, zexp=2.0)
        lval, mval = hf.angular_basis(kw["lmax"], kw["mmax"])
        basis = hf.AtomicTwoDBasis(kw["Z"], kw["nnodes"], 5 * kw["nnodes"], grid, lval, mval)
        nel, Enucr = kw["Z"], 0.0
    else:
        Rh = 0.5 * kw["Rbond"]
        lval, mval = hf.lm_to_l_m(kw["lmmax"])
        grid = hf.get_grid(float(np.arccosh(40.0 / Rh)), kw["nelem"], 4, 1.0)
        basis = hf.TwoDBasis(kw["Z1"], kw["Z2"], Rh, kw["nnodes"], 5 * kw["nnodes"], grid, lval, mval, 10)
        nel, Enucr = kw["Z1"] + kw["Z2"], kw["Z1"] * kw["Z2"] / kw["Rbond"]
    basis.compute_tei(True)
    M = kw["M"]
    nela, nelb = (nel + M - 1) // 2, (nel - M + 1) // 2
    step = cls(basis, 0, 0, 0, 0, (nela, nelb), symmetry=1, device=0, rank=rank, nranks=nranks, kfrac=1.0)
    S = basis.overlap()
    step.set_matrices(basis.kinetic() + basis.nuclear(), hf.scf.form_Sinvh(S, False, step.blocks, ctx=step.ctx))
    return step, S, Enucr


def driver_keywords(name):
    """the driver's keywords of the restricted open-shell run: M < 0"""
    kw = dict(CASES[name][1])
    kw["M"] = -kw["M"]
    return kw
