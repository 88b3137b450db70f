"""Set-up shared by tests/test_gpu_rs_step.py and its worker: step objects prepared the way the atomic driver prepares its
run (src/atomic/main.cpp as helfem_amd/csrc/hip/scf_gpu.cpp restates it) for the range-separated hybrids, so that run() and
scf_atomic solve the same problem."""

BASIS = dict(lmax=0, mmax=0, nelem=4, nnodes=6)
# name: (step class, driver keywords)
CASES = {
    "He_CAM-LDA0": ("DeviceSCFStep", dict(BASIS, Z=2, method="hyb_lda_xc_cam_lda0", M=1)),
    "Be_CAM-B3LYP": ("DeviceSCFStep", dict(BASIS, Z=4, method="hyb_gga_xc_cam_b3lyp", M=1)),
    "Li_CAMY-B3LYP": ("DeviceUSCFStep", dict(BASIS, Z=3, method="hyb_gga_xc_camy_b3lyp", M=2)),
    "Li_CAM-B3LYP_ROHF": ("DeviceROHFStep", dict(BASIS, Z=3, method="hyb_gga_xc_cam_b3lyp", M=-2)),
}


def make_step(hf, name, rank=0, nranks=1):
    """(step, S, Enucr) with the matrices set and no density: run() starts from the core guess"""
    cls, kw = CASES[name]
    grid = hf.atomic_grid(kw["nelem"], Rmax=40.0, igrid=4, zexp=2.0)
    lval, mval = hf.angular_basis(kw["lmax"], kw["mmax"])
    basis = hf.AtomicTwoDBasis(kw["Z"], kw["nnodes"], 5 * kw["nnodes"], grid, lval, mval)
    x, c = hf.xc_func_ids(kw["method"])
    omega, kfrac, kshort = hf.xc_exact_exchange(x)
    ldft, mdft = 4 * kw["lmax"] + 10, 4 * kw["mmax"] + 5  # the atomic driver's defaults
    basis.compute_tei(True)
    nel, M = kw["Z"], abs(kw["M"])
    nela, nelb = (nel + M - 1) // 2, (nel - M + 1) // 2
    nocc = nela if cls == "DeviceSCFStep" else (nela, nelb)
    step = getattr(hf, cls)(basis, x, c, ldft, mdft, nocc, symmetry=1, device=0, rank=rank, nranks=nranks, kfrac=kfrac,
                            kshort=kshort, omega=omega)
    S = basis.overlap()
    step.set_matrices(basis.kinetic() + basis.nuclear(), hf.scf.form_Sinvh(S, False, step.blocks, ctx=step.ctx))
    return step, S, 0.0


def run_driver(hf, name, convthr, maxit=50):
    """the atomic driver (hfg_scf_run) for the same options as make_step: core guess, symmetry 1 and NO damping of the Fock
    matrix -- the atomic program damps by 0.7 while the DIIS error is above 0.1 by default, which run() leaves to the drivers
    (it refuses dampfock != 1), so the comparison switches it off in the driver"""
    kw = dict(CASES[name][1])
    M = kw.pop("M")
    return hf.scf_run_atomic(kw.pop("Z"), kw.pop("lmax"), kw.pop("mmax"), kw.pop("nelem"), kw.pop("nnodes"), kw.pop("method"),
                             M=abs(M), restricted=1 if M < 0 else -1, dampfock=1.0, iguess=0, symmetry=1, convthr=convthr, maxit=maxit)
