"""helfem_amd — MI355X-native (gfx950) implementation of HelFEM's SCF hot path.

Thin ctypes binding over the C ABI of include/helfem_gpu.h (helfem_amd/lib/libhelfem_amd.so).  The
class and method names mirror the reference's C++ interface for this path so that tests and drivers
read like the reference's own code:

    reference (C++)                                   here
    ------------------------------------------------  ---------------------------------------------
    diatomic::basis::TwoDBasis(Z1,Z2,Rhalf,poly,      TwoDBasis(Z1,Z2,Rhalf,nnodes,nquad,bval,lval,mval,lpad)
        n_quad,bval,lval,mval,lpad)   basis.cpp:307
    basis.overlap()/kinetic()/nuclear()               same
    basis.compute_tei(exchange)        basis.cpp:1166  same
    basis.coulomb(P) / exchange(P)     basis.cpp:1359  same (numpy in / numpy out)
    (no counterpart)                                   basis.coulomb_batch(Ps) / coulomb_energy_matrix(Ps)
    dftgrid::DFTGrid(&basis,ldft,mdft).eval_Fxc(...)  DFTGrid(basis,ldft,mdft).eval_Fxc(x_func,c_func,P,thr)
    scf::eig_gsym / eig_gsym_sub / form_density       scf.eig_gsym / scf.eig_gsym_sub / scf.form_density

There is no CPU fallback: every compute call needs a gfx950 device and raises RuntimeError otherwise.
Matrices are numpy float64 arrays in Fortran (column-major) order, i.e. arma::mat memory.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("HELFEM_AMD_LIB") or os.path.join(_HERE, "lib", "libhelfem_amd.so")  # HELFEM_AMD_LIB: A/B builds (tools/ab_build.py)
_lib = None

c_double_p = ctypes.POINTER(ctypes.c_double)
c_int_p = ctypes.POINTER(ctypes.c_int)
c_i64_p = ctypes.POINTER(ctypes.c_int64)


class hfg_diatomic_desc(ctypes.Structure):
    _fields_ = [("Z1", ctypes.c_int), ("Z2", ctypes.c_int), ("Rhalf", ctypes.c_double), ("primbas", ctypes.c_int),
                ("nnodes", ctypes.c_int), ("nquad", ctypes.c_int), ("bval", c_double_p), ("nbval", ctypes.c_int),
                ("lval", c_int_p), ("mval", c_int_p), ("nang", ctypes.c_int), ("lpad", ctypes.c_int)]


class hfg_model_pot(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("Z", ctypes.c_int), ("d", ctypes.c_double), ("H", ctypes.c_double)]


class hfg_atomic_desc(ctypes.Structure):
    _fields_ = [("Z", ctypes.c_int), ("primbas", ctypes.c_int), ("nnodes", ctypes.c_int), ("nquad", ctypes.c_int),
                ("bval", c_double_p), ("nbval", ctypes.c_int), ("lval", c_int_p), ("mval", c_int_p),
                ("nang", ctypes.c_int)]


class hfg_atomic_desc_ex(ctypes.Structure):
    _fields_ = [("base", hfg_atomic_desc), ("finitenuc", ctypes.c_int), ("Rrms", ctypes.c_double), ("zeroder", ctypes.c_int),
                ("Zl", ctypes.c_int), ("Zr", ctypes.c_int), ("Rmid", ctypes.c_double)]


class hfg_scf_options(ctypes.Structure):
    """hfg_scf_options of include/helfem_gpu.h, field by field"""
    _fields_ = [("program", ctypes.c_int), ("Z1", ctypes.c_int), ("Z2", ctypes.c_int), ("Rbond", ctypes.c_double),
                ("nela", ctypes.c_int), ("nelb", ctypes.c_int), ("Q", ctypes.c_int), ("M", ctypes.c_int),
                ("lmmax", ctypes.c_int * 16), ("nlm", ctypes.c_int), ("lmax", ctypes.c_int), ("mmax", ctypes.c_int),
                ("lpad", ctypes.c_int), ("Rmax", ctypes.c_double), ("grid", ctypes.c_int), ("zexp", ctypes.c_double),
                ("nelem", ctypes.c_int), ("nnodes", ctypes.c_int), ("nquad", ctypes.c_int), ("maxit", ctypes.c_int),
                ("convthr", ctypes.c_double), ("diag", ctypes.c_int), ("method", ctypes.c_char * 128), ("ldft", ctypes.c_int),
                ("mdft", ctypes.c_int), ("dftthr", ctypes.c_double), ("restricted", ctypes.c_int), ("symmetry", ctypes.c_int),
                ("primbas", ctypes.c_int), ("diiseps", ctypes.c_double), ("diisthr", ctypes.c_double), ("diisorder", ctypes.c_int),
                ("iguess", ctypes.c_int), ("x_pars", ctypes.c_void_p), ("n_x_pars", ctypes.c_int), ("c_pars", ctypes.c_void_p),
                ("n_c_pars", ctypes.c_int), ("maverage", ctypes.c_int), ("dampfock", ctypes.c_double), ("dampthr", ctypes.c_double),
                ("save", ctypes.c_char * 512), ("load", ctypes.c_char * 512), ("Ez", ctypes.c_double), ("Qzz", ctypes.c_double),
                ("Bz", ctypes.c_double), ("finitenuc", ctypes.c_int), ("readocc", ctypes.c_int), ("occs", ctypes.c_void_p),
                ("occ_rows", ctypes.c_int), ("occ_cols", ctypes.c_int), ("perturb", ctypes.c_double), ("iconf", ctypes.c_int),
                ("zeroder", ctypes.c_int), ("verbose", ctypes.c_int)]


class hfg_scf_result(ctypes.Structure):
    _fields_ = [("Etot", ctypes.c_double), ("Ekin", ctypes.c_double), ("Epot", ctypes.c_double), ("Enucr", ctypes.c_double),
                ("Ecoul", ctypes.c_double), ("Exx", ctypes.c_double), ("Exc", ctypes.c_double), ("iterations", ctypes.c_int),
                ("converged", ctypes.c_int), ("nela", ctypes.c_int), ("nelb", ctypes.c_int), ("Nbf", ctypes.c_int64),
                ("tJ", ctypes.c_double), ("tK", ctypes.c_double), ("tXC", ctypes.c_double), ("tdiag", ctypes.c_double)]


class hfg_scf_atomic_extras(ctypes.Structure):
    _fields_ = [("Rrms", ctypes.c_double), ("conf_N", ctypes.c_int), ("conf_R", ctypes.c_double),
                ("conf_barrier", ctypes.c_double), ("shift_conf", ctypes.c_double), ("add_conf", ctypes.c_int),
                ("Zl", ctypes.c_int), ("Zr", ctypes.c_int), ("Rmid", ctypes.c_double), ("nelem0", ctypes.c_int),
                ("grid0", ctypes.c_int), ("zexp0", ctypes.c_double), ("Econf", ctypes.c_double)]


def lib():
    """Load the native library (fails loudly if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError("%s is missing: run `python -m helfem_amd.build` (or __graft_entry__.build()) first; "
                               "there is no Python/CPU fallback for the hot path" % _LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64/libhsa-runtime.  If this library
        # (linked against /opt/rocm) is loaded first and torch afterwards, torch reports "No HIP GPUs are
        # available"; loading torch first makes both resolve to the same runtime (same SONAME).  torch is only
        # plumbing here (HBM buffers, streams, torch.distributed), so import it first when it is installed.
        if os.environ.get("HELFEM_NO_TORCH", "0") != "1":
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        L = ctypes.CDLL(_LIB_PATH)
        L.hfg_last_error.restype = ctypes.c_char_p
        L.hfg_version.restype = ctypes.c_char_p
        L.hfg_gaunt_coefficient.restype = ctypes.c_double
        L.hfg_gaunt_coefficient.argtypes = [ctypes.c_int] * 6
        L.hfg_modified_gaunt_coefficient.restype = ctypes.c_double
        L.hfg_modified_gaunt_coefficient.argtypes = [ctypes.c_int] * 6
        L.hfg_theta_lm.restype = ctypes.c_double
        L.hfg_theta_lm.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double]
        L.hfg_legendre_PQ.restype = None
        L.hfg_legendre_PQ.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, c_double_p, c_double_p]
        for nm in ("hfg_bessel_il", "hfg_bessel_kl"):
            getattr(L, nm).restype = ctypes.c_double
            getattr(L, nm).argtypes = [ctypes.c_double, ctypes.c_int]
        L.hfg_erfc_phi.restype = ctypes.c_double
        L.hfg_erfc_phi.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_double]
        L.hfg_compute_rs_tei.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
        L.hfg_compute_rs_tei_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
        L.hfg_rs_special_dev.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, ctypes.c_int64, c_double_p]
        L.hfg_set_erfc_binomial_mode.restype = None
        L.hfg_set_erfc_binomial_mode.argtypes = [ctypes.c_int]
        L.hfg_model_potential.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(hfg_model_pot),
                                          ctypes.POINTER(hfg_model_pot), c_double_p]
        L.hfg_chebyshev_rule.restype = None
        L.hfg_chebyshev_rule.argtypes = [ctypes.c_int, c_double_p, c_double_p]
        L.hfg_lobatto_nodes.restype = None
        L.hfg_lobatto_nodes.argtypes = [ctypes.c_int, c_double_p]
        L.hfg_radial_grid.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_double_p]
        L.hfg_basis_confinement.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                            ctypes.c_double, c_double_p]
        L.hfg_atomic_grid.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_double,
                                      ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_double, ctypes.c_int, ctypes.c_double, c_double_p, c_int_p]
        L.hfg_scf_options_check_ex.argtypes = [ctypes.POINTER(hfg_scf_options), ctypes.POINTER(hfg_scf_atomic_extras)]
        L.hfg_scf_run_ex.argtypes = [ctypes.c_void_p, ctypes.POINTER(hfg_scf_options), ctypes.POINTER(hfg_scf_atomic_extras),
                                     ctypes.POINTER(hfg_scf_result), c_double_p, c_double_p]
        L.hfg_ctx_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_void_p]
        L.hfg_xc_fock.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p,
                                  c_double_p, c_double_p, c_double_p, ctypes.c_double]
        L.hfg_xc_fock_pol.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p,
                                      c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, ctypes.c_double]
        L.hfg_xc_fock_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double]
        L.hfg_coulomb_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, c_double_p, c_double_p]
        L.hfg_coulomb_energy_matrix.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, c_double_p, c_double_p]
        L.hfg_coulomb_batch_devptr.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
        for name in ("hfg_exchange_batch", "hfg_rs_exchange_batch"):
            getattr(L, name).argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, c_double_p, c_double_p]
        for name in ("hfg_exchange_batch_devptr", "hfg_rs_exchange_batch_devptr"):
            getattr(L, name).argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
        L.hfg_exchange_occ_batch_devptr.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                    c_i64_p, ctypes.c_int64, ctypes.c_void_p]
        L.hfg_exchange_batch_plan.argtypes = [ctypes.c_int64, c_int_p, ctypes.c_int, c_int_p, c_int_p]
        L.hfg_exl_last_plan.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        L.hfg_fock_compact_pol_size.restype = ctypes.c_int64
        L.hfg_fock_compact_pol_size.argtypes = [ctypes.c_void_p]
        L.hfg_fock_compact_pol_devptr.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double]
        L.hfg_fock_finish_pol_devptr.argtypes = [ctypes.c_void_p] * 7
        L.hfg_eig_gsym_sub_pair_devptr.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_int, c_i64_p, c_i64_p] + [ctypes.c_void_p] * 4
        L.hfg_profile_get.argtypes = [ctypes.c_void_p, ctypes.c_char_p, c_double_p, c_i64_p]
        L.hfg_measure_kernel.argtypes = [ctypes.c_void_p, ctypes.c_char_p, c_double_p, c_i64_p]
        L.hfg_profile_names.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.hfg_diis_create.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                      ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.hfg_diis_destroy.argtypes = [ctypes.c_void_p]
        L.hfg_diis_set_metric_devptr.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
        L.hfg_diis_set_blocks.argtypes = [ctypes.c_void_p, ctypes.c_int, c_i64_p, c_i64_p]
        L.hfg_diis_update_devptr.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                             c_double_p]
        L.hfg_diis_solve_devptr.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_int_p]
        L.hfg_diis_size.argtypes = [ctypes.c_void_p]
        L.hfg_diis_get.argtypes = [ctypes.c_void_p, ctypes.c_int, c_double_p, ctypes.c_int64]
        L.hfg_coulomb_dev.argtypes = [ctypes.c_void_p] * 4
        # the step objects' entries (DeviceSCFStep and its subclasses)
        L.hfg_fock_compact_size.restype = ctypes.c_int64
        L.hfg_eig_block_buf_size.restype = ctypes.c_int64
        L.hfg_fock_compact_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double]
        for name in ("hfg_exchange_dev", "hfg_rs_exchange_dev", "hfg_mix_exchange_devptr"):
            getattr(L, name).argtypes = [ctypes.c_void_p] * 4
        for name in ("hfg_exchange_occ_dev", "hfg_mix_exchange_occ_devptr"):
            getattr(L, name).argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_void_p]
        L.hfg_mix_exchange_occ_batch_devptr.argtypes = L.hfg_exchange_occ_batch_devptr.argtypes
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise RuntimeError(lib().hfg_last_error().decode())


def _f(a):
    return np.asfortranarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(c_double_p)


def device_count():
    return int(lib().hfg_device_count())


class Context(object):
    """hfg_ctx: one device + one stream."""

    def __init__(self, device=0, stream=None):
        """stream: None -> the context creates its own stream; an integer hipStream_t handle -> enqueue there, where
        the handle 0 (what torch.cuda.current_stream().cuda_stream returns for the default stream) means the null
        stream itself (HFG_NULL_STREAM), so that the kernels stay ordered with torch operations and collectives"""
        h = ctypes.c_void_p()
        if stream is None:
            sp = None
        elif int(stream) == 0:
            sp = ctypes.c_void_p(-1)  # HFG_NULL_STREAM
        else:
            sp = ctypes.c_void_p(int(stream))
        _check(lib().hfg_ctx_create(ctypes.byref(h), int(device), sp))
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            lib().hfg_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(lib().hfg_ctx_synchronize(self.h))

    def set_shard(self, rank, nranks):
        _check(lib().hfg_ctx_set_shard(self.h, int(rank), int(nranks)))

    def set_fock_blocks(self, basis, blockid_ptr):
        """declare which entries of the compact Fock buffer are read (hfg_ctx_set_fock_blocks): blockid_ptr is the address
        of the device array of per-function block ids that hfg_fock_finish_dev masks with; None clears the declaration"""
        f = lib().hfg_ctx_set_fock_blocks
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _check(f(self.h, basis.h, ctypes.c_void_p(blockid_ptr or 0)))

    def fix_sinvh(self, device_ptr):
        """declare the device matrix at this address constant (None withdraws): see hfg_ctx_fix_sinvh"""
        _check(lib().hfg_ctx_fix_sinvh(self.h, ctypes.c_void_p(device_ptr or 0)))

    FOCK_BAND_STATES = ("none", "declared", "refused")

    def declare_fock_band(self, basis, H0_ptr=None, blockid_ptr=None):
        """declare, beside fix_sinvh, that every Fock matrix of the blocked eigensolves is local in the radial element index
        (F = H0 + J + XC; hfg_ctx_declare_fock_band).  H0_ptr / blockid_ptr: device addresses of H0 (N x N) and of the
        per-function block ids; an H0 with a non-zero entry outside the pattern refuses the declaration.  Returns
        fock_band_state()."""
        f = lib().hfg_ctx_declare_fock_band
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_int_p]
        st = ctypes.c_int()
        _check(f(self.h, basis.h, ctypes.c_void_p(H0_ptr or 0), ctypes.c_void_p(blockid_ptr or 0), ctypes.byref(st)))
        return self.FOCK_BAND_STATES[st.value]

    def fock_band_state(self):
        """"none", "declared" or "refused" (H0 had an entry outside the pattern): what the last declare_fock_band left;
        fix_sinvh resets it to "none" """
        f = lib().hfg_ctx_fock_band_state
        f.argtypes = [ctypes.c_void_p, c_int_p]
        st = ctypes.c_int()
        _check(f(self.h, ctypes.byref(st)))
        return self.FOCK_BAND_STATES[st.value]

    def profile(self, on=True):
        _check(lib().hfg_profile_enable(self.h, 1 if on else 0))

    def profile_reset(self):
        _check(lib().hfg_profile_reset(self.h))

    def measure_kernel(self, name):
        ms = ctypes.c_double()
        n = ctypes.c_int64()
        _check(lib().hfg_measure_kernel(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def profile_names(self):
        buf = ctypes.create_string_buffer(1 << 16)
        _check(lib().hfg_profile_names(self.h, buf, len(buf)))
        return [x for x in buf.value.decode().split("\n") if x]

    def profile_get(self, name):
        ms = ctypes.c_double()
        n = ctypes.c_int64()
        _check(lib().hfg_profile_get(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def cuhf_update(self, S, Ca, na, Cb, nb, Fa, Fb):
        """hfg_cuhf_update_devptr on torch tensors of this context's device (contiguous float64, column-major): the
        constrained-UHF form of ROHF, Fa += lambda and Fb -= lambda in place.  S: overlap (N x N); Ca, Cb: orbitals whose
        first na / nb columns formed Pa / Pb; N is taken from Fa.  na == nb or min(na, nb) == 0 changes nothing."""
        N = int(round(Fa.numel() ** 0.5))
        na, nb = int(na), int(nb)
        for t, count, what in ((S, N * N, "S"), (Ca, N * na, "Ca"), (Cb, N * nb, "Cb"), (Fa, N * N, "Fa"), (Fb, N * N, "Fb")):
            if t is None or not (t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch.float64" and t.numel() >= count):
                raise ValueError("Context.cuhf_update: %s must be a contiguous float64 tensor on the device with at least %d elements"
                                 % (what, count))
        if N * N != Fa.numel() or Fb.numel() != Fa.numel():
            raise ValueError("Context.cuhf_update: Fa and Fb are N x N")
        f = lib().hfg_cuhf_update_devptr
        f.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                      ctypes.c_void_p, ctypes.c_void_p]
        _check(f(self.h, N, S.data_ptr(), Ca.data_ptr(), na, Cb.data_ptr(), nb, Fa.data_ptr(), Fb.data_ptr()))

    def occupy_blocks(self, E, C, blockid, occupations, out=None):
        """hfg_occupy_blocks_devptr on torch tensors of this context's device: fractional occupations by symmetry block.  E
        (ncols) and C (N x ncols, column-major, contiguous float64) as the blocked eigensolve leaves them; blockid (N, int32):
        the block of every row; occupations: one list of values in [0, 1] per block, lowest level first.  Slot
        sum(len(occupations[:b])) + k receives the k-th lowest column of block b times the square root of its occupation.
        Returns (Cocc, Eocc, Focc): N x nslots, nslots, nslots; out = (Cocc, Eocc, Focc) writes into tensors at hand.
        Queued on the context's stream.  The host waits only when something is new: the first call with a blockid tensor
        reads it back once to count the rows of every block (the refusal of more occupations than a block has rows needs
        them), and occupation lists that differ from the previous call's drain the stream before they are staged.  The
        counts are kept per (address, N, number of blocks) of blockid: after writing into a blockid tensor in place, or
        when a new tensor may have received the address of a freed one, call forget_block_ids() first -- stale counts
        refuse a valid call or let one pass whose surplus slots then come back as zero columns of energy 0."""
        import torch
        N = int(blockid.numel())
        ncols = int(E.numel())
        occ_ptr = np.zeros(len(occupations) + 1, dtype=np.int64)
        occ_ptr[1:] = np.cumsum([len(o) for o in occupations])
        occ = np.ascontiguousarray(np.concatenate([np.asarray(o, dtype=np.float64).ravel() for o in occupations] + [np.zeros(0)]))
        nslots = int(occ_ptr[-1])
        if str(blockid.dtype) != "torch.int32" or not (blockid.is_cuda and blockid.is_contiguous()):
            raise ValueError("Context.occupy_blocks: blockid must be a contiguous int32 tensor on the device")
        if out is None:
            f64 = dict(dtype=torch.float64, device=C.device)
            out = (torch.zeros(N * max(nslots, 1), **f64), torch.zeros(max(nslots, 1), **f64), torch.zeros(max(nslots, 1), **f64))
        for t, count, what in ((E, ncols, "E"), (C, N * ncols, "C"), (out[0], N * nslots, "Cocc"), (out[1], nslots, "Eocc"),
                               (out[2], nslots, "Focc")):
            if t is None or not (t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch.float64" and t.numel() >= count):
                raise ValueError("Context.occupy_blocks: %s must be a contiguous float64 tensor on the device with at least %d elements"
                                 % (what, count))
        f = lib().hfg_occupy_blocks_devptr
        f.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                      c_i64_p, c_double_p] + [ctypes.c_void_p] * 3
        _check(f(self.h, N, ncols, E.data_ptr(), C.data_ptr(), blockid.data_ptr(), len(occupations), occ_ptr.ctypes.data_as(c_i64_p),
                 _p(occ), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()))
        return out

    def forget_block_ids(self):
        """drop the rows per block counted for the blockid tensor that occupy_blocks saw last (hfg_occupy_forget_blocks)"""
        f = lib().hfg_occupy_forget_blocks
        f.argtypes = [ctypes.c_void_p]
        _check(f(self.h))


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def tuning_table():
    """the HELFEM_* environment switches of the native library (hfg_tuning_table; no device needed): a list of dicts with
    name, kind, default, value (in this process), read ("once" per process or "live" at every use) and meaning"""
    buf = ctypes.create_string_buffer(1 << 16)
    _check(lib().hfg_tuning_table(buf, ctypes.c_size_t(len(buf))))
    keys = ("name", "kind", "default", "value", "read", "meaning")
    return [dict(zip(keys, line.split("\t"))) for line in buf.value.decode().split("\n") if line]


def lm_to_l_m(lmmax):
    """diatomic::basis::lm_to_l_m (basis.cpp:287)."""
    lmmax = list(lmmax)
    cap = sum(2 * (l + 1) for l in lmmax) + 4
    lv = (ctypes.c_int * cap)()
    mv = (ctypes.c_int * cap)()
    n = ctypes.c_int(cap)
    arr = (ctypes.c_int * len(lmmax))(*lmmax)
    _check(lib().hfg_lm_list(arr, len(lmmax), lv, mv, ctypes.byref(n)))
    return list(lv[:n.value]), list(mv[:n.value])


def get_grid(mumax, nelem, igrid=4, zexp=1.0):
    """utils::get_grid (libhelfem/src/grid.cpp:18)."""
    b = np.zeros(nelem + 1)
    _check(lib().hfg_radial_grid(float(mumax), int(nelem), int(igrid), float(zexp), _p(b)))
    return b


class TwoDBasis(object):
    """diatomic::basis::TwoDBasis — setup on the host, coulomb/exchange on the GPU."""

    def __init__(self, Z1, Z2, Rhalf, nnodes, nquad, bval, lval, mval, lpad=10, ctx=None):
        self._bval = np.ascontiguousarray(bval, dtype=np.float64)
        self._lval = (ctypes.c_int * len(lval))(*lval)
        self._mval = (ctypes.c_int * len(mval))(*mval)
        d = hfg_diatomic_desc(int(Z1), int(Z2), float(Rhalf), 4, int(nnodes), int(nquad), _p(self._bval),
                              len(self._bval), self._lval, self._mval, len(lval), int(lpad))
        h = ctypes.c_void_p()
        _check(lib().hfg_diatomic_basis_create(ctypes.byref(d), ctypes.byref(h)))
        self.h = h
        self.ctx = ctx
        self.lval, self.mval = list(lval), list(mval)
        self._uploaded = None
        dims = [ctypes.c_int64() for _ in range(5)]
        _check(lib().hfg_basis_dims(self.h, *[ctypes.byref(x) for x in dims]))
        self._Nbf, self._Ndummy, self._Nrad, self._Nang, self._Nel = [x.value for x in dims]

    def __del__(self):
        try:
            if self.h:
                lib().hfg_basis_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def Nbf(self):
        return self._Nbf

    def Ndummy(self):
        return self._Ndummy

    def Nrad(self):
        return self._Nrad

    def Nang(self):
        return self._Nang

    def Nel(self):
        return self._Nel

    def _mat(self, fn):
        M = np.zeros((self._Nbf, self._Nbf), order="F")
        _check(fn(self.h, _p(M)))
        return M

    def overlap(self):
        return self._mat(lib().hfg_basis_overlap)

    def kinetic(self):
        return self._mat(lib().hfg_basis_kinetic)

    def nuclear(self):
        return self._mat(lib().hfg_basis_nuclear)

    def get_sym_idx(self, symm):
        n = ctypes.c_int()
        _check(lib().hfg_basis_sym_blocks(self.h, int(symm), ctypes.byref(n), None, None))
        ptr = np.zeros(n.value + 1, dtype=np.int64)
        idx = np.zeros(self._Nbf, dtype=np.int64)
        _check(lib().hfg_basis_sym_blocks(self.h, int(symm), ctypes.byref(n), ptr.ctypes.data_as(c_i64_p),
                                          idx.ctypes.data_as(c_i64_p)))
        return [idx[ptr[i]:ptr[i + 1]].copy() for i in range(n.value)]

    def compute_tei(self, exchange=True, device=False, ctx=None):
        """TwoDBasis::compute_tei.  device=True builds the in-element tables on the GPU (hfg_compute_tei_dev): the
        1 GB of primitive integrals at Nbf~4000 then never exists on the host"""
        if device:
            ctx = ctx or self.ctx or default_context()
            self.ctx = ctx
            _check(lib().hfg_compute_tei_dev(ctx.h, self.h, 1 if exchange else 0))
        else:
            _check(lib().hfg_compute_tei(self.h, 1 if exchange else 0))
        self._uploaded = None

    def overlap_with(self, other):
        """TwoDBasis::overlap(const TwoDBasis &rh), basis.cpp:713: <self | other>"""
        out = np.zeros((self.Nbf(), other.Nbf()), order="F")
        f = lib().hfg_basis_interbasis_overlap
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, c_double_p]
        _check(f(self.h, other.h, _p(out)))
        return out

    def lm_map(self):
        """the sorted (L, |M|) channels of the constructor (basis.cpp:333-375)"""
        n = ctypes.c_int(4096)
        L = (ctypes.c_int * 4096)()
        M = (ctypes.c_int * 4096)()
        _check(lib().hfg_basis_lm_map(self.h, L, M, ctypes.byref(n)))
        return [(L[i], M[i]) for i in range(n.value)]

    PRIM_TABLES = ("tei00", "tei02", "tei20", "tei22", "ktei00", "ktei02", "ktei20", "ktei22", "P0", "P2", "Q0", "Q2")

    def prim_table(self, name, ilm, iel):
        """one table of compute_tei (prim_tei**, prim_ktei**, disjoint_**) in the reference's shape; device-built
        tables are copied back from HBM"""
        which = self.PRIM_TABLES.index(name)
        r, c = ctypes.c_int64(), ctypes.c_int64()
        ctxh = self.ctx.h if self.ctx is not None else None
        f = lib().hfg_basis_get_prim
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p,
                      ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
        _check(f(ctxh, self.h, which, int(ilm), int(iel), None, ctypes.byref(r), ctypes.byref(c)))
        out = np.zeros((r.value, c.value), order="F")
        _check(f(ctxh, self.h, which, int(ilm), int(iel), _p(out), ctypes.byref(r), ctypes.byref(c)))
        return out

    def upload(self, ldft=0, mdft=0, ctx=None):
        """tables -> HBM (also sets up the XC grid of DFTGrid(basis, ldft, mdft))"""
        ctx = ctx or self.ctx or default_context()
        self.ctx = ctx
        _check(lib().hfg_basis_upload(ctx.h, self.h, int(ldft), int(mdft)))
        self._uploaded = (ldft, mdft)

    def _ensure(self):
        if self._uploaded is None:
            self.upload()
        return self.ctx

    def coulomb(self, P):
        ctx = self._ensure()
        P = _f(P)
        J = np.zeros_like(P, order="F")
        _check(lib().hfg_coulomb(ctx.h, self.h, _p(P), _p(J)))
        return J

    def exchange(self, P):
        ctx = self._ensure()
        P = _f(P)
        K = np.zeros_like(P, order="F")
        _check(lib().hfg_exchange(ctx.h, self.h, _p(P), _p(K)))
        return K

    def exchange_last_plan(self, which="coulomb"):
        """what the last low-rank exchange builds on a table set took (hfg_exl_last_plan; which: "coulomb", "screened" or
        "mix"): {"single": record or None, "batch": record or None}, the kernels, tiles and launchers chosen, see
        include/helfem_gpu.h"""
        import json
        buf = ctypes.create_string_buffer(1 << 14)
        _check(lib().hfg_exl_last_plan(self.h, which.encode(), buf, ctypes.c_size_t(len(buf))))
        return json.loads(buf.value.decode())

    def _batch(self, Ps, ctx):
        """the context of a batched call (uploading to it when the tables are nowhere yet) and the densities in the layout
        of hfg_coulomb_batch: row b holds P_b column by column"""
        if ctx is not None and self._uploaded is None:
            self.upload(ctx=ctx)
        ctx = ctx or self._ensure()
        N = self.Nbf()
        Ps = [np.asarray(P, dtype=np.float64) for P in Ps]
        if any(P.shape != (N, N) for P in Ps):
            raise ValueError("coulomb_batch: every density is an Nbf x Nbf matrix")
        buf = np.empty((len(Ps), N * N))
        for b, P in enumerate(Ps):
            buf[b] = P.ravel(order="F")
        return ctx, buf

    def coulomb_batch(self, Ps, ctx=None):
        """J[P_b] for every density of Ps (a sequence of symmetric Nbf x Nbf matrices, or an array (nP, Nbf, Nbf)) with the
        in-element tables read once for the batch (hfg_coulomb_batch).  Returns an array (nP, Nbf, Nbf): out[b] = coulomb(Ps[b])."""
        ctx, buf = self._batch(Ps, ctx)
        N, out = self.Nbf(), np.zeros_like(buf)
        _check(lib().hfg_coulomb_batch(ctx.h, self.h, len(buf), _p(buf), _p(out)))
        return out.reshape(len(buf), N, N).transpose(0, 2, 1)

    def coulomb_energy_matrix(self, Ps, ctx=None):
        """W[a, b] = tr(P_a J[P_b]) for the densities of Ps, formed on the device (hfg_coulomb_energy_matrix); symmetric by
        the symmetry of the integrals, not symmetrised"""
        ctx, buf = self._batch(Ps, ctx)
        W = np.zeros((len(buf), len(buf)), order="F")
        _check(lib().hfg_coulomb_energy_matrix(ctx.h, self.h, len(buf), _p(buf), _p(W)))
        return W

    def coulomb_batch_torch(self, dP, out=None, ctx=None):
        """hfg_coulomb_batch_devptr on torch tensors in HBM: dP holds nP densities of Nbf x Nbf, one after the other, each
        column-major (float64, contiguous, any shape of nP * Nbf * Nbf elements).  The build is enqueued on the context's
        stream, honours its shard and is not waited for; returns `out` (a new tensor like dP when None)."""
        import torch
        if ctx is not None and self._uploaded is None:
            self.upload(ctx=ctx)
        ctx = ctx or self._ensure()
        N2 = self.Nbf() ** 2
        if out is None:
            out = torch.empty_like(dP)
        for t in (dP, out):
            if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.numel() % N2 or t.numel() != dP.numel():
                raise ValueError("coulomb_batch_torch: contiguous float64 device tensors of nP * Nbf * Nbf elements")
        _check(lib().hfg_coulomb_batch_devptr(ctx.h, self.h, dP.numel() // N2, ctypes.c_void_p(dP.data_ptr()),
                                              ctypes.c_void_p(out.data_ptr())))
        return out

    def exchange_batch(self, Ps, ctx=None, _entry="hfg_exchange_batch"):
        """K[P_b] for every density of Ps (as coulomb_batch takes them) with the exchange-ordered element tables read once
        per chunk of densities (hfg_exchange_batch).  Returns an array (nP, Nbf, Nbf): out[b] is bitwise exchange(Ps[b])."""
        ctx, buf = self._batch(Ps, ctx)
        N, out = self.Nbf(), np.zeros_like(buf)
        _check(getattr(lib(), _entry)(ctx.h, self.h, len(buf), _p(buf), _p(out)))
        return out.reshape(len(buf), N, N).transpose(0, 2, 1)

    def exchange_batch_torch(self, dP, out=None, ctx=None, rs=False):
        """hfg_exchange_batch_devptr (rs: hfg_rs_exchange_batch_devptr) on torch tensors in HBM, laid out and checked as
        coulomb_batch_torch does.  The build is enqueued on the context's stream and honours its shard; returns `out`."""
        import torch
        if ctx is not None and self._uploaded is None:
            self.upload(ctx=ctx)
        ctx = ctx or self._ensure()
        N2 = self.Nbf() ** 2
        if out is None:
            out = torch.empty_like(dP)
        for t in (dP, out):
            if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.numel() % N2 or t.numel() != dP.numel():
                raise ValueError("exchange_batch_torch: contiguous float64 device tensors of nP * Nbf * Nbf elements")
        f = lib().hfg_rs_exchange_batch_devptr if rs else lib().hfg_exchange_batch_devptr
        _check(f(ctx.h, self.h, dP.numel() // N2, ctypes.c_void_p(dP.data_ptr()), ctypes.c_void_p(out.data_ptr())))
        return out

    def model_potential(self, p1, p2=None):
        """TwoDGrid::model_potential(p1, p2) / atomic TwoDBasis::model_potential(p1): p = (kind, Z[, d[, H]]) with kind
        0 point nucleus, 1 GSZ (screening length d), 3 Thomas-Fermi.  The diatomic form needs upload(ldft, mdft)."""
        ctx = self._ensure()

        def mk(p):
            p = tuple(p) + (0.0, 0.0)
            return hfg_model_pot(int(p[0]), int(p[1]), float(p[2]), float(p[3]))
        a, b = mk(p1), mk(p2 if p2 is not None else p1)
        N = self.Nbf()
        H = np.zeros((N, N), order="F")
        _check(lib().hfg_model_potential(ctx.h, self.h, ctypes.byref(a), ctypes.byref(b), _p(H)))
        return H


def angular_basis(lmax, mmax):
    """atomic::basis::angular_basis (src/atomic/basis.cpp:174)."""
    cap = (lmax + 1) * (2 * mmax + 1) + 4
    lv = (ctypes.c_int * cap)()
    mv = (ctypes.c_int * cap)()
    n = ctypes.c_int(cap)
    _check(lib().hfg_angular_basis(int(lmax), int(mmax), lv, mv, ctypes.byref(n)))
    return list(lv[:n.value]), list(mv[:n.value])


def atomic_grid(nelem, Rmax=40.0, igrid=4, zexp=2.0, finitenuc=0, Rrms=0.0, nelem0=0, igrid0=4, zexp0=2.0, Z=0, Zl=0, Zr=0,
                Rmid=0.0, add_conf=False, shift_conf=0.0):
    """atomic::basis::form_grid (src/atomic/basis.cpp:119-172): element boundaries of the atomic program"""
    cap = int(nelem) + 3 * int(nelem0) + 4
    b = np.zeros(cap)
    n = ctypes.c_int(cap)
    _check(lib().hfg_atomic_grid(int(finitenuc), float(Rrms), int(nelem), float(Rmax), int(igrid), float(zexp), int(nelem0),
                                 int(igrid0), float(zexp0), int(Z), int(Zl), int(Zr), float(Rmid), 1 if add_conf else 0,
                                 float(shift_conf), _p(b), ctypes.byref(n)))
    return b[:n.value].copy()


class AtomicTwoDBasis(TwoDBasis):
    """atomic::basis::TwoDBasis — setup on the host, coulomb/exchange on the GPU.  finitenuc / Rrms: nuclear model of the
    central charge (1 Gaussian, 2 uniform sphere, 3 hollow sphere); zeroder: zero derivative at the last grid point; Zl, Zr:
    point charges at z = -Rmid, +Rmid (on an element boundary)."""

    def __init__(self, Z, nnodes, nquad, bval, lval, mval, ctx=None, finitenuc=0, Rrms=0.0, zeroder=False, Zl=0, Zr=0, Rmid=0.0):
        self._bval = np.ascontiguousarray(bval, dtype=np.float64)
        self._lval = (ctypes.c_int * len(lval))(*lval)
        self._mval = (ctypes.c_int * len(mval))(*mval)
        d = hfg_atomic_desc(int(Z), 4, int(nnodes), int(nquad), _p(self._bval), len(self._bval), self._lval,
                            self._mval, len(lval))
        h = ctypes.c_void_p()
        if finitenuc or zeroder or Zl or Zr:
            dx = hfg_atomic_desc_ex(d, int(finitenuc), float(Rrms), 1 if zeroder else 0, int(Zl), int(Zr), float(Rmid))
            _check(lib().hfg_atomic_basis_create_ex(ctypes.byref(dx), ctypes.byref(h)))
        else:
            _check(lib().hfg_atomic_basis_create(ctypes.byref(d), ctypes.byref(h)))
        self.h = h
        self.ctx = ctx
        self.lval, self.mval = list(lval), list(mval)
        self._uploaded = None
        dims = [ctypes.c_int64() for _ in range(5)]
        _check(lib().hfg_basis_dims(self.h, *[ctypes.byref(x) for x in dims]))
        self._Nbf, self._Ndummy, self._Nrad, self._Nang, self._Nel = [x.value for x in dims]

    def confinement(self, iconf, N=0, R=0.0, V=0.0, shift=0.0):
        """TwoDBasis::confinement(N, R, iconf, V, shift) (src/atomic/TwoDBasis.cpp:480)"""
        out = np.zeros((self._Nbf, self._Nbf), order="F")
        _check(lib().hfg_basis_confinement(self.h, int(iconf), int(N), float(R), float(V), float(shift), _p(out)))
        return out

    ATOMIC_TABLES = {"prim_tei": 0, "prim_ktei": 4, "disjoint_L": 8, "disjoint_m1L": 10, "disjoint_iL": 12, "disjoint_kL": 13,
                     "rs_tei": 14, "rs_ktei": 15}

    def atomic_table(self, name, L, iel, kel=None):
        """one table of compute_tei / compute_yukawa / compute_erfc in the reference's shape (erfc: element pair iel, kel)"""
        which = self.ATOMIC_TABLES[name]
        idx = int(iel) if kel is None else int(iel) * self._Nel + int(kel)
        r, c = ctypes.c_int64(), ctypes.c_int64()
        ctxh = self.ctx.h if self.ctx is not None else None
        f = lib().hfg_basis_get_prim
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p,
                      ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
        _check(f(ctxh, self.h, which, int(L), idx, None, ctypes.byref(r), ctypes.byref(c)))
        out = np.zeros((r.value, c.value), order="F")
        _check(f(ctxh, self.h, which, int(L), idx, _p(out), ctypes.byref(r), ctypes.byref(c)))
        return out

    RADIAL_TABLES = {"bf": 0, "df": 1, "lf": 2, "r": 3}

    def radial_table(self, name, iel):
        """RadialBasis::get_bf / get_df / get_lf (B/r and its first and second radial derivatives) at the quadrature points
        of element iel, nquad x Nprim(iel); "r": the radial coordinates of those points"""
        f = lib().hfg_basis_radial_table
        f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_double_p, ctypes.POINTER(ctypes.c_int64),
                      ctypes.POINTER(ctypes.c_int64)]
        r, c = ctypes.c_int64(), ctypes.c_int64()
        _check(f(self.h, self.RADIAL_TABLES[name], int(iel), None, ctypes.byref(r), ctypes.byref(c)))
        out = np.zeros((r.value, c.value), order="F")
        _check(f(self.h, self.RADIAL_TABLES[name], int(iel), _p(out), ctypes.byref(r), ctypes.byref(c)))
        return out[:, 0] if name == "r" else out

    def _compute_rs(self, kind, omega, device, ctx):
        if device:
            ctx = ctx or self.ctx
            if ctx is None:
                raise ValueError("device=True needs a context (ctx=... here or at construction)")
            self.ctx = ctx
            _check(lib().hfg_compute_rs_tei_dev(ctx.h, self.h, kind, float(omega)))
        else:
            _check(lib().hfg_compute_rs_tei(self.h, kind, float(omega)))
        self._uploaded = None

    def compute_yukawa(self, lam, device=False, ctx=None):
        """TwoDBasis::compute_yukawa (src/atomic/TwoDBasis.cpp:741): tables of exp(-lambda r12)/r12, on the host or,
        device=True, on the GPU of ctx (hfg_compute_rs_tei_dev)"""
        self._compute_rs(1, lam, device, ctx)

    def compute_erfc(self, mu, device=False, ctx=None):
        """TwoDBasis::compute_erfc (src/atomic/TwoDBasis.cpp:780): tables of erfc(mu r12)/r12, on the host or,
        device=True, on the GPU of ctx (hfg_compute_rs_tei_dev)"""
        self._compute_rs(2, mu, device, ctx)

    def rs_exchange_batch(self, Ps, ctx=None):
        """rs_exchange(P_b) for every density of Ps in one pass over the range-separated tables per chunk (hfg_rs_exchange_batch;
        an erfc basis loops over the single build inside the entry)"""
        return self.exchange_batch(Ps, ctx=ctx, _entry="hfg_rs_exchange_batch")

    def rs_exchange(self, P):
        """TwoDBasis::rs_exchange (src/atomic/TwoDBasis.cpp:1142) on the GPU"""
        ctx = self._ensure()
        P = _f(P)
        K = np.zeros_like(P, order="F")
        _check(lib().hfg_rs_exchange(ctx.h, self.h, _p(P), _p(K)))
        return K

    # ---- the mixed-kernel table set: alpha K[1/r12] + beta K[screened kernel] in one build ----------------
    def mix_exchange_tables(self, alpha, beta, ctx=None):
        """hfg_mix_exchange_tables: mix the uploaded Coulomb and range-separated tables on the device for
        K = alpha K[1/r12] + beta K[screened].  Uploads first when nothing is uploaded.  True: the set is there (a repeated
        call with the same values does no work); False: it would exceed the bound of the pair path, nothing was allocated
        and K is to be built from the two table sets."""
        if ctx is not None and self._uploaded is None:
            self.upload(ctx=ctx)
        ctx = ctx or self._ensure()
        f = lib().hfg_mix_exchange_tables
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double]
        rc = f(ctx.h, self.h, float(alpha), float(beta))
        if rc == 4:
            return False
        _check(rc)
        return True

    def mix_exchange(self, P):
        """alpha K[P] + beta K_screened[P] from the mixed set (hfg_mix_exchange); numpy in, numpy out"""
        if self.ctx is None:
            raise RuntimeError("The mixed exchange tables have not been built (mix_exchange_tables)!")
        P = _f(P)
        K = np.zeros_like(P, order="F")
        f = lib().hfg_mix_exchange
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, c_double_p, c_double_p]
        _check(f(self.ctx.h, self.h, _p(P), _p(K)))
        return K

    def mix_exchange_torch(self, dP, dC=None, nocc=None, out=None, ctx=None):
        """the device-pointer entries on torch tensors in HBM (contiguous float64).  dP: nP densities of Nbf x Nbf, one after
        the other, column-major; dC (optional): nP sets of Nbf x Nbf orbital columns, the first nocc[b] of set b being the
        factors of P_b.  One density goes through hfg_mix_exchange_devptr / hfg_mix_exchange_occ_devptr (nocc an integer or
        a list of one), more through hfg_mix_exchange_occ_batch_devptr.  Queued on the context's stream, honours its shard,
        not waited for; returns `out`."""
        import torch
        ctx = ctx or self.ctx
        N = self.Nbf()
        N2 = N * N
        if out is None:
            out = torch.empty_like(dP)
        for t in (dP, out) + ((dC,) if dC is not None else ()):
            if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.numel() % N2 or t.numel() != dP.numel():
                raise ValueError("mix_exchange_torch: contiguous float64 device tensors of nP * Nbf * Nbf elements")
        nP = dP.numel() // N2
        L = lib()
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        if dC is not None:
            counts = np.ascontiguousarray(np.atleast_1d(nocc), dtype=np.int64)
            if len(counts) != nP:
                raise ValueError("mix_exchange_torch: one count of occupied orbitals per density")
        if nP == 1 and dC is None:
            _check(L.hfg_mix_exchange_devptr(ctx.h, self.h, ptr(dP), ptr(out)))
        elif nP == 1:
            _check(L.hfg_mix_exchange_occ_devptr(ctx.h, self.h, ptr(dP), ptr(dC), int(counts[0]), ptr(out)))
        else:
            _check(L.hfg_mix_exchange_occ_batch_devptr(ctx.h, self.h, nP, ptr(dP), ptr(dC) if dC is not None else None,
                                                       counts.ctypes.data_as(c_i64_p) if dC is not None else None, N, ptr(out)))
        return out

    def mixed_table(self, L, iel, kel):
        """one block of the mixed set read back from the device, padded: p^2 x p^2, rows = primitives of element iel, columns
        = primitives of element kel (hfg_basis_get_prim, which = 16)"""
        f = lib().hfg_basis_get_prim
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p,
                      ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
        r, c = ctypes.c_int64(), ctypes.c_int64()
        ctxh = self.ctx.h if self.ctx is not None else None
        idx = int(iel) * self._Nel + int(kel)
        _check(f(ctxh, self.h, 16, int(L), idx, None, ctypes.byref(r), ctypes.byref(c)))
        out = np.zeros((r.value, c.value), order="F")
        _check(f(ctxh, self.h, 16, int(L), idx, _p(out), ctypes.byref(r), ctypes.byref(c)))
        return out


def exchange_batch_plan(ranks, max_members=0):
    """chunks of a batched exchange build (hfg_exchange_batch_plan, no device): (chunk_of, nchunks) for the ranks of the
    batch's densities; chunk_of[b] = -1 for a zero matrix.  max_members = 0: HELFEM_EXCHANGE_BATCH_CHUNK's value."""
    r = np.ascontiguousarray(ranks, dtype=np.int32)
    out = np.full(len(r), -2, dtype=np.int32)
    n = ctypes.c_int(0)
    _check(lib().hfg_exchange_batch_plan(len(r), r.ctypes.data_as(c_int_p), int(max_members), out.ctypes.data_as(c_int_p), ctypes.byref(n)))
    return out.tolist(), n.value


def eig_band_plan(node, pm, E):
    """plan of the banded F X of one symmetry block (hfg_eig_band_plan, no device): node[i] = radial node of position i of
    the block's index list, pm = nodes per element - 1, E elements.  Returns (perm, steps, banded): the positions
    radial-major (the row order of F in the product), for every 64-row tile in that order the starts of its k steps (16
    columns each, in the caller's column order), and whether the block takes the row tasks (False: every tile has all steps)."""
    nd = np.ascontiguousarray(node, dtype=np.int32)
    n = len(nd)
    nt = (n + 63) // 64
    cap = nt * ((n + 15) // 16)
    perm = np.zeros(n, dtype=np.int64)
    toff, ks = np.zeros(nt + 1, dtype=np.int32), np.zeros(max(cap, 1), dtype=np.int32)
    banded = ctypes.c_int(0)
    f = lib().hfg_eig_band_plan
    f.argtypes = [ctypes.c_int64, c_int_p, ctypes.c_int, ctypes.c_int, c_i64_p, c_int_p, c_int_p, ctypes.c_int64, c_int_p]
    _check(f(n, nd.ctypes.data_as(c_int_p), int(pm), int(E), perm.ctypes.data_as(c_i64_p), toff.ctypes.data_as(c_int_p),
             ks.ctypes.data_as(c_int_p), cap, ctypes.byref(banded)))
    return perm, [ks[toff[t]:toff[t + 1]].copy() for t in range(nt)], bool(banded.value)


class DFTGrid(object):
    """diatomic::dftgrid::DFTGrid (dftgrid.cpp:760)."""

    def __init__(self, basis, ldft, mdft):
        self.basis, self.ldft, self.mdft = basis, int(ldft), int(mdft)

    def eval_Fxc(self, x_func, c_func, P, thr=1e-12):
        """returns (H, Exc, Nel, Ekin) — DFTGrid::eval_Fxc, restricted (dftgrid.cpp:769)."""
        b = self.basis
        if b._uploaded != (self.ldft, self.mdft):
            b.upload(self.ldft, self.mdft)
        P = _f(P)
        H = np.zeros_like(P, order="F")
        exc, nel, ekin = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _check(lib().hfg_xc_fock(b.ctx.h, b.h, int(x_func), int(c_func), _p(P), _p(H), ctypes.byref(exc),
                                 ctypes.byref(nel), ctypes.byref(ekin), float(thr)))
        return H, exc.value, nel.value, ekin.value

    def eval_Fxc_pol(self, x_func, c_func, Pa, Pb, thr=1e-12):
        """returns (Ha, Hb, Exc, Nel, Ekin) — DFTGrid::eval_Fxc, unrestricted (dftgrid.cpp:812)."""
        b = self.basis
        if b._uploaded != (self.ldft, self.mdft):
            b.upload(self.ldft, self.mdft)
        Pa, Pb = _f(Pa), _f(Pb)
        Ha, Hb = np.zeros_like(Pa, order="F"), np.zeros_like(Pb, order="F")
        exc, nel, ekin = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _check(lib().hfg_xc_fock_pol(b.ctx.h, b.h, int(x_func), int(c_func), _p(Pa), _p(Pb), _p(Ha), _p(Hb),
                                     ctypes.byref(exc), ctypes.byref(nel), ctypes.byref(ekin), float(thr)))
        return Ha, Hb, exc.value, nel.value, ekin.value


    def eval_Fxc_dev(self, x_func, c_func, P, Pb=None, thr=1e-12):
        """the device-buffer entry points hfg_xc_fock_dev / hfg_xc_fock_pol_dev, which honour the context's shard
        (Context.set_shard: only the radial points Q % n == rank contribute, dftgrid.cpp:779): the partial matrices
        and sums one rank of a multi-GPU run produces.  torch tensors serve as the HBM buffers.
        Returns (H, Exc, Nel, Ekin) or, with Pb, (Ha, Hb, Exc, Nel, Ekin)."""
        import torch
        b = self.basis
        if b._uploaded != (self.ldft, self.mdft):
            b.upload(self.ldft, self.mdft)
        dev = torch.device("cuda", b.ctx.device)
        N = b.Nbf()

        def up(M):
            return torch.from_numpy(np.asfortranarray(M, dtype=np.float64).ravel(order="F").copy()).to(dev)

        def ptr(t):
            return ctypes.c_void_p(t.data_ptr())
        scal = torch.zeros(3, dtype=torch.float64, device=dev)
        dP = up(P)
        dH = torch.zeros(N * N, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        L = lib()
        if Pb is None:
            L.hfg_xc_fock_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double]
            _check(L.hfg_xc_fock_dev(b.ctx.h, b.h, int(x_func), int(c_func), ptr(dP), ptr(dH), ptr(scal), float(thr)))
            b.ctx.synchronize()
            sc = scal.cpu().numpy()
            return dH.cpu().numpy().reshape((N, N), order="F"), sc[0], sc[1], sc[2]
        dPb = up(Pb)
        dHb = torch.zeros(N * N, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        L.hfg_xc_fock_pol_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_double]
        _check(L.hfg_xc_fock_pol_dev(b.ctx.h, b.h, int(x_func), int(c_func), ptr(dP), ptr(dPb), ptr(dH), ptr(dHb), ptr(scal),
                                     float(thr)))
        b.ctx.synchronize()
        sc = scal.cpu().numpy()
        return (dH.cpu().numpy().reshape((N, N), order="F"), dHb.cpu().numpy().reshape((N, N), order="F"), sc[0], sc[1],
                sc[2])


class scf(object):
    """namespace helfem::scf (src/general/scf_helpers.h)."""

    @staticmethod
    def _blocks(m_idx):
        ptr = np.zeros(len(m_idx) + 1, dtype=np.int64)
        for i, b in enumerate(m_idx):
            ptr[i + 1] = ptr[i] + len(b)
        idx = np.concatenate([np.asarray(b, dtype=np.int64) for b in m_idx]) if len(m_idx) else np.zeros(0, np.int64)
        return ptr, np.ascontiguousarray(idx)

    @staticmethod
    def eig_gsym(F, Sinvh, ctx=None):
        ctx = ctx or default_context()
        F, Sinvh = _f(F), _f(Sinvh)
        N, n = Sinvh.shape
        E = np.zeros(n)
        C = np.zeros((N, n), order="F")
        _check(lib().hfg_eig_gsym(ctx.h, ctypes.c_int64(N), ctypes.c_int64(n), _p(F), _p(Sinvh), _p(E), _p(C)))
        return E, C

    @staticmethod
    def eig_gsym_sub(F, Sinvh, m_idx, ctx=None):
        ctx = ctx or default_context()
        F, Sinvh = _f(F), _f(Sinvh)
        N = F.shape[0]
        ptr, idx = scf._blocks(m_idx)
        E = np.zeros(N)
        C = np.zeros((N, N), order="F")
        _check(lib().hfg_eig_gsym_sub(ctx.h, ctypes.c_int64(N), _p(F), _p(Sinvh), len(m_idx),
                                      ptr.ctypes.data_as(c_i64_p), idx.ctypes.data_as(c_i64_p), _p(E), _p(C)))
        return E, C

    @staticmethod
    def eig_gsym_sub_pair(Fa, Fb, Sinvh, m_idx, ctx=None):
        """the alpha and beta eig_gsym_sub calls of an unrestricted iteration as one batch (hfg_eig_gsym_sub_pair)"""
        ctx = ctx or default_context()
        Fa, Fb, Sinvh = _f(Fa), _f(Fb), _f(Sinvh)
        N = Fa.shape[0]
        ptr, idx = scf._blocks(m_idx)
        Ea, Eb = np.zeros(N), np.zeros(N)
        Ca, Cb = np.zeros((N, N), order="F"), np.zeros((N, N), order="F")
        f = lib().hfg_eig_gsym_sub_pair
        f.argtypes = [ctypes.c_void_p, ctypes.c_int64, c_double_p, c_double_p, c_double_p, ctypes.c_int, c_i64_p, c_i64_p, c_double_p,
                      c_double_p, c_double_p, c_double_p]
        _check(f(ctx.h, N, _p(Fa), _p(Fb), _p(Sinvh), len(m_idx), ptr.ctypes.data_as(c_i64_p), idx.ctypes.data_as(c_i64_p), _p(Ea), _p(Ca),
                 _p(Eb), _p(Cb)))
        return Ea, Ca, Eb, Cb

    @staticmethod
    def eig_sym(A, ctx=None):
        ctx = ctx or default_context()
        A = _f(A)
        n = A.shape[0]
        E = np.zeros(n)
        C = np.zeros((n, n), order="F")
        _check(lib().hfg_eig_sym(ctx.h, ctypes.c_int64(n), _p(A), _p(E), _p(C)))
        return E, C

    @staticmethod
    def eig_sel_count(m_idx, nev):
        """number of eigenpairs eig_gsym_sub_sel returns: the sum over the blocks of min(nev, block size)"""
        ptr, _ = scf._blocks(m_idx)
        f = lib().hfg_eig_sel_count
        f.restype = ctypes.c_int64
        f.argtypes = [ctypes.c_int, c_i64_p, ctypes.c_int64]
        return int(f(len(m_idx), ptr.ctypes.data_as(c_i64_p), int(nev)))

    @staticmethod
    def eig_sym_sel(A, nev, ctx=None):
        """the lowest min(nev, n) eigenpairs of a symmetric matrix (hfg_eig_sym_sel): E ascending, C n x len(E)"""
        ctx = ctx or default_context()
        A = _f(A)
        n = A.shape[0]
        K = max(0, min(int(nev), n))
        E = np.zeros(K)
        C = np.zeros((n, K), order="F")
        f = lib().hfg_eig_sym_sel
        f.argtypes = [ctypes.c_void_p, ctypes.c_int64, c_double_p, ctypes.c_int64, c_double_p, c_double_p]
        _check(f(ctx.h, n, _p(A), int(nev), _p(E), _p(C)))
        return E, C

    @staticmethod
    def eig_gsym_sub_sel(F, Sinvh, m_idx, nev, ctx=None):
        """the lowest min(nev, block size) eigenpairs of every symmetry block, sorted globally (hfg_eig_gsym_sub_sel): E (K),
        C (N x K), K = eig_sel_count(m_idx, nev).  The lowest m <= nev levels of the full problem are the first m returned."""
        ctx = ctx or default_context()
        F, Sinvh = _f(F), _f(Sinvh)
        N = F.shape[0]
        ptr, idx = scf._blocks(m_idx)
        K = scf.eig_sel_count(m_idx, nev) if nev >= 1 else 0
        E = np.zeros(K)
        C = np.zeros((N, K), order="F")
        f = lib().hfg_eig_gsym_sub_sel
        f.argtypes = [ctypes.c_void_p, ctypes.c_int64, c_double_p, c_double_p, ctypes.c_int, c_i64_p, c_i64_p, ctypes.c_int64, c_double_p,
                      c_double_p]
        _check(f(ctx.h, N, _p(F), _p(Sinvh), len(m_idx), ptr.ctypes.data_as(c_i64_p), idx.ctypes.data_as(c_i64_p), int(nev), _p(E), _p(C)))
        return E, C

    @staticmethod
    def form_Sinvh(S, chol, m_idx, ctx=None):
        ctx = ctx or default_context()
        S = _f(S)
        N = S.shape[0]
        ptr, idx = scf._blocks(m_idx)
        X = np.zeros((N, N), order="F")
        _check(lib().hfg_form_sinvh(ctx.h, ctypes.c_int64(N), _p(S), 1 if chol else 0, len(m_idx),
                                    ptr.ctypes.data_as(c_i64_p), idx.ctypes.data_as(c_i64_p), _p(X)))
        return X

    @staticmethod
    def form_density(C, nocc, ctx=None):
        ctx = ctx or default_context()
        C = _f(C)
        N, nc = C.shape
        P = np.zeros((N, N), order="F")
        _check(lib().hfg_form_density(ctx.h, ctypes.c_int64(N), ctypes.c_int64(nc), _p(C), ctypes.c_int64(nocc), _p(P)))
        return P

    @staticmethod
    def gemm(A, B, transA=False, transB=False, ctx=None):
        ctx = ctx or default_context()
        A, B = _f(A), _f(B)
        m = A.shape[1] if transA else A.shape[0]
        k = A.shape[0] if transA else A.shape[1]
        n = B.shape[0] if transB else B.shape[1]
        C = np.zeros((m, n), order="F")
        _check(lib().hfg_gemm(ctx.h, int(transA), int(transB), ctypes.c_int64(m), ctypes.c_int64(n), ctypes.c_int64(k),
                              _p(A), ctypes.c_int64(A.shape[0]), _p(B), ctypes.c_int64(B.shape[0]), _p(C),
                              ctypes.c_int64(m)))
        return C


# ---- host-side special functions (pinned against the reference's known-answer tests) ----
def gaunt_coefficient(L, M, l, m, lp, mp):
    return lib().hfg_gaunt_coefficient(L, M, l, m, lp, mp)


def modified_gaunt_coefficient(lj, mj, L, M, li, mi):
    return lib().hfg_modified_gaunt_coefficient(lj, mj, L, M, li, mi)


def legendre_PQ(Lmax, Mmax, xi):
    """(P, Q) arrays [L, M] — layout of the Fortran wrapper calc_Plm_arr / calc_Qlm_arr."""
    P = np.zeros((Mmax + 1, Lmax + 1))
    Q = np.zeros((Mmax + 1, Lmax + 1))
    lib().hfg_legendre_PQ(int(Lmax), int(Mmax), float(xi), _p(P), _p(Q))
    return P.T.copy(), Q.T.copy()


def bessel_il(x, L):
    return lib().hfg_bessel_il(float(x), int(L))


def bessel_kl(x, L):
    return lib().hfg_bessel_kl(float(x), int(L))


def erfc_phi(n, Xi, xi):
    return lib().hfg_erfc_phi(int(n), float(Xi), float(xi))


def set_erfc_binomial_mode(mode):
    """binomials of the short-range series of Phi_L: 0 exact (default), 1 the reference's helper"""
    lib().hfg_set_erfc_binomial_mode(int(mode))


def rs_special_dev(which, L, a, b=None, ctx=None):
    """the device versions of bessel_il (which 0), bessel_kl (1) and erfc_phi (2, b = xi) at the points a (hfg_rs_special_dev)"""
    ctx = ctx or default_context()
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(a if b is None else b, dtype=np.float64)
    out = np.zeros_like(a)
    _check(lib().hfg_rs_special_dev(ctx.h, int(which), int(L), _p(a), _p(b), a.size, _p(out)))
    return out


def theta_lm(l, m, cth):
    return lib().hfg_theta_lm(int(l), int(m), float(cth))


def chebyshev(n):
    x, w = np.zeros(n), np.zeros(n)
    lib().hfg_chebyshev_rule(int(n), _p(x), _p(w))
    return x, w


def lobatto_nodes(n):
    x = np.zeros(n)
    lib().hfg_lobatto_nodes(int(n), _p(x))
    return x


def xc_eval(func_id, rho, sigma=None, lapl=None, tau=None, nspin=1, thr=0.0, pars=None):
    """one functional at points, libxc's xc_mgga_exc_vxc layout (hfg_xc_eval; host only, no device): nspin 1 takes arrays of
    shape (np,), nspin 2 rho, lapl, tau of shape (np, 2) and sigma of shape (np, 3) (aa, ab, bb).  Returns a dict with exc
    (per particle) and vrho, vsigma, vlapl, vtau in the shapes of the inputs."""
    nspin = int(nspin)
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    npt = rho.shape[0]
    shp = {"rho": (npt,) if nspin == 1 else (npt, 2), "sigma": (npt,) if nspin == 1 else (npt, 3)}
    shp["lapl"] = shp["tau"] = shp["rho"]
    if rho.shape != shp["rho"]:
        raise ValueError("rho must have shape %s" % (shp["rho"],))
    ins = {}
    for k, v in (("sigma", sigma), ("lapl", lapl), ("tau", tau)):
        ins[k] = np.zeros(shp[k]) if v is None else np.ascontiguousarray(np.broadcast_to(v, shp[k]), dtype=np.float64)
    out = {"exc": np.zeros(npt)}
    for k, src in (("vrho", "rho"), ("vsigma", "sigma"), ("vlapl", "lapl"), ("vtau", "tau")):
        out[k] = np.zeros(shp[src])
    if pars is not None and len(pars):
        pv = np.ascontiguousarray(pars, dtype=np.float64)
        f = lib().hfg_xc_eval_ext
        f.argtypes = [ctypes.c_int, c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64] + [c_double_p] * 9 + [ctypes.c_double]
        _check(f(int(func_id), _p(pv), len(pv), nspin, npt, _p(rho), _p(ins["sigma"]), _p(ins["lapl"]), _p(ins["tau"]),
                 _p(out["exc"]), _p(out["vrho"]), _p(out["vsigma"]), _p(out["vlapl"]), _p(out["vtau"]), float(thr)))
        return out
    f = lib().hfg_xc_eval
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64] + [c_double_p] * 9 + [ctypes.c_double]
    _check(f(int(func_id), nspin, npt, _p(rho), _p(ins["sigma"]), _p(ins["lapl"]), _p(ins["tau"]), _p(out["exc"]),
             _p(out["vrho"]), _p(out["vsigma"]), _p(out["vlapl"]), _p(out["vtau"]), float(thr)))
    return out


def xc_eval_ext(func_id, pars, rho, sigma=None, lapl=None, tau=None, nspin=1, thr=0.0):
    """xc_eval with the external parameters of the functional for this call (hfg_xc_eval_ext): lda_x [alpha], gga_x_pbe
    [kappa, mu], gga_c_pbe [beta, gamma, BB], gga_x_ityh / gga_x_sfat / gga_x_ityh_pbe / gga_x_sfat_pbe [omega]"""
    return xc_eval(func_id, rho, sigma, lapl, tau, nspin, thr, pars=pars)


def xc_func_ids(method):
    """--method string -> (x_func, c_func) libxc ids (the drivers' parse_xc_func)"""
    x, c = ctypes.c_int(), ctypes.c_int()
    f = lib().hfg_xc_func_ids
    f.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    _check(f(method.encode(), ctypes.byref(x), ctypes.byref(c)))
    return x.value, c.value


def xc_func_name(func_id):
    f = lib().hfg_xc_func_name
    f.restype = ctypes.c_char_p
    f.argtypes = [ctypes.c_int]
    return f(int(func_id)).decode()


def xc_exact_exchange(x_func):
    """exact exchange the drivers add for an exchange id (hfg_xc_exact_exchange): (omega, alpha, beta) of
    K = alpha K[1/r12] + beta K[screened kernel of range omega]"""
    o, a, b = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    f = lib().hfg_xc_exact_exchange
    f.argtypes = [ctypes.c_int] + [ctypes.POINTER(ctypes.c_double)] * 3
    _check(f(int(x_func), ctypes.byref(o), ctypes.byref(a), ctypes.byref(b)))
    return o.value, a.value, b.value


def xc_func_table():
    """the functionals of the native library (hfg_xc_func_table; no device needed): a list of dicts, one per functional, with
    id, name, role ("x", "c", "xc"), the inputs it needs (grad, tau, lapl), ext (0, or which branch of the EXT instantiation
    evaluates it), skip_dead (left out as a whole where a spin channel is below the threshold), what the drivers add as exact
    exchange (kfrac, kshort, omega, rs_kind), its external parameters (npar, pars: a tuple of names) and a remark"""
    buf = ctypes.create_string_buffer(1 << 16)
    _check(lib().hfg_xc_func_table(buf, ctypes.c_size_t(len(buf))))
    keys = ("id", "name", "role", "grad", "tau", "lapl", "ext", "skip_dead", "kfrac", "kshort", "omega", "rs_kind", "npar", "pars", "remark")
    conv = dict(id=int, grad=lambda v: v == "1", tau=lambda v: v == "1", lapl=lambda v: v == "1", ext=int, skip_dead=lambda v: v == "1",
                kfrac=float, kshort=float, omega=float, rs_kind=int, npar=int, pars=lambda v: tuple(v.split(",")) if v else ())
    rows = [dict(zip(keys, line.split("\t"))) for line in buf.value.decode().split("\n") if line]
    return [{k: conv.get(k, str)(v) for k, v in row.items()} for row in rows]


def xc_rs_kind(x_func):
    """screened kernel of an exchange id (hfg_xc_rs_kind): 0 none, 1 Yukawa, 2 erfc -- the rs_kind of compute_rs_tei"""
    f = lib().hfg_xc_rs_kind
    f.argtypes = [ctypes.c_int]
    f.restype = ctypes.c_int
    return int(f(int(x_func)))


def scf_set_iguess(iguess):
    """--iguess of the drivers for the following scf_* calls of this thread: 0 core Hamiltonian, 3 Thomas-Fermi"""
    _check(lib().hfg_scf_set_iguess(int(iguess)))


def scf_diatomic(Z1, Z2, Rbond, lmmax, nelem, nnodes, method, nquad=0, Rmax=40.0, igrid=4, zexp=1.0, lpad=10, ldft=0,
                 mdft=0, symmetry=1, maxit=50, convthr=1e-7, verbose=0, ctx=None, M=1, occs=None, readocc=-1):
    """Restricted closed-shell (M=1) or unrestricted (M=2S+1>1) diatomic SCF with every per-iteration step on the GPU
    (the loop of src/diatomic/main.cpp:780-995; flags as in main.cpp:89-133)."""
    ctx = ctx or default_context()
    L = lib()
    L.hfg_scf_diatomic.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_int_p, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                   ctypes.c_double, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, c_double_p]
    out = np.zeros(12)
    lm = (ctypes.c_int * len(lmmax))(*lmmax)
    scf_set_occupations(occs, readocc)
    try:
        _check(L.hfg_scf_diatomic(ctx.h, Z1, Z2, Rbond, lm, len(lmmax), nelem, nnodes, nquad, Rmax, igrid, zexp, lpad,
                                  method.encode(), ldft, mdft, symmetry, M, maxit, convthr, verbose, _p(out)))
    finally:
        scf_set_occupations(None)
    keys = ["Etot", "Ekin", "Epot", "Ecoul", "Exx", "Exc", "Enucr"]
    r = dict(zip(keys, out[:7]))
    r["iterations"] = int(out[7])
    r["converged"] = (out[7] - int(out[7])) > 0.25
    r["tJ"], r["tK"], r["tXC"], r["tdiag"] = out[8:12]
    return r


def scf_run_atomic(Z, lmax, mmax, nelem, nnodes, method="HF", ctx=None, check_only=False, E=None, C=None, extras=None, **kw):
    """One run of the atomic program through hfg_scf_run_ex.  extras: dict of hfg_scf_atomic_extras fields (Rrms, conf_N, conf_R,
    conf_barrier, shift_conf, add_conf, Zl, Zr, Rmid, nelem0, grid0, zexp0), None for hfg_scf_run's behaviour; kw: fields of
    hfg_scf_options (finitenuc, iconf, zeroder, symmetry, save, load, ...).  Returns a dict of the result fields plus Econf.
    check_only: hfg_scf_options_check_ex alone (no device)."""
    o = hfg_scf_options()
    _check(lib().hfg_scf_options_default(ctypes.byref(o), 1))
    o.Z1, o.lmax, o.mmax, o.nelem, o.nnodes = int(Z), int(lmax), int(mmax), int(nelem), int(nnodes)
    o.method = method.encode()
    o.verbose = 0
    o.save = b""
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError("hfg_scf_options has no field %s" % k)
        setattr(o, k, v.encode() if isinstance(v, str) else v)
    x = None
    if extras is not None:
        x = hfg_scf_atomic_extras()
        _check(lib().hfg_scf_atomic_extras_default(ctypes.byref(x)))
        for k, v in extras.items():
            if not hasattr(x, k):
                raise TypeError("hfg_scf_atomic_extras has no field %s" % k)
            setattr(x, k, v)
    xp = ctypes.byref(x) if x is not None else None
    if check_only:
        _check(lib().hfg_scf_options_check_ex(ctypes.byref(o), xp))
        return None
    ctx = ctx or default_context()
    r = hfg_scf_result()
    _check(lib().hfg_scf_run_ex(ctx.h, ctypes.byref(o), xp, ctypes.byref(r), _p(E) if E is not None else None,
                                _p(C) if C is not None else None))
    out = dict((f[0], getattr(r, f[0])) for f in hfg_scf_result._fields_)
    out["Econf"] = x.Econf if x is not None else 0.0
    return out


def scf_set_occupations(occs=None, readocc=-1):
    """--readocc for the following scf_diatomic / scf_atomic calls of this thread: occs = rows of occs.dat (nalpha, nbeta, m
    [, parity | l, m]); None switches it off"""
    L = lib()
    L.hfg_scf_set_occupations.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    if occs is None:
        _check(L.hfg_scf_set_occupations(0, 0, 0, None))
        return
    a = np.ascontiguousarray(np.asarray(occs, dtype=np.int32))
    _check(L.hfg_scf_set_occupations(int(readocc), a.shape[0], a.shape[1], a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))


def scf_atomic(Z, lmax, mmax, nelem, nnodes, method, Q=0, nquad=0, Rmax=40.0, igrid=4, zexp=2.0, ldft=0, mdft=0,
               symmetry=1, maxit=50, convthr=1e-7, verbose=0, ctx=None, M=1, maverage=False, occs=None, readocc=-1):
    """Restricted closed-shell (M=1), unrestricted (M=2S+1>1) or restricted open-shell (M<0) atomic SCF with every per-iteration step on the GPU
    (the loop of src/atomic/main.cpp:760-1005; flags as in main.cpp:66-100)."""
    ctx = ctx or default_context()
    L = lib()
    L.hfg_scf_atomic.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 7 + [ctypes.c_double, ctypes.c_int,
                                ctypes.c_double, ctypes.c_char_p] + [ctypes.c_int] * 6 + [ctypes.c_double,
                                ctypes.c_int, c_double_p]
    out = np.zeros(12)
    scf_set_occupations(occs, readocc)
    try:
        _check(L.hfg_scf_atomic(ctx.h, Z, Q, lmax, mmax, nelem, nnodes, nquad, Rmax, igrid, zexp, method.encode(), ldft,
                                mdft, symmetry, M, 1 if maverage else 0, maxit, convthr, verbose, _p(out)))
    finally:
        scf_set_occupations(None)
    keys = ["Etot", "Ekin", "Epot", "Ecoul", "Exx", "Exc", "Enucr"]
    r = dict(zip(keys, out[:7]))
    r["iterations"] = int(out[7])
    r["converged"] = (out[7] - int(out[7])) > 0.25
    r["tJ"], r["tK"], r["tXC"], r["tdiag"] = out[8:12]
    return r


class DeviceDIIS(object):
    """hfg_diis: the reference's uDIIS (update / solve_F, src/general/diis.cpp) on matrices in HBM.  Matrices are torch
    tensors on the context's device holding N x N (Sinvh: N x n) doubles column-major, flat or two-dimensional, as the step
    objects keep theirs; the calls are queued on the context's stream, update() synchronises it once in steady state (the
    first use of a ring slot uploads its task list, with one more), solve() not at all."""

    def __init__(self, ctx, N, nspin, order=5, diiseps=1e-2, diisthr=1e-3, mode=0):
        self.h = None
        self.ctx, self.N, self.nspin, self.order, self.n = ctx, int(N), int(nspin), int(order), int(N)
        h = ctypes.c_void_p()
        _check(lib().hfg_diis_create(ctx.h, self.N, self.nspin, self.order, float(diiseps), float(diisthr), int(mode), ctypes.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            if self.ctx.h:  # (a context closed first has taken its stream with it: nothing to wait for or to free on)
                lib().hfg_diis_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _dp(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def _mat(self, t, cols, what):
        if t is None:
            return None
        if not (t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch.float64" and t.numel() >= self.N * cols):
            raise ValueError("DeviceDIIS: %s must be a contiguous float64 tensor on the device with at least %d x %d elements"
                             % (what, self.N, cols))
        return t

    def set_metric(self, S, Sinvh):
        """overlap S (N x N) and Sinvh (N x n); both are copied.  Empties the history and forgets the blocks"""
        n = Sinvh.numel() // self.N
        if n * self.N != Sinvh.numel():
            raise ValueError("DeviceDIIS.set_metric: Sinvh is N x n")
        _check(lib().hfg_diis_set_metric_devptr(self.h, self._dp(self._mat(S, self.N, "S")), self._dp(self._mat(Sinvh, n, "Sinvh")), n))
        self.n = n

    def set_blocks(self, m_idx):
        """symmetry blocks (lists of basis-function indices, as scf.eig_gsym_sub takes them); None or [] removes them"""
        ptr, idx = scf._blocks(m_idx or [])
        _check(lib().hfg_diis_set_blocks(self.h, len(m_idx or []), ptr.ctypes.data_as(c_i64_p), idx.ctypes.data_as(c_i64_p)))

    def update(self, E, Fa, Pa, Ca=None, nocca=0, Fb=None, Pb=None, Cb=None, noccb=0):
        """new entry; returns max |err|.  Ca / Cb: the orbitals whose first nocca / noccb columns formed Pa / Pb"""
        if self.nspin == 2 and (Fb is None or Pb is None):
            raise ValueError("DeviceDIIS.update: nspin = 2 needs Fb and Pb")
        if self.nspin == 1 and (Fb is not None or Pb is not None):
            raise ValueError("DeviceDIIS.update: nspin = 1 takes one spin")
        err = ctypes.c_double()
        _check(lib().hfg_diis_update_devptr(self.h, float(E), self._dp(self._mat(Fa, self.N, "Fa")), self._dp(self._mat(Pa, self.N, "Pa")),
                                            self._dp(self._mat(Ca, int(nocca), "Ca")), int(nocca) if Ca is not None else 0,
                                            self._dp(self._mat(Fb, self.N, "Fb")), self._dp(self._mat(Pb, self.N, "Pb")),
                                            self._dp(self._mat(Cb, int(noccb), "Cb")), int(noccb) if Cb is not None else 0,
                                            ctypes.byref(err)))
        return err.value

    def solve(self, Fa, Fb=None):
        """the extrapolated Fock matrices into Fa (and Fb); returns the number of old entries the extrapolation dropped"""
        if self.nspin == 2 and Fb is None:
            raise ValueError("DeviceDIIS.solve: nspin = 2 needs Fb")
        dropped = ctypes.c_int()
        _check(lib().hfg_diis_solve_devptr(self.h, self._dp(self._mat(Fa, self.N, "Fa")), self._dp(self._mat(Fb, self.N, "Fb")),
                                           ctypes.byref(dropped)))
        return dropped.value

    @property
    def size(self):
        return int(lib().hfg_diis_size(self.h))

    def _get(self, which, count):
        out = np.zeros(max(count, 1))
        _check(lib().hfg_diis_get(self.h, which, _p(out), count))
        return out[:count]

    @property
    def B(self):
        k = self.size
        return self._get(0, k * k).reshape(k, k)

    @property
    def T(self):
        k = self.size
        return self._get(1, k * k).reshape(k, k)

    @property
    def weights(self):
        """weights of the last solve, oldest entry first"""
        return self._get(2, self.size)

    @property
    def error(self):
        """error matrix of the newest entry, (nspin, n, n)"""
        n = self.n
        return self._get(3, self.nspin * n * n).reshape(self.nspin, n, n).transpose(0, 2, 1)


# HELFEM_EXL_MIX unset: whether a screened kernel's hybrids (1 Yukawa, 2 erfc) take the mixed-kernel table set; as measured
# (profiles/exl_mix_time.txt) the one build's latency is 1.9 to 3.3 times shorter than that of the step objects' two builds, for both kernels
MIX_BY_DEFAULT = {1: True, 2: True}


def _refuse_out_of_scope(who, rohf, cuhf, readocc, maverage, dampfock):
    """what the step objects' run() leaves to the drivers (hfg_scf_run)"""
    bad = [name for name, on in (("ROHF", rohf), ("CUHF", cuhf), ("readocc", readocc is not None and int(readocc) >= 0),
                                 ("maverage", maverage), ("dampfock", float(dampfock) != 1.0)) if on]
    if bad:
        raise NotImplementedError("%s.run: %s not supported by the step objects; use the SCF drivers (scf_diatomic, scf_atomic, "
                                  "scf_run_atomic)" % (who, ", ".join(bad)))


def _exchange_route(mix, kfrac, kshort, have_C, batch):
    """the library entries of one exchange build, in call order, as (entry, destination): "K" the matrix handed on, "Krs" the
    screened matrix of the two-build route, which the caller then adds (K = kfrac K + kshort Krs).  mix: the mixed-kernel
    table set is there and one build returns the weighted sum; have_C: the occupied orbitals the density was formed from
    are at hand (the screened build never takes them); batch: several densities in one pass (HELFEM_USCF_KBATCH)"""
    if mix:
        if batch:  # the one batched entry takes null orbitals and counts without have_C
            return [("hfg_mix_exchange_occ_batch_devptr", "K")]
        return [("hfg_mix_exchange_occ_devptr" if have_C else "hfg_mix_exchange_devptr", "K")]
    plain, occ, screened = (("hfg_exchange_batch_devptr", "hfg_exchange_occ_batch_devptr", "hfg_rs_exchange_batch_devptr") if batch
                            else ("hfg_exchange_dev", "hfg_exchange_occ_dev", "hfg_rs_exchange_dev"))
    route = []
    if kfrac != 0.0:
        route.append((occ if have_C else plain, "K"))
    if kshort != 0.0:
        route.append((screened, "Krs"))
    return route


class DeviceSCFStep(object):
    """One SCF iteration's hot path, device resident (torch tensors are only used as HBM buffers):

        P --(J + XC, compact, sharded)--> all-reduce --> F = sym(H0+J+XC) --(eig blocks, sharded)-->
        all-reduce --> (E, C) --> P' = C_occ C_occ^T

    i.e. main.cpp:784-788, 808-900 and 934-971 of the reference's diatomic driver without DIIS.

    step() and run() are written once, here, as compositions of stages, and the stages that act spin by spin (eigensolve,
    density, core guess, adding K) loop over _spins(), of which this class has one.  A subclass supplies its buffers and
    what differs for them: the Fock build's entries, the exchange densities, the energy terms, the DIIS hand-over, the
    one-call eigensolve and when it is taken (_eig_in_one_call), and the hook between Fock build and eigensolve (_constrain).
    """

    def __init__(self, basis, x_func, c_func, ldft, mdft, nocc, symmetry=1, device=0, rank=0, nranks=1,
                 dens_thr=1e-12, kfrac=0.0, device_tei=False, fock_shard="auto", kshort=0.0, omega=0.0, rs_kind=None):
        self.nocc = int(nocc)
        self._setup(basis, x_func, c_func, ldft, mdft, symmetry, device, rank, nranks, dens_thr, kfrac, device_tei, fock_shard,
                    kshort, omega, rs_kind)
        f64 = dict(dtype=self.torch.float64, device=self.dev)
        L, N = lib(), self.N
        self.Fc = self.torch.zeros(int(L.hfg_fock_compact_size(basis.h)), **f64)
        self.scal = self.torch.zeros(3, **f64)
        self.F = self.torch.zeros(N * N, **f64)
        self.E = self.torch.zeros(N, **f64)
        self.C = self.torch.zeros(N * N, **f64)
        self.P = self.torch.zeros(N * N, **f64)
        nb = int(L.hfg_eig_block_buf_size(len(self.blocks), self.blk_ptr.ctypes.data_as(c_i64_p)))
        self.blockbuf = self.torch.zeros(nb, **f64)
        if self.anyK:
            self.K = self.torch.zeros(N * N, **f64)
            self.Pa = self.torch.zeros(N * N, **f64)

    def _setup(self, basis, x_func, c_func, ldft, mdft, symmetry, device, rank, nranks, dens_thr, kfrac, device_tei, fock_shard,
               kshort=0.0, omega=0.0, rs_kind=None):
        """what the restricted and the unrestricted step share: context, shard, tables, symmetry blocks and their declaration"""
        # range-separated hybrids: F += kfrac K[1/r12] + kshort K[screened kernel of range omega] (atomic/main.cpp:763-780)
        self.kshort, self.omega = float(kshort), float(omega)
        self.rs_kind = 0
        self.mix = False  # K from one build on the mixed-kernel table set
        self.Krs = None   # the screened matrix of the two-build route
        if self.kshort != 0.0:
            if not isinstance(basis, AtomicTwoDBasis):
                raise RuntimeError("Range separated functionals are not supported.")  # diatomic/main.cpp:393
            self.rs_kind = xc_rs_kind(x_func) if rs_kind is None else int(rs_kind)
            if self.rs_kind not in (1, 2) or self.omega == 0.0:
                raise ValueError("kshort != 0 needs a screened kernel (rs_kind 1 Yukawa or 2 erfc, from the exchange functional "
                                 "when None) and its range omega != 0")
        import torch
        self.torch = torch
        self.basis = basis
        self.x_func, self.c_func, self.thr = int(x_func), int(c_func), float(dens_thr)
        self.dev = torch.device("cuda", device)
        torch.cuda.set_device(self.dev)
        self.ctx = Context(device, stream=torch.cuda.current_stream(self.dev).cuda_stream)
        self.ctx.set_shard(rank, nranks)
        self.rank, self.nranks = int(rank), int(nranks)
        # J + XC: "always" shards the build over the ranks ((L,|M|) channels, radial points) and all-reduces the compact
        # buffer; "never" lets every rank build all of it.  "auto" = never: after sum factorisation the whole J + XC build
        # takes 1.1 ms at Nbf = 4230 and 2.9 ms at 6102, less than an all-reduce of its 33 / 69 MB compact buffer over
        # xGMI.  The exchange build (tens of ms) and the eigensolve's blocks are always sharded.
        self.fock_shard = os.environ.get("HELFEM_FOCK_SHARD", fock_shard)  # the environment wins (tests, A/B runs)
        if device_tei:  # in-element tables (with the exchange-ordered ones when K is wanted) built on this context's device
            basis.compute_tei(float(kfrac) != 0.0 or self.kshort != 0.0, device=True, ctx=self.ctx)
        if self.kshort != 0.0:
            # the screened tables: on the device with device_tei, otherwise where HELFEM_RS_TEI puts the drivers' (host: threaded
            # host code and upload)
            switches = {r["name"]: r["value"] for r in tuning_table()}
            on_device = bool(device_tei) or switches["HELFEM_RS_TEI"] == "dev"
            basis._compute_rs(self.rs_kind, self.omega, on_device, self.ctx)
        basis.upload(ldft, mdft, ctx=self.ctx)
        if self.kshort != 0.0:
            # HELFEM_EXL_MIX: 0 the two builds (checker), positive the mixed set, negative (default) by kernel kind as measured
            want = int(switches["HELFEM_EXL_MIX"])
            if want > 0 or (want < 0 and MIX_BY_DEFAULT[self.rs_kind]):
                # False: beyond the bound of the pair path, nothing allocated -- the two-build route
                self.mix = basis.mix_exchange_tables(float(kfrac), self.kshort, ctx=self.ctx)
        N = basis.Nbf()
        self.N = N
        self.blocks = basis.get_sym_idx(symmetry)
        self.blk_ptr, self.blk_idx = scf._blocks(self.blocks)
        blockid = np.zeros(N, dtype=np.int32)
        for ib, b in enumerate(self.blocks):
            blockid[b] = ib
        self.blockid = torch.from_numpy(blockid).to(self.dev)
        # fock_finish masks F with these blocks: the build need not compute the shell pairs outside them
        self.ctx.set_fock_blocks(basis, self.blockid.data_ptr())
        self.H0 = None
        self.Sinvh = None
        # hybrid functionals: F += kfrac K[Pa] (main.cpp:820-877); K is dense, its shards (output shells j % n == rank) sum
        self.kfrac = float(kfrac)
        self.anyK = self.kfrac != 0.0 or self.kshort != 0.0
        # what _add_exchange and the energy multiply self.K with: with a screened term exchange() leaves the weighted sum
        self.kscale = self.kfrac if self.kshort == 0.0 else 1.0
        self.have_C = False
        self.have_density = False  # set_density() or density() has filled the density buffers
        if self.kshort != 0.0 and not self.mix:
            self.Krs = torch.zeros(N * N, dtype=torch.float64, device=self.dev)

    def _ptr(self, t):
        return ctypes.c_void_p(t.data_ptr())

    def set_matrices(self, H0, Sinvh):
        t = self.torch
        self.H0 = t.from_numpy(np.asfortranarray(H0).ravel(order="F").copy()).to(self.dev)
        self.ctx.fix_sinvh(None)
        self.Sinvh = t.from_numpy(np.asfortranarray(Sinvh).ravel(order="F").copy()).to(self.dev)
        self.ctx.fix_sinvh(self.Sinvh.data_ptr())  # constant until the next set_matrices
        # F = H0 + J + XC is local in the radial element index: the eigensolve skips the structural zeros of F in F X.  Not with
        # exact or screened exchange in F, not under the CUHF constraint; an H0 with an entry outside the pattern refuses it
        # (ctx.fock_band_state() tells)
        if not self.anyK and not self._applies_cuhf:
            self.ctx.declare_fock_band(self.basis, self.H0.data_ptr(), self.blockid.data_ptr())

    def set_density(self, P, C=None):
        """total density P = 2 C_occ C_occ^T; C (N x >= nocc, optional): the orbitals it was formed from, which the exact
        exchange takes as the factors of P/2 (as inside the SCF loop, where the driver has just formed P from them)"""
        self.P.copy_(self.torch.from_numpy(np.asfortranarray(P).ravel(order="F").copy()))
        self.have_density = True
        self.have_C = C is not None
        if C is not None:
            self.C[:self.N * self.nocc].copy_(self.torch.from_numpy(np.asfortranarray(C[:, :self.nocc]).ravel(order="F").copy()))

    def exchange(self):
        """K[Pa], Pa = P/2 (closed shell; basis.exchange(Pa) of main.cpp:822) into self.K"""
        self.torch.mul(self.P, 0.5, out=self.Pa)
        self._build_K(self.Pa, self.C, ctypes.c_int64(self.nocc), self.K)

    def _build_K(self, P, C, nocc, K, batch=0):
        """the exchange matrix of one density into K, or (batch = their number) of several, stored one after the other in P,
        C and K with nocc a pointer to their counts: K[P] without a screened term (the caller weights it with kfrac); with
        one, kfrac K[P] + kshort K_screened[P], from one build on the mixed set or (HELFEM_EXL_MIX=0, a set beyond the bound)
        from the two table sets, added on the device.  Which entries: _exchange_route"""
        L = lib()
        head = (self.ctx.h, self.basis.h, batch) if batch else (self.ctx.h, self.basis.h)
        for name, dest in _exchange_route(self.mix, self.kfrac, self.kshort, self.have_C, bool(batch)):
            args = [self._ptr(P)]
            if "_occ_" in name:
                args += [self._ptr(C), nocc] if self.have_C else [None, None]
                if batch:
                    args.append(self.N)  # columns per set of orbitals
            _check(getattr(L, name)(*head, *args, self._ptr(K if dest == "K" else self.Krs)))
        if self.kshort != 0.0 and not self.mix:
            if self.kfrac != 0.0:
                K.mul_(self.kfrac).add_(self.Krs, alpha=self.kshort)
            else:
                self.torch.mul(self.Krs, self.kshort, out=K)

    def fock_partial(self):
        _check(lib().hfg_fock_compact_dev(self.ctx.h, self.basis.h, self.x_func, self.c_func, self._ptr(self.P),
                                          self._ptr(self.Fc), self._ptr(self.scal), self.thr))

    def fock_finish(self):
        _check(lib().hfg_fock_finish_dev(self.ctx.h, self.basis.h, self._ptr(self.Fc), self._ptr(self.H0),
                                         self._ptr(self.blockid), self._ptr(self.F)))

    def _spins(self):
        """(P, F, E, C, nocc) per spin: what the stages below loop over"""
        return ((self.P, self.F, self.E, self.C, self.nocc),)

    def _blockbufs(self):
        """the eigensolve's block slots, one buffer per spin"""
        return (self.blockbuf,)

    def _spin_K(self):
        """the exchange matrix of each spin, as exchange() leaves them"""
        return (self.K,)

    def eig_partial(self):
        for (_, F, _, _, _), buf in zip(self._spins(), self._blockbufs()):
            _check(lib().hfg_eig_blocks_dev(self.ctx.h, ctypes.c_int64(self.N), self._ptr(F), self._ptr(self.Sinvh),
                                            len(self.blocks), self.blk_ptr.ctypes.data_as(c_i64_p),
                                            self.blk_idx.ctypes.data_as(c_i64_p), self._ptr(buf)))

    def eig_finish(self):
        for (_, _, E, C, _), buf in zip(self._spins(), self._blockbufs()):
            _check(lib().hfg_eig_assemble_dev(self.ctx.h, ctypes.c_int64(self.N), len(self.blocks),
                                              self.blk_ptr.ctypes.data_as(c_i64_p), self.blk_idx.ctypes.data_as(c_i64_p),
                                              self._ptr(buf), self._ptr(E), self._ptr(C)))

    def eig_whole(self):
        """the eigensolve of one rank in one call (hfg_eig_gsym_sub_dev): no block slots between two phases"""
        _check(lib().hfg_eig_gsym_sub_dev(self.ctx.h, ctypes.c_int64(self.N), self._ptr(self.F), self._ptr(self.Sinvh),
                                          len(self.blocks), self.blk_ptr.ctypes.data_as(c_i64_p),
                                          self.blk_idx.ctypes.data_as(c_i64_p), self._ptr(self.E), self._ptr(self.C)))

    def density(self):
        """P_s = C_s,occ C_s,occ^T of every spin; a spin without electrons gets a zero density"""
        for P, _, _, C, nocc in self._spins():
            if nocc == 0:
                P.zero_()
                continue
            _check(lib().hfg_form_density_dev(self.ctx.h, ctypes.c_int64(self.N), ctypes.c_int64(self.N), self._ptr(C),
                                              ctypes.c_int64(nocc), self._ptr(P)))
        self.have_density = True

    def step(self, allreduce=None, exchange_blocks=None):
        """one iteration: Fock build, the subclass's constraint (DeviceROHFStep), eigensolve, density.  allreduce(tensor)
        sums a tensor over ranks in place (None: single GPU); exchange_blocks(buffer, nblk) completes the per-block
        eigenvector slots on every rank (parallel.broadcast_block_slots_: one broadcast per block from its owner; None: the
        sum all-reduce, which the zero padding of the slots owned elsewhere also makes correct).  Every rank issues the same
        collectives in the same order: Fc, scal, K, then the block buffer of each spin.
        The restricted step leaves P = C_occ C_occ^T, half the total density that set_density() and the Fock build take:
        the caller doubles it before the next step() (run() does, through _density_stage)."""
        self._fock_stage(allreduce)
        self._constrain()
        self._eig_stage(allreduce, exchange_blocks)
        self.density()
        self.have_C = True  # C now holds the orbitals P was formed from

    def _whole_shard(self, fn):
        """fn() with the context unsharded: what every rank computes whole (J + XC under fock_shard != "always", the J of
        the Coulomb energy)"""
        if self.nranks > 1:
            self.ctx.set_shard(0, 1)
        try:
            fn()
        finally:
            if self.nranks > 1:
                self.ctx.set_shard(self.rank, self.nranks)

    def _fock_stage(self, allreduce):
        """the Fock-build half of step(): fock_partial, collectives, fock_finish, exchange.  J + XC is built whole on every
        rank, without a collective, unless fock_shard is "always"; K is always sharded"""
        shard_fock = self.nranks > 1 and self.fock_shard == "always"
        if shard_fock or self.nranks == 1:
            self.fock_partial()
            if allreduce is not None:
                allreduce(self.Fc)
                allreduce(self.scal)
        else:
            self._whole_shard(self.fock_partial)
        self.fock_finish()
        if self.anyK:
            self.exchange()
            if allreduce is not None:
                allreduce(self.K)
            self._add_exchange()

    def _add_exchange(self):
        """F_s += kscale K_s.  K of a block-diagonal density is block diagonal: no mask needed"""
        for (_, F, _, _, _), K in zip(self._spins(), self._spin_K()):
            F.add_(K, alpha=self.kscale)

    def _eig_in_one_call(self, allreduce, exchange_blocks):
        return self.nranks == 1 and allreduce is None and exchange_blocks is None

    def _eig_stage(self, allreduce, exchange_blocks):
        """the eigensolve half of step(): one call (eig_whole) where _eig_in_one_call allows, else eig_partial, the block
        buffers' collective spin by spin (exchange_blocks wins over allreduce), eig_finish"""
        if self._eig_in_one_call(allreduce, exchange_blocks):
            self.eig_whole()
            return
        self.eig_partial()
        for buf in self._blockbufs():
            if exchange_blocks is not None:
                exchange_blocks(buf, len(self.blocks))
            elif allreduce is not None:
                allreduce(buf)
        self.eig_finish()

    # ---- the converging loop: main.cpp:780-995 composed from the stages above, DIIS by a DeviceDIIS --------------------
    def _nn_buffer(self, name):
        """the N x N device buffer self.<name>, created when first asked for: step() alone needs none of them (J is 298 MB
        at Nbf = 6102)"""
        buf = getattr(self, name, None)
        if buf is None:
            buf = self.torch.zeros(self.N * self.N, dtype=self.torch.float64, device=self.dev)
            setattr(self, name, buf)
        return buf

    def _coulomb_energy_matrix(self, P):
        J = self._nn_buffer("J")
        self._whole_shard(lambda: _check(lib().hfg_coulomb_dev(self.ctx.h, self.basis.h, self._ptr(P), self._ptr(J))))
        return J

    def _energy_terms(self):
        """device scalars [E1, 2 Ecoul, Exx / _exx_factor()]"""
        t = self.torch
        J = self._coulomb_energy_matrix(self.P)
        terms = [t.dot(self.P, self.H0), t.dot(self.P, J)]
        terms.append(t.dot(self.Pa, self.K) if self.anyK else t.zeros((), dtype=t.float64, device=self.dev))
        return terms

    def energy(self, Enucr=0.0):
        """energies of main.cpp:808-900 for the density of the last Fock build (fock_partial ... exchange): E1 = tr(P H0),
        Ecoul = 1/2 tr(P J[P]) with J built whole on every rank (one extra Coulomb build: the fused build returns only
        J + XC), Exx from the K that exchange() left, Exc = scal[0].  One read-back of four doubles."""
        t = self.torch
        v = t.stack(self._energy_terms() + [self.scal[0]]).cpu().numpy()
        r = dict(E1=float(v[0]), Ecoul=0.5 * float(v[1]), Exx=self._exx_factor() * float(v[2]), Exc=float(v[3]), Enucr=float(Enucr))
        r["Etot"] = r["E1"] + r["Ecoul"] + r["Exx"] + r["Exc"] + r["Enucr"]
        return r

    def _exx_factor(self):
        return self.kscale  # Exx = tr(Pa kfrac K[Pa]), Pa = P / 2, both spins (a screened term: K holds the weighted sum)

    def _nspin(self):
        return 1

    def _density_stage(self):
        """density() leaves C_occ C_occ^T in P; the Fock build takes the total density of the closed shell, twice that"""
        self.density()
        self.P.mul_(2.0)
        self.have_C = True

    def _core_guess(self, allreduce, exchange_blocks):
        for _, F, _, _, _ in self._spins():
            F.copy_(self.H0)
        self._eig_stage(allreduce, exchange_blocks)
        self._density_stage()

    def _diis_update(self, diis, E):
        Pa = self.torch.mul(self.P, 0.5, out=self._nn_buffer("Pa"))  # (a hybrid's constructor has made Pa already)
        if self.have_C:
            return diis.update(E, self.F, Pa, self.C, self.nocc)
        return diis.update(E, self.F, Pa)

    def _diis_solve(self, diis):
        diis.solve(self.F)

    # the hook of run() between energy() and the DIIS update: nothing here, the CUHF constraint in DeviceROHFStep
    _applies_cuhf = False

    def _constraint_begin(self, S):
        pass

    def _constrain(self):
        pass

    def run(self, S, maxit=50, convthr=1e-7, Enucr=0.0, allreduce=None, exchange_blocks=None, diis=None, callback=None,
            rohf=False, cuhf=False, readocc=None, maverage=False, dampfock=1.0):
        """SCF to convergence: the loop of main.cpp:780-995 with the reference's ADIIS + CDIIS.  S: the overlap matrix (numpy,
        N x N).  Without a density (set_density) the loop starts from the core guess, the eigenvectors of H0 from this step's
        own eigensolver.  Per iteration: Fock build, energy, diis.update with F, P and the occupied orbitals, the driver's
        test max |err| < convthr and |dE| < convthr; unless it holds, diis.solve into F, eigensolve, density.  allreduce and
        exchange_blocks as in step(); every rank runs its own DeviceDIIS on identical inputs, so DIIS adds no collective.
        diis: a DeviceDIIS with its metric set (default: order 5, this step's Sinvh and symmetry blocks); callback(it, Etot,
        maxerr) after every iteration.  Returns the energies of energy() plus iterations, converged and the trace
        [(Etot, maxerr), ...].  Restricted open-shell runs are DeviceROHFStep's, whose hook between energy() and the DIIS
        update applies the CUHF constraint; readocc, maverage and dampfock stay with the drivers.  The keywords rohf, cuhf,
        readocc, maverage and dampfock exist only so that a script ported from the drivers fails loudly (NotImplementedError)
        instead of running without them; they have no other effect (rohf and cuhf are accepted by DeviceROHFStep, which
        applies the constraint with or without them)."""
        _refuse_out_of_scope(type(self).__name__, rohf and not self._applies_cuhf, cuhf and not self._applies_cuhf, readocc, maverage,
                             dampfock)
        if self.H0 is None:
            raise RuntimeError("run: set_matrices first")
        self._constraint_begin(S)
        t = self.torch
        if diis is None:
            diis = DeviceDIIS(self.ctx, self.N, self._nspin())
            dS = t.from_numpy(np.asfortranarray(S, dtype=np.float64).ravel(order="F").copy()).to(self.dev)
            diis.set_metric(dS, self.Sinvh)
            if len(self.blocks) > 1:
                diis.set_blocks(self.blocks)
        if not self.have_density:
            self._core_guess(allreduce, exchange_blocks)
        trace, Eold, res, converged, it = [], 0.0, None, False, 0
        for it in range(1, int(maxit) + 1):
            self._fock_stage(allreduce)
            res = self.energy(Enucr)
            self._constrain()  # (the energy is that of the unconstrained build, as in the drivers)
            maxerr = self._diis_update(diis, res["Etot"])
            dE = res["Etot"] - Eold
            Eold = res["Etot"]
            trace.append((res["Etot"], maxerr))
            if callback is not None:
                callback(it, res["Etot"], maxerr)
            if maxerr < convthr and abs(dE) < convthr:
                converged = True
                break
            self._diis_solve(diis)
            self._eig_stage(allreduce, exchange_blocks)
            self._density_stage()
        res = dict(res or {})
        res.update(iterations=it, converged=converged, trace=trace)
        return res

    def numpy(self, t, shape):
        return t.cpu().numpy().reshape(shape, order="F")


class DeviceUSCFStep(DeviceSCFStep):
    """DeviceSCFStep for an unrestricted iteration (the unrestricted branch of main.cpp:808-900 and 934-971, without DIIS):

        (Pa, Pb) --(J[Pa + Pb] + XC_a | XC_b, compact, sharded)--> all-reduce --> Fa, Fb --(eig blocks of both spins)-->
        (Ea, Ca), (Eb, Cb) --> Pa' = Ca_occ Ca_occ^T, Pb' likewise

    nocc = (nela, nelb) orbitals per spin; nelb = 0 (one-electron systems) leaves Pb and K[Pb] zero.  Set-up (_setup), step(),
    run() and the stages over _spins() are the restricted step's.  What this class overrides: its buffers and the two-entry
    _spins(), set_density, the Fock build's _pol entries, the exchange of two densities, the one-call eigensolve (eig_pair,
    taken on one rank whatever the collectives: the block buffers exist only with several ranks), the energy terms, and
    the DIIS hand-over.
    """

    def __init__(self, basis, x_func, c_func, ldft, mdft, nocc, symmetry=1, device=0, rank=0, nranks=1,
                 dens_thr=1e-12, kfrac=0.0, device_tei=False, fock_shard="auto", kshort=0.0, omega=0.0, rs_kind=None):
        self.nela, self.nelb = int(nocc[0]), int(nocc[1])
        if self.nela < 1 or self.nelb < 0:
            raise ValueError("DeviceUSCFStep: nocc = (nela >= 1, nelb >= 0)")
        self._setup(basis, x_func, c_func, ldft, mdft, symmetry, device, rank, nranks, dens_thr, kfrac, device_tei, fock_shard,
                    kshort, omega, rs_kind)
        t, N, L = self.torch, self.N, lib()
        f64 = dict(dtype=t.float64, device=self.dev)
        self.nc = int(L.hfg_fock_compact_size(basis.h))
        self.Fc = t.zeros(int(L.hfg_fock_compact_pol_size(basis.h)), **f64)
        self.scal = t.zeros(3, **f64)
        for name in ("Pa", "Pb", "Fa", "Fb", "Ca", "Cb"):
            setattr(self, name, t.zeros(N * N, **f64))
        self.Ea, self.Eb = t.zeros(N, **f64), t.zeros(N, **f64)
        if self.nranks > 1:  # the blocks of each spin, solved by their owners
            nb = int(L.hfg_eig_block_buf_size(len(self.blocks), self.blk_ptr.ctypes.data_as(c_i64_p)))
            self.blockbuf_a, self.blockbuf_b = t.zeros(nb, **f64), t.zeros(nb, **f64)
        self.kbatch = False
        if self.anyK:  # one buffer, so that one all-reduce serves both spins
            self.K = t.zeros(2 * N * N, **f64)
            self.Ka, self.Kb = self.K[:N * N], self.K[N * N:]
            # HELFEM_USCF_KBATCH=1 (off by default): both spins through one batched exchange build, from staging buffers
            # that hold (Pa, Pb) and (Ca, Cb) one after the other
            self.kbatch = {r["name"]: r["value"] for r in tuning_table()}["HELFEM_USCF_KBATCH"] == "on"
            if self.kbatch:
                self.Pab, self.Cab = t.zeros(2 * N * N, **f64), t.zeros(2 * N * N, **f64)
                self._nocc = np.array([self.nela, self.nelb], dtype=np.int64)
                if self.Krs is not None:  # the two-build route: both spins' screened matrices side by side
                    self.Krs = t.zeros(2 * N * N, **f64)

    def _spins(self):
        return ((self.Pa, self.Fa, self.Ea, self.Ca, self.nela), (self.Pb, self.Fb, self.Eb, self.Cb, self.nelb))

    def _blockbufs(self):
        return (self.blockbuf_a, self.blockbuf_b)

    def _spin_K(self):
        return (self.Ka, self.Kb)

    def set_density(self, Pa, Pb, Ca=None, Cb=None):
        """spin densities P_s = C_s,occ C_s,occ^T; Ca, Cb (optional, both or neither): the orbitals they were formed from,
        handed to the exact exchange as their factors"""
        as_dev = lambda M: self.torch.from_numpy(np.asfortranarray(M).ravel(order="F").copy())
        self.Pa.copy_(as_dev(Pa))
        self.Pb.copy_(as_dev(Pb))
        self.have_density = True
        self.have_C = Ca is not None and (Cb is not None or self.nelb == 0)
        if self.have_C:
            self.Ca[:self.N * self.nela].copy_(as_dev(Ca[:, :self.nela]))
            if self.nelb:
                self.Cb[:self.N * self.nelb].copy_(as_dev(Cb[:, :self.nelb]))

    def exchange(self):
        """K[Pa] and K[Pb] (basis.exchange of main.cpp:822-829) into self.Ka, self.Kb"""
        if self.kbatch:
            N2 = self.N * self.N
            self.Pab[:N2].copy_(self.Pa)
            self.Pab[N2:].copy_(self.Pb)
            if self.have_C:
                self.Cab[:N2].copy_(self.Ca)
                self.Cab[N2:].copy_(self.Cb)
            self._build_K(self.Pab, self.Cab, self._nocc.ctypes.data_as(c_i64_p), self.K, batch=2)
            return
        for (P, _, _, C, nocc), K in zip(self._spins(), self._spin_K()):
            if nocc == 0:
                K.zero_()
            else:
                self._build_K(P, C, ctypes.c_int64(nocc), K)

    def fock_partial(self):
        _check(lib().hfg_fock_compact_pol_devptr(self.ctx.h, self.basis.h, self.x_func, self.c_func, self._ptr(self.Pa),
                                                 self._ptr(self.Pb), self._ptr(self.Fc), self._ptr(self.scal), self.thr))

    def fock_finish(self):
        _check(lib().hfg_fock_finish_pol_devptr(self.ctx.h, self.basis.h, self._ptr(self.Fc), self._ptr(self.H0),
                                                self._ptr(self.blockid), self._ptr(self.Fa), self._ptr(self.Fb)))

    def eig_pair(self):
        """both spins' blocks in one batch (one rank)"""
        _check(lib().hfg_eig_gsym_sub_pair_devptr(self.ctx.h, ctypes.c_int64(self.N), self._ptr(self.Fa), self._ptr(self.Fb),
                                                  self._ptr(self.Sinvh), len(self.blocks), self.blk_ptr.ctypes.data_as(c_i64_p),
                                                  self.blk_idx.ctypes.data_as(c_i64_p), self._ptr(self.Ea), self._ptr(self.Ca),
                                                  self._ptr(self.Eb), self._ptr(self.Cb)))

    eig_whole = eig_pair  # the eigensolve of one rank in one call, for two spins

    def _eig_in_one_call(self, allreduce, exchange_blocks):
        return self.nranks == 1  # with or without collectives: one rank has no block buffers

    def _energy_terms(self):
        t = self.torch
        Pt = t.add(self.Pa, self.Pb, out=self._nn_buffer("Pt"))
        J = self._coulomb_energy_matrix(Pt)
        terms = [t.dot(Pt, self.H0), t.dot(Pt, J)]
        terms.append(t.dot(self.Pa, self.Ka) + t.dot(self.Pb, self.Kb) if self.anyK
                     else t.zeros((), dtype=t.float64, device=self.dev))
        return terms

    def _exx_factor(self):
        return 0.5 * self.kscale  # Exx = 1/2 (tr Pa kfrac K[Pa] + tr Pb kfrac K[Pb]); a screened term: the weighted sums

    def _nspin(self):
        return 2

    def _density_stage(self):
        self.density()
        self.have_C = True

    def _diis_update(self, diis, E):
        if self.have_C:
            return diis.update(E, self.Fa, self.Pa, self.Ca, self.nela, self.Fb, self.Pb, self.Cb if self.nelb else None, self.nelb)
        return diis.update(E, self.Fa, self.Pa, Fb=self.Fb, Pb=self.Pb)

    def _diis_solve(self, diis):
        diis.solve(self.Fa, self.Fb)


class DeviceROHFStep(DeviceUSCFStep):
    """DeviceUSCFStep for a restricted open-shell iteration, the constrained-UHF form of ROHF (scf::ROHF_update,
    scf_helpers.cpp:470-523; --restricted 1 with nela != nelb in the drivers): after the Fock build, Fa += lambda and
    Fb -= lambda, with lambda the core-virtual coupling of (Fa - Fb) / 2 between the natural orbitals of Pa + Pb, from the
    occupied orbitals the densities were formed from (Context.cuhf_update, hfg_cuhf_update_devptr).  The eigensolve and the
    DIIS history see the constrained matrices; the energy is that of the unconstrained build, as in the drivers.  The
    constraint needs the overlap matrix (run() takes it; set_overlap() before step()) and the orbitals: a density set
    without them (set_density without Ca, Cb) is refused.  Every rank applies it to identical inputs: no collective.
    With symmetry blocks lambda is block diagonal up to rounding when the orbitals are; the eigensolve and the blocked DIIS
    error read the diagonal blocks only.  The class overrides only the hooks of step() and run(): _constrain, between the
    Fock build and the eigensolve, and _constraint_begin, which takes run()'s overlap matrix."""

    _applies_cuhf = True

    def __init__(self, *args, **kw):
        super(DeviceROHFStep, self).__init__(*args, **kw)
        self.S = None

    def set_overlap(self, S):
        """the overlap matrix (numpy, N x N) the constraint is formed with; kept on the device"""
        S = np.asfortranarray(S, dtype=np.float64)
        if S.shape != (self.N, self.N):
            raise ValueError("DeviceROHFStep.set_overlap: S is N x N")
        self.S = self.torch.from_numpy(S.ravel(order="F").copy()).to(self.dev)

    def _constraint_begin(self, S):
        if S is not None:
            self.set_overlap(S)

    def _constrain(self):
        if self.S is None:
            raise RuntimeError("DeviceROHFStep: set_overlap first")
        if not self.have_C:
            raise RuntimeError("DeviceROHFStep: the constraint needs the orbitals the densities were formed from "
                               "(set_density with Ca and Cb, or start from the core guess)")
        self.ctx.cuhf_update(self.S, self.Ca, self.nela, self.Cb, self.nelb, self.Fa, self.Fb)


def spherical_occupations(basis, shells):
    """Occupations per spin orbital of a spherically averaged atom, one list per (l, m) block of basis.get_sym_idx(2): what
    DeviceFracSCFStep takes.  shells = {l: [electrons in the 1st, 2nd, ... shell of that l]}, e.g. carbon {0: [2, 2], 1: [2]}:
    the n electrons of a shell are spread evenly over its 2 (2l + 1) spin orbitals, so every (l, m) block gets the list
    n / (2 (2l + 1)).  ValueError for an l the basis lacks, an l whose m values in the basis do not hold all of -l .. l, a
    shell with more than 2 (2l + 1) electrons, and a diatomic basis (whose blocks carry no l)."""
    if not isinstance(basis, AtomicTwoDBasis):
        raise ValueError("spherical_occupations: an atomic basis is needed: the blocks of a diatomic basis carry no l")
    lm = list(zip(basis.lval, basis.mval))
    for l, electrons in shells.items():
        l = int(l)
        if l < 0 or l not in basis.lval:
            raise ValueError("spherical_occupations: l = %d is beyond the basis (l = 0 .. %d)" % (l, max(basis.lval)))
        missing = [m for m in range(-l, l + 1) if (l, m) not in lm]
        if missing:
            raise ValueError("spherical_occupations: the basis lacks m = %s of l = %d: a shell cannot be spread over all of m = -l .. l"
                             % (", ".join(str(m) for m in missing), l))
        for n in electrons:
            if not 0.0 <= float(n) <= 2 * (2 * l + 1):
                raise ValueError("spherical_occupations: %g electrons in a shell of l = %d, which holds 0 to %d" % (n, l, 2 * (2 * l + 1)))
    by_l = {int(l): [float(n) / (2 * (2 * int(l) + 1)) for n in electrons] for l, electrons in shells.items()}
    return [list(by_l.get(l, [])) for l, _ in lm]


class DeviceFracSCFStep(DeviceSCFStep):
    """DeviceSCFStep with fractional occupations by symmetry block (the occupations of the reference's sadatom program;
    spherical_occupations gives those of a spherically averaged atom).  occupations: one list of floats in [0, 1] per block
    of basis.get_sym_idx(symmetry), lowest level first, each the occupation per spin orbital: the total density is
    P = 2 sum_i f_i c_i c_i^T.  After every eigensolve Context.occupy_blocks puts sqrt(f_i) c_i into the fixed slot of (block,
    level) of the N x nslots panel Cocc, on the device; P/2 = Cocc Cocc^T, so the panel stands wherever the occupied
    orbitals stand in the restricted step, and nocc is nslots: the density build, the factors handed to the exact exchange
    and the rank-nslots DIIS error (which forms X^T (F C C^T S - S C C^T F) X from the columns and nowhere assumes them
    orthonormal).  More than 64 slots take the dense paths, as more than 64 orbitals do.  The class overrides only those
    three hand-overs and set_density, whose optional C is the panel (N x nslots, P/2 = C C^T).  occupied() returns the
    slots' energies and occupations."""

    def __init__(self, basis, x_func, c_func, ldft, mdft, occupations, symmetry=2, **kw):
        nblk = len(basis.get_sym_idx(symmetry))
        if len(occupations) != nblk:
            raise ValueError("DeviceFracSCFStep: %d occupation lists for %d symmetry blocks" % (len(occupations), nblk))
        self.occupations = [[float(f) for f in o] for o in occupations]
        if any(not 0.0 <= f <= 1.0 for o in self.occupations for f in o):
            raise ValueError("DeviceFracSCFStep: occupations per spin orbital lie in [0, 1]")
        nslots = sum(len(o) for o in self.occupations)
        if nslots < 1:
            raise ValueError("DeviceFracSCFStep: no occupation given")
        super(DeviceFracSCFStep, self).__init__(basis, x_func, c_func, ldft, mdft, nslots, symmetry=symmetry, **kw)
        f64 = dict(dtype=self.torch.float64, device=self.dev)
        self.Cocc = self.torch.zeros(self.N * nslots, **f64)
        self.Eocc = self.torch.zeros(nslots, **f64)
        self.Focc = self.torch.zeros(nslots, **f64)

    def set_density(self, P, C=None):
        """total density P = 2 sum_i f_i c_i c_i^T; C (N x nslots, optional): the scaled columns sqrt(f_i) c_i it was formed
        from, slot by slot, which the exact exchange and the DIIS error take as the factors of P/2"""
        super(DeviceFracSCFStep, self).set_density(P, None)
        self.have_C = C is not None
        if C is not None:
            self.Cocc.copy_(self.torch.from_numpy(np.asfortranarray(C[:, :self.nocc]).ravel(order="F").copy()))

    def exchange(self):
        """K[P/2] into self.K, from the factors Cocc"""
        self.torch.mul(self.P, 0.5, out=self.Pa)
        self._build_K(self.Pa, self.Cocc, ctypes.c_int64(self.nocc), self.K)

    def density(self):
        """Cocc from (E, C) by the occupations, then P = Cocc Cocc^T = sum_i f_i c_i c_i^T"""
        self.ctx.occupy_blocks(self.E, self.C, self.blockid, self.occupations, out=(self.Cocc, self.Eocc, self.Focc))
        _check(lib().hfg_form_density_dev(self.ctx.h, ctypes.c_int64(self.N), ctypes.c_int64(self.nocc), self._ptr(self.Cocc),
                                          ctypes.c_int64(self.nocc), self._ptr(self.P)))
        self.have_density = True

    def _diis_update(self, diis, E):
        Pa = self.torch.mul(self.P, 0.5, out=self._nn_buffer("Pa"))
        if self.have_C:
            return diis.update(E, self.F, Pa, self.Cocc, self.nocc)
        return diis.update(E, self.F, Pa)

    def occupied(self):
        """(E, f) of the slots, block after block and lowest level first, as numpy arrays: one read-back"""
        v = self.torch.stack((self.Eocc, self.Focc)).cpu().numpy()
        return v[0].copy(), v[1].copy()
