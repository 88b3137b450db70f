"""The restricted compact Fock build after a refused XC part.  hfg_fock_compact_dev enqueues J on the context's side stream
before the XC part looks its functionals up; an unsupported id makes that part throw "Functional not found!" on the host
while J is under way into the caller's buffer.  The driver of J beside XC (fock_j_beside_xc, hip/fock.hip) then makes the
main stream wait for J before the error leaves, as the unrestricted build always did, so that whatever the caller enqueues
next comes behind it.  Here: the refusal, then a valid build on the same context and into the same buffers, bitwise equal
to the build of a fresh context with its own tables.  Smallest basis of the suite; no kernel faults, the refusal is a host
exception before any XC kernel is launched."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

PBE = (101, 130)


def _build(hf, torch, common, ctx, refuse_first):
    L, V = hf.lib(), ctypes.c_void_p
    gb, _ = common.make_bases(1, 1, 1.4, (1,), 1, 4, oracle=False)
    gb.compute_tei(False)
    gb.upload(4 * 1 + 12, 4 * 1 + 5, ctx=ctx)
    N = gb.Nbf()
    f64 = dict(dtype=torch.float64, device="cuda:0")
    P = torch.tensor(common.random_density(N, 1, seed=3), **f64).contiguous()
    Fc = torch.zeros(int(L.hfg_fock_compact_size(gb.h)), **f64)
    scal = torch.zeros(3, **f64)
    torch.cuda.synchronize()
    args = (V(P.data_ptr()), V(Fc.data_ptr()), V(scal.data_ptr()), 1e-12)
    if refuse_first:
        assert L.hfg_fock_compact_dev(ctx.h, gb.h, 987654, 0, *args) != 0
        assert b"Functional not found!" in L.hfg_last_error()
    hf._check(L.hfg_fock_compact_dev(ctx.h, gb.h, PBE[0], PBE[1], *args))
    ctx.synchronize()
    torch.cuda.synchronize()
    return Fc.cpu(), scal.cpu()


def test_valid_build_after_a_refused_functional_is_that_of_a_fresh_context(native_libs):
    import torch
    import common
    import helfem_amd as hf
    used, fresh = hf.Context(0), hf.Context(0)
    Fc, scal = _build(hf, torch, common, used, True)
    Fc0, scal0 = _build(hf, torch, common, fresh, False)
    assert float(Fc0.abs().max()) > 0.0 and float(scal0[1]) > 0.0  # J + XC and the electron count are there
    assert torch.equal(Fc, Fc0) and torch.equal(scal, scal0)
    used.close()
    fresh.close()
