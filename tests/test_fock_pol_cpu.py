"""The C ABI of the unrestricted fused Fock build, as far as it shows without a device: the header declares the four entries,
the library exports them, the compact size is twice the restricted one, and none of them is named *_dev -- the header's
hfg_*_dev entries are exactly the plan of tests/stream_order_worker.py (tests/test_stream_order_plan_cpu.py); the stream
ordering of the new entries is tested in tests/test_gpu_fock_pol.py."""
import ctypes
import re

import stream_order_worker as sow

NEW = ("hfg_fock_compact_pol_size", "hfg_fock_compact_pol_devptr", "hfg_fock_finish_pol_devptr", "hfg_eig_gsym_sub_pair_devptr")
# the hfg_*_dev entries of the header before these four were added
DEV = {"hfg_compute_tei_dev", "hfg_compute_rs_tei_dev", "hfg_rs_special_dev", "hfg_coulomb_dev", "hfg_exchange_dev", "hfg_rs_exchange_dev",
       "hfg_exchange_occ_dev", "hfg_xc_fock_dev", "hfg_xc_fock_pol_dev", "hfg_fock_compact_dev", "hfg_fock_finish_dev",
       "hfg_eig_gsym_sub_dev", "hfg_eig_gsym_sub_sel_dev", "hfg_eig_blocks_dev", "hfg_eig_assemble_dev", "hfg_form_density_dev",
       "hfg_gemm_dev"}


def test_header_declares_the_entries_and_the_library_exports_them(native_libs):
    import helfem_amd as hf
    text = open(sow.HEADER).read()
    L = hf.lib()
    for name in NEW:
        assert re.search(r"^int(64_t)? %s\(" % name, text, re.M), name
        assert getattr(L, name) is not None
    assert "hfg_fock_compact_pol_devptr" in hf.DeviceUSCFStep.fock_partial.__code__.co_names


def test_dev_named_entries_are_unchanged():
    assert set(sow.header_dev_symbols()) == DEV


def test_compact_size_is_twice_the_restricted_one(native_libs):
    import common
    import helfem_amd as hf
    L = hf.lib()
    L.hfg_fock_compact_size.restype = ctypes.c_int64
    for gb in (common.make_bases(7, 7, 2.068, (3, 2), 2, 5, oracle=False)[0], common.make_atomic_bases(10, 2, 1, 3, 4, oracle=False)[0]):
        nc = int(L.hfg_fock_compact_size(gb.h))
        assert nc > 0 and nc % (gb.Nang() ** 2 * gb.Nel()) == 0
        assert int(L.hfg_fock_compact_pol_size(gb.h)) == 2 * nc
