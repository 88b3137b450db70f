"""Every row of the list of functionals (hfg_xc_func_table) through the XC kernels on the smallest atomic basis of
test_gpu_lapl.py, where the Laplacian rows are legal: each row reaches a launch plan (planes, EXT instantiation) that
integrates the same density.  The values are pinned by the parity tests; here Nel, which no functional enters, is compared
exactly."""
import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu


def test_every_row_reaches_its_launch_plan():
    import helfem_amd as hf
    if hf.device_count() < 1:
        pytest.fail("no HIP device visible")
    gb, _ = common.make_atomic_bases(2, 0, 0, 3, 6, oracle=False)
    gb.compute_tei(True)
    ldft, mdft = 10, 5
    gb.upload(ldft, mdft)
    P = common.random_density(gb.Nbf(), 2, seed=3, blocks=gb.get_sym_idx(1))
    grid = hf.DFTGrid(gb, ldft, mdft)
    rows = hf.xc_func_table()
    assert len(rows) >= 33
    nels = {}
    for r in rows:
        ids = (0, r["id"]) if r["role"] == "c" else (r["id"], 0)
        H, Exc, Nel, _ = grid.eval_Fxc(ids[0], ids[1], P)
        Ha, Hb, Excp, Nelp, _ = grid.eval_Fxc_pol(ids[0], ids[1], 0.5 * P, 0.5 * P)
        print(r["id"], r["name"], repr(Nel), repr(Nelp), Exc, Excp)
        for M in (H, Ha, Hb):
            # (i, j) and (j, i) are the same sums in another order: the parity tests' own bound on H, 1e-10 relative
            asym = np.max(np.abs(M - M.T))
            print("   asymmetry", asym, np.max(np.abs(M)))
            assert np.all(np.isfinite(M)) and asym <= 1e-10 * np.max(np.abs(M)), r["name"]
        assert np.isfinite(Exc) and np.isfinite(Excp) and Exc != 0.0, r["name"]
        assert Nel == Nelp, (r["name"], Nel, Nelp)
        nels[r["name"]] = Nel
    assert len(set(nels.values())) == 1, nels
