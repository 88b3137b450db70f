"""The FP64 GEMM tile engine (hip/gemm.hip) launcher by launcher and variant by variant, against the host in higher
precision (tests/gemm_engine_worker.py through tests/gpu_probe/libgemm_engine_probe.so).

exact    integer operands in [-8, 8]: NumPy int64 is the reference and np.array_equal the criterion -- a dropped, doubled or
         misplaced term cannot hide under a tolerance, whatever the order of summation or of the split-K additions
rounded  uniform data with every row of op(A) and every column of op(B) scaled by a power of two in 2^[-30, 30], reference and
         |op A| |op B| in np.longdouble, componentwise |C - ref| <= (K + 4) 2^-53 (|alpha| |op A| |op B| + |beta| |C0|): the
         bound of a length-K dot product summed in any order, one scaling, one addition -- derived, not measured, and
         invariant under the scalings, so a reduced-precision path cannot hide behind a large neighbour
Every C buffer holds a finite sentinel where no task stores (rows M..ldc-1, columns outside cmap, the tiles sym = 2 skips
keep C0): those must come back bit for bit.  The operand buffers hold NaN outside M x K and K x N.

HELFEM_GEMM_TILE and HELFEM_MFMA are read once per process, so the worker runs once per setting, as a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SETTINGS = {
    "default": {},
    "tile128": {"HELFEM_GEMM_TILE": "128"},
    "mfma4x4x4": {"HELFEM_MFMA": "4x4x4"},
    "mfma4x4x4-tile128": {"HELFEM_MFMA": "4x4x4", "HELFEM_GEMM_TILE": "128"},
}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_gemm_engine(native_libs, tmp_path, setting):
    """Every launcher of hip/gemm.hip under one setting of the tile and matrix-instruction switches: shapes around the tile
    edges, the four transpositions on the 16-byte and the element-wise load paths, over = 1/2/3 against over = 0, sym = 1 with
    the mirror, sym = 2 with the accumulating epilogues, column maps, split K with an empty second half, work lists whose
    length leaves 0, 1 and 7 modulo 8, empty tasks, and the public entry points hfg_gemm / hfg_gemm_dev with padded leading
    dimensions, bases advanced by 8 bytes, odd lda and k = 0.

    Under the default setting one product of 2688 x 40 x 2688 also goes through hfg_gemm: 441 tiles of 128 x 128, which the
    default rule (gemm_prefers_128: whole rounds of 2 x CUs slots filled to 85 %) sends to k_dgemm<128, 128> on a part with
    256 CUs.  That depends on the CU count; HELFEM_GEMM_TILE=128 is what guarantees the large-tile kernels."""
    from helfem_amd import build
    build.build_gemm_probe(verbose=False)  # (no-op when the library is newer than its source and the product library)
    env = dict(os.environ)
    env.pop("HELFEM_GEMM_TILE", None)
    env.pop("HELFEM_MFMA", None)
    env.update(SETTINGS[setting])
    out = str(tmp_path / "gemm_engine.npz")
    cmd = [sys.executable, os.path.join(ROOT, "tests", "gemm_engine_worker.py"), out] + (["--big"] if setting == "default" else [])
    p = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = p.stdout.decode(errors="replace")
    assert p.returncode == 0, text[-4000:]
    r = np.load(out)
    assert str(r["gemm_tile"]) == SETTINGS[setting].get("HELFEM_GEMM_TILE", "0")
    assert str(r["mfma"]) == ("on" if "HELFEM_MFMA" in SETTINGS[setting] else "off")
    names = [str(x) for x in r["name"]]
    assert len(names) >= 150, text[-2000:]  # every group reported
    for fam in ("edges/", "transposes/", "over/", "over-equals-plain/", "sym1/", "sym2/", "acc/", "map/", "splitk/", "worklist0/",
                "worklist1/", "worklist7/", "empty/", "public/hfg_gemm[", "public/hfg_gemm_dev["):
        assert any(n.startswith(fam) for n in names), fam
    assert ("public/hfg_gemm-2688x40x2688[exact]" in names) == (setting == "default")
    failed = ["%s: value %s, sentinel %s, error / bound %.3g; %s" % (n, v, s, q, d)
              for n, v, s, q, d in zip(names, r["value_ok"], r["sentinel_ok"], r["ratio"], r["detail"]) if not (v and s)]
    assert not failed, "\n".join(failed)
    assert np.all(r["ratio"] <= 1.0)
