"""Every hfg:: function that crosses translation units of helfem_amd/csrc/hip/ is declared once, in hip/internal.h, and
the file that defines it includes that header: a host-only syntax pass with -Wmissing-prototypes over every HIP source and
both probes may then name kernels (k_*: they keep their linkage, profiles/ and DESIGN.md refer to their names) and nothing
else.  A function that turns up here is either file-local (make it static) or lacks its line in internal.h.  No GPU needed."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

from helfem_amd.build import CSRC, HIP_SRCS, ROOT

SOURCES = [os.path.join(CSRC, rel) for rel in HIP_SRCS] + [os.path.join(ROOT, "tests", "gpu_probe", f) for f in ("gemm_engine.hip", "two_stage.hip")]
WARNING = re.compile(r"warning: no previous prototype for function '([^']+)'")


def missing_prototypes(src):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-fsyntax-only", "-Wmissing-prototypes", src]
    if not src.endswith(".hip"):
        cmd[1:1] = ["-x", "hip"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    return sorted(set(WARNING.findall(p.stdout)))


def test_only_kernels_lack_a_prototype():
    with ThreadPoolExecutor(max_workers=8) as pool:
        found = dict(zip(SOURCES, pool.map(missing_prototypes, SOURCES)))
    assert any(found.values()), "the pass reports the kernels themselves: no warning at all means it did not run as meant"
    stray = {os.path.relpath(src, ROOT): [f for f in names if not f.startswith("k_")] for src, names in found.items()}
    stray = {src: names for src, names in stray.items() if names}
    assert not stray, "functions with external linkage and no declaration in hip/internal.h: %r" % stray
