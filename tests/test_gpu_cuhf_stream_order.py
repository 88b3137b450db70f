"""The stream-ordering contract ("Stream ordering") for hfg_cuhf_update_devptr: the call reads its inputs
after everything the caller enqueued earlier on the context's stream, writes Fa and Fb before anything the caller enqueues
later, and is finished with its inputs by then.  tests/cuhf_stream_worker.py runs the protocol of
tests/test_gpu_stream_order.py for this one entry in a child process on the three stream kinds: delay, copy-in over decoys,
call, copy-out, overwrite.  The entry's baselines repeat bitwise (fixed summation orders), so bitwise equality is asserted."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cuhf_stream_worker as wk  # noqa: E402


@pytest.fixture(scope="module")
def run(native_libs, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cuhf_stream") / "out.json")
    e = dict(os.environ)
    e.pop("HELFEM_CUHF_LOWRANK", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cuhf_stream_worker.py"), path], env=e, cwd=ROOT, timeout=300,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = out.stdout.decode(errors="replace")[-3000:]
    if out.returncode != 0 or "ok" not in text.split():
        pytest.fail("worker: status %d\n%s" % (out.returncode, text))
    return json.load(open(path))


@pytest.mark.parametrize("kind", wk.STREAM_KINDS)
def test_entry_keeps_the_stream_order(run, kind):
    rec = [r for r in run["records"] if r["kind"] == kind]
    assert len(rec) == 1
    rec = rec[0]
    print(rec)
    assert rec["changed"], "the update must change Fa and Fb for the case to mean anything"
    assert rec["decoy_differs"], "the decoy inputs give the true result: the case cannot tell them apart"
    assert rec["baselines_bitwise"]
    if kind == "own":
        assert rec["own_vs_null"], "after hfg_ctx_synchronize, against the null-stream context"
    else:
        assert rec["delay_ms"] >= run["delay_min_ms"], "the delay is too short for the run to mean anything"
        assert not rec["ordered_is_decoy"], "the call read its inputs before the copies enqueued ahead of it"
        assert rec["ordered_bitwise"]
