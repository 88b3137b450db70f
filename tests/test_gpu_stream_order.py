"""The stream-ordering contract of every device-pointer entry point ("Stream ordering"): a call on a context
reads its inputs after everything the caller enqueued earlier on the context's stream, writes its outputs before anything the
caller enqueues later, and is finished with its inputs by then.

tests/stream_order_worker.py runs the protocol in a child process per setting (the switches are read once per process), one
after the other: defaults; HELFEM_FOCK_OVERLAP=0; HELFEM_BT_FOLD=0 HELFEM_BT_SIDE=1; HELFEM_TRD=chain; defaults with profiling
on.  Inside every process three stream kinds: the null stream (Context(stream=0)), a non-default torch stream, a context that
owns its stream (there the contract is hfg_ctx_synchronize alone).  Per entry: two synchronised baselines and the host-pointer
twin; then, without any host synchronisation, a delay of about 50 ms, device-to-device copies of the true inputs over decoys,
the call, a copy of the outputs, and decoys and a fill value over inputs and outputs.  The copied outputs must be the
baseline.  A decoy is a valid input of the same kind (another seeded density, another Fock matrix ...), never NaN.

Entries: every hfg_*_dev function of include/helfem_gpu.h (enumerated from the header; test_stream_order_plan_cpu.py keeps a
new one from escaping), except, knowingly:
  - hfg_compute_tei_dev, hfg_compute_rs_tei_dev: they take no device pointer; they build the basis' tables on the device from
    the host-side basis and are complete when they return;
  - hfg_rs_special_dev: takes host arrays, copies in, evaluates, copies out and synchronises.

Bounds.  Where an entry's two baselines are bitwise equal the ordered run must be bitwise the baseline; where they are not,
the entry's parity bound of test_gpu_parity.py holds (J, K: relerr < 1e-12; XC: 1e-10 on the matrix, 1e-11 on Exc and Nel;
compact Fock and its finish: 1e-11 of the largest element, the sharded step's bound; eigenpairs: 1e-10 scale on E and
orthonormality, 1e-9 scale on the residual against the TRUE F; density 1e-13; GEMM 1e-12 k).  Which of the two applied is
decided per run and printed; on the MI355X all fourteen entries repeated bitwise in every setting and on every stream kind, so
bitwise equality is what was asserted throughout (measured delay: 49.5 to 49.7 ms of torch.cuda._sleep per ordered run).
The baseline is also compared once with the host-pointer twin at the parity bound (hfg_exchange for hfg_exchange_occ_dev; the
compact Fock entries, hfg_eig_blocks_dev and hfg_eig_assemble_dev have none).

HELFEM_TRD=chain: a context gives its side stream up when a block of 1024 or more goes through the chain of launches
(tridiagonalize_takes_chain), not at the 257-block of the protocol, so that setting adds an eigensolve with the blocks
(1024, 130, 3) under the same protocol and then hfg_fock_compact_dev and hfg_eig_gsym_sub_dev once more on the same context,
also compared with what the context returned while it was fresh (parity bound: the two are different code paths).

Control (once per process, hfg_gemm_dev, 200 x 300 x 129): the same delay and copy-in on a second stream with no event between
it and the context's stream must make the call return the DECOY product; the true product would mean the delay is too short
to catch anything."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stream_order_worker as wk  # noqa: E402

FAULT_LIKE = (134, 139, -6, -11)
# a worker takes a few seconds once torch and the library are loaded; the bound covers a cold start of both
WORKER_TIMEOUT_S = 300
PLAN = wk.plan()
SETTING_NAMES = [n for n, _ in wk.SETTINGS]


@pytest.fixture(scope="module")
def runs(native_libs, tmp_path_factory):
    """the settings in order, one GPU process at a time; after a fault-like end (abort, segmentation fault, time limit)
    nothing more is started and the remaining settings count as failed"""
    d = tmp_path_factory.mktemp("stream_order")
    res, stopped = {}, None
    for setting, env in wk.SETTINGS:
        if stopped:
            res[setting] = dict(error="not run: %s" % stopped)
            continue
        e = dict(os.environ)
        for k in wk.SWITCHES:
            e.pop(k, None)
        e.update(env)
        path = str(d / (setting + ".json"))
        try:
            out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stream_order_worker.py"), setting, path], env=e, cwd=ROOT,
                                 timeout=WORKER_TIMEOUT_S, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        except subprocess.TimeoutExpired as x:
            stopped = "the worker of '%s' ran into its time limit" % setting
            res[setting] = dict(error=stopped + "\n" + (x.stdout or b"").decode(errors="replace")[-3000:])
            continue
        text = out.stdout.decode(errors="replace")[-3000:]
        if out.returncode in FAULT_LIKE:
            stopped = "the worker of '%s' ended with status %d" % (setting, out.returncode)
        if out.returncode != 0 or "ok" not in text.split():
            res[setting] = dict(error="status %d\n%s" % (out.returncode, text))
            continue
        res[setting] = json.load(open(path))
    return res


def _run(runs, setting):
    r = runs[setting]
    if "error" in r:
        pytest.fail("worker of '%s': %s" % (setting, r["error"]))
    return r


def _show(what, v):
    print("  %s: bitwise %s; %s" % (what, v["bitwise"], ", ".join("%s %.3e (< %.0e)" % tuple(f) for f in v["figs"])))


@pytest.mark.parametrize("setting", SETTING_NAMES)
def test_worker_ran_every_planned_case(runs, setting):
    r = _run(runs, setting)
    got = sorted((x["kind"], x["entry"]) for x in r["records"])
    assert got == sorted((k, e) for s, k, e in PLAN if s == setting)
    print(setting, "switches:", r["tuning"], "delay:", r["delay_units"])


@pytest.mark.parametrize("setting,kind,entry", PLAN, ids=["%s-%s-%s" % p for p in PLAN])
def test_entry_keeps_the_stream_order(runs, setting, kind, entry):
    """bitwise where the entry's baselines repeat bitwise (every entry did on the MI355X), else its parity bound"""
    r = _run(runs, setting)
    rec = [x for x in r["records"] if x["kind"] == kind and x["entry"] == entry]
    assert len(rec) == 1
    rec = rec[0]
    print("%s %s %s: baselines bitwise equal: %s -> %s" % (setting, kind, entry, rec["baselines_bitwise"],
                                                          "bitwise" if rec["baselines_bitwise"] else "parity bound"))
    assert rec["decoy_differs"], "the decoy inputs give the true result: the case cannot tell them apart"
    _show("second baseline against the first", rec["repeat"])
    assert rec["repeat"]["ok"]
    if "twin" in rec:
        _show("baseline against the host-pointer twin", rec["twin"])
        assert rec["twin"]["ok"]
    if kind == "own":
        _show("after hfg_ctx_synchronize, against the null-stream context", rec["own_vs_null"])
        assert rec["own_vs_null"]["ok"]
    else:
        print("  delay %.1f ms" % rec["delay_ms"])
        assert rec["delay_ms"] >= wk.DELAY_MIN_MS, "the delay is too short for the run to mean anything"
        _show("ordered run against the baseline", rec["ordered"])
        assert not rec["ordered_is_decoy"], "the call read its inputs before the copies enqueued ahead of it"
        assert rec["ordered"]["ok"]
    if "vs_fresh" in rec:
        _show("after the side stream was given up, against the fresh context", rec["vs_fresh"])
        assert rec["vs_fresh"]["ok"]


@pytest.mark.parametrize("setting", SETTING_NAMES)
def test_control_unordered_copy_in_gives_the_decoy_product(runs, setting):
    c = _run(runs, setting)["control"]
    print("%s: control delay %.1f ms, decoy product %s, true product %s" % (setting, c["delay_ms"], c["got_decoy"], c["got_true"]))
    assert c["delay_ms"] >= wk.DELAY_MIN_MS
    assert not c["got_true"], "toothless: the copy-in on an unordered stream was seen, the delay is too short"
    assert c["got_decoy"]


def test_profile_is_readable_after_the_sequence(runs):
    """with profiling on the Coulomb brackets are recorded on the side stream; hfg_profile_get after the sequence"""
    p = _run(runs, "profile")["profile"]
    assert sorted(p) == sorted(wk.STREAM_KINDS)
    for kind, fam in p.items():
        print(kind, {k: (round(v[0], 3), v[1]) for k, v in fam.items()})
        for name in ("coulomb", "xc", "exchange", "eig_tridiag", "eig_backtransform", "gemm", "density", "scatter"):
            assert fam[name][1] >= 1 and fam[name][0] > 0.0, (kind, name)
