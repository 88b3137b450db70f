"""The mixed-kernel exchange tables on the device (hfg_mix_exchange_tables, hip/exchange_mix.hip) and the exchange entries on
them (hfg_mix_exchange_devptr, _occ_devptr, _occ_batch_devptr), in a worker process (tests/exchange_mix_worker.py).

Shapes (elements x nodes): 1 x 4 (no cross-element pair), 2 x 5 (e < f and e > f adjacent), 3 x 4 (a non-adjacent pair; the
short last element and the dropped first primitive both meet a cross pair), 3 x 15 with lmax = 2, mmax = 1 (the element
order of the benchmark, five table slots, M != 0 couplings); both screened kernels; (alpha, beta) = (0.19, 0.46),
(0.25, -0.25) and (0.3, 0).

Bounds.  Table: every entry within 4 eps (|alpha coulomb| + |beta ratio screened|) of the NumPy restatement
(tests/exchange_mix_restatement.py) -- the outer product, the two scalings and the sum round once each, fused or not -- and
exactly zero wherever the restatement is, which covers the padding.  K: the deviation of the mixed build from the
oracle's alpha K + beta K_rs is at most 4 times that of the two-build sum alpha hfg_exchange + beta hfg_rs_exchange, with a
floor of N eps max|K|; the factor covers the rounding of the outer products of the Coulomb blocks, which the factorised
path never forms.  With beta = 0 the same bound holds against hfg_exchange alone.  Batch against single, rebuild against
build, repeated call: bitwise."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exchange_mix_worker as wk  # noqa: E402

EPS = wk.EPS


def _child(mode, path, limit=600):
    e = {k: v for k, v in os.environ.items() if k not in ("HELFEM_EXL_MIX", "HELFEM_EXL_PAIR", "HELFEM_EXCHANGE")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "exchange_mix_worker.py"), mode, path], cwd=ROOT, env=e, timeout=limit,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    # a child that ends with a signal (negative return code) or an error ends the test here: nothing else is started
    assert out.returncode == 0 and "ok" in out.stdout.decode().split(), (out.returncode, out.stdout.decode()[-3000:])


@pytest.fixture(scope="module")
def figures(native_libs, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("mix") / "figures.json")
    _child("figures", path)
    return json.load(open(path))


def _cases(figures):
    return [r for r in figures if "K" in r]


def test_every_case_ran(figures):
    assert len(_cases(figures)) == len(wk.SHAPES) * 2 * len(wk.WEIGHTS)
    assert sorted(set(tuple(r["shape"]) for r in _cases(figures))) == sorted(wk.SHAPES)


def test_table_against_the_restatement(figures):
    seen = 0
    for r in _cases(figures):
        seen += 1
        print("table %s kind %d alpha %.2f beta %.2f: %.3f units of 4 eps magnitude, %d zero entries" %
              (r["shape"], r["kind"], r["alpha"], r["beta"], r["table_units"], r["padding_entries"]))
        assert r["table_units"] <= 1.0
        assert r["padding_zero"] and r["padding_entries"] > 0
    assert seen == len(wk.SHAPES) * 2 * len(wk.WEIGHTS) == 4 * 2 * 3


def test_rebuild_and_repeated_call(figures):
    for r in _cases(figures):
        assert r["builds_after_repeat"] == 1, "the second call with the same weights built the set again"
        assert r["repeat_unchanged"] and r["rebuild_bitwise"] and r["gone_after_upload"]


def test_K_against_the_two_builds_and_the_oracle(figures):
    for r in _cases(figures):
        for k in r["K"]:
            floor = r["N"] * EPS * k["scale"]
            bound = max(4 * k["two"], floor)
            print("K %s kind %d alpha %.2f beta %.2f rank %d: two builds %.3e, mixed %.3e (orbitals) %.3e (density), floor %.3e" %
                  (r["shape"], r["kind"], r["alpha"], r["beta"], k["rank"], k["two"], k["mix_C"], k["mix_P"], floor))
            assert k["scale"] > 1e-3
            assert k["mix_C"] <= bound and k["mix_P"] <= bound
            # and directly against the two-call sum (beta = 0: against hfg_exchange alone): both within their bounds of the oracle
            assert k["mix_vs_two"] <= bound + k["two"]
            assert k["host"], "hfg_mix_exchange is the device-pointer entry behind a staging copy"


def test_batch_is_the_single_entry_per_density(figures):
    for r in _cases(figures):
        assert r["batch_bitwise"] and r["batch_without_orbitals_bitwise"]  # (with the orbitals handed over, and factorising P)


def test_shards_sum_to_the_whole(figures):
    recs = [r for r in figures if r.get("shards")]
    assert len(recs) == 2
    for r in recs:
        assert r["scale"] > 1e-3 and r["err"] <= r["N"] * EPS * r["scale"]


def test_new_screened_tables_take_the_mixed_set_with_them(figures):
    recs = [r for r in figures if r.get("invalidation")]
    assert len(recs) == 2
    for r in recs:
        assert r["outcome"] == ["refused", "refused"], "stale numbers or another error: %r" % (r["outcome"],)
        assert r["changed"] > 1e-6, "the rebuilt set is that of the new range"


def test_devptr_entries_keep_the_stream_order(native_libs, tmp_path):
    """the protocol of tests/stream_order_worker.py on a non-default torch stream: inputs written by copies enqueued just
    before the call and overwritten right after it, output read by a copy enqueued just after, no host synchronisation"""
    import stream_order_worker as sow
    path = str(tmp_path / "stream.json")
    _child("stream", path)
    recs = json.load(open(path))
    assert [r["entry"] for r in recs] == ["hfg_mix_exchange_devptr", "hfg_mix_exchange_occ_devptr", "hfg_mix_exchange_occ_batch_devptr"]
    for rec in recs:
        print(rec)
        assert rec["decoy_differs"] and rec["repeat"]["ok"] and rec["twin"]["ok"]
        assert rec["baselines_bitwise"], "results repeat bitwise from call to call"
        assert rec["delay_ms"] >= sow.DELAY_MIN_MS, "the delay is too short for the run to mean anything"
        assert not rec["ordered_is_decoy"], "the call read its inputs before the copy enqueued ahead of it"
        assert rec["ordered"]["ok"] and rec["ordered"]["bitwise"]


def test_adapter_program_on_the_device(native_libs):
    p = subprocess.run([os.path.join(ROOT, "tests", "cpp", "mix_exchange_adapter_check"), "run"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = p.stdout.decode()
    print(text)
    assert p.returncode == 0 and "adapter ok" in text and "logic_error_on_shape 1" in text
    lines = [line.split() for line in text.splitlines() if line.startswith("kind")]
    assert [int(w[1]) for w in lines] == [1, 2]
    for w in lines:
        N, dev, scale = int(w[3]), float(w[5]), float(w[7])
        assert scale > 1e-3 and dev <= 1e-12 * scale, (N, dev, scale)  # the parity bound of the exchange builds against each other
