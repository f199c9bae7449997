"""The streams of tests/cpr_sweep.py through the host twin's tracker: the rows equal the rows expected from the reference's
recorded answers field by field, in file order and shuffled, no gate comes within 1 m of its limit, and the counters are
the ones the files predict.  This is what makes the expected rows trustworthy before test_gpu_cpr_sweep.py holds the
device to them."""
import numpy as np
import pytest

import cpr_sweep as cs


@pytest.fixture(scope="module")
def reference(pkg):
    return cs.reference_stream(pkg)


@pytest.fixture(scope="module")
def chained(pkg):
    return cs.chained_stream(pkg)


def check(pkg, sweep, capacity):
    for s in (sweep, cs.shuffled(sweep)):
        got, st = cs.run(pkg, s, True, capacity)
        n, bad = cs.mismatches(s, got)
        assert n == 0, (n, bad)
        assert st["min_gate_margin_m"] >= 1.0, st["min_gate_margin_m"]
        assert {k: st[k] for k in cs.COUNTERS} == sweep["counters"]
    return st


def test_reference_stream_on_the_twin(pkg, reference):
    st = check(pkg, reference, 1 << 17)
    print("reference stream: %d records, min_gate_margin_m %.2f" % (len(reference["m"]), st["min_gate_margin_m"]))
    assert reference["cases"] == 52889 and len(reference["m"]) == 89185 and len(reference["receivers"]) == 13386
    c = reference["counters"]
    assert (c["cpr_global_ok"], c["cpr_global_bad"], c["cpr_global_skipped"]) == (23014, 1466, 11816)
    assert (c["cpr_local_receiver_relative"], c["cpr_local_range_checks"]) == (16066, 465)


def test_chained_stream_on_the_twin(pkg, chained):
    st = check(pkg, chained, 1 << 16)
    c = chained["counters"]
    print("chained stream: %d cases, min_gate_margin_m %.2f, aircraft-relative %d, range refusals %d, half-cell refusals %d"
          % (chained["cases"], st["min_gate_margin_m"], c["cpr_local_aircraft_relative"], c["cpr_local_range_checks"],
             chained["half_cell_refusals"]))
    assert c["cpr_local_aircraft_relative"] > 10000 and c["cpr_local_range_checks"] > 1000 and chained["half_cell_refusals"] > 1000
    assert c["cpr_surface"] > 5000


def test_the_shuffle_keeps_each_case_in_order_and_mixes_the_kinds(reference):
    s = cs.shuffled(reference)
    assert not np.array_equal(s["case"], reference["case"]) and np.array_equal(np.sort(s["case"]), reference["case"])
    t, case = s["m"]["sysTimestampMsg"].astype(np.int64), s["case"]
    same = case[1:] == case[:-1]
    assert (t[1:][same] > t[:-1][same]).all() and int(same.sum()) == len(case) - reference["cases"]  # cases stay whole
    for i in range(0, 64 * 50, 64):  # a wavefront's worth of records holds all three kinds
        assert len(set(s["kind"][i:i + 64].tolist())) == 3, i
