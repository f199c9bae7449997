"""The host twin of the position tracker (libmsd_host.so, msd_pos_host_*) against the second reading of track.c in
tests/indep_positions.py, record by record and bit by bit, on the constructed streams of tests/pos_streams.py; the
counters and the gate margin as well (both sides use the C library's sin / cos / acos / atan2).  Every stream must keep
every plausibility gate at least 1 m from its limit: a stream that sits on a gate fails here, loudly, instead of
making a comparison between two libms flake."""
import math

import numpy as np
import pytest

import pos_streams as ps


@pytest.fixture(scope="module")
def scen(pkg):
    return ps.scenarios(pkg)


NAMES = ["pair_10s", "clock_from_zero", "surface_windows", "surface_version_and_no_reference", "type_and_source_mismatch",
         "global_failure", "aircraft_relative", "receiver_relative", "speed_check", "backwards", "expiry_and_ttl",
         "refusals", "surface_speed_check", "surface_movement_codes", "global_max_range", "negative_max_range",
         "higher_source_skips_speed_check", "reliable_sides", "odd_latitude_alone_out_of_range"]


def test_scenario_list_is_complete(scen):
    assert sorted(scen) == sorted(NAMES)


def twin_run(pkg, receivers, fp, steps, pieces=None):
    t = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, filter_persistence=fp, host=True)
    out = ps.run_library(t, steps, pieces)
    st = t.stats()
    t.close()
    return out, st


@pytest.mark.parametrize("name", NAMES)
def test_twin_equals_the_second_reading(pkg, scen, name):
    receivers, fp, steps = scen[name]
    out, st = twin_run(pkg, receivers, fp, steps)
    rows, mst = ps.run_model(receivers, fp, steps)
    assert ps.rows_of(out) == ps.rows_of_model(rows)
    assert st == mst
    assert st["min_gate_margin_m"] >= 1.0, st["min_gate_margin_m"]


def results(pkg, scen, name):
    receivers, fp, steps = scen[name]
    out, st = twin_run(pkg, receivers, fp, steps)
    return [int(x) for x in out["result"]], out, st


def test_the_scenarios_reach_what_they_are_named_for(pkg, scen):
    """Known answers, so that the two readings cannot agree on streams that never reach the rules in question."""
    r, out, st = results(pkg, scen, "pair_10s")
    assert r == [-1, 0, -1, -1] and st["cpr_global_ok"] == 1
    assert abs(out["lat"][1] - 51.5) < 1e-4 and abs(out["lon"][1] - 3.5) < 1e-4
    r, out, st = results(pkg, scen, "clock_from_zero")
    assert r == [1, 1, -1] and st["cpr_local_aircraft_relative"] == 2
    assert st["cpr_local_range_checks"] == 1  # 51.5 N 3.5 E decoded in the cell around (0, 0): more than 100 NM away
    r, out, st = results(pkg, scen, "surface_windows")
    assert r == [-1, 0, -1, -1, -1, 0, -1, -1, -1, -1, -1, 0] and st["cpr_surface"] == 12
    assert abs(out["lat"][1] - 52.3) < 1e-4 and abs(out["lon"][1] - 4.76) < 1e-4 and out["surface"].all()
    r, out, st = results(pkg, scen, "surface_version_and_no_reference")
    assert r == [-3, -1, 0, -1, -1]
    r, out, st = results(pkg, scen, "type_and_source_mismatch")
    assert r == [-1, -1, -1, -1, -3, -1, 0] and st["cpr_global_ok"] == 1
    r, out, st = results(pkg, scen, "global_failure")
    #          one good pair, the bad pair invalidates the position       four good pairs, the position survives
    assert r == [-1, 0, -2, -1, 1, 0] + [-1, 0, 0, 0, 0, 0, 0, 0, -2, -1, 1, 0]
    assert st["cpr_global_bad"] == 2  # the mixed halves decode to a latitude out of range or fail the speed check
    r, out, st = results(pkg, scen, "aircraft_relative")
    assert r == [-1, 0, 1, 1, 1, -1]
    r, out, st = results(pkg, scen, "receiver_relative")
    #           no range          150 NM: the 190 NM pair is out    250 NM: 110 NM locally    400 NM: no local
    assert r == [-1, -1, -1, 0] + [2, 2, -1, -2] + [2, -1, -1, 0] + [-1, -1, -1, 0]
    assert st["cpr_local_receiver_relative"] == 3 and st["cpr_local_range_checks"] == 3 and st["cpr_global_range_checks"] == 1
    r, out, st = results(pkg, scen, "speed_check")
    #           none: 700 kt     gs 100, tas 100 and ias 80 kt: at most 213 kt x 4/3 -- too slow for 5.6 km in 11 s      gs 1000 kt
    assert r == [-1, 0, 1, 0] + [-1, 0, -3, -1, -2] + [-1, 0, -3, -1, -2] + [-1, 0, -3, -1, -2] + [-1, 0, -3, 1, 0]
    assert st["cpr_local_speed_checks"] == 3 and st["cpr_global_speed_checks"] == 3
    r, out, st = results(pkg, scen, "backwards")
    assert r == [-1, 0, -3, 0, -2] and st["cpr_global_skipped"] == 1 and st["cpr_global_bad"] == 0
    r, out, st = results(pkg, scen, "expiry_and_ttl")
    assert r == [-1, 0, -1, -3, -3] + [1, 0, -1] + [-1] and st["aircraft"] == 1
    for name in ["refusals"] + sorted(ps.KNOWN):
        r, out, st = results(pkg, scen, name)
        ps.known(name, out, st)
    r, out, st = results(pkg, scen, "refusals")
    assert r == [x for case in ps.REFUSAL_RESULTS for x in case]
    assert st["cpr_local_receiver_relative"] == 5 and st["cpr_local_aircraft_relative"] == 1 and st["cpr_global_skipped"] == 1
    assert st["cpr_global_ok"] == 1 and st["cpr_local_speed_checks"] == 0 and st["cpr_local_range_checks"] == 0
    r, out, st = results(pkg, scen, "surface_speed_check")
    #           no speed: 1800 m, 2350 m    24 kt: 850 m, 1350 m
    assert r == [-1, 0, 1] + [-1, 0, -1] + [-1, 0, 1] + [-1, 0, -1] and st["cpr_local_speed_checks"] == 2 and st["cpr_surface"] == 12
    assert abs(out["lat"][2] - (52.3 + 1800.0 / ps.M_PER_DEG)) < 1e-4 and abs(out["lat"][8] - (52.3 + 850.0 / ps.M_PER_DEG)) < 1e-4
    r, out, st = results(pkg, scen, "surface_movement_codes")
    assert r == [-1, -1] * 6 + [-1, 0] * 2 and st["cpr_global_ok"] == 2
    r, out, st = results(pkg, scen, "global_max_range")
    #           no location    190 NM   40 NM
    assert r == [-1, 0] + [-1, -2] + [2, 0] and st["cpr_global_range_checks"] == 1 and st["cpr_local_range_checks"] == 1
    assert abs(out["lat"][1] - 53.0) < 1e-4 and abs(out["lon"][1] - 9.0) < 1e-4
    r, out, st = results(pkg, scen, "negative_max_range")
    assert r == [2] and st["cpr_local_range_checks"] == 0 and abs(out["lat"][0] - 52.5) < 1e-4 and abs(out["lon"][0] - 5.0) < 1e-4
    r, out, st = results(pkg, scen, "higher_source_skips_speed_check")
    assert r == [-1, 0, -1, 0] + [-1, 0, -1, -2] + [-1, 0, 1] + [-1, 0, -1]
    assert st["cpr_global_speed_checks"] == 1 and st["cpr_local_speed_checks"] == 1 and st["cpr_local_range_checks"] == 2
    assert abs(out["lat"][3] - 52.0) < 1e-4 and abs(out["lat"][10] - 50.5) < 1e-4
    r, out, st = results(pkg, scen, "reliable_sides")
    assert r == [-1, 0, 0, 0, -2] + [-1, 0, 0, 0, 0, -2] and st["cpr_global_bad"] == 2
    r, out, st = results(pkg, scen, "odd_latitude_alone_out_of_range")
    assert r == [-1, -2, -1, -2] and st["cpr_global_bad"] == 2 and st["cpr_global_range_checks"] == 0 and st["cpr_global_speed_checks"] == 0
    # the aircraft alive after each step: the one-message aircraft leaves after more than 60 s, the other after 10 min
    receivers, fp, steps = scen["expiry_and_ttl"]
    t = pkg.capi.PositionTracker(capacity=64, receivers=receivers, host=True)
    alive = []
    for s in steps:
        ps.run_library(t, [s])
        alive.append(t.stats()["aircraft"])
    assert alive == [2, 2, 1, 1, 2, 1, 0, 0, 1]
    t.close()


def test_create_refuses_every_configuration_the_check_names(pkg):
    """msd_pos_config_ok: a capacity below 64, above 2^24 or not a power of two, no receiver or more than 65536, a
    negative --filter-persistence, no configuration at all; and the bounds themselves are accepted"""
    import ctypes as C
    make = lambda **kw: pkg.capi.PositionTracker(host=True, **kw)  # noqa: E731
    for kw in (dict(capacity=32), dict(capacity=1 << 25), dict(capacity=96), dict(capacity=64, receivers=[]),
               dict(capacity=64, receivers=[None] * 65537), dict(capacity=64, filter_persistence=-1)):
        with pytest.raises(pkg.MsdError):
            make(**kw)
    h = C.c_void_p()
    assert pkg.capi._pos_lib(True)[1]["create"](None, C.byref(h)) == -22 and not h.value  # -EINVAL
    for kw in (dict(capacity=64), dict(capacity=1 << 24, receivers=[None] * 65536)):
        make(**kw).close()


def test_margin_is_reported_and_resets(pkg, scen):
    receivers, fp, steps = scen["speed_check"]
    t = pkg.capi.PositionTracker(capacity=64, receivers=receivers, filter_persistence=fp, host=True)
    assert t.stats()["min_gate_margin_m"] == math.inf
    ps.run_library(t, steps)
    assert 1.0 <= t.stats()["min_gate_margin_m"] < 1e6
    t.reset()
    assert t.stats()["min_gate_margin_m"] == math.inf and t.stats()["aircraft"] == 0 and t.stats()["cpr_airborne"] == 0
    t.close()


def test_mixed_stream_and_cutting_invariance(pkg):
    receivers, m, f, r = ps.mixed_stream(pkg)
    steps = [("update", m, f, r)]
    whole, st = twin_run(pkg, receivers, 0, steps)
    rows, mst = ps.run_model(receivers, 0, steps)
    assert ps.rows_of(whole) == ps.rows_of_model(rows) and st == mst
    assert st["min_gate_margin_m"] >= 1.0, st["min_gate_margin_m"]
    # the stream reaches every counter
    for k, v in st.items():
        assert v > 0, k
    for pieces in (1, 7, 64):
        cut, cst = twin_run(pkg, receivers, 0, steps, pieces)
        assert np.array_equal(cut.view(np.uint8), whole.view(np.uint8)) and cst == st


def test_table_full_changes_nothing(pkg, scen):
    receivers, fp, steps = scen["pair_10s"]
    t = pkg.capi.PositionTracker(capacity=64, receivers=[None], host=True)
    b = ps.Builder(pkg)
    for k in range(64):
        b.pos(ps.T0, 0x100 + k, 10.0, 10.0, 0)
    _, m, f, r = b.step()
    t.update(m[:60], f[:60], r[:60])
    before = t.stats()
    with pytest.raises(pkg.MsdError) as e:
        b2 = ps.Builder(pkg)
        for k in range(5):
            b2.pos(ps.T0 + 1, 0x900 + k, 10.0, 10.0, 1)
        _, m2, f2, r2 = b2.step()
        t.update(m2, f2, r2)
    assert e.value.code == -28 and t.stats() == before  # -ENOSPC
    t.update(m[60:], f[60:], r[60:])                    # exactly full is fine
    assert t.stats()["aircraft"] == 64
    t.close()


# ---- the streams of tests/test_gpu_positions_machinery.py, fixed here before they meet the device ----
def twin_at(pkg, capacity, receivers, fp, steps, pieces=None):
    t = pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, filter_persistence=fp, host=True)
    out = ps.run_library(t, steps, pieces)
    st = t.stats()
    t.close()
    return out, st


def test_wide_stream_twin_equals_the_second_reading(pkg):
    receivers, m, f, r = ps.wide_stream(pkg, aircraft=700, records=5600, receivers=3, skipped_every=17)
    steps = [("update", m, f, r)]
    out, st = twin_run(pkg, receivers, 0, steps)
    rows, mst = ps.run_model(receivers, 0, steps)
    assert ps.rows_of(out) == ps.rows_of_model(rows)
    assert st == mst
    assert st["min_gate_margin_m"] >= 1.0, st["min_gate_margin_m"]
    # what the stream is: round robin in time order, three receivers, every 17th record skipped in both ways, and
    # nearly every other record from the second round on a global decode
    assert (np.diff(m["sysTimestampMsg"].astype(np.int64)) >= 0).all() and set(r.tolist()) == {0, 1, 2}
    skipped = (m["msgtype"] == 32) | (f["addr"] == 0)
    assert (f["addr"][~skipped] == 0x100000 + (np.arange(5600) % 700)[~skipped]).all()
    assert skipped.sum() == 5600 // 17 and skipped[16::17].all() and (m["msgtype"] == 32).sum() == 165 and (f["addr"] == 0).sum() == 164
    assert (out["result"][skipped] == pkg.capi.POS_NOT_TRIED).all()
    assert st["aircraft"] == 700 and st["cpr_global_ok"] > 4400 and st["cpr_airborne"] == 5600 - skipped.sum()


def test_wide_stream_without_options_is_one_receiver_and_all_positions(pkg):
    receivers, m, f, r = ps.wide_stream(pkg, aircraft=7, records=70)
    assert receivers == [None] and not r.any() and f["cpr_valid"].all() and (m["msgtype"] == 17).all()
    assert (f["cpr_odd"] == (np.arange(70) // 7) % 2).all()
    assert (np.diff(m["sysTimestampMsg"][::7].astype(np.int64)) == 500).all()
    out, st = twin_run(pkg, receivers, 0, [("update", m, f, r)])
    assert st["cpr_global_ok"] == 63 and st["min_gate_margin_m"] >= 1.0


@pytest.mark.parametrize("kw", [dict(aircraft=300, records=2048, skipped_every=17),
                                dict(aircraft=5000, records=20000, receivers=3, skipped_every=17)])
def test_wide_streams_of_the_gpu_tests_keep_their_margin_and_cut_anywhere(pkg, kw):
    receivers, m, f, r = ps.wide_stream(pkg, **kw)
    steps = [("update", m, f, r)]
    whole, st = twin_at(pkg, 8192, receivers, 0, steps)
    assert st["min_gate_margin_m"] >= 1.0, st["min_gate_margin_m"]
    assert st["aircraft"] == kw["aircraft"] and st["cpr_global_ok"] > len(m) // 2
    cut, cst = twin_at(pkg, 8192, receivers, 0, steps, pieces=257)
    assert cut.tobytes() == whole.tobytes() and cst == st


def test_chain_addresses_share_one_chain_across_the_end(pkg):
    for cap in (64, 256):
        addrs = ps.chain_addresses(pkg, cap)
        assert len(set(addrs)) == 5
        assert [pkg.capi.pos_home_slot(0, a, cap) for a in addrs] == [cap - 1, cap - 1, cap - 1, 0, 1]


@pytest.mark.parametrize("variant", ps.CHAIN_VARIANTS)
def test_chain_scenario(pkg, variant):
    receivers, fp, steps = ps.chain_scenario(pkg, 64, variant)
    out, st = twin_at(pkg, 64, receivers, fp, steps)
    rows, mst = ps.run_model(receivers, fp, steps)
    assert ps.rows_of(out) == ps.rows_of_model(rows)
    assert st == mst
    assert st["min_gate_margin_m"] >= 1.0, st["min_gate_margin_m"]
    # known answers: step 1 pairs the survivors, step 2 is aircraft-relative, step 4 global at the survivors' places
    n1 = 8
    first, even, late = out[:n1], out[n1:n1 + 3], out[n1 + 3:]
    assert sorted(int(x) for x in first["result"]) == [-1] * 5 + [0] * 3
    assert [int(x) for x in even["result"]] == [1, 1, 1]
    assert [int(x) for x in late["result"]] == [0, 0, 0] and late["decoded"].all() and not late["relative"].any()
    survivors = [4, 2, 0] if variant == "reversed" else [0, 2, 4]
    for o, j in zip(late, survivors):
        lat, lon = ps.chain_place(j)
        assert abs(o["lat"] - lat) < 1e-4 and abs(o["lon"] - lon) < 1e-4
    assert st["cpr_global_ok"] == 6 and st["cpr_local_aircraft_relative"] == 3 and st["cpr_global_speed_checks"] == 0
    # the aircraft alive after each step
    t = pkg.capi.PositionTracker(capacity=64, receivers=receivers, host=True)
    alive = []
    for s in steps:
        ps.run_library(t, [s])
        alive.append(t.stats()["aircraft"])
    t.close()
    assert alive == ps.CHAIN_ALIVE[variant]


def test_nothing_delivered_depends_on_the_capacity(pkg):
    receivers, m, f, r = ps.mixed_stream(pkg)
    steps = [("update", m, f, r)]
    small, sst = twin_at(pkg, 64, receivers, 0, steps)
    large, lst = twin_at(pkg, 1024, receivers, 0, steps)
    assert small.tobytes() == large.tobytes() and sst == lst
    assert sst["min_gate_margin_m"] >= 1.0
