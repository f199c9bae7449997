"""The host object's receiver range (libmsd_host.so, msd_pos_host_range_*) against the second reading of track.c:238-308
and :683-686 in tests/indep_range.py, on the constructed streams of tests/range_streams.py: the rows of range_read, the
distances and the position records after every step, and the two margins (both sides use the C library's libm, so even
the margins are the same doubles).  Every stream must keep the gates 1 m, the ranges 0.05 m and the bearings 0.01 degrees
from where two libms could part: a stream that does not fails here, loudly."""
import math

import pytest

import indep_range as ir
import range_streams as rs

NAMES = ["one_pair", "no_location", "non_adsb", "relative_0_0", "longest_no_limit", "longest_limit", "three_receivers",
         "three_receivers_no_polar", "out_and_back", "chain", "contention", "limit_beside_the_range"]


def host_tracker(pkg, scenario, capacity=1024, table=False):
    receivers, fp, _, polar = scenario
    return pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, filter_persistence=fp, host=True, table=table,
                                    range=True, polar=polar)


def assert_margins(tracker):
    m, st = tracker.range_margins(), tracker.stats()
    assert st["min_gate_margin_m"] >= rs.GATE_MARGIN, st
    assert m["min_range_margin_m"] >= rs.RANGE_MARGIN, m
    assert m["min_bearing_margin_deg"] >= rs.BEARING_MARGIN, m
    return m


def host_equals_model(pkg, scenario, name=None, **kw):
    t, m = host_tracker(pkg, scenario, **kw), rs.model(scenario)
    got, want = rs.run(t, scenario[2]), rs.run(m, scenario[2])
    assert got == want
    assert assert_margins(t) == m.range_margins()
    if name:
        rs.known_answers(name, got)
    t.close()
    return got


@pytest.mark.parametrize("name", NAMES)
def test_host_object_equals_the_second_reading(pkg, name):
    host_equals_model(pkg, rs.scenarios(pkg)[name], name, capacity=64 if name == "chain" else 1024, table=name == "chain")


def test_bucket_wrap_and_bucket_edge(pkg):
    scenario, aimed = rs.bucket_wrap(pkg)
    rows, _, _ = host_equals_model(pkg, scenario)[-1]
    assert [b for _, b in aimed] == [0, 0, 18, 19]
    assert aimed[0][0] < 2.5 and aimed[1][0] > 357.5 and 0.02 <= aimed[3][0] - aimed[2][0] <= 0.025
    polar = rows[0][0]
    assert sorted(k for k, v in enumerate(polar) if v) == [0, 18, 19] and rows[0][3] == 4


def test_the_limit_beside_the_range_is_the_margin(pkg):
    scenario, rng, limit = rs.limit_beside_the_range(pkg)
    t = host_tracker(pkg, scenario)
    rs.run(t, scenario[2])
    m = assert_margins(t)
    assert abs(m["min_range_margin_m"] - 0.3) < 1e-6 and 0.45 <= rng - math.floor(rng) <= 0.55 and limit - rng == m["min_range_margin_m"]
    t.close()


@pytest.mark.parametrize("polar", [True, False])
def test_a_range_below_one_metre(pkg, polar):
    """0.4 m from the receiver: distance 0, evaluated, and with the polar range a bearing margin of 0 -- the host object
    says itself that the bucket of such a position is not covered by the contract; without it there is no bearing."""
    scenario = rs.below_one_metre(pkg, polar)
    t, m = host_tracker(pkg, scenario), rs.model(scenario)
    got, want = rs.run(t, scenario[2]), rs.run(m, scenario[2])
    assert got == want and t.range_margins() == m.range_margins()
    (row,), (d,) = got[-1][0], got[-1][1]
    assert d == 0 and row[1] == 0 and row[3] == 1 and not any(row[0])
    margins = t.range_margins()
    assert abs(margins["min_range_margin_m"] - 0.4) < 1e-3
    assert margins["min_bearing_margin_deg"] == (0.0 if polar else math.inf)
    assert t.stats()["min_gate_margin_m"] >= rs.GATE_MARGIN
    t.close()


def test_a_range_that_is_not_a_number(pkg):
    """A receiver whose latitude is not a number: greatcircle gives NaN, which compares false in update_polar_range's two
    tests (track.c:290, :302) -- the record is evaluated, the distance is 0, nothing becomes the longest -- and the host
    object reports a range margin of 0: such a stream is outside the contract.  Host object only: the reference's
    (uint32_t) of a NaN is undefined, so there is no second reading, and the device is not held to it."""
    b = rs.Builder(pkg)
    rs.pair(b, rs.T0, 0xA00091, 52.3, 4.5)
    t = pkg.capi.PositionTracker(capacity=64, receivers=[dict(lat=math.nan, lon=4.0, latlon_valid=1)], host=True, range=True, polar=False)
    out = t.update(*b.step()[1:])
    assert [int(x) for x in out["result"]] == [-1, 0]
    (row,) = rs.read_rows(t.range_read())
    assert row == ((0,) * 72, 0, 0, 1) and list(t.range_distances()) == [0]
    assert t.range_margins()["min_range_margin_m"] == 0.0
    t.close()


def test_cut_into_single_records(pkg):
    scenario = rs.scenarios(pkg)["out_and_back"]
    whole, cut = host_tracker(pkg, scenario), host_tracker(pkg, scenario)
    assert rs.run(whole, scenario[2]) == rs.run(cut, scenario[2], pieces=1)
    assert whole.range_read().tobytes() == cut.range_read().tobytes()


def test_mixed_stream(pkg):
    scenario = rs.mixed_stream(pkg)
    got = host_equals_model(pkg, scenario, table=True)
    rows, dist, _ = got[-1]
    assert [r[3] > 250 for r in rows] == [True, True, False, True] and rows[2] == ((0,) * 72, 0, 0, 0)
    assert len(dist) == 48 and sum(1 for d in dist if d) >= 25


def test_table_and_plain_trackers_agree(pkg):
    scenario = rs.scenarios(pkg)["three_receivers"]
    a, b = host_tracker(pkg, scenario, table=False), host_tracker(pkg, scenario, table=True)
    assert rs.run(a, scenario[2]) == rs.run(b, scenario[2])
    keys = [(int(e["receiver"]), int(e["addr"])) for e in b.snapshot()]
    m = rs.model(scenario)
    rs.run(m, scenario[2])
    assert keys == m.snapshot_keys()  # range_distances' order is the snapshot's


def test_enable_late_starts_every_aircraft_at_zero(pkg):
    scenario = rs.scenarios(pkg)["three_receivers"]
    receivers, fp, steps, _ = scenario
    t = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, filter_persistence=fp, host=True)
    rs_first = steps[0]
    t.update(*rs_first[1:])
    t.range_enable(pkg.capi.RANGE_POLAR)
    assert list(t.range_distances()) == [0] * 65
    assert rs.read_rows(t.range_read()) == [((0,) * 72, 0, 0, 0)] * 3
    assert t.range_margins() == dict(min_range_margin_m=math.inf, min_bearing_margin_deg=math.inf)


def last_time(steps):
    return max(int(s[1]["sysTimestampMsg"].max()) for s in steps if s[0] == "update")


@pytest.mark.parametrize("name", ["three_receivers", "non_adsb", "mixed"])
def test_protobuf_outputs(pkg, name):
    """range_pb and aircraft.pb with distance (13) on the host object against the second reading: `68 <varint>` stands
    between rssi (12) and air_ground (15) or what follows, in the entries of the aircraft with a distance and no other."""
    import indep_range_pb
    scenario = rs.mixed_stream(pkg) if name == "mixed" else rs.scenarios(pkg)[name]
    receivers, fp, steps, polar = scenario
    t = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, filter_persistence=fp, host=True, table=True, pb=True,
                                 range=True, polar=polar)
    m = rs.model(scenario)
    rs.run(t, steps), rs.run(m, steps)
    now = last_time(steps) + 1000
    snapshot = t.snapshot()
    got, want = rs.pb_of(t, scenario, now), rs.pb_of_model(pkg, m, snapshot, now)
    assert got[0] == want[0] and got[1] == want[1]
    assert t.pb_margin >= pkg.capi.PB_RSSI_MARGIN_ULPS
    for r, f in enumerate(got[1]):
        for addr, d, before, after in indep_range_pb.distance_places(f):
            a = m.aircraft[(r, addr)]
            assert (d or 0) == getattr(a, "distance", 0)
            assert d is None or (before == 12 and after >= 15)
    with_distance = sum(1 for f in got[1] for _, d, _, _ in indep_range_pb.distance_places(f) if d)
    assert with_distance == {"three_receivers": 65, "non_adsb": 0, "mixed": sum(1 for d in t.range_distances() if d)}[name]
    if name == "mixed":
        assert with_distance >= 25
    # a tracker without the range writes the entries without the field
    plain = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, filter_persistence=fp, host=True, table=True, pb=True)
    rs_run_plain(plain, steps)
    for f in plain.aircraft_pb(now):
        assert all(d is None for _, d, _, _ in indep_range_pb.distance_places(f))
    t.close(), plain.close()


def rs_run_plain(tracker, steps):
    for s in steps:
        if s[0] == "update":
            tracker.update(*s[1:])
        elif s[0] == "expire":
            tracker.expire(s[1])


def test_second_reading_units():
    assert ir.c_round(2.5) == 3 and ir.c_round(0.49) == 0 and ir.c_round(71.5) == 72
    assert abs(ir.edge_distance(2.5)) < 1e-12 and abs(ir.edge_distance(357.5)) < 1e-12 and abs(ir.edge_distance(5.0) - 2.5) < 1e-12
    assert ir.polar_range_pb([0] * 72)[:8] == bytes.fromhex("3200320208013202") and len(ir.polar_range_pb([0] * 72)) == 2 + 71 * 4
    assert ir.polar_range_pb([300] + [0] * 71)[:5] == bytes.fromhex("320310ac02")
