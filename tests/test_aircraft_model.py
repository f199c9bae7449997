"""The aircraft table on the CPU: the host twin (libmsd_host.so, msd_trk_impl.h compiled for the host) against the second
reading of track.c in tests/indep_aircraft.py -- every msd_aircraft member of every snapshot, field by field, and the
NIC / Rc of every record --, on one small scenario per rule and on a 2000-record mixed stream; each scenario's decisive
value against an expectation derived by hand; and the properties the table promises: results do not depend on how a
stream is cut into calls, and a table tracker's msd_position rows are a table-less tracker's."""
import errno

import numpy as np
import pytest

import aircraft_streams as acs
import pos_streams as ps
import range_streams as rs
import whole_stack as ws


@pytest.fixture(scope="module")
def scen(pkg):
    return acs.scenarios(pkg)


NAMES = acs.NAMES


def twin(pkg, receivers, fp, steps, pieces=None, capacity=1024):
    t = pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, filter_persistence=fp, host=True, table=True)
    out = acs.run_library(t, steps, pieces)
    st = t.stats()
    t.close()
    assert st["min_gate_margin_m"] >= 1.0
    return out


def same_as_model(pkg, receivers, fp, steps, got):
    rows, nic, snaps = got
    mrows, mnic, msnaps = acs.run_model(pkg, receivers, fp, steps)
    assert ps.rows_of(rows) == ps.rows_of_model(mrows)
    assert [(int(q["nic"]), int(q["rc"]), int(q["set"])) for q in nic] == mnic
    assert len(snaps) == len(msnaps)
    for k, (s, w) in enumerate(zip(snaps, msnaps)):
        assert acs.differences(s, w) == [], k


def test_scenario_list_is_complete(scen):
    assert sorted(scen) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_twin_equals_second_reading(pkg, scen, name):
    receivers, fp, steps, _ = scen[name]
    same_as_model(pkg, receivers, fp, steps, twin(pkg, receivers, fp, steps))


@pytest.mark.parametrize("name", NAMES)
def test_scenario_reaches_what_it_is_named_for(pkg, scen, name):
    receivers, fp, steps, check = scen[name]
    rows, nic, snaps = twin(pkg, receivers, fp, steps)
    check([{int(e["addr"]): e for e in s} for s in snaps], [(int(q["nic"]), int(q["rc"]), int(q["set"])) for q in nic])
    assert all(int(q["set"]) == int(o["decoded"]) for q, o in zip(nic, rows))


@pytest.fixture(scope="module")
def mixed(pkg):
    receivers, m, f, r = acs.mixed_stream(pkg)
    steps = [("update", m, f, r)]
    return receivers, steps, twin(pkg, receivers, 0, steps)


def test_mixed_stream_equals_second_reading(pkg, mixed):
    receivers, steps, got = mixed
    same_as_model(pkg, receivers, 0, steps, got)
    snap = got[2][-1]
    assert len(snap) == 40 and sorted(set(int(x) for x in snap["receiver"])) == [0, 1]
    key = [(int(e["receiver"]), int(e["addr"])) for e in snap]
    assert key == sorted(key)
    assert int(got[1]["set"].sum()) > 800
    # the stream reaches the table's members: every validity but the rare true heading has been set for some aircraft
    AC = pkg.capi.AC
    reached = {k for k in pkg.capi.AC_MEMBERS if snap["updated"][:, AC[k]].any()}
    assert set(pkg.capi.AC_MEMBERS) - reached <= {"true_heading"}, set(pkg.capi.AC_MEMBERS) - reached


@pytest.mark.parametrize("pieces", [1, 7])
def test_cutting_does_not_matter(pkg, mixed, pieces):
    receivers, steps, (rows, nic, snaps) = mixed
    crows, cnic, csnaps = twin(pkg, receivers, 0, steps, pieces=pieces)
    assert crows.tobytes() == rows.tobytes() and cnic.tobytes() == nic.tobytes()
    assert csnaps[-1].tobytes() == snaps[-1].tobytes()


@pytest.mark.parametrize("name", ["gate_countdown", "derived_geom", "nic_relative_minimum", "heading_hrd_tah", "refusals",
                                  "combine_single_source"])
def test_cutting_does_not_matter_in_scenarios(pkg, scen, name):
    receivers, fp, steps, _ = scen[name]
    whole = twin(pkg, receivers, fp, steps)
    for pieces in (1, 7):
        cut = twin(pkg, receivers, fp, steps, pieces=pieces)
        assert cut[0].tobytes() == whole[0].tobytes() and cut[1].tobytes() == whole[1].tobytes()
        assert [s.tobytes() for s in cut[2]] == [s.tobytes() for s in whole[2]]


# ---- the drawn stream through everything at once (whole_stack.py) ----
@pytest.fixture(scope="module")
def drawn(pkg):
    receivers, m, f, r = acs.random_stream(pkg)
    steps, now = ws.steps_of(m, f, r)
    t = ws.tracker(pkg, receivers, True)
    host = ws.run_library(t, steps, now)
    t.close()
    return receivers, (m, f, r), steps, now, host


def test_drawn_stream_is_what_it_says(pkg, drawn):
    receivers, (m, f, r), steps, now, host = drawn
    tracked = (m["msgtype"] != 32) & (f["addr"] != 0)
    assert len(m) == 4000 and len(receivers) == 3 and set(r.tolist()) == {0, 1, 2}
    assert len(host["obs"][-1]["snap_raw"]) == 48 and len(set(f["addr"][tracked].tolist())) == 48
    assert sorted(set(f["source"][tracked].tolist())) == list(range(8))
    t = m["sysTimestampMsg"].astype(np.int64)
    behind = np.maximum.accumulate(t) - t
    assert 300 <= int((behind[tracked] > 400).sum()) <= 500 and 80000 < int(behind.max()) <= 90040  # one in ten, up to 90 s
    assert int((m["msgtype"] == 32).sum()) > 100 and int((m["msgtype"] == 11).sum()) > 50 and int((f["addr"] == 0).sum()) > 20
    # no gate, range or bearing where two libms could part, on the host object, with the figures of the range's tests
    assert host["stats"]["min_gate_margin_m"] >= rs.GATE_MARGIN
    assert host["margins"]["min_range_margin_m"] >= rs.RANGE_MARGIN and host["margins"]["min_bearing_margin_deg"] >= rs.BEARING_MARGIN
    assert host["pb_margin"] >= pkg.capi.PB_RSSI_MARGIN_ULPS
    # and the stream reaches the outputs: positions of every kind, hits, verdicts both ways, distances, text
    st = host["stats"]
    assert st["cpr_global_ok"] > 200 and st["cpr_local_aircraft_relative"] > 100 and st["cpr_global_bad"] > 10
    assert int(host["nic"]["set"].sum()) > 400
    hits = host["obs"][-1]["hits_raw"]
    assert int(hits["mode_a_hit"].sum()) >= 3
    assert 400 < int((host["fwd"] & 1).sum()) < 3600
    assert sum(1 for d in host["obs"][-1]["range"][1] if d) >= 10 and all(row[3] > 50 for row in host["obs"][-1]["range"][0])
    assert len(host["sbs_wire"][0]) > 100000 and all(len(x) > 200 for x in host["pb"]) and all(len(x) > 200 for x in host["vrs"])


def test_drawn_stream_equals_the_second_readings(pkg, drawn):
    """Rows, NIC / Rc, every step's snapshot, hits and codes, the verdicts and the reduced stream, the SBS rows and lines,
    the range after every step, aircraft.pb with distances, the polar range and the VRS list: the host object's against
    the second readings'.  The second reading of the table counts accept_data's verdicts: every member is accepted and
    refused at least RANDOM_MIN times, so no member's rule can hide."""
    receivers, _, steps, now, host = drawn
    counting = ws.run_models(pkg, receivers, steps, now, host)
    counts = {k: (counting.accepted.get(k, 0), counting.refused.get(k, 0)) for k in pkg.capi.AC_MEMBERS}
    print("accepted, refused:", counts)
    assert all(min(v) >= acs.RANDOM_MIN for v in counts.values()), {k: v for k, v in counts.items() if min(v) < acs.RANDOM_MIN}


@pytest.mark.parametrize("pieces", [1, 64, 97])
def test_drawn_stream_cut_into_calls(pkg, drawn, pieces):
    receivers, _, steps, now, host = drawn
    t = ws.tracker(pkg, receivers, True)
    ws.same_bytes(ws.run_library(t, steps, now, pieces), host)
    t.close()


def test_positions_of_a_table_tracker_are_a_table_less_trackers(pkg):
    receivers, m, f, r = ps.mixed_stream(pkg)
    res = []
    for table in (False, True):
        t = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, host=True, table=table)
        res.append((t.update(m, f, r).tobytes(), t.stats()))
        t.close()
    assert res[0] == res[1]


def test_table_less_twin_refuses_the_table_calls(pkg):
    receivers, m, f, r = ps.mixed_stream(pkg, n=50)
    t = pkg.capi.PositionTracker(capacity=64, receivers=receivers, host=True)
    for call in (lambda: t.update_nicrc(m, f, r), lambda: t.snapshot(4)):
        with pytest.raises(pkg.MsdError) as e:
            call()
        assert e.value.code == -errno.EINVAL
    t.close()


def test_snapshot_capacity_and_reset(pkg, scen):
    receivers, fp, steps, _ = scen["gate_fpm_default"]
    t = pkg.capi.PositionTracker(capacity=64, receivers=receivers, host=True, table=True)
    assert len(t.snapshot()) == 0
    acs.run_library(t, steps)
    assert t.live() == 2
    with pytest.raises(pkg.MsdError) as e:
        t.snapshot(1)
    assert e.value.code == -errno.ENOSPC and t.snapshot_count == 2
    assert len(t.snapshot(2)) == 2 and len(t.snapshot(5)) == 2
    t.reset()
    assert len(t.snapshot()) == 0 and t.live() == 0
    t.close()


def test_struct_sizes_and_padding(pkg):
    assert pkg.capi.AIRCRAFT_DTYPE.itemsize == 592 and pkg.capi.NICRC_DTYPE.itemsize == 4
    assert pkg.capi.POSITION_DTYPE.itemsize == 24
    names = pkg.capi.AIRCRAFT_DTYPE.names
    end = 0
    for k in names:  # no implicit padding: every member starts where the one before ends
        dt, off = pkg.capi.AIRCRAFT_DTYPE.fields[k][:2]
        assert off == end, k
        end = off + dt.itemsize
    assert end == 592
