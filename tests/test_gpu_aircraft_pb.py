"""aircraft.pb on the GPU (msd_pos_pb_enable, msd_pos_aircraft_pb) against the host object, which test_pb_model.py holds
equal to a second reading of net_io.c / readsb.proto and to files written out by hand.  Everything is compared by bytes --
the stream of every receiver's file and the rows beside it --: the contract is the table's and has no tolerance, given
that the one libm call (rssi's log10) stays MSD_PB_RSSI_MARGIN_ULPS from a rounding boundary on the host object.  Every
test asserts that margin first, for every table it writes, so that no comparison is ever skipped.
Beside the rules this covers what exists on the device only: the items (file heads between the aircraft, empty receivers),
the store kernel's image of pb_streams.TILE items and its two rounds per workgroup, the written state beside the table --
new aircraft, the rebuilt table, reset, a refused call -- and the ordering by key whatever slots the aircraft are in."""
import errno

import numpy as np
import pytest

import aircraft_streams as acs
import indep_aircraft_pb as ipb
import pb_streams as pbs

pytestmark = pytest.mark.gpu


def tracker(pkg, host, receivers, capacity=1024, pb=True):
    return pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, host=host, table=True, pb=pb)


def run(pkg, host, scenario, capacity=1024, **kw):
    t = tracker(pkg, host, scenario[0], capacity)
    out = pbs.run(t, scenario, **kw)
    t.close()
    return out


def same(pkg, got, want):
    """got: the device's writes, want: the host object's"""
    assert len(got) == len(want) and len(want) > 0
    for (_, _, margin) in want:  # first: the condition under which the contract holds, for every table written
        assert margin >= pkg.capi.PB_RSSI_MARGIN_ULPS, margin
    for w, ((stream, rx, _), (hstream, hrx, _)) in enumerate(zip(got, want)):
        assert rx.tobytes() == hrx.tobytes(), (w, rx, hrx)
        if stream != hstream:
            a, b = pbs.split(stream, rx), pbs.split(hstream, hrx)
            r = [i for i in range(len(b)) if a[i] != b[i]][0]
            da, db = ipb.read(ipb.UPDATE, a[r]).get("aircraft", []), ipb.read(ipb.UPDATE, b[r]).get("aircraft", [])
            k = [i for i in range(len(db)) if i >= len(da) or da[i] != db[i]][:1]
            raise AssertionError((w, r, k, da[k[0]].hex() if k and k[0] < len(da) else None, db[k[0]].hex() if k else None))


@pytest.fixture(scope="module")
def host_runs(pkg):
    """every table's scenario and the host object's writes of it, computed once"""
    out = {}
    for name, make in pbs.TABLES.items():
        sc = make(pkg)
        out[name] = (sc, run(pkg, True, sc))
    return out


@pytest.mark.parametrize("name", list(pbs.TABLES))
def test_table(pkg, torch_cuda, host_runs, name):
    sc, want = host_runs[name]
    same(pkg, run(pkg, False, sc), want)


def test_counts_meet_the_tile_seams(pkg, host_runs):
    """0, 1, TILE - 1, TILE, TILE + 1 and 2 x TILE + 1 aircraft per receiver, an empty receiver in the middle and at the end"""
    T = pbs.TILE
    (stream, rx, _), = host_runs["counts"][1]
    assert [int(x) for x in rx["aircraft"]] == [1, 0, T - 1, T, T + 1, 2 * T + 1, 0]
    files = pbs.split(stream, rx)
    assert [len(ipb.read_file(f)["aircraft"]) for f in files] == [1, 0, T - 1, T, T + 1, 2 * T + 1, 0]
    assert ipb.read_file(files[6]) == dict(now=(pbs.T0 + 5000) // 1000, messages=6000, aircraft=[])
    (stream, rx, _), = host_runs["three"][1]
    assert [int(x) for x in rx["aircraft"]] == [3, 0, 2] and int(rx["end"][1]) - int(rx["end"][0]) == 9
    (stream, rx, _), = host_runs["filter"][1]
    assert [int(x) for x in rx["aircraft"]] == [0, 2]
    assert [a["addr"] for a in ipb.read_file(pbs.split(stream, rx)[1])["aircraft"]] == [0x410003, 0x410004]


def test_one_and_two_byte_length_prefix(pkg, host_runs):
    (stream, rx, _), = host_runs["sizes"][1]
    sizes = {len(a) for a in ipb.read(ipb.UPDATE, stream)["aircraft"]}
    assert 127 in sizes and 128 in sizes and min(sizes) < 100 and max(sizes) > 150


def test_kinds_are_all_there(pkg, host_runs):
    (stream, rx, _), = host_runs["kinds"][1]
    ac = {a["addr"] & 0xFF: a for a in ipb.read_file(stream)["aircraft"]}
    assert len(ac) == 18 and (int(rx["with_positions"][0]), int(rx["tisb_positions"][0])) == (2, 1)
    assert ac[1]["rssi"] == np.float32(10 * np.log10(9e-5 / 8)) and ac[2]["track"] == 315 and ac[3]["track"] == 90
    assert "track" not in ac[4] and ac[5]["mag_heading"] == 351 and ac[6]["true_heading"] == 180 and ac[6]["mag_heading"] == 357
    assert ac[7]["track"] == 92 and ac[8]["track"] == 359 and ac[9]["track"] == 180 and "track" not in ac[10]
    assert ac[8]["roll"] < 0 < ac[9]["roll"] and ac[8]["track_rate"] < 0 < ac[9]["track_rate"]
    assert ac[11]["mag_heading"] == 263 and abs(ac[11]["mach"] - 0.76) < 1e-6
    assert ac[12]["nav_altitude_mcp"] == -1000 and abs(ac[12]["nav_qnh"] - 1013.2) < 1e-3
    assert ac[13]["nav_heading"] == 359 and abs(ac[13]["nav_qnh"] - 1012.8) < 1e-3 and ac[14]["nav_heading"] == 359
    assert ac[15]["alt_baro"] == -975 and ac[15]["geom_rate"] == -2048
    assert abs(ac[16]["lat"] - 50.0) < 1e-3 and ac[17]["valid_source"]["lat"] == 5 and ac[17]["addr_type"] == 3
    assert ac[18]["ias"] == 280 and ac[18]["tas"] == 420


def test_stickiness_over_three_writes(pkg, host_runs):
    w1, w2, w3 = [{a["addr"] & 0xF: a for a in ipb.read_file(s)["aircraft"]} for s, _, _ in host_runs["sticky"][1]]
    assert sorted(w1) == [1, 4] and sorted(w2) == [1, 2, 3, 4] and sorted(w3) == [1, 2, 3, 4]
    for w in (w1, w2, w3):  # A: valid at the first write, expired at the others, still written; seen_pos keeps its value
        assert w[1]["flight"] == b"STICKY  " and w[1]["nav_modes"] == dict(autopilot=1, althold=1) and w[1]["seen_pos"] == 5
        assert w[4]["nav_modes"] == {} and "flight" not in w[4]
    assert w1[1]["valid_source"]["callsign"] == 7 and w2[1]["valid_source"]["callsign"] == 7
    for w in (w2, w3):  # B: the bytes are stored, but were never valid at a write
        assert not {"flight", "nav_modes", "seen_pos"} & set(w[2]) and w[2]["valid_source"]["callsign"] == 7 and w[2]["lat"] != 0
        assert w[3]["flight"] == b"LATE"


def test_refused_call_moves_no_state(pkg, torch_cuda, host_runs):
    """every write first offered one byte less than it needs: -ENOSPC with the size, then the same bytes as a tracker that
    was never refused -- over the three sticky writes the state advanced exactly once per write"""
    for name in ("sticky", "kinds"):
        sc, want = host_runs[name]
        same(pkg, run(pkg, False, sc, refuse=True), want)
        same(pkg, run(pkg, True, sc, refuse=True), want)


def test_slots_do_not_matter(pkg, torch_cuda, host_runs):
    """the same records aircraft by aircraft in the opposite order, in a table two thirds full, and cut into calls of 61"""
    sc, want = host_runs["counts"]
    _, m, f, r = sc[1][0]
    order = np.argsort(-f["addr"].astype(np.int64), kind="stable")
    back = (sc[0], [("update", m[order], f[order], r[order])], sc[2])
    same(pkg, run(pkg, False, back), want)
    same(pkg, run(pkg, False, sc, pieces=61), want)
    same(pkg, run(pkg, False, sc, capacity=1 << 14), want)


def test_mixed_stream_with_expiries(pkg, torch_cuda):
    """the aircraft table's mixed stream of 40 aircraft on two receivers, a file every 20 s of it and an expiry before each"""
    receivers, m, f, r = acs.mixed_stream(pkg)
    t = m["sysTimestampMsg"].astype(np.int64)
    steps, writes = [], []
    cuts = list(range(int(t.min()) + 20000, int(t.max()) + 20000, 20000))
    lo = int(t.min())
    for hi in cuts:
        sel = (t >= lo) & (t < hi)
        steps += [("update", m[sel], f[sel], r[sel]), ("expire", hi)]
        writes.append((len(steps) - 1, hi, [len(steps), 7]))
        lo = hi
    writes.append((len(steps) - 1, cuts[-1] + 60000, None))  # most members have expired, the aircraft have not
    sc = (receivers, steps, writes)
    want = run(pkg, True, sc)
    assert sum(int(rx["aircraft"].sum()) for _, rx, _ in want) > 100 and any(int(rx["with_positions"].sum()) for _, rx, _ in want)
    same(pkg, run(pkg, False, sc), want)


def test_reset_and_late_enable(pkg, torch_cuda, host_runs):
    """msd_pos_reset forgets the written state; msd_pos_pb_enable on a table that already has aircraft starts them at 0"""
    sc, _ = host_runs["sticky"]
    outs = []
    for host in (True, False):
        t = tracker(pkg, host, sc[0])
        pbs.run(t, sc)
        t.reset()
        again = acs.Builder(pkg)  # A in its old slot: nothing of what was written before the reset may show
        pbs.two(again, pbs.T0 + 200000, 0x440001, signal=0.02)
        got = pbs.run(t, (sc[0], [again.step()], [(0, pbs.T0 + 200500, None)]))
        late = tracker(pkg, host, sc[0], pb=False)
        late.update_nicrc(*sc[1][0][1:])
        late.pb_enable()
        late.pb_enable()
        got += pbs.run(late, (sc[0], sc[1][1:], [(w[0] - 1,) + w[1:] for w in sc[2][1:]]))
        outs.append(got)
        t.close(), late.close()
    a = {x["addr"] & 0xF: x for x in ipb.read_file(outs[0][0][0])["aircraft"]}
    assert sorted(a) == [1] and not {"flight", "nav_modes", "seen_pos"} & set(a[1])
    same(pkg, outs[1], outs[0])


def test_tracker_without_pb(pkg, torch_cuda, host_runs):
    """-EINVAL, and the table is what the enabled tracker's is"""
    sc, _ = host_runs["kinds"]
    snaps = []
    for pb in (False, True):
        t = tracker(pkg, False, sc[0], pb=pb)
        t.update_nicrc(*sc[1][0][1:])
        snaps.append(t.snapshot().tobytes())
        if not pb:
            with pytest.raises(pkg.capi.MsdError) as e:
                t.aircraft_pb_stream(pbs.T0)
            assert str(-errno.EINVAL) in str(e.value)
        t.close()
    assert snaps[0] == snaps[1] and len(snaps[0]) == 18 * 592
