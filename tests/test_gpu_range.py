"""The receiver range on the GPU (msd_pos_range_*: the range instantiation of the position walk, msd_pos_range_kernel and
the per-slot distance) against the host object and against the second reading of tests/indep_range.py, on the constructed
streams of tests/range_streams.py: after every step the rows of range_read, the distances and the position records are
the same in all three, and the device's and the host object's arrays are the same bytes.  The host object's margins are
asserted on every stream: gates 1 m, ranges 0.05 m, bearings 0.01 degrees -- fifty and a thousand times the contract."""
import ctypes as C
import errno

import numpy as np
import pytest

import range_streams as rs
from test_range_model import NAMES, assert_margins, last_time, rs_run_plain

pytestmark = pytest.mark.gpu


def trackers(pkg, scenario, capacity=1024, table=False, range=True):
    receivers, fp, _, polar = scenario
    return [pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, filter_persistence=fp, host=host, table=table,
                                     range=range, polar=polar) for host in (False, True)]


def three_ways(pkg, scenario, name=None, pieces=None, **kw):
    dev, host = trackers(pkg, scenario, **kw)
    got, twin, want = rs.run(dev, scenario[2], pieces), rs.run(host, scenario[2], pieces), rs.run(rs.model(scenario), scenario[2])
    assert_margins(host)
    assert got == want and twin == want
    assert dev.range_read().tobytes() == host.range_read().tobytes()
    assert dev.range_distances().tobytes() == host.range_distances().tobytes()
    m = dev.range_margins()  # the device's own, with its own libm: close to the host's, not the same doubles
    h = host.range_margins()
    for k in m:
        assert m[k] == h[k] or abs(m[k] - h[k]) < 1e-3, (k, m, h)
    if name:
        rs.known_answers(name, got)
    dev.close(), host.close()
    return got


@pytest.mark.parametrize("name", NAMES)
def test_scenario(pkg, torch_cuda, name):
    """1-4, 6-11: one pair; no receiver location and set_receiver; a TIS-B position; a receiver-relative decode at 0 / 0;
    longest with and without --max-range and MSD_RANGE_TAKE_LONGEST; 65 aircraft on three receivers, with and without
    MSD_RANGE_POLAR; 300 records of one aircraft; the probe chain through expiry and reset in a table of 64 slots; 4096
    records into one bucket."""
    three_ways(pkg, rs.scenarios(pkg)[name], name, capacity=64 if name == "chain" else 1024, table=name == "chain")


def test_bucket_wrap_and_bucket_edge(pkg, torch_cuda):
    """5: bearings just above 0 and just below 360 share bucket 0; 0.02 degrees across an edge are two buckets."""
    scenario, aimed = rs.bucket_wrap(pkg)
    rows, _, _ = three_ways(pkg, scenario)[-1]
    assert [b for _, b in aimed] == [0, 0, 18, 19]
    assert sorted(k for k, v in enumerate(rows[0][0]) if v) == [0, 18, 19] and rows[0][3] == 4


def test_cut_into_single_records(pkg, torch_cuda):
    """8: the same stream in pieces of one record gives the same bytes."""
    scenario = rs.scenarios(pkg)["out_and_back"]
    whole, _ = trackers(pkg, scenario)
    rs.run(whole, scenario[2])
    assert three_ways(pkg, scenario, "out_and_back", pieces=1)[-1][:2] == (rs.read_rows(whole.range_read()),
                                                                           [int(d) for d in whole.range_distances()])
    whole.close()


def test_distances_align_with_the_snapshot(pkg, torch_cuda):
    """7: range_distances' row j belongs to snapshot()'s row j; a plain tracker keeps the same distances as a table one."""
    scenario = rs.scenarios(pkg)["three_receivers"]
    dev, host = trackers(pkg, scenario, table=True)
    plain, _ = trackers(pkg, scenario, table=False)
    m = rs.model(scenario)
    for t in (dev, host, plain, m):
        rs.run(t, scenario[2])
    assert [(int(e["receiver"]), int(e["addr"])) for e in dev.snapshot()] == m.snapshot_keys()
    assert list(dev.range_distances()) == list(plain.range_distances()) == list(host.range_distances()) == m.range_distances()
    d_out = torch_cuda.zeros(70, dtype=torch_cuda.int32, device="cuda")
    assert dev.range_distances_device(d_out.data_ptr(), 70) == 65
    assert d_out.cpu().numpy()[:65].tolist() == m.range_distances() and not d_out.cpu().numpy()[65:].any()
    for t in (dev, host, plain):
        t.close()


def test_mixed_stream(pkg, torch_cuda):
    """14: 2000 records over four receivers, everything at once; and cut into calls of 97 records."""
    scenario = rs.mixed_stream(pkg)
    whole = three_ways(pkg, scenario, table=True)
    cut = three_ways(pkg, scenario, table=True, pieces=97)
    assert whole[-1][:2] == cut[-1][:2] and [r[3] > 250 for r in whole[-1][0]] == [True, True, False, True]


@pytest.mark.parametrize("name", ["three_receivers", "non_adsb", "mixed"])
def test_protobuf_outputs(pkg, torch_cuda, name):
    """13: range_pb, and aircraft_pb() with `68 <varint>` exactly where the second reading says, on the device, the host
    object and the second reading; a tracker without the range writes what indep_aircraft_pb.py -- the reading of the
    field-less file -- says."""
    import indep_aircraft_pb
    import indep_range_pb
    scenario = rs.mixed_stream(pkg) if name == "mixed" else rs.scenarios(pkg)[name]
    receivers, fp, steps, polar = scenario
    dev, host = [pkg.capi.PositionTracker(capacity=1024, receivers=receivers, filter_persistence=fp, host=h, table=True, pb=True,
                                          range=True, polar=polar) for h in (False, True)]
    m = rs.model(scenario)
    for t in (dev, host, m):
        rs.run(t, steps)
    now = last_time(steps) + 1000
    snapshot = host.snapshot()
    assert dev.snapshot().tobytes() == snapshot.tobytes()
    got, twin, want = rs.pb_of(dev, scenario, now), rs.pb_of(host, scenario, now), rs.pb_of_model(pkg, m, snapshot, now)
    assert host.pb_margin >= pkg.capi.PB_RSSI_MARGIN_ULPS
    assert_margins(host)
    assert got[0] == want[0] and twin[0] == want[0]
    assert got[1] == want[1] and twin[1] == want[1]
    places = [p for f in got[1] for p in indep_range_pb.distance_places(f)]
    assert sum(1 for p in places if p[1]) == sum(1 for d in dev.range_distances() if d)
    assert all(p[1] is None or (p[2] == 12 and p[3] >= 15) for p in places)
    if name != "non_adsb":
        assert sum(1 for p in places if p[1]) >= 25
    # a second write: the written state moved the same way with the field in the entries
    assert dev.aircraft_pb(now + 1000) == host.aircraft_pb(now + 1000)
    plain = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, filter_persistence=fp, table=True, pb=True)
    rs_run_plain(plain, steps)
    w = indep_aircraft_pb.Writer(pkg.capi.AC, len(receivers))
    assert plain.aircraft_pb(now) == w.files(plain.snapshot(), now)[0]
    for t in (dev, host, plain):
        t.close()


def test_range_pb_sizes_and_refusals(pkg, torch_cuda):
    """12: -ENOSPC from range_pb reports the size and writes nothing; -EINVAL without MSD_RANGE_POLAR and without the
    enable; an untouched tracker writes 32 00 and 71 entries of four bytes per receiver."""
    scenario = rs.scenarios(pkg)["three_receivers"]
    receivers, fp, steps, _ = scenario
    for host in (False, True):
        t = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, host=host, range=True)
        empty = bytes.fromhex("3200") + b"".join(bytes([0x32, 0x02, 0x08, b]) for b in range(1, 72))
        assert t.range_pb() == [empty] * 3
        rs.run(t, steps)
        out, end, need = np.full(4096, 0xEE, dtype=np.uint8), np.full(3, 77, dtype=np.uint64), C.c_size_t(0)
        for cap in (0, 1, 3 * len(empty)):
            assert t.f["range_pb"](t.h, out.ctypes.data, cap, C.byref(need), end.ctypes.data) == -errno.ENOSPC
            assert need.value > 3 * len(empty) and (out == 0xEE).all() and (end == 77).all()
        size = need.value
        assert t.f["range_pb"](t.h, None, 4096, C.byref(need), end.ctypes.data) == -errno.EINVAL
        assert t.f["range_pb"](t.h, out.ctypes.data, 4096, None, end.ctypes.data) == -errno.EINVAL
        assert t.f["range_pb"](t.h, out.ctypes.data, size, C.byref(need), None) == 0 and need.value == size  # end may be NULL
        assert (out[size:] == 0xEE).all()
        stream, ends = t.range_pb_stream()
        assert stream == out[:size].tobytes() and int(ends[-1]) == size
        assert stream == b"".join(rs.ir.polar_range_pb(r[0]) for r in rs.read_rows(t.range_read()))
        t.close()
        t = pkg.capi.PositionTracker(capacity=64, host=host, range=True, polar=False)
        assert code_of(pkg, t.range_pb) == -errno.EINVAL
        t.close()
        t = pkg.capi.PositionTracker(capacity=64, host=host)
        assert code_of(pkg, t.range_pb) == -errno.EINVAL
        t.close()


def code_of(pkg, call):
    with pytest.raises(pkg.MsdError) as e:
        call()
    return e.value.code


def test_error_paths(pkg, torch_cuda):
    """12: -EINVAL without the enable and for unknown flags; -ENOSPC from range_distances reports the size and writes
    nothing; an update that fails with -ENOSPC leaves arrays and distances as they were."""
    capi = pkg.capi
    scenario = rs.scenarios(pkg)["three_receivers"]
    for host in (False, True):
        t = capi.PositionTracker(capacity=64, host=host)
        for call in (t.range_read, t.range_distances, t.range_margins):
            assert code_of(pkg, call) == -errno.EINVAL
        assert code_of(pkg, lambda: t.range_enable(2)) == -errno.EINVAL
        assert code_of(pkg, t.range_read) == -errno.EINVAL  # still not enabled
        t.range_enable(0)
        t.range_enable(capi.RANGE_POLAR)  # a second call changes nothing: still without the polar range
        t.close()
        receivers, fp, steps, _ = scenario
        t = capi.PositionTracker(capacity=128, receivers=receivers, host=host, range=True)
        rs.run(t, steps)
        for bad in (dict(first=4), dict(first=2, count=2), dict(flags=2), dict(first=3, count=1)):
            assert code_of(pkg, lambda: t.range_read(**bad)) == -errno.EINVAL, bad
        assert len(t.range_read(first=3, count=0)) == 0 and len(t.range_read(first=1)) == 2
        out, n = np.full(70, 0xEEEEEEEE, dtype=np.uint32), C.c_size_t(0)
        dev = [] if host else [0]
        for cap in (0, 1, 64):
            assert t.f["range_distances"](t.h, out.ctypes.data, cap, *dev, C.byref(n)) == -errno.ENOSPC
            assert n.value == 65 and (out == 0xEEEEEEEE).all()
        assert t.f["range_distances"](t.h, None, 70, *dev, C.byref(n)) == -errno.EINVAL
        assert t.f["range_distances"](t.h, out.ctypes.data, 70, *dev, None) == -errno.EINVAL
        assert t.f["range_distances"](t.h, out.ctypes.data, 70, *dev, C.byref(n)) == 0 and n.value == 65
        assert (out[65:] == 0xEEEEEEEE).all() and out[:65].all()
        # 65 aircraft live in 128 slots; a call that brings 64 new ones (and decodes positions for the known ones) is refused
        before = (t.range_read().tobytes(), t.range_distances().tobytes(), t.range_margins())
        b = rs.Builder(pkg)
        for k in range(65):
            rs.pair(b, rs.T0 + 5000, 0xA10000 + 7 * k, 40.0, 40.0, rx=k % 3)  # the known aircraft, far away: would change everything
        for k in range(64):
            b.pos(rs.T0 + 5000, 0xB00000 + k, 50.0, 5.0, 0)
        _, m, f, r = b.step()
        assert code_of(pkg, lambda: t.update(m, f, r)) == -errno.ENOSPC
        assert (t.range_read().tobytes(), t.range_distances().tobytes(), t.range_margins()) == before
        t.close()


def test_a_tracker_without_the_range_is_untouched(pkg, torch_cuda):
    """A tracker that never enables the range delivers what one that does delivers for the positions, NIC / Rc and the
    table: the range adds outputs and changes none."""
    scenario = rs.mixed_stream(pkg)
    receivers, fp, steps, _ = scenario
    a = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, table=True)
    b = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, table=True, range=True)
    for s in steps:
        if s[0] == "update":
            for x, y in zip(a.update_nicrc(*s[1:]), b.update_nicrc(*s[1:])):
                assert x.tobytes() == y.tobytes()
        else:
            a.expire(s[1]), b.expire(s[1])
    assert a.snapshot().tobytes() == b.snapshot().tobytes() and a.stats() == b.stats()
    assert code_of(pkg, a.range_read) == -errno.EINVAL
    a.close(), b.close()
