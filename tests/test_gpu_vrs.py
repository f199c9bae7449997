"""The VRS output on the GPU (msd_pos_vrs_enable, msd_pos_vrs) against the host object, which test_vrs_model.py holds equal
to a second reading of generateVRS and to documents written by hand.  Everything is compared by bytes -- the stream of every
receiver's document and the rows beside it --: the contract is the table's and has no margin.
Beside the rules this covers what exists on the device only: the items (heads and tails between the aircraft, empty
receivers), the comma's two prefix counts across workgroups and store tiles of vrs_streams.TILE items, the table shared
with aircraft.pb in either order of the two enables, reset, the rebuilt table, refused calls, and the ordering by key
whatever slots the aircraft are in."""
import ctypes as C
import errno
import json

import numpy as np
import pytest

import indep_aircraft_pb as ipb
import pb_streams as pbs
import vrs_streams as vs

pytestmark = pytest.mark.gpu


def tracker(pkg, host, receivers, capacity=2048, vrs=True, **kw):
    return pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, host=host, table=True, vrs=vrs, **kw)


def run(pkg, host, scenario, capacity=2048, **kw):
    t = tracker(pkg, host, scenario[0], capacity)
    out = vs.run(t, scenario, **kw)
    t.close()
    return out


def same(got, want):
    """got: the device's writes, want: the host object's"""
    assert len(got) == len(want) and len(want) > 0
    for w, ((stream, rx), (hstream, hrx)) in enumerate(zip(got, want)):
        assert rx.tobytes() == hrx.tobytes(), (w, rx, hrx)
        if stream != hstream:
            a, b = vs.split(stream, rx), vs.split(hstream, hrx)
            r = [i for i in range(len(b)) if a[i] != b[i]][0]
            k = [i for i in range(len(b[r])) if i >= len(a[r]) or a[r][i] != b[r][i]][0]
            raise AssertionError((w, r, k, a[r][max(k - 60, 0):k + 60], b[r][max(k - 60, 0):k + 60]))


@pytest.fixture(scope="module")
def host_runs(pkg):
    """every table's scenario and the host object's writes of it, computed once"""
    out = {}
    for name, make in vs.TABLES.items():
        sc = make(pkg)
        out[name] = (sc, run(pkg, True, sc))
    return out


@pytest.mark.parametrize("name", list(vs.TABLES))
def test_table(pkg, torch_cuda, host_runs, name):
    sc, want = host_runs[name]
    same(run(pkg, False, sc), want)


def test_tables_are_what_they_are_named_for(pkg, host_runs):
    """the counts around the tile, an empty receiver in the middle and at the end; the comma table's selected counts with
    its first selected aircraft on a tile's first and last item (asserted where the table is built); staleness; one
    aircraft per branch; the escapes; the widest object records can build and the signal levels beyond the range"""
    T = vs.TILE
    (stream, rx), = host_runs["counts"][1]
    assert [int(x) for x in rx["aircraft"]] == [1, 0, T - 1, T, T + 1, 2 * T + 1, 0]
    assert [len(json.loads(d)["acList"]) for d in vs.split(stream, rx)] == [1, 0, T - 1, T, T + 1, 2 * T + 1, 0]
    (stream, rx), = host_runs["comma"][1]
    assert [int(x) for x in rx["aircraft"]] == vs.COMMA_COUNTS
    assert [len(json.loads(d)["acList"]) for d in vs.split(stream, rx)] == vs.COMMA_COUNTS
    (stream, rx), = host_runs["stale"][1]
    assert [a["Icao"] for a in json.loads(stream)["acList"]] == ["4C0001", "4C0004"]
    (stream, rx), = host_runs["kinds"][1]
    assert int(rx["aircraft"][0]) == 28 and stream.count(b'"Tisb":true') == 2 and stream.count(b'"Lat"') == 2
    (stream, rx), = host_runs["escapes"][1]
    assert stream.count(b"\\u00") == 8 and b'\\"' in stream and b"\\\\" in stream and b"\x7f" in stream
    (stream, rx), = host_runs["bounds"][1]
    assert [a["Sig"] for a in json.loads(stream)["acList"]] == [956250000, 4271250000, 0, 0, 0, 0, 0, 3825000000]


def test_parts(pkg, torch_cuda):
    """n_parts of 1, 8 and 2048 over addresses whose low eleven bits are 0, 255, 256, 2047 and 2048 + 255: every part equals
    the host object's, each aircraft is in the part the formula gives, and the parts together hold each exactly once"""
    sc = vs.parts_table(pkg)
    dev, host = tracker(pkg, False, sc[0], 64), tracker(pkg, True, sc[0], 64)
    for t in (dev, host):
        t.update_nicrc(*sc[1][0][1:])
    everyone = sorted((r, 0x4B0000 + 0x1000 * r + low) for r in range(2) for low in vs.PART_LOWS)
    for n_parts in (1, 8, 2048):
        seen = []
        for part in range(n_parts):
            stream, rx = dev.vrs_stream(vs.T0 + 100, part, n_parts, cap=4096)
            hstream, hrx = host.vrs_stream(vs.T0 + 100, part, n_parts, cap=4096)
            assert stream == hstream and rx.tobytes() == hrx.tobytes(), (n_parts, part)
            if len(stream) == 28:
                continue
            for r, doc in enumerate(vs.split(stream, rx)):
                for a in json.loads(doc)["acList"]:
                    addr = int(a["Icao"], 16)
                    assert (addr & 2047) >> (11 - n_parts.bit_length() + 1) == part
                    seen.append((r, addr))
        assert sorted(seen) == everyone, n_parts
    dev.close(), host.close()


def test_staleness_against_aircraft_pb(pkg, torch_cuda, host_runs):
    """the aircraft seen one millisecond after now_ms: VRS leaves it out, aircraft.pb on the same tracker writes it"""
    sc, want = host_runs["stale"]
    t = tracker(pkg, False, sc[0], 64, pb=True)
    t.update_nicrc(*sc[1][0][1:])
    now = sc[2][0][1]
    assert [a["addr"] & 0xFF for a in ipb.read_file(t.aircraft_pb(now)[0])["aircraft"]] == [1, 2, 3, 4]
    same([t.vrs_stream(now)], want)
    t.close()


def test_refused_and_repeated_calls(pkg, torch_cuda, host_runs):
    """-ENOSPC at cap = 0 and at cap = need - 1 with the size, then the same bytes; two calls in a row give the same"""
    for name in ("comma", "kinds", "expiring"):
        sc, want = host_runs[name]
        same(run(pkg, False, sc, refuse=True), want)
    sc, want = host_runs["counts"]
    t = tracker(pkg, False, sc[0])
    t.update_nicrc(*sc[1][0][1:])
    first, again = t.vrs_stream(vs.T0 + 5000), t.vrs_stream(vs.T0 + 5000)
    same([first], want), same([again], want)
    out = np.full(len(want[0][0]) + 8, 0xEE, dtype=np.uint8)
    rx = np.zeros(7, dtype=pkg.capi.VRS_RECEIVER_DTYPE)
    rx["end"] = 77
    opt, need = pkg.capi.VrsOptions(now_ms=vs.T0 + 5000, part=0, n_parts=1), C.c_size_t(0)
    assert t.f["vrs"](t.h, C.byref(opt), out.ctypes.data, len(want[0][0]) - 1, C.byref(need), rx.ctypes.data) == -errno.ENOSPC
    assert need.value == len(want[0][0]) and (out == 0xEE).all() and (rx["end"] == 77).all()  # nothing was written
    assert t.f["vrs"](t.h, C.byref(opt), out.ctypes.data, len(out), C.byref(need), None) == 0  # rx may be NULL
    assert out[:need.value].tobytes() == want[0][0] and (out[need.value:] == 0xEE).all()
    t.close()


def test_both_enable_orders_share_one_table_with_pb(pkg, torch_cuda):
    """aircraft.pb's bytes with VRS enabled before it, after it, and not at all are the same, and so are VRS's"""
    sc = pbs.TABLES["kinds"](pkg)
    pb_out, vrs_out = [], []
    for order in ("pb", "pb vrs", "vrs pb", "vrs"):
        t = pkg.capi.PositionTracker(capacity=1024, receivers=sc[0], host=False, table=True)
        for what in order.split():
            getattr(t, what + "_enable")()
            getattr(t, what + "_enable")()  # a second call changes nothing
        t.update_nicrc(*sc[1][0][1:])
        if "vrs" in order:
            vrs_out.append(t.vrs_stream(pbs.T0 + 2000))
        if "pb" in order:
            stream, rx = t.aircraft_pb_stream(*sc[2][0][1:])
            pb_out.append((stream, rx.tobytes()))
        if "vrs" in order:  # and after the pb write, which moved its own state alone
            vrs_out.append(t.vrs_stream(pbs.T0 + 2000))
        t.close()
    assert len(pb_out) == 3 and pb_out[0] == pb_out[1] == pb_out[2] and len(pb_out[0][0]) > 800
    host = pkg.capi.PositionTracker(capacity=1024, receivers=sc[0], host=True, table=True, vrs=True)
    host.update_nicrc(*sc[1][0][1:])
    want = host.vrs_stream(pbs.T0 + 2000)
    host.close()
    assert len(vrs_out) == 6
    for got in vrs_out:
        same([got], [want])


def test_reset_and_the_rebuilt_table(pkg, torch_cuda, host_runs):
    """msd_pos_reset leaves the tracker enabled and empty; the expiring table's writes straddle a rebuild (test_table);
    here the tracker is reset after it and fed another table"""
    sc, _ = host_runs["expiring"]
    other, want = host_runs["three"]
    outs = []
    for host in (True, False):
        t = tracker(pkg, host, other[0])
        vs.run(t, (other[0], sc[1], sc[2]))
        t.reset()
        empty = t.vrs_stream(vs.T0)
        assert empty[0] == b'{"acList":[]}\n' * 3 and not empty[1]["aircraft"].any()
        outs.append(vs.run(t, other))
        t.close()
    same(outs[0], want), same(outs[1], want)


def test_refusals(pkg, torch_cuda):
    capi = pkg.capi

    def code(call):
        with pytest.raises(pkg.MsdError) as e:
            call()
        return e.value.code
    t = capi.PositionTracker(capacity=64, host=False)  # no table
    assert code(t.vrs_enable) == -errno.EINVAL
    t.close()
    sc = vs.TABLES["three"](pkg)
    t = capi.PositionTracker(capacity=64, receivers=sc[0], host=False, table=True)
    t.update_nicrc(*sc[1][0][1:])
    snap = t.snapshot().tobytes()
    assert code(lambda: t.vrs_stream(vs.T0)) == -errno.EINVAL  # not enabled
    t.vrs_enable()
    assert t.snapshot().tobytes() == snap
    for bad in (dict(flags=1), dict(flags=1 << 31), dict(reserved=1), dict(n_parts=0), dict(n_parts=3), dict(n_parts=4096),
                dict(n_parts=6), dict(part=1), dict(part=8, n_parts=8), dict(part=2048, n_parts=2048)):
        assert code(lambda: t.vrs_stream(vs.T0 + 5000, **bad)) == -errno.EINVAL, bad
    fn = t.f["vrs"]
    opt, need = capi.VrsOptions(now_ms=vs.T0 + 5000, part=0, n_parts=1), C.c_size_t(7)
    out = np.zeros(4096, dtype=np.uint8)
    assert fn(None, C.byref(opt), out.ctypes.data, 4096, C.byref(need), None) == -errno.EINVAL
    assert fn(t.h, None, out.ctypes.data, 4096, C.byref(need), None) == -errno.EINVAL
    assert fn(t.h, C.byref(opt), out.ctypes.data, 4096, None, None) == -errno.EINVAL
    assert fn(t.h, C.byref(opt), None, 4096, C.byref(need), None) == -errno.EINVAL
    assert t.snapshot().tobytes() == snap  # the call is stateless
    t.close()


def test_slots_do_not_matter(pkg, torch_cuda, host_runs):
    """the same records aircraft by aircraft in the opposite order, in a larger table, and cut into calls of 61"""
    for name in ("counts", "comma"):
        sc, want = host_runs[name]
        _, m, f, r = sc[1][0]
        order = np.argsort(-f["addr"].astype(np.int64), kind="stable")
        back = (sc[0], [("update", m[order], f[order], r[order])], sc[2])
        same(run(pkg, False, back), want)
        same(run(pkg, False, sc, pieces=61), want)
        same(run(pkg, False, sc, capacity=1 << 14), want)
