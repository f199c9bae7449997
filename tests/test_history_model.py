"""history_N.pb on the CPU: the host object (msd_pos_host_history_pb) == the second reading (tests/indep_history.py) ==
bytes written by hand, on the smallest tables at which each rule of modes_hip.h "history_N.pb" flips
(tests/history_streams.py), the values no decoder delivers on constructed entries, the refusals, and the statelessness
against aircraft.pb.  The device is held to the same in tests/test_gpu_history_pb.py."""
import ctypes as C
import errno
import struct

import numpy as np
import pytest

import history_streams as hs
import indep_aircraft_pb as ipb
import indep_history as ih


def host(pkg, receivers, **kw):
    return pkg.capi.PositionTracker(capacity=1 << 12, receivers=receivers, host=True, table=True, **kw)


@pytest.fixture(scope="module")
def tables(pkg):
    """every table once: name -> (scenario, [(stream, rows)] of the host object, [(files, rows)] of the second reading),
    and how often the second reading met each refusal and each altitude arm"""
    counts, out = {}, {}
    for name, make in hs.TABLES.items():
        sc = make(pkg)
        t = host(pkg, sc[0])
        got = hs.run(t, sc, refuse=True)
        t.close()
        t = host(pkg, sc[0])
        want = hs.run_model(pkg, t, sc, counts)
        t.close()
        out[name] = (sc, got, want)
    return out, counts


@pytest.mark.parametrize("name", sorted(hs.TABLES))
def test_host_object_is_the_second_reading(pkg, tables, name):
    sc, got, want = tables[0][name]
    assert len(got) == len(want) == len(sc[2])
    for (stream, rx), (files, rows) in zip(got, want):
        assert hs.split(stream, rx) == files
        assert [int(n) for n in rx["aircraft"]] == rows and not rx["reserved"].any()
        for f, n in zip(files, rows):
            assert len(ih.read_file(f)["history"]) == n


def test_every_refusal_and_every_altitude_arm_occurred(tables):
    counts = tables[1]
    for k in ih.REFUSALS + tuple("alt_" + a for a in ih.ALTITUDES):
        assert counts.get(k, 0) > 0, (k, counts)


def test_selection_by_hand(pkg, tables):
    sc, got, want = tables[0]["selection"]
    now = sc[2][0][1]
    files = hs.split(*got[0])
    head = b"\x08" + ipb.varint(now // 1000)
    assert files[0] == head and files[1] == head  # three refused aircraft; nobody: `now` alone
    d = ih.read_file(files[2])
    assert d["now"] == now // 1000
    # messages 1 and 2, seen + 90001, position + 70000 are out; seen + 90000, seen after now, position + 69999 are in
    assert [h["addr"] for h in d["history"]] == [0x410004, 0x410005, 0x410006, hs.NON_ICAO | 0x410008]
    assert int(got[0][1]["aircraft"][2]) == 4
    # one entry byte for byte: tag 0x72, length, addr as a four-byte varint with the non-ICAO bit, lat, lon; no altitude
    lat, lon = d["history"][3]["lat"], d["history"][3]["lon"]
    addr = hs.NON_ICAO | 0x410008
    by_hand = (b"\x08" + bytes([addr & 0x7F | 0x80, addr >> 7 & 0x7F | 0x80, addr >> 14 & 0x7F | 0x80, addr >> 21])
               + b"\x41" + struct.pack("<d", lat) + b"\x49" + struct.pack("<d", lon))
    assert len(by_hand) == 23 and files[2].endswith(b"\x72\x17" + by_hand)
    assert abs(lat - hs.where(8)[0]) < 1e-4 and abs(lon - hs.where(8)[1]) < 1e-4


def test_altitudes_by_hand(pkg, tables):
    sc, got, want = tables[0]["altitude"]
    d = ih.read_file(hs.split(*got[0])[0])
    a = 0x420000
    alt = {h["addr"] - a: h.get("alt_baro") for h in d["history"]}
    assert alt == {1: -9999,  # on the ground, by ADS-B
                   2: 2300,   # on the ground by a source below MODE_S_CHECKED: the altitude
                   3: None,   # altitude_baro_reliable 2
                   4: 31000,  # 3
                   5: -975, 6: None,  # negative; 0 is absent
                   7: 9007,   # a geometric altitude one ms before its expiry
                   8: None,   # at its expiry
                   9: 4100,   # airground expired
                   10: None}
    # -9999 and -975 are sign-extended to ten bytes
    stream = got[0][0]
    assert b"\x28\xf1\xb1\xff\xff\xff\xff\xff\xff\xff\x01" in stream and b"\x28\xb1\xf8\xff\xff\xff\xff\xff\xff\xff\x01" in stream


def test_nothing_to_write(pkg, tables):
    sc, got, want = tables[0]["nothing"]
    assert got[0][0] == b"" and [int(e) for e in got[0][1]["end"]] == [0, 0]   # now_ms < 1000: zero bytes
    assert got[1][0] == b"\x08\x01\x08\x01" and [int(e) for e in got[1][1]["end"]] == [2, 4]
    assert not got[0][1]["aircraft"].any() and not got[1][1]["aircraft"].any()


def test_three_receivers_with_the_middle_one_empty(pkg, tables):
    sc, got, want = tables[0]["three"]
    stream, rx = got[0]
    assert [int(n) for n in rx["aircraft"]] == [3, 0, 2]
    files = hs.split(stream, rx)
    assert files[1] == b"\x08" + ipb.varint(sc[2][0][1] // 1000)
    assert int(rx["end"][1]) - int(rx["end"][0]) == len(files[1])


def entry_bytes(pkg, e, now):
    L, _ = pkg.capi._pos_lib(True)
    out = np.full(pkg.capi.HISTORY_ENTRY_MAX + 4, 0xEE, dtype=np.uint8)
    n = L.msd_pos_host_history_entry(e.ctypes.data, now, out.ctypes.data)
    assert n == L.msd_pos_host_history_entry(e.ctypes.data, now, None)  # the length alone
    assert (out[n:] == 0xEE).all()
    return out[:n].tobytes()


def test_values_no_decoder_delivers(pkg):
    """lat == 0.0 and -0.0 are absent and NaN is written, on an entry built by hand"""
    capi = pkg.capi
    now = 1_700_000_000_000
    e = np.zeros((), dtype=capi.AIRCRAFT_DTYPE)
    e["addr"], e["messages"], e["seen"] = 0x4840D6, 2, now
    e["source"][capi.AC["position"]], e["updated"][capi.AC["position"]] = 7, now
    addr = b"\x08\xd6\x81\xa1\x02"
    for lat, lon, body in ((0.0, 0.0, addr), (-0.0, 4.5, addr + b"\x49" + struct.pack("<d", 4.5)),
                           (52.25, -0.0, addr + b"\x41" + struct.pack("<d", 52.25)),
                           (float("nan"), 1.0, addr + b"\x41" + struct.pack("<d", float("nan")) + b"\x49" + struct.pack("<d", 1.0))):
        e["lat"], e["lon"] = lat, lon
        got = entry_bytes(pkg, e, now)
        assert got == b"\x72" + bytes([len(body)]) + body, (lat, lon)
        assert got == ih.entry(e, capi.AC, now)
    e["addr"] = 0  # an entry with nothing to say is a tag and a length of 0
    e["lat"] = e["lon"] = 0.0
    assert entry_bytes(pkg, e, now) == b"\x72\x00" == ih.entry(e, capi.AC, now)


def test_refusals(pkg):
    capi = pkg.capi

    def code(call):
        with pytest.raises(pkg.MsdError) as e:
            call()
        return e.value.code
    t = capi.PositionTracker(capacity=64, host=True)  # no table
    assert code(lambda: t.history_pb_stream(hs.T0)) == -errno.EINVAL
    t.close()
    sc = hs.TABLES["three"](pkg)
    t = host(pkg, sc[0])
    hs.feed(t, sc[1][0])
    now = sc[2][0][1]
    for bad in (dict(flags=1), dict(flags=1 << 31), dict(reserved=1)):
        assert code(lambda: t.history_pb_stream(now, **bad)) == -errno.EINVAL, bad
    fn = t.f["history_pb"]
    opt, need = capi.HistoryOptions(now_ms=now), C.c_size_t(7)
    out = np.full(4096, 0xEE, dtype=np.uint8)
    rx = np.zeros(3, dtype=capi.HISTORY_RECEIVER_DTYPE)
    assert fn(None, C.byref(opt), out.ctypes.data, 4096, C.byref(need), rx.ctypes.data) == -errno.EINVAL
    assert fn(t.h, None, out.ctypes.data, 4096, C.byref(need), rx.ctypes.data) == -errno.EINVAL
    assert fn(t.h, C.byref(opt), out.ctypes.data, 4096, None, rx.ctypes.data) == -errno.EINVAL
    assert fn(t.h, C.byref(opt), None, 4096, C.byref(need), rx.ctypes.data) == -errno.EINVAL
    # -ENOSPC one byte short: the size, nothing written; then the same bytes, with and without rows
    rx["end"] = 77
    assert fn(t.h, C.byref(opt), None, 0, C.byref(need), rx.ctypes.data) == -errno.ENOSPC
    size = need.value
    assert fn(t.h, C.byref(opt), out.ctypes.data, size - 1, C.byref(need), rx.ctypes.data) == -errno.ENOSPC
    assert need.value == size and (out == 0xEE).all() and (rx["end"] == 77).all()
    assert fn(t.h, C.byref(opt), out.ctypes.data, size, C.byref(need), None) == 0 and need.value == size  # rx may be NULL
    first = out[:size].tobytes()
    assert (out[size:] == 0xEE).all()
    stream, rows = t.history_pb_stream(now)
    assert stream == first and int(rows["end"][-1]) == size
    assert t.history_pb(now) == hs.split(stream, rows)
    assert t.history_pb_stream(now, rx=False) == (stream, None)
    t.close()


def test_the_call_leaves_aircraft_pb_alone(pkg):
    """aircraft.pb keeps a written state per aircraft; a history file in between moves none of it"""
    sc = hs.TABLES["expire"](pkg)
    files = {}
    for with_history in (False, True):
        t = host(pkg, sc[0], pb=True)
        out = []
        for i, s in enumerate(sc[1]):
            hs.feed(t, s)
            for after, now in sc[2]:
                if after == i:
                    if with_history:
                        t.history_pb_stream(now)
                        t.history_pb_stream(now + 30000)
                    out.append(t.aircraft_pb_stream(now + 1000))
        files[with_history] = [(s, r.tobytes()) for s, r in out]
        t.close()
    assert files[True] == files[False] and len(files[True]) == 3 and all(len(s) > 100 for s, _ in files[True])
