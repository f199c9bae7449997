"""Constructed records and streams for the tests of the SBS output (test_sbs_model.py on the CPU, test_gpu_sbs.py on the
GPU): one small scenario per rule of modesSendSBSOutput (net_io.c:1038-1241) and of the delivery conditions around it
(net_io.c:1266-1270, mode_s.c:2164-2172), each with the lines it must write, written out by hand, and runners for the
three implementations (the GPU object, the host twin, the second reading of tests/indep_sbs.py).

A scenario is a dict:
  receivers, capacity,
  steps -- ("update", msgs, fields, receiver) or ("expire", now_ms): the records go through the tracker, which makes the
           rows; or
  rows  -- with a single update step: rows written by hand (SBS_TRACK_DTYPE), for what only the writer can show;
  cases -- [(options of sbs_wire, [the line of every record in order, b"" for one that writes nothing])].
T is T0 = 2020-09-13 12:26:40.000 UTC; D0 is that time as fields 7-8 (and 9-10) print it."""
import numpy as np

import indep_sbs as isbs
import reduce_streams as rs

T0 = rs.T0
D0 = "2020/09/13,12:26:40.000"
E12 = ",,,,,,,,,,,,"  # fields 11 to 22, all empty
RECEIVED = dict(now_is_received=True)
TS = isbs.TRACKED | isbs.SEEN_TWICE


def stamp(ms_after_t0):
    """fields 7-8 of a record received ms_after_t0 (below 20 s) after T0"""
    return "2020/09/13,12:26:%02d.%03d" % (40 + ms_after_t0 // 1000, ms_after_t0 % 1000)


def tail(**f):
    """fields 11 to 22 from the ones that are not empty: tail(f12="10000")"""
    assert all(k[0] == "f" and 11 <= int(k[1:]) <= 22 for k in f)
    return "".join("," + f.get("f%d" % k, "") for k in range(11, 23))


def line(kind, addr, when, tail, now=None):
    return ("MSG,%d,1,1,%06X,1,%s,%s%s\r\n" % (kind, addr, when, now or when, tail)).encode()


NAMES = ["types", "non_icao", "delivery", "altitude", "vertical_rate", "gs_by_version", "commb_track", "velocity_track",
         "positions", "callsign_squawk_flags", "times", "decoded_position"]


def scenarios(pkg):
    out = {}
    B = lambda: rs.Builder(pkg)  # noqa: E731
    T = T0

    def add(name, steps, cases, rows=None, receivers=None, capacity=1024):
        out[name] = dict(receivers=receivers or [None], capacity=capacity, steps=steps, cases=cases, rows=rows)

    def hand_rows(n, **kw):
        rows = np.zeros(n, dtype=pkg.capi.SBS_TRACK_DTYPE)
        rows["flags"] = TS
        for k, v in kw.items():
            rows[k] = v
        return rows

    # the eight SBS types, and every DF / ME type that writes nothing; --net-only, so that first messages count
    b, want = B(), []
    for df, kind in ((4, 5), (20, 5), (5, 6), (21, 6), (0, 7), (16, 7), (11, 8), (24, None), (19, None), (1, None)):
        b.rec(T, 0x4840D6, source=rs.S4, msgtype=df)
        want.append(line(kind, 0x4840D6, D0, E12) if kind else b"")
    for df in (17, 18):
        for me, kind in ((0, None), (1, 1), (4, 1), (5, 2), (8, 2), (9, 3), (18, 3), (19, 4), (20, None), (22, None), (23, None),
                         (28, None), (29, None), (31, None)):
            b.rec(T, 0x4840D6, msgtype=df, metype=me)
            want.append(line(kind, 0x4840D6, D0, E12) if kind else b"")
    add("types", [b.step()], [(dict(net_only=True, **RECEIVED), want)])

    # a non-ICAO address writes nothing, whatever the flags
    b = B().rec(T, 0x1ABCDEF, metype=4).rec(T + 1, 0x1ABCDEF, metype=4).rec(T + 2, 0xABCDEF, metype=4).rec(T + 3, 0xABCDEF, metype=4)
    add("non_icao", [b.step()], [(dict(verbatim=True, net_only=True, **RECEIVED), [b"", b"", line(1, 0xABCDEF, stamp(2), E12),
                                                                                 line(1, 0xABCDEF, stamp(3), E12)]),
                                 (RECEIVED, [b"", b"", b"", line(1, 0xABCDEF, stamp(3), E12)])])

    # correctedbits 0 / 1 / 2 and an aircraft's first message under every flag combination: two repaired bits never go
    # out, not with --net-verbatim either (net_io.c:1266); a first message needs --net-only or --net-verbatim
    b, lines = B(), []
    for k, addr in enumerate((0x100000, 0x100001, 0x100002)):
        for dt in (0, 1):
            b.rec(T + dt, addr, metype=4, msg=dict(correctedbits=k))
            lines.append(line(1, addr, stamp(dt), E12))
    second = [b"", lines[1], b"", lines[3], b"", b""]
    both = lines[:4] + [b"", b""]
    add("delivery", [b.step()], [(RECEIVED, second), (dict(net_only=True, **RECEIVED), both),
                                 (dict(verbatim=True, **RECEIVED), both), (dict(verbatim=True, net_only=True, **RECEIVED), both)])

    # the altitude's four cases under both --gnss settings, with the aircraft's geometric delta (250 ft at T) valid, stale
    # but valid (69.999 s old: stale after 60, valid until 70) and expired at the record's time (70 s: now < expires fails)
    A = 0x200001
    b = B().rec(T, A, metype=19, geom_delta_valid=1, geom_delta=250)
    kinds = (dict(altitude_baro_valid=1, altitude_baro=10000), dict(altitude_geom_valid=1, altitude_geom=9000),
             dict(altitude_baro_valid=1, altitude_baro=10000, altitude_geom_valid=1, altitude_geom=9000), dict())
    for k in kinds:
        b.rec(T + 1000, A, metype=19, **k)
    first = b.step()
    for dt in (69999, 70000):
        for k in kinds[:2]:
            b.rec(T + dt, A, metype=19, **k)
    old, gone = "2020/09/13,12:27:49.999", "2020/09/13,12:27:50.000"

    def alt(when, a):
        return line(4, A, when, tail(f12=a))
    add("altitude", [first, b.step()],
        [(RECEIVED, [b"", alt(stamp(1000), "10000"), alt(stamp(1000), "8750"), alt(stamp(1000), "10000"), alt(stamp(1000), ""),
                     alt(old, "10000"), alt(old, "8750"), alt(gone, "10000"), alt(gone, "")]),
         (dict(gnss=True, **RECEIVED), [b"", alt(stamp(1000), "10250H"), alt(stamp(1000), "9000H"), alt(stamp(1000), "9000H"),
                                        alt(stamp(1000), ""), alt(old, "10250H"), alt(old, "9000H"), alt(gone, "10000"),
                                        alt(gone, "9000H")])])

    # the vertical rate: barometric first, or geometric first and marked H with --gnss
    b, A = B(), 0x210001
    for k in (dict(baro_rate_valid=1, baro_rate=-640), dict(geom_rate_valid=1, geom_rate=1280),
              dict(baro_rate_valid=1, baro_rate=-640, geom_rate_valid=1, geom_rate=1280), dict()):
        b.rec(T, A, metype=19, **k)

    def vr(v):
        return line(4, A, D0, tail(f17=v))
    add("vertical_rate", [b.step()], [(dict(net_only=True, **RECEIVED), [vr("-640"), vr("1280"), vr("-640"), vr("")]),
                                      (dict(net_only=True, gnss=True, **RECEIVED), [vr("-640"), vr("1280H"), vr("1280H"), vr("")])])

    # the ground speed of a surface movement is the table of the aircraft's ADS-B version: code 5 is 0.5625 kt in
    # version 0 (-> 1) and 0.125 + 2.5 * 0.875 / 6 = 0.4896 kt in version 2 (-> 0); the halves go to the even neighbour:
    # codes 39 and 40 are 15.5 and 16.5 kt, both 16.  A surface heading is HEADING_TRACK_OR_HEADING: field 14 stays empty
    b = B()
    b.pos(T, 0x220001, 52.0, 4.0, 0, surface=True, movement=5).opstatus(T, 0x220002, 2)
    b.pos(T + 1, 0x220002, 52.0, 4.0, 0, surface=True, movement=5)
    b.pos(T + 2, 0x220001, 52.0, 4.0, 0, surface=True, movement=39, heading_valid=1, heading_type=5, heading_raw=64)
    b.pos(T + 3, 0x220001, 52.0, 4.0, 0, surface=True, movement=40)

    def gs(addr, dt, v):
        return line(2, addr, stamp(dt), tail(f13=v))
    add("gs_by_version", [b.step()], [(dict(net_only=True, **RECEIVED), [gs(0x220001, 0, "1"), b"", gs(0x220002, 1, "0"),
                                                                        gs(0x220001, 2, "16"), gs(0x220001, 3, "16")])])

    # BDS 5,0: the track is raw * 90 / 512 (+ 180 with bit 10), a ground track: 128 is 22.5 (-> 22), 384 is 67.5 (-> 68),
    # 1024 + 1023 is 359.82 (-> 360); its ground speed is the integer sent.  BDS 6,0's heading is magnetic: nothing
    b, A = B(), 0x230001
    for raw in (128, 384, 2047):
        b.rec(T, A, source=rs.S4, msgtype=20, commb_format=8, heading_valid=1, heading_type=1, heading_raw=raw, commb_valid=2, gs=450)
    b.rec(T, A, source=rs.S4, msgtype=21, commb_format=9, heading_valid=1, heading_type=3, heading_raw=384)

    def trk(kind, g, t):
        return line(kind, A, D0, tail(f13=g, f14=t))
    add("commb_track", [b.step()], [(dict(net_only=True, **RECEIVED), [trk(5, "450", "22"), trk(5, "450", "68"), trk(5, "450", "360"),
                                                                      trk(6, "", "")])])

    # the velocity's ground track atan2(ew, ns) in each quadrant and on each axis, with sqrtf(ns^2 + ew^2 + 0.5) beside it;
    # (-1, 1000) is 359.94 (-> 360); (0, 0) has a speed of sqrtf(0.5) (-> 1) and a track of 0.  The type 19 heading of
    # subtypes 3 / 4 is HEADING_MAGNETIC_OR_TRUE: nothing
    b, A, want = B(), 0x240001, []
    for ew, ns, g, t in ((100, 100, "141", "45"), (100, -100, "141", "135"), (-100, -100, "141", "225"), (-100, 100, "141", "315"),
                         (0, 100, "100", "0"), (100, 0, "100", "90"), (0, -100, "100", "180"), (-100, 0, "100", "270"),
                         (-1, 1000, "1000", "360"), (0, 0, "1", "0"), (4088, -4088, "5781", "135")):
        b.vel(T, A, ew, ns, mesub=2 if ew == 4088 else 1)
        want.append(line(4, A, D0, tail(f13=g, f14=t)))
    b.rec(T, A, metype=19, mesub=3, heading_valid=1, heading_type=4, heading_raw=512, ias_valid=1, ias=250)
    want.append(line(4, A, D0, E12))
    add("velocity_track", [b.step()], [(dict(net_only=True, **RECEIVED), want)])

    # latitude and longitude as %1.5f: a negative value that rounds to zero keeps its sign, the exact ties 1/64 and 3/64
    # go to the even neighbour, the poles and the date line.  Rows by hand: no CPR pair decodes to these
    b, A = B(), 0x250001
    coords = ((-0.000001, 0.000004, "-0.00000", "0.00000"), (0.015625, 0.046875, "0.01562", "0.04688"),
              (-0.015625, -0.046875, "-0.01562", "-0.04688"), (90.0, -180.0, "90.00000", "-180.00000"),
              (-90.0, 179.99999, "-90.00000", "179.99999"), (52.2572, 3.919371, "52.25720", "3.91937"))
    for _ in coords:
        b.rec(T, A, metype=11)
    rows = hand_rows(len(coords), flags=TS | isbs.CPR_DECODED)
    rows["lat"], rows["lon"] = [c[0] for c in coords], [c[1] for c in coords]
    want = [line(3, A, D0, tail(f15=c[2], f16=c[3])) for c in coords]
    add("positions", [b.step()], [(RECEIVED, want)], rows=rows)

    # the callsign's eight characters as they are; squawk %04x with the emergency flag of 7500 / 7600 / 7700; alert, SPI
    # and the ground flag absent, 0 and -1; AG_UNCERTAIN (3) writes nothing
    b, A = B(), 0x260001
    b.rec(T, A, metype=4, callsign_valid=1, callsign=b"KL M 23 ")
    b.rec(T, A, source=rs.S4, msgtype=5, squawk_valid=1, squawk=0x0000, alert_valid=1, alert=0, spi_valid=1, spi=0, airground=2)
    b.rec(T, A, source=rs.S4, msgtype=5, squawk_valid=1, squawk=0x7700, alert_valid=1, alert=1, spi_valid=1, spi=1, airground=1)
    b.rec(T, A, source=rs.S4, msgtype=5, squawk_valid=1, squawk=0x7500, airground=3)
    b.rec(T, A, source=rs.S4, msgtype=21, squawk_valid=1, squawk=0x7600, spi_valid=1, spi=1)
    b.rec(T, A, source=rs.S4, msgtype=4, alert_valid=1, alert=1, airground=1)
    add("callsign_squawk_flags", [b.step()], [(dict(net_only=True, **RECEIVED), [
        line(1, A, D0, tail(f11="KL M 23 ")), line(6, A, D0, tail(f18="0000", f19="0", f20="0", f21="0", f22="0")),
        line(6, A, D0, tail(f18="7700", f19="-1", f20="-1", f21="-1", f22="-1")), line(6, A, D0, tail(f18="7500", f20="-1")),
        line(6, A, D0, tail(f18="7600", f20="-1", f21="-1")), line(5, A, D0, tail(f19="-1", f22="-1"))])])

    # times: a day, a month, the leap day and a year boundary crossed by the offset in either direction; a record time
    # beyond year 9999 prints the year modulo 10000, a sum below zero prints as zero.  Fields 9-10 are now_ms, shifted too
    A = 0x270001
    when = (1600041599999, 1601510399999, 1583022600000, 1609459200000, 253402300800000, 1000)
    b = B()
    for t in when:
        b.rec(t, A, metype=4)
    rows = hand_rows(len(when))
    plus = ["2020/09/14,00:00:00.000", "2020/10/01,00:00:00.000", "2020/03/01,00:30:00.001", "2021/01/01,00:00:00.001",
            "0000/01/01,00:00:00.001", "1970/01/01,00:00:01.001"]
    minus = ["2020/09/13,22:59:59.999", "2020/09/30,22:59:59.999", "2020/02/29,23:30:00.000", "2020/12/31,23:00:00.000",
             "9999/12/31,23:00:00.000", "1970/01/01,00:00:00.000"]
    add("times", [b.step()], [(dict(now_ms=T, utc_offset_ms=1), [line(1, A, p, E12, now="2020/09/13,12:26:40.001") for p in plus]),
                              (dict(now_ms=T, utc_offset_ms=-3600000), [line(1, A, p, E12, now="2020/09/13,11:26:40.000") for p in minus])],
        rows=rows)

    # the tracker's own position: an even and an odd half of (52.0, 4.0) 500 ms apart decode globally; the CPR grid
    # (latitudes 360 / 60 / 2^17 = 4.6e-5 degrees apart, longitudes 360 / 36 / 2^17 = 7.6e-5 in that zone) puts the latitude
    # at 52.00001 and the longitude at 3.99997; the first half alone
    # writes no position, and the line of the first message is held back
    b, A = B(), 0x280001
    b.pos(T, A, 52.0, 4.0, 0).pos(T + 500, A, 52.0, 4.0, 1)
    add("decoded_position", [b.step()], [(RECEIVED, [b"", line(3, A, stamp(500), tail(f15="52.00001", f16="3.99997"))])])
    assert sorted(out) == sorted(NAMES)
    return out


def records(steps):
    return rs.records(steps)


# ---- runners -------------------------------------------------------------------------------------------------------
def run_library(tracker, steps, pieces=None):
    """steps through a capi.PositionTracker with sbs=True -> (POSITION_DTYPE rows, NICRC_DTYPE rows, SBS_TRACK_DTYPE rows).
    pieces: cut every update into calls of that many records"""
    rows, nic, trk = [], [], []
    for s in steps:
        if s[0] == "expire":
            tracker.expire(s[1])
            continue
        _, m, f, r = s
        k = pieces or max(len(m), 1)
        for i in range(0, len(m), k):
            o, q, _, t = tracker.update_sbs(m[i:i + k], f[i:i + k], r[i:i + k])
            rows.append(o), nic.append(q), trk.append(t)
    return np.concatenate(rows), np.concatenate(nic), np.concatenate(trk)


def run_model(receivers, steps, capacity=None):
    """-> (rows, nicrc, sbs rows) from the second reading"""
    t = isbs.Tracker(receivers, 8, capacity)
    rows, nic, sbs = [], [], []
    for s in steps:
        if s[0] == "expire":
            t.expire(s[1])
        else:
            o, q, w = t.update_sbs(s[1], s[2], s[3])
            rows += o
            nic += q
            sbs += w
    return rows, nic, sbs


def same_rows(trk, model_rows):
    """a SBS_TRACK_DTYPE array against the second reading's rows, exactly"""
    got = isbs.rows_of(trk)
    assert len(got) == len(model_rows)
    for i, (g, w) in enumerate(zip(got, model_rows)):
        assert g[0] == w[0] and g[2] == w[2], (i, g, w)
        assert np.float32(g[1]).tobytes() == np.float32(w[1]).tobytes(), (i, g, w)
        assert np.float64(g[3]).tobytes() == np.float64(w[3]).tobytes() and np.float64(g[4]).tobytes() == np.float64(w[4]).tobytes(), (i, g, w)
    assert not trk["pad"].any()


def split(stream, ends):
    """a stream and its ends -> the line of every record"""
    at, out = 0, []
    for e in ends:
        out.append(stream[at:int(e)])
        at = int(e)
    assert at == len(stream)
    return out
