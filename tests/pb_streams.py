"""Constructed tables for the aircraft.pb tests (test_pb_model.py on the CPU, test_gpu_aircraft_pb.py on the GPU):
aircraft_streams.Builder records that leave the aircraft table in the states the writer's rules turn on, and runners for
the trackers and the second reading of tests/indep_aircraft_pb.py.

A scenario is (receivers, steps, writes): steps as in aircraft_streams, writes a list of (after step, now_ms,
messages_total or None) -- the file is written after that step (several writes may follow one step)."""
import errno

import numpy as np

import aircraft_streams as acs
import indep_aircraft as ia
import indep_aircraft_pb as ipb
import indep_positions as ip

T0 = acs.T0
TILE = 128  # the store kernel's items per LDS image (MSD_PB_TILE, msd_pos.h)
S4 = ip.MODE_S_CHECKED


def two(b, t, addr, rx=0, signal=0.0, **kw):
    """an aircraft that is written: two messages, the second with the members given"""
    b.rec(t, addr, rx=rx, source=ip.MODE_S, msgtype=11, signal=signal)
    return b.rec(t + 1, addr, rx=rx, signal=signal, **kw)


def counts_table(pkg, counts):
    """counts[r] aircraft on receiver r, two DF11 squitters each with a signal level that differs by aircraft"""
    b = acs.Builder(pkg)
    k = 0
    for r, c in enumerate(counts):
        for j in range(c):
            two(b, T0 + k, 0x400000 + 7 * k, rx=r, signal=0.001 * (1 + k % 500))
            k += 1
    return [None] * len(counts), [b.step()], [(0, T0 + 5000, np.arange(len(counts), dtype=np.uint64) * 1000)]


def filter_table(pkg):
    """receiver 0: one aircraft heard once, one seen 90001 ms before the write: all filtered.  receiver 1: one seen
    exactly 90000 ms before, which stays, and one seen after the write, which stays too"""
    b = acs.Builder(pkg)
    now = T0 + 100000
    b.rec(now - 10, 0x410001, rx=0, source=ip.MODE_S, msgtype=11)
    two(b, now - 90002, 0x410002, rx=0)
    two(b, now - 90001, 0x410003, rx=1)
    two(b, now + 50, 0x410004, rx=1)
    return [None, None], [b.step()], [(0, now, None)]


def sizes_table(pkg):
    """bodies around the one- and two-byte length prefix: a ladder of members by aircraft, callsigns of 0 to 8 bytes"""
    b = acs.Builder(pkg)
    k = 0
    for ladder in range(20):
        # the second ten: no category, every body three bytes shorter, so that both 127 and 128 bytes are met
        plain, extras = ladder >= 10, ladder % 10
        for n in range(9):
            a = 0x420000 + k
            kw = dict(callsign_valid=1, callsign=(b"ABCDEFGH"[:n] + bytes(8 - n)), squawk_valid=1, squawk=0x1200 + extras,
                      altitude_baro_valid=1, altitude_baro=-1000 if extras % 2 else 35000, category_valid=1,
                      category=0 if plain else 0xA3, airground=ia.AG_AIRBORNE, emergency_valid=1, emergency=extras % 8,
                      alert_valid=1, alert=extras > 4, spi_valid=1, spi=extras > 6)
            if extras > 1:
                kw.update(baro_rate_valid=1, baro_rate=-64 * extras)
            if extras > 2:
                kw.update(geom_rate_valid=1, geom_rate=64 * extras)
            if extras > 3:
                kw.update(nac_v_valid=1, nac_v=2)
            two(b, T0 + k, a, signal=0.01 + 0.001 * k, **kw)
            if extras > 5:
                b.rec(T0 + k + 2, a, source=S4, msgtype=20, commb_format=7, nav_valid=1 | 4 | 8 | 16 | 64,
                      nav_mcp_altitude=36000, nav_fms_altitude=-500 if extras > 7 else 37000, nav_qnh_raw=2132,
                      nav_modes=extras, nav_altitude_source=2)
            k += 1
    return [None], [b.step()], [(0, T0 + 3000, None)]


def kinds_table(pkg):
    """every heading kind in every heading member, the two QNH and the two selected-heading forms, Comm-B roll, track rate
    and Mach with both signs, a negative altitude, lat / lon from a decoded pair, a signal level never written"""
    b = acs.Builder(pkg)
    a = 0x430000
    two(b, T0, a + 1, signal=0.0)                                                       # signal_level: 8 x 1e-5
    two(b, T0, a + 2, signal=0.25, velocity_valid=1, ew_vel=-100, ns_vel=100, metype=19)  # HDG_VELOCITY in track: 315
    two(b, T0, a + 3, signal=0.02, velocity_valid=1, ew_vel=4088, ns_vel=-4, metype=19, mesub=2)
    two(b, T0, a + 4, signal=0.03, velocity_valid=1, ew_vel=1023, ns_vel=2, metype=19)   # a pair no message carries: 0
    two(b, T0, a + 5, signal=0.04, metype=19, heading_valid=1, heading_type=ia.MAGNETIC_OR_TRUE, heading_raw=1000)
    b.ops(T0 + 5, a + 6, 2, hrd=ia.TRUE, tah=ia.MAGNETIC, signal=0.05)
    b.rec(T0 + 6, a + 6, metype=19, heading_valid=1, heading_type=ia.MAGNETIC_OR_TRUE, heading_raw=513, signal=0.05)
    b.rec(T0 + 7, a + 6, metype=7, heading_valid=1, heading_type=ia.TRACK_OR_HEADING, heading_raw=127, signal=0.05)
    two(b, T0, a + 7, signal=0.06, metype=7, heading_valid=1, heading_type=ia.TRACK_OR_HEADING, heading_raw=33)
    for j, (raw, roll, rate) in enumerate(((2047, -200, -100), (1025, 199, 99), (1, -1, 1))):
        two(b, T0, a + 8 + j, signal=0.07 + 0.01 * j, source=S4, msgtype=21, commb_format=8, commb_valid=1 | 4, roll_q=roll,
            track_rate_q=rate, heading_valid=1, heading_type=ia.GROUND_TRACK, heading_raw=raw)
    two(b, T0, a + 11, signal=0.11, source=S4, msgtype=21, commb_format=9, commb_valid=8, mach_raw=190, heading_valid=1,
        heading_type=ia.MAGNETIC, heading_raw=1500)
    two(b, T0, a + 12, signal=0.12, source=S4, msgtype=20, commb_format=7, nav_valid=4 | 16 | 64, nav_mcp_altitude=-1000,
        nav_qnh_raw=2132)                                                                # QNH, Comm-B form
    two(b, T0, a + 13, signal=0.13, metype=29, mesub=1, nav_valid=2 | 32 | 16, nav_heading_raw=511, nav_qnh_raw=267)
    two(b, T0, a + 14, signal=0.14, metype=29, mesub=0, nav_valid=2, nav_heading_raw=359)  # selected heading in degrees
    two(b, T0, a + 15, signal=0.15, altitude_baro_valid=1, altitude_baro=-975, geom_rate_valid=1, geom_rate=-2048)
    b.half(T0 + 20, a + 16, 50.0, 8.0, 0, 11, signal=0.16).half(T0 + 400, a + 16, 50.0, 8.0, 1, 11, signal=0.16)
    b.half(T0 + 20, a + 17, 50.0, 8.0, 0, 11, signal=0.17, source=ip.TISB, addrtype=3)
    b.half(T0 + 400, a + 17, 50.0, 8.0, 1, 11, signal=0.17, source=ip.TISB, addrtype=3)
    b.rec(T0 + 30, a + 18, signal=0.18, metype=19, ias_valid=1, ias=280).rec(T0 + 31, a + 18, metype=19, tas_valid=1, tas=420)
    return [None], [b.step()], [(0, T0 + 2000, [123456789])]


def sticky_table(pkg):
    """three writes.  A: callsign, nav_modes and position valid at write 1, expired at write 2: still written, seen_pos
    keeps its last value.  B: callsign, nav_modes and position stored, but never valid at a write: not written.  C:
    callsign valid first at write 2.  D: nav_modes attached with no mode set: an empty sub-message.  Between the first
    two writes an expiry removes an aircraft heard once, so the table is rebuilt and every state moves with its slot"""
    b = acs.Builder(pkg)
    a = 0x440000
    nav = dict(source=S4, msgtype=20, commb_format=7, nav_valid=1)
    two(b, T0, a + 1, signal=0.02, callsign_valid=1, callsign=b"STICKY  ")
    b.rec(T0 + 2, a + 1, nav_modes=5, **nav)
    b.half(T0 + 20, a + 1, 50.0, 8.0, 0, 11).half(T0 + 400, a + 1, 50.0, 8.0, 1, 11)
    two(b, T0, a + 4, signal=0.05, nav_modes=0, **nav)
    b.rec(T0, a + 5, source=ip.MODE_S, msgtype=11)  # heard once: the expiry removes it and the table is rebuilt
    first = b.step()
    # B is first heard 80 s before the second write: every member has expired then, the aircraft has not
    two(b, T0 + 10000, a + 2, signal=0.03, callsign_valid=1, callsign=b"NEVER   ")
    b.rec(T0 + 10002, a + 2, nav_modes=63, **nav)
    b.half(T0 + 10020, a + 2, 51.0, 9.0, 0, 11).half(T0 + 10400, a + 2, 51.0, 9.0, 1, 11)
    b.rec(T0 + 89000, a + 1, source=ip.MODE_S, msgtype=11, signal=0.02)
    b.rec(T0 + 89000, a + 2, source=ip.MODE_S, msgtype=11, signal=0.03)
    b.rec(T0 + 89000, a + 4, source=ip.MODE_S, msgtype=11, signal=0.05)
    two(b, T0 + 89000, a + 3, signal=0.04, callsign_valid=1, callsign=b"LATE")
    second = b.step()
    b.rec(T0 + 170000, a + 1, source=ip.MODE_S, msgtype=11, signal=0.02)
    b.rec(T0 + 170000, a + 2, source=ip.MODE_S, msgtype=11, signal=0.03)
    third = b.step()
    return ([None], [first, ("expire", T0 + 61000), second, third],
            [(0, T0 + 5999, None), (2, T0 + 90000, None), (3, T0 + 171000, None)])


TABLES = dict(counts=lambda pkg: counts_table(pkg, [1, 0, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 0]),
              three=lambda pkg: counts_table(pkg, [3, 0, 2]), empty=lambda pkg: counts_table(pkg, [0, 0]),
              filter=filter_table, sizes=sizes_table, kinds=kinds_table, sticky=sticky_table)


def run(tracker, scenario, pieces=None, refuse=False):
    """the scenario through a capi.PositionTracker with pb -> [(stream, rx rows, margin or None) per write].  refuse: every
    write is first offered one byte less than it needs"""
    receivers, steps, writes = scenario
    out = []
    for i, s in enumerate(steps):
        if s[0] == "expire":
            tracker.expire(s[1])
        else:
            _, m, f, r = s
            k = pieces or max(len(m), 1)
            for j in range(0, len(m), k):
                tracker.update_nicrc(m[j:j + k], f[j:j + k], r[j:j + k])
        for after, now, total in writes:
            if after != i:
                continue
            if refuse:  # the size, a buffer one byte short, then the write itself
                try:
                    tracker.aircraft_pb_stream(now, total, cap=0)
                    need = 0
                except Exception as e:
                    assert getattr(e, "code", None) == -errno.ENOSPC, e
                    need = tracker.pb_needed
                if need > 1:
                    try:
                        tracker.aircraft_pb_stream(now, total, cap=need - 1)
                        raise AssertionError("a buffer one byte short was accepted")
                    except Exception as e:
                        assert getattr(e, "code", None) == -errno.ENOSPC and tracker.pb_needed == need, e
                stream, rx = tracker.aircraft_pb_stream(now, total, cap=need)
            else:
                stream, rx = tracker.aircraft_pb_stream(now, total)
            out.append((stream, rx, tracker.pb_margin if tracker.host else None))
    return out


def split(stream, rx):
    ends = [0] + [int(e) for e in rx["end"]]
    assert ends == sorted(ends) and ends[-1] == len(stream)
    return [stream[a:b] for a, b in zip(ends[:-1], ends[1:])]


def run_model(pkg, tracker_factory, scenario):
    """the second reading over the snapshots of a tracker fed the same steps -> [(files, rows, margin) per write]"""
    receivers, steps, writes = scenario
    t = tracker_factory(receivers)
    w = ipb.Writer(pkg.capi.AC, len(receivers))
    out = []
    for i, s in enumerate(steps):
        if s[0] == "expire":
            t.expire(s[1])
        else:
            t.update_nicrc(s[1], s[2], s[3])
        for after, now, total in writes:
            if after == i:
                out.append(w.files(t.snapshot(), now, total))
    t.close()
    return out
