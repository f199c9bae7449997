"""Constructed tables for the VRS tests (test_vrs_model.py on the CPU, test_gpu_vrs.py on the GPU): aircraft_streams.Builder
records that leave the aircraft table in the states the writer's rules turn on, and runners for the trackers and the
second reading of tests/indep_vrs.py.

A scenario is (receivers, steps, writes): steps as in aircraft_streams, writes a list of (after step, now_ms, part,
n_parts) -- the documents are written after that step (several writes may follow one step)."""
import errno

import aircraft_streams as acs
import indep_aircraft as ia
import indep_positions as ip
import indep_vrs as iv

T0 = acs.T0
TILE = 128  # the store kernel's items per LDS image (MSD_VRS_TILE, msd_pos.h)
S4 = ip.MODE_S_CHECKED
NON_ICAO = iv.NON_ICAO


def two(b, t, addr, rx=0, signal=0.0, **kw):
    """an aircraft that is written: two messages, the second with the members given"""
    b.rec(t, addr, rx=rx, source=ip.MODE_S, msgtype=11, signal=signal)
    return b.rec(t + 1, addr, rx=rx, signal=signal, **kw)


def counts_table(pkg, counts):
    """counts[r] selected aircraft on receiver r, two DF11 squitters each with a signal level that differs by aircraft"""
    b = acs.Builder(pkg)
    k = 0
    for r, c in enumerate(counts):
        for j in range(c):
            two(b, T0 + k, 0x400000 + 7 * k, rx=r, signal=0.001 * (1 + k % 500))
            k += 1
    return [None] * len(counts), [b.step()], [(0, T0 + 5000, 0, 1)]


PART, N_PARTS = 3, 8  # the comma table's write: buckets 768 .. 1023


def comma_table(pkg):
    """the first selected aircraft of a document carries no comma, whatever stands in the table before it.  Written as part
    3 of 8 at `now`.  Addresses are base + 2048 k + low: k orders them, low says whether they are in the part.
    receiver 0: one unselected aircraft in front (messages = 1);  1: two (stale, out of part);  2: TILE of them, the four
    causes that can stand in front in turn -- heard once, stale, out of part, seen after now --, then three selected;
    3: the only selected aircraft is the table's last;  4, 5: unselected padding so that the first selected aircraft is the
    first item of a store tile, then the last item of one;  6: nothing selected at all;  7: selected, unselected, selected.
    A non-ICAO address has bit 24 set and so sorts behind every ICAO address of its receiver: it can follow the selected
    aircraft but not precede them; receivers 0 and 3 end in one."""
    b = acs.Builder(pkg)
    now = T0 + 100000
    state = dict(k=0, item=0)

    def addr(inside):
        state["k"] += 1
        return 0x4A0000 + 2048 * state["k"] + (800 if inside else 100)

    def sel(rx):
        two(b, now - 1000, addr(True), rx=rx, signal=0.01, squawk_valid=1, squawk=0x1200 + rx)
        state["item"] += 1

    def unsel(rx, cause):
        if cause == "once":
            b.rec(now - 10, addr(True), rx=rx, source=ip.MODE_S, msgtype=11)
        elif cause == "stale":
            two(b, now - 5002, addr(True), rx=rx)
        elif cause == "part":
            two(b, now - 1000, addr(False), rx=rx)
        elif cause == "future":
            two(b, now, addr(True), rx=rx)  # seen = now + 1
        else:
            two(b, now - 1000, addr(True) | NON_ICAO, rx=rx)
        state["item"] += 1

    causes = ("once", "stale", "part", "future")
    seams = {}
    for rx in range(8):
        state["item"] += 1  # the head
        if rx == 0:
            unsel(0, "once"), sel(0), sel(0), unsel(0, "non_icao")
        elif rx == 1:
            unsel(1, "stale"), unsel(1, "part"), sel(1), sel(1)
        elif rx == 2:
            for j in range(TILE):
                unsel(2, causes[j % 4])
            sel(2), sel(2), sel(2)
        elif rx == 3:
            unsel(3, "part"), unsel(3, "once"), unsel(3, "future"), sel(3), unsel(3, "non_icao")
        elif rx in (4, 5):
            want = 0 if rx == 4 else TILE - 1  # the first selected aircraft's item index modulo TILE
            while state["item"] % TILE != want:
                unsel(rx, causes[state["item"] % 4])
            seams[rx] = state["item"]
            sel(rx), sel(rx)
        elif rx == 6:
            unsel(6, "stale"), unsel(6, "part")
        else:
            sel(7), unsel(7, "part"), sel(7)
        state["item"] += 1  # the tail
    assert seams[4] % TILE == 0 and seams[5] % TILE == TILE - 1
    return [None] * 8, [b.step()], [(0, now, PART, N_PARTS)]


COMMA_COUNTS = [2, 2, 3, 1, 2, 2, 0, 2]
PART_LOWS = (0, 255, 256, 2047, 2048 + 255)


def parts_table(pkg):
    """addresses whose low eleven bits are 0, 255, 256, 2047 and 255 again one bucket round later, on two receivers, with
    one non-ICAO address per receiver; written whole, in eight parts and in 2048 (test_gpu_vrs.py runs over the parts)"""
    b = acs.Builder(pkg)
    for rx in range(2):
        for j, low in enumerate(PART_LOWS):
            two(b, T0 + j, 0x4B0000 + 0x1000 * rx + low, rx=rx, signal=0.02)
        two(b, T0, (0x4B0000 + 255) | NON_ICAO, rx=rx)
    return [None, None], [b.step()], []


def stale_table(pkg):
    """seen exactly 5000 ms before the write is written; 5001 ms before is not; one millisecond after is not either --
    the unsigned difference wraps -- though aircraft.pb writes that one"""
    b = acs.Builder(pkg)
    now = T0 + 50000
    two(b, now - 5001, 0x4C0001)   # seen = now - 5000
    two(b, now - 5002, 0x4C0002)   # seen = now - 5001
    two(b, now, 0x4C0003)          # seen = now + 1
    two(b, now - 1, 0x4C0004)      # seen = now
    return [None], [b.step()], [(0, now, 0, 1)]


def kinds_table(pkg):
    """one aircraft per branch of generateVRS; test_vrs_model.py names what each must print"""
    b = acs.Builder(pkg)
    a = 0x4D0000
    two(b, T0 - 80000, a + 4, geom_delta_valid=1, geom_delta=125)
    early = b.step()
    alt = dict(altitude_baro_valid=1, altitude_baro=-975)
    # 1: Alt with altitude_baro_reliable 2 (two accepted altitudes: not written);  2: 3 (written, negative)
    b.alt(T0, a + 1, 31000).alt(T0 + 1, a + 1, 31000)
    for k in range(3):
        b.alt(T0 + k, a + 2, -975)
    # 3: GAlt from a geometric altitude of its own
    two(b, T0, a + 3, signal=0.03, altitude_geom_valid=1, altitude_geom=-1200)
    # 4: GAlt valid only through the barometric altitude's validity, copied whole: the geometric delta was heard 80 s ago
    # and has expired (its source cleared by the expiry between the steps), the altitude itself was never sent
    for k in range(3):
        b.alt(T0 + k, a + 4, 12000)
    # 5, 6, 7: TAlt from mcp, from fms, none; 5 with the QNH in its Comm-B form, 7 in the ES form
    two(b, T0, a + 5, source=S4, msgtype=20, commb_format=7, nav_valid=4 | 8 | 16 | 64, nav_mcp_altitude=36000,
        nav_fms_altitude=37000, nav_qnh_raw=2132)
    two(b, T0, a + 6, source=S4, msgtype=20, commb_format=7, nav_valid=8, nav_fms_altitude=-500)
    two(b, T0, a + 7, metype=29, mesub=1, nav_valid=2 | 32 | 16, nav_heading_raw=511, nav_qnh_raw=267)
    # 8-11: Spd from gs (and Trak from the velocity: the table path), ias, tas, none
    two(b, T0, a + 8, signal=0.25, velocity_valid=1, ew_vel=-100, ns_vel=100, metype=19)
    two(b, T0, a + 9, metype=19, ias_valid=1, ias=280, tas_valid=1, tas=420)
    two(b, T0, a + 10, metype=19, tas_valid=1, tas=421)
    two(b, T0, a + 11)
    # 12-14: Trak from a BDS 5,0 track, a magnetic heading, a true heading
    two(b, T0, a + 12, source=S4, msgtype=21, commb_format=8, heading_valid=1, heading_type=ia.GROUND_TRACK, heading_raw=2047)
    two(b, T0, a + 13, metype=19, heading_valid=1, heading_type=ia.MAGNETIC_OR_TRUE, heading_raw=1000)
    b.ops(T0, a + 14, 2, hrd=ia.TRUE)
    b.rec(T0 + 1, a + 14, metype=19, heading_valid=1, heading_type=ia.MAGNETIC_OR_TRUE, heading_raw=513)
    # 15-17: Vsi from geom (negative), baro, none beside a squawk
    two(b, T0, a + 15, geom_rate_valid=1, geom_rate=-2048, baro_rate_valid=1, baro_rate=640)
    two(b, T0, a + 16, baro_rate_valid=1, baro_rate=-64)
    two(b, T0, a + 17, squawk_valid=1, squawk=0x7700)
    # 18-21: Gnd with a source of 3 and of 4, airborne and ground
    two(b, T0, a + 18, source=ip.MODE_S, msgtype=11, airground=ia.AG_GROUND)
    two(b, T0, a + 19, source=S4, msgtype=4, airground=ia.AG_GROUND, **alt)
    two(b, T0, a + 20, source=S4, msgtype=4, airground=ia.AG_AIRBORNE, **alt)
    two(b, T0, a + 21, airground=ia.AG_GROUND)
    # 22-25: Trt for versions -1 (Mode S only), 0, 1, 2
    two(b, T0, a + 22, source=ip.MODE_S, msgtype=11)
    for v in (0, 1, 2):
        b.ops(T0, a + 23 + v, v).rec(T0 + 1, a + 23 + v)
    # 26: a southern and western position;  27: TIS-B, the position expired at the write (Tisb true, no Lat);  28: TIS-B valid
    b.half(T0 + 20, a + 26, -33.9, -70.8, 0, 11, signal=0.16).half(T0 + 400, a + 26, -33.9, -70.8, 1, 11, signal=0.16)
    b.half(T0 - 80000, a + 27, 50.0, 8.0, 0, 11, source=ip.TISB, addrtype=3)
    b.half(T0 - 79600, a + 27, 50.0, 8.0, 1, 11, source=ip.TISB, addrtype=3)
    b.rec(T0, a + 27, source=ip.TISB, addrtype=3)
    b.half(T0 + 20, a + 28, 50.0, 8.0, 0, 11, source=ip.TISB, addrtype=3)
    b.half(T0 + 400, a + 28, 50.0, 8.0, 1, 11, source=ip.TISB, addrtype=3)
    return [None], [early, ("expire", T0 - 9000), b.step()], [(2, T0 + 2000, 0, 1)]


ESCAPES = [b'AB"CD   ', b"EF\\GH   ", b"\x01\x1f\x7f\x80\xff   ", b"ABC\0DEFG", b"12345678", b'""\\\\\xfe\xfd\xfc\xfb', bytes(8)]


def escapes_table(pkg):
    b = acs.Builder(pkg)
    for k, cs in enumerate(ESCAPES):
        two(b, T0, 0x4E0000 + k, callsign_valid=1, callsign=cs)
    return [None], [b.step()], [(0, T0 + 2000, 0, 1)]


# two records each: Sig = 255 * (2 s + 7e-5) / 8 -- 956250000, 4271250000 (ten digits), 4335000000 (at or above 2^32: 0),
# beyond every integer, infinite, 0.06, and 0.5 to the last place or so
SIGNALS = [1.5e7, 6.7e7, 6.8e7, 1e300, float("inf"), 0.001, (0.5 * 8 / 255 - 7e-5) / 2]


def bounds_table(pkg):
    """the widest object records can build -- a ten-digit Sig, eight callsign bytes of six characters each, the most
    negative altitudes and rates the table takes, both positions negative -- and signal levels no demodulator delivers.
    (The object of exactly MSD_VRS_AIRCRAFT_MAX needs a messages count and a position time of twenty digits, which no
    stream of records reaches: test_vrs_abi.py and tests/c/vrs_units.c build it from an entry.)"""
    b = acs.Builder(pkg)
    a = 0x4FFFF0
    wide = dict(signal=1.5e7, source=S4)
    for k in range(3):
        b.rec(T0 + k, a, msgtype=20, crc=0x123456, altitude_baro_valid=1, altitude_baro=-99900, **wide)
    b.rec(T0 + 3, a, msgtype=20, commb_format=7, nav_valid=4 | 16, nav_mcp_altitude=-2147483648, nav_qnh_raw=65535, **wide)
    b.rec(T0 + 3, a, msgtype=21, commb_format=8, heading_valid=1, heading_type=ia.GROUND_TRACK, heading_raw=2047,
          callsign_valid=1, callsign=b"\xff" * 8, squawk_valid=1, squawk=0xFFFF, geom_rate_valid=1, geom_rate=-32768,
          altitude_geom_valid=1, altitude_geom=-2147483648, **wide)
    b.rec(T0 + 3, a, msgtype=20, commb_format=7, nav_valid=2, nav_heading_raw=65535, **wide)
    b.half(T0 + 20, a, -89.9, -179.9, 0, 11, signal=1.5e7).half(T0 + 400, a, -89.9, -179.9, 1, 11, signal=1.5e7)
    for k, s in enumerate(SIGNALS):
        two(b, T0, 0x4F0000 + k, signal=s)
    return [None], [b.step()], [(0, T0 + 2000, 0, 1)]


def expiring_table(pkg):
    """a write, an expiry that removes an aircraft heard once and so rebuilds the table, more records, a write"""
    b = acs.Builder(pkg)
    a = 0x480000
    for k in range(40):
        two(b, T0 + 60000 + k, a + 3 * k, rx=k % 2, signal=0.01 * (k + 1), squawk_valid=1, squawk=0x1000 + k)
    b.rec(T0, a + 1000, source=ip.MODE_S, msgtype=11)
    first = b.step()
    for k in range(0, 40, 3):
        b.rec(T0 + 64000, a + 3 * k, rx=k % 2, source=ip.MODE_S, msgtype=11)
    second = b.step()
    return ([None, None], [first, ("expire", T0 + 62000), second],
            [(0, T0 + 61000, 0, 1), (1, T0 + 63000, 0, 1), (2, T0 + 66000, 0, 1), (2, T0 + 66000, 0, 32)])


TABLES = dict(counts=lambda pkg: counts_table(pkg, [1, 0, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 0]),
              three=lambda pkg: counts_table(pkg, [3, 0, 2]), empty=lambda pkg: counts_table(pkg, [0, 0]),
              comma=comma_table, stale=stale_table, kinds=kinds_table, escapes=escapes_table, bounds=bounds_table,
              expiring=expiring_table)


def write(tracker, now, part, n_parts, refuse=False):
    """one msd_pos_vrs call -> (stream, rows).  refuse: first offered nothing, then one byte less than it needs"""
    if not refuse:
        return tracker.vrs_stream(now, part, n_parts)
    need = None
    for cap in (0, None):
        try:
            tracker.vrs_stream(now, part, n_parts, cap=cap if cap is not None else need - 1)
            raise AssertionError("a buffer too short was accepted")
        except Exception as e:
            assert getattr(e, "code", None) == -errno.ENOSPC, e
            assert need in (None, tracker.vrs_needed)
            need = tracker.vrs_needed
    return tracker.vrs_stream(now, part, n_parts, cap=need)


def run(tracker, scenario, pieces=None, refuse=False):
    """the scenario through a capi.PositionTracker with vrs -> [(stream, rx rows) per write]"""
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
        for after, now, part, n_parts in writes:
            if after == i:
                out.append(write(tracker, now, part, n_parts, refuse))
    return out


def split(stream, rx):
    ends = [0] + [int(e) for e in rx["end"]]
    assert ends == sorted(ends) and ends[-1] == len(stream)
    return [stream[a:b] for a, b in zip(ends[:-1], ends[1:])]


def run_model(pkg, tracker_factory, scenario):
    """the second reading over the snapshots of a tracker fed the same steps -> [(documents, counts) per write]"""
    receivers, steps, writes = scenario
    t = tracker_factory(receivers)
    out = []
    for i, s in enumerate(steps):
        if s[0] == "expire":
            t.expire(s[1])
        else:
            t.update_nicrc(s[1], s[2], s[3])
        for after, now, part, n_parts in writes:
            if after == i:
                out.append(iv.documents(t.snapshot(), pkg.capi.AC, len(receivers), now, part, n_parts))
    t.close()
    return out
