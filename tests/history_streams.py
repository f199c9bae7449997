"""Constructed tables for the history_N.pb tests (test_history_model.py on the CPU, test_gpu_history_pb.py on the GPU):
aircraft_streams.Builder records that leave the aircraft table in the states the writer's rules turn on -- the smallest
tables at which each rule flips -- and runners for the trackers and the second reading of tests/indep_history.py.

A scenario is (receivers, steps, writes): steps as in aircraft_streams, writes a list of (after step, now_ms) -- the files
are written after that step (several writes may follow one step)."""
import errno

import aircraft_streams as acs
import indep_aircraft as ia
import indep_history as ih
import indep_positions as ip

T0 = acs.T0
WT = 256  # the writer's workgroup, and the items of its LDS image (HISTORY_TILE, msd_history_kernels.hip)
S4 = ip.MODE_S_CHECKED
NON_ICAO = 1 << 24  # MSD_NON_ICAO_ADDRESS


def where(k):
    """a place of its own for aircraft k, inside one CPR zone pair"""
    return 40.0 + 0.05 * (k % 200), 5.0 + 0.05 * (k // 200)


def located(b, t, addr, rx=0, k=0, **kw):
    """an aircraft with a position: an even and an odd airborne half 400 ms apart decode globally at t; two messages.
    kw: further members of the second half (an ADS-B squitter: crc 0, so a barometric altitude is reliable at once)"""
    lat, lon = where(k)
    return b.half(t - 400, addr, lat, lon, 0, 11, rx=rx).half(t, addr, lat, lon, 1, 11, rx=rx, **kw)


def seen_at(b, t, addr, rx=0):
    """a DF11 with nothing but its time: `seen` becomes t, also when t lies before the records in front"""
    return b.rec(t, addr, rx=rx, source=ip.MODE_S, msgtype=11)


def counts_table(pkg, counts, every=1):
    """counts[r] aircraft on receiver r; every `every`-th of them has a position and an altitude, the others are heard
    twice and have none"""
    b = acs.Builder(pkg)
    k = 0
    for r, c in enumerate(counts):
        for j in range(c):
            if k % every == 0:
                located(b, T0 + 400 + k % 1000, 0x400000 + 7 * k, rx=r, k=k, altitude_baro_valid=1,
                        altitude_baro=(-1000 + 25 * k) if k % 3 else 0)
            else:
                seen_at(b, T0, 0x400000 + 7 * k, rx=r)
                seen_at(b, T0 + 1, 0x400000 + 7 * k, rx=r)
            k += 1
    return [None] * len(counts), [b.step()], [(0, T0 + 5000)]


def selection_table(pkg):
    """one write at `now`.  Receiver 0: heard once; heard twice without a position; seen 90 001 ms before, with a position
    decoded 69 s before (an older record moves `seen` back, not the position): all three are refused.  Receiver 1 is
    empty.  Receiver 2: seen exactly 90 000 ms before (written); seen after the write (written); a position 69 999 ms old
    (written) and one 70 000 ms old (refused); a non-ICAO address (written, with its bit)"""
    b = acs.Builder(pkg)
    now = T0 + 200000
    seen_at(b, now - 10, 0x410001)
    seen_at(b, now - 20, 0x410002)
    seen_at(b, now - 10, 0x410002)
    located(b, now - 69000, 0x410003, k=3)
    seen_at(b, now - 90001, 0x410003)
    located(b, now - 69000, 0x410004, rx=2, k=4)
    seen_at(b, now - 90000, 0x410004, rx=2)
    located(b, now + 50, 0x410005, rx=2, k=5)
    located(b, now - 69999, 0x410006, rx=2, k=6)
    located(b, now - 70000, 0x410007, rx=2, k=7)
    located(b, now - 1000, NON_ICAO | 0x410008, rx=2, k=8)
    return [None, None, None], [b.step()], [(0, now)]


def altitude_table(pkg):
    """one write at `now`, every aircraft with a position 1 s old.  On the ground by an ADS-B record (-9999), on the ground
    by a DF11's source 3 (not -9999: its reliable barometric altitude instead); barometric altitudes with
    altitude_baro_reliable 2 (not taken: absent) and 3 (taken), a negative one (a ten-byte varint) and 0 (absent); a
    geometric altitude one ms inside its own expiry (taken) and at it (absent); an airground on the ground that is
    70 s old (expired: the altitude instead)"""
    b = acs.Builder(pkg)
    now = T0 + 300000
    a = 0x420000
    located(b, now - 1000, a + 1, k=1, airground=ia.AG_GROUND, altitude_baro_valid=1, altitude_baro=1200)
    located(b, now - 1000, a + 2, k=2, altitude_baro_valid=1, altitude_baro=2300)
    b.rec(now - 900, a + 2, source=ip.MODE_S, msgtype=11, airground=ia.AG_GROUND)
    for addr, n in ((a + 3, 2), (a + 4, 3)):
        located(b, now - 1000, addr, k=addr - a)
        for j in range(n):
            b.alt(now - 800 + j, addr, 31000)
    located(b, now - 1000, a + 5, k=5, altitude_baro_valid=1, altitude_baro=-975)
    located(b, now - 1000, a + 6, k=6, altitude_baro_valid=1, altitude_baro=0)
    for addr, age in ((a + 7, 69999), (a + 8, 70000)):
        b.rec(now - age, addr, metype=20, altitude_geom_valid=1, altitude_geom=9000 + addr - a)
        located(b, now - 1000, addr, k=addr - a)
    b.rec(now - 70000, a + 9, airground=ia.AG_GROUND)
    located(b, now - 1000, a + 9, k=9, altitude_baro_valid=1, altitude_baro=4100)
    located(b, now - 1000, a + 10, k=10)
    return [None], [b.step()], [(0, now)]


def expire_table(pkg):
    """writes around an expiry that removes aircraft and rebuilds the table: the survivors sit in other slots afterwards
    and are written as before"""
    b = acs.Builder(pkg)
    for k in range(40):
        if k % 4 == 0:
            seen_at(b, T0, 0x430000 + 11 * k, rx=k % 2)  # heard once: gone after 60 s
        else:
            located(b, T0 + 400 + k, 0x430000 + 11 * k, rx=k % 2, k=k, altitude_baro_valid=1, altitude_baro=100 * k)
    first = b.step()
    for k in range(40):
        if k % 4 == 1:
            located(b, T0 + 64000 + k, 0x430000 + 11 * k, rx=k % 2, k=k + 1)
    return [None, None], [first, ("expire", T0 + 61000), b.step()], [(0, T0 + 5000), (1, T0 + 61000), (2, T0 + 66000)]


def nothing_table(pkg):
    """now_ms < 1000 and nobody to write: aircraft heard once or without a position"""
    b = acs.Builder(pkg)
    seen_at(b, T0, 0x440001)
    seen_at(b, T0, 0x440002, rx=1)
    seen_at(b, T0 + 1, 0x440002, rx=1)
    return [None, None], [b.step()], [(0, 999), (0, 1000)]


TABLES = dict(selection=selection_table, altitude=altitude_table, expire=expire_table, nothing=nothing_table,
              three=lambda pkg: counts_table(pkg, [3, 0, 2]), empty=lambda pkg: counts_table(pkg, [0, 0]))


def split(stream, rx):
    ends = [0] + [int(e) for e in rx["end"]]
    assert ends == sorted(ends) and ends[-1] == len(stream)
    return [stream[a:b] for a, b in zip(ends[:-1], ends[1:])]


def feed(tracker, step):
    if step[0] == "expire":
        tracker.expire(step[1])
    else:
        tracker.update_nicrc(step[1], step[2], step[3])


def refused_then_written(tracker, now):
    """the size, a buffer one byte short, then the write itself -> (stream, rows)"""
    def enospc(cap):
        try:
            tracker.history_pb_stream(now, cap=cap)
        except Exception as e:
            assert getattr(e, "code", None) == -errno.ENOSPC, e
            return tracker.history_needed
        return None
    need = enospc(0)
    if need is None:
        need = 0
    else:
        assert need > 0 and enospc(need - 1) == need
    return tracker.history_pb_stream(now, cap=need)


def run(tracker, scenario, refuse=False):
    """the scenario through a table capi.PositionTracker -> [(stream, rx rows) per write]"""
    receivers, steps, writes = scenario
    out = []
    for i, s in enumerate(steps):
        feed(tracker, s)
        for after, now in writes:
            if after == i:
                out.append(refused_then_written(tracker, now) if refuse else tracker.history_pb_stream(now))
    return out


def run_model(pkg, tracker, scenario, counts=None):
    """the second reading over the snapshots of a tracker fed the same steps -> [(files, rows) per write]"""
    receivers, steps, writes = scenario
    out = []
    for i, s in enumerate(steps):
        feed(tracker, s)
        for after, now in writes:
            if after == i:
                out.append(ih.files(tracker.snapshot(), pkg.capi.AC, len(receivers), now, counts))
    return out
