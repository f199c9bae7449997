"""Constructed record streams for the aircraft table's tests (test_aircraft_model.py on the CPU,
test_gpu_aircraft_table.py on the GPU): pos_streams.Builder with the message's crc and signal level, one small named
scenario per rule of the table's feed function, a 2000-record mixed stream of DF4 / 5 / 11 / 17 / 20 / 21 records, and
runners for the three implementations (the GPU object, the host twin, the second reading of tests/indep_aircraft.py).

A scenario is (receivers, filter_persistence, steps, check); a step is ("update", msgs, fields, receiver) or
("expire", now_ms); check(snaps, nicrc) asserts the value the scenario is named for against an expectation derived by
hand from track.c -- snaps[i] is the snapshot after step i as {addr: entry}, nicrc the (nic, rc, set) rows of all update
steps in order."""
import numpy as np

import indep_aircraft as ia
import indep_modeac as im
import indep_positions as ip
import pos_streams as ps

T0 = ps.T0
S4 = ip.MODE_S_CHECKED


class Builder(ps.Builder):
    def rec(self, t, addr, rx=0, source=ip.ADSB, msgtype=17, crc=0, signal=0.0, **kw):
        super().rec(t, addr, rx=rx, source=source, msgtype=msgtype, **kw)
        self.m[-1]["crc"], self.m[-1]["signalLevel"] = crc, signal
        return self

    def alt(self, t, addr, feet, crc=0x123456, source=S4, msgtype=4, **kw):
        """a surveillance altitude reply (address/parity: the crc word is not zero); crc=0 with DF17 for a squitter"""
        return self.rec(t, addr, source=source, msgtype=msgtype, crc=crc, altitude_baro_valid=1, altitude_baro=feet, **kw)

    def half(self, t, addr, lat, lon, odd, metype, **kw):
        """an airborne CPR half with any ME type"""
        y, x = ip.cpr_encode(lat, lon, odd, False)
        return self.rec(t, addr, cpr_valid=1, cpr_type=1, cpr_odd=odd, cpr_lat=y, cpr_lon=x, metype=metype, **kw)

    def ops(self, t, addr, version, hrd=0, tah=0, **kw):
        return self.rec(t, addr, opstatus=1 | (version << 1) | (hrd << 23) | (tah << 26), metype=31, **kw)


# the scenarios of scenarios(), one per rule
NAMES = ["stale_15s", "stale_60s", "older_than_updated", "gate_small_jump", "gate_fpm_default", "gate_rate_bounds",
         "gate_countdown", "gate_good_crc", "gate_age_30s", "airground_uncertain", "heading_hrd_tah", "sil_type_unknown",
         "v0_nacp_sil", "nic_rc_table", "nic_relative_minimum", "derived_geom", "expire_asymmetries", "signal_ring",
         "refusals", "metric_altitudes", "version_arms", "combine_single_source", "baro_gate_arms", "surface_movement_codes",
         "reliable_sides"]
NIC_CASES = [(me, v, a, b, c) for me in [0] + list(range(5, 23)) for v in (0, 1, 2) for a in (0, 1) for b in (0, 1) for c in (0, 1)]


# (NIC, Rc) by ME type, ADS-B version and the NIC supplements, typed from track.c:690-892.  A row is the eight
# combinations of (A, B, C) in the order 000 001 010 011 100 101 110 111.
def _all(nic, rc):
    return [(nic, rc)] * 8


def _by_a(without, with_a):
    return [without] * 4 + [with_a] * 4


_EVERY = lambda row: {0: row, 1: row, 2: row}  # noqa: E731
NIC_RC = {
    0: _EVERY(_all(0, 0)), 18: _EVERY(_all(0, 0)), 19: _EVERY(_all(0, 0)), 22: _EVERY(_all(0, 0)),
    5: _EVERY(_all(11, 8)), 9: _EVERY(_all(11, 8)), 20: _EVERY(_all(11, 8)),
    6: _EVERY(_all(10, 25)), 10: _EVERY(_all(10, 25)), 21: _EVERY(_all(10, 25)),
    7: {0: _all(8, 186), 1: _by_a((8, 186), (9, 75)),  # version 2: A and not C
        2: [(8, 186), (8, 186), (8, 186), (8, 186), (9, 75), (8, 186), (9, 75), (8, 186)]},
    8: {0: _all(0, 0), 1: _all(0, 0),                  # version 2: A and C; A, not C; C, not A; neither
        2: [(0, 0), (6, 926), (0, 0), (6, 926), (6, 556), (7, 371), (6, 556), (7, 371)]},
    11: {0: _all(8, 186), 1: _by_a((8, 186), (9, 75)),  # version 2: A and B
         2: [(8, 186), (8, 186), (8, 186), (8, 186), (8, 186), (8, 186), (9, 75), (9, 75)]},
    12: _EVERY(_all(7, 371)),
    13: {0: _all(6, 926), 1: _by_a((6, 926), (6, 1112)),  # version 2: B, not A; neither; both; A, not B is "unknown"
         2: [(6, 926), (6, 926), (6, 556), (6, 556), (6, 0), (6, 0), (6, 1112), (6, 1112)]},
    14: _EVERY(_all(5, 1852)), 15: _EVERY(_all(4, 3704)),
    16: {0: [(2, 18520)] * 6 + [(3, 18520)] * 2,         # the NIC is 3 with A and B in every version
         1: [(2, 14816)] * 4 + [(2, 7408)] * 2 + [(3, 7408)] * 2,
         2: [(2, 14816)] * 6 + [(3, 7408)] * 2},
    17: _EVERY(_all(1, 37040)),
}

# ---- the refusal family: every member msd_trk_feed accepts, as (member, stale interval in ms, the fields of a record that
# carries value 0 / value 1, what the entry shows for each).  The lesser source's records are DF20 replies.
_HDG = lambda t: lambda raw: dict(heading_valid=1, heading_type=t, heading_raw=raw)  # noqa: E731


def _hdg_of(member):
    return lambda e: int(e[member]["raw"])


TRK_MEMBERS = [
    # member, stale, fields(value), values, read
    ("callsign", 60000, lambda v: dict(callsign_valid=1, callsign=v), (b"FIRST   ", b"SECOND  "), lambda e: bytes(e["callsign"])),
    ("altitude_baro", 15000, lambda v: dict(altitude_baro_valid=1, altitude_baro=v), (10000, 10100), lambda e: int(e["alt_baro"])),
    ("altitude_geom", 60000, lambda v: dict(altitude_geom_valid=1, altitude_geom=v), (9000, 9500), lambda e: int(e["alt_geom"])),
    ("geom_delta", 60000, lambda v: dict(geom_delta_valid=1, geom_delta=v), (250, -125), lambda e: int(e["geom_delta"])),
    ("mach", 60000, lambda v: dict(commb_valid=8, mach_raw=v), (190, 205), lambda e: int(e["mach_raw"])),
    ("track", 60000, _HDG(1), (100, 200), _hdg_of("track")),
    ("track_rate", 60000, lambda v: dict(commb_valid=4, track_rate_q=v), (12, -40), lambda e: int(e["track_rate_q"])),
    ("roll", 60000, lambda v: dict(commb_valid=1, roll_q=v), (-37, 55), lambda e: int(e["roll_q"])),
    ("mag_heading", 60000, _HDG(3), (300, 400), _hdg_of("mag_heading")),
    ("true_heading", 60000, _HDG(2), (500, 600), _hdg_of("true_heading")),
    ("baro_rate", 60000, lambda v: dict(baro_rate_valid=1, baro_rate=v), (1500, -640), lambda e: int(e["baro_rate"])),
    ("geom_rate", 60000, lambda v: dict(geom_rate_valid=1, geom_rate=v), (-1280, 704), lambda e: int(e["geom_rate"])),
    ("squawk", 15000, lambda v: dict(squawk_valid=1, squawk=v), (0x1200, 0x7000), lambda e: int(e["squawk"])),
    ("airground", 15000, lambda v: dict(airground=v), (1, 2), lambda e: int(e["air_ground"])),  # ground, airborne: both certain
    ("nav_qnh", 60000, lambda v: dict(nav_valid=16, nav_qnh_raw=v), (2132, 2000), lambda e: int(e["nav_qnh_raw"])),
    ("nav_altitude_mcp", 60000, lambda v: dict(nav_valid=4, nav_mcp_altitude=v), (36000, 24000), lambda e: int(e["nav_altitude_mcp"])),
    ("nav_altitude_fms", 60000, lambda v: dict(nav_valid=8, nav_fms_altitude=v), (37000, 25000), lambda e: int(e["nav_altitude_fms"])),
    ("nav_altitude_src", 60000, lambda v: dict(nav_altitude_source=v), (2, 4), lambda e: int(e["nav_altitude_src"])),
    ("nav_heading", 60000, lambda v: dict(nav_valid=2, nav_heading_raw=v), (128, 300), lambda e: int(e["nav_heading_raw"])),
    # the flags are only ever set (track.c:1281-1298): an accepted 2 after 1 shows 3
    ("nav_modes", 60000, lambda v: dict(nav_valid=1, nav_modes=v & 2 or 1), (1, 3), lambda e: int(e["nav_modes"])),
    ("nic_a", 60000, lambda v: dict(acc_valid=4, nic_a=v), (1, 0), lambda e: int(e["nic_a"])),
    ("nic_c", 60000, lambda v: dict(acc_valid=8, nic_c=v), (1, 0), lambda e: int(e["nic_c"])),
    ("nic_baro", 60000, lambda v: dict(acc_valid=2, nic_baro=v), (1, 0), lambda e: int(e["nic_baro"])),
    ("nac_p", 60000, lambda v: dict(acc_valid=1, nac_p=v), (9, 5), lambda e: int(e["nac_p"])),
    ("nac_v", 60000, lambda v: dict(nac_v_valid=1, nac_v=v), (2, 4), lambda e: int(e["nac_v"])),
    ("sil", 60000, lambda v: dict(sil_type=2, sil=v), (3, 1), lambda e: int(e["sil"])),
    ("gva", 60000, lambda v: dict(acc_valid=16, gva=v), (2, 1), lambda e: int(e["gva"])),
    ("sda", 60000, lambda v: dict(acc_valid=32, sda=v), (3, 2), lambda e: int(e["sda"])),
    ("emergency", 60000, lambda v: dict(emergency_valid=1, emergency=v), (4, 1), lambda e: int(e["emergency"])),
    ("alert", 60000, lambda v: dict(alert_valid=1, alert=v), (1, 0), lambda e: int(e["alert"])),
    ("spi", 60000, lambda v: dict(spi_valid=1, spi=v), (1, 0), lambda e: int(e["spi"])),
]
POS_MEMBER_VALUES = dict(gs=(500, 100), ias=(250, 180), tas=(420, 390))


def trk_refusal_addr(k, case):
    return 0xB00000 + 0x100 * k + case


def trk_refusal_offsets(member, stale):
    """(last refused, first accepted) offset of a lesser source's record.  accept_data: refused while now < updated +
    stale interval.  The barometric altitude does not get that far: :1091-1093 lets a lesser source in only when the
    altitude is *more* than 15 s old, so 15 000 ms is still refused and 15 001 ms is the first accepted."""
    return (15000, 15001) if member == "altitude_baro" else (stale - 1, stale)


def nic_addr(k):
    return 0x500000 + k


def scenarios(pkg):
    AC = pkg.capi.AC
    S = {}
    B = lambda: Builder(pkg)  # noqa: E731

    def src(e, k):
        return int(e["source"][AC[k]])

    def upd(e, k):
        return int(e["updated"][AC[k]])

    # squawk goes stale after 15 s: a Mode S squawk against an ADS-B one, one ms before and at the limit
    b = B()
    for a, dt in ((0x100001, 14999), (0x100002, 15000)):
        b.rec(T0, a, squawk_valid=1, squawk=0x1200).rec(T0 + dt, a, source=S4, msgtype=5, squawk_valid=1, squawk=0x7000)

    def check(snaps, nicrc):
        s = snaps[-1]
        assert int(s[0x100001]["squawk"]) == 0x1200 and src(s[0x100001], "squawk") == ip.ADSB
        assert int(s[0x100002]["squawk"]) == 0x7000 and src(s[0x100002], "squawk") == S4
    S["stale_15s"] = ([None], 0, [b.step()], check)

    # the callsign after 60 s
    b = B()
    for a, dt in ((0x110001, 59999), (0x110002, 60000)):
        b.rec(T0, a, callsign_valid=1, callsign=b"KLM1023 ").rec(T0 + dt, a, source=S4, msgtype=20, callsign_valid=1, callsign=b"TEST    ")

    def check(snaps, nicrc):
        s = snaps[-1]
        assert bytes(s[0x110001]["callsign"]) == b"KLM1023 " and bytes(s[0x110002]["callsign"]) == b"TEST    "
    S["stale_60s"] = ([None], 0, [b.step()], check)

    # a record older than the member's `updated` is refused whatever its source
    b = B()
    b.rec(T0 + 1000, 0x120001, squawk_valid=1, squawk=0x1200).rec(T0 + 500, 0x120001, squawk_valid=1, squawk=0x3333)
    b.rec(T0 + 500, 0x120001, callsign_valid=1, callsign=b"OLDER   ")  # the callsign was never set: accepted

    def check(snaps, nicrc):
        e = snaps[-1][0x120001]
        assert int(e["squawk"]) == 0x1200 and upd(e, "squawk") == T0 + 1000
        assert bytes(e["callsign"]) == b"OLDER   " and upd(e, "callsign") == T0 + 500 and int(e["seen"]) == T0 + 500
    S["older_than_updated"] = ([None], 0, [b.step()], check)

    # the altitude gate: a jump of 299 ft passes without a look at the rate
    b = B()
    b.alt(T0, 0x130001, 10000).alt(T0 + 100, 0x130001, 10299)

    def check(snaps, nicrc):
        e = snaps[-1][0x130001]
        assert int(e["alt_baro"]) == 10299 and int(e["altitude_baro_reliable"]) == 2
    S["gate_small_jump"] = ([None], 0, [b.step()], check)

    # a jump judged by the default bounds: after 2 s, 400 ft are 400 * 600 / 30 = 8000 ft/min (accepted), 1000 ft are
    # 20000 (refused, altitude_baro_reliable 3 -> 2)
    b = B()
    for a, jump in ((0x140001, 400), (0x140002, 1000)):
        for k in range(3):
            b.alt(T0 + 1000 * k, a, 10000)
        b.alt(T0 + 4000, a, 10000 + jump)

    def check(snaps, nicrc):
        s = snaps[-1]
        assert int(s[0x140001]["alt_baro"]) == 10400 and int(s[0x140001]["altitude_baro_reliable"]) == 4
        assert int(s[0x140002]["alt_baro"]) == 10000 and int(s[0x140002]["altitude_baro_reliable"]) == 2
    S["gate_fpm_default"] = ([None], 0, [b.step()], check)

    # bounds from the younger of geom_rate and baro_rate.  The altitude is 10 s old at the jump: fpm = delta * 600 / 110;
    # the rate is 11.5 s old: +- (1500 + 5750).  geom_rate 3000 younger: max 10250, 2017 ft = 11001 ft/min is refused
    # (the default 12500 would pass it); baro_rate 6000 younger: max 13250, 2384 ft = 13003 ft/min passes (the default
    # would refuse it)
    b = B()
    b.rec(T0, 0x150001, metype=19, baro_rate_valid=1, baro_rate=0).rec(T0 + 500, 0x150001, metype=19, geom_rate_valid=1, geom_rate=3000)
    b.rec(T0, 0x150002, metype=19, geom_rate_valid=1, geom_rate=0).rec(T0 + 500, 0x150002, metype=19, baro_rate_valid=1, baro_rate=6000)
    for a, jump in ((0x150001, 2017), (0x150002, 2384)):
        for k in range(3):
            b.alt(T0 + 1000 * k, a, 10000)
        b.alt(T0 + 12000, a, 10000 + jump)

    def check(snaps, nicrc):
        s = snaps[-1]
        assert int(s[0x150001]["alt_baro"]) == 10000 and int(s[0x150001]["altitude_baro_reliable"]) == 2
        assert int(s[0x150002]["alt_baro"]) == 12384 and int(s[0x150002]["altitude_baro_reliable"]) == 4
    S["gate_rate_bounds"] = ([None], 0, [b.step()], check)

    # refused jumps count altitude_baro_reliable down: 3 -> 2 -> 1 -> 0 and the altitude is invalid; the next is taken
    b = B()
    for k in range(3):
        b.alt(T0 + 1000 * k, 0x160001, 10000)
    for k in range(3):
        b.alt(T0 + 3000 + 1000 * k, 0x160001, 30000)
    down = b.step()
    after = b.alt(T0 + 6000, 0x160001, 30000).step()

    def check(snaps, nicrc):
        e = snaps[0][0x160001]
        assert src(e, "altitude_baro") == 0 and int(e["altitude_baro_reliable"]) == 0 and int(e["alt_baro"]) == 10000
        e = snaps[1][0x160001]
        assert src(e, "altitude_baro") == S4 and int(e["altitude_baro_reliable"]) == 1 and int(e["alt_baro"]) == 30000
    S["gate_countdown"] = ([None], 0, [down, after], check)

    # a squitter (crc 0) counts 10: reliability 10 after the first, and at <= 12 a wild jump is let through (20 then);
    # at 20 the next wild jump is refused and costs 10
    b = B()
    b.alt(T0, 0x170001, 10000, crc=0, source=ip.ADSB, msgtype=17).alt(T0 + 1000, 0x170001, 30000, crc=0, source=ip.ADSB, msgtype=17)
    first = b.step()
    second = b.alt(T0 + 2000, 0x170001, 5000, crc=0, source=ip.ADSB, msgtype=17).step()

    def check(snaps, nicrc):
        assert int(snaps[0][0x170001]["alt_baro"]) == 30000 and int(snaps[0][0x170001]["altitude_baro_reliable"]) == 20
        assert int(snaps[1][0x170001]["alt_baro"]) == 30000 and int(snaps[1][0x170001]["altitude_baro_reliable"]) == 10
    S["gate_good_crc"] = ([None], 0, [first, second], check)

    # an altitude 30 s old or more resets the reliability and is replaced; at 29999 ms the limit is 20 - 19 = 1, the
    # jump is refused and the last point goes
    b = B()
    for a, dt in ((0x180001, 29999), (0x180002, 30000)):
        for k in range(3):
            b.alt(T0 + 10 * k, a, 10000)
        b.alt(T0 + 20 + dt, a, 30000)

    def check(snaps, nicrc):
        s = snaps[-1]
        assert src(s[0x180001], "altitude_baro") == 0 and int(s[0x180001]["alt_baro"]) == 10000
        assert src(s[0x180002], "altitude_baro") == S4 and int(s[0x180002]["alt_baro"]) == 30000
        assert int(s[0x180002]["altitude_baro_reliable"]) == 1
    S["gate_age_30s"] = ([None], 0, [b.step()], check)

    # air / ground: an uncertain state does not replace fresh certain data, it does replace stale data
    b = B()
    for a, dt in ((0x190001, 14999), (0x190002, 15000)):
        b.rec(T0, a, airground=ia.AG_GROUND).rec(T0 + dt, a, airground=ia.AG_UNCERTAIN)

    def check(snaps, nicrc):
        s = snaps[-1]
        assert int(s[0x190001]["air_ground"]) == ia.AG_GROUND and int(s[0x190002]["air_ground"]) == ia.AG_UNCERTAIN
    S["airground_uncertain"] = ([None], 0, [b.step()], check)

    # headings routed by HRD / TAH: magnetic-or-true is magnetic until an operational status says true; track-or-heading
    # is the ground track until it says magnetic
    b = B()
    b.rec(T0, 0x1A0001, metype=19, heading_valid=1, heading_type=ia.MAGNETIC_OR_TRUE, heading_raw=256)
    b.rec(T0 + 10, 0x1A0001, metype=7, heading_valid=1, heading_type=ia.TRACK_OR_HEADING, heading_raw=32)
    before = b.step()
    b.ops(T0 + 20, 0x1A0001, 2, hrd=ia.TRUE, tah=ia.MAGNETIC)
    b.rec(T0 + 30, 0x1A0001, metype=19, heading_valid=1, heading_type=ia.MAGNETIC_OR_TRUE, heading_raw=512)
    b.rec(T0 + 40, 0x1A0001, metype=7, heading_valid=1, heading_type=ia.TRACK_OR_HEADING, heading_raw=64)
    b.vel(T0 + 50, 0x1A0001, -100, 100)

    def check(snaps, nicrc):
        e = snaps[0][0x1A0001]
        assert (int(e["mag_heading"]["kind"]), int(e["mag_heading"]["raw"])) == (ia.HDG_ES19, 256)
        assert (int(e["track"]["kind"]), int(e["track"]["raw"])) == (ia.HDG_SURFACE, 32) and src(e, "true_heading") == 0
        e = snaps[1][0x1A0001]
        assert (int(e["true_heading"]["kind"]), int(e["true_heading"]["raw"])) == (ia.HDG_ES19, 512)
        assert (int(e["mag_heading"]["kind"]), int(e["mag_heading"]["raw"])) == (ia.HDG_SURFACE, 64) and upd(e, "mag_heading") == T0 + 40
        assert (int(e["track"]["kind"]), int(e["track"]["ew"]), int(e["track"]["ns"])) == (ia.HDG_VELOCITY, -100, 100)
        f = pkg.capi.aircraft_to_float(e)
        assert float(f["true_heading"]) == 180.0 and float(f["mag_heading"]) == 180.0 and float(f["track"]) == 315.0
    S["heading_hrd_tah"] = ([None], 0, [before, b.step()], check)

    # sil_type: `unknown` does not replace a known type, it does fill an invalid one
    b = B()
    b.ops(T0, 0x1B0001, 2, sil_type=3, sil=3).rec(T0 + 10, 0x1B0001, metype=29, sil_type=1, sil=2)
    b.ops(T0, 0x1B0002, 2).rec(T0 + 10, 0x1B0002, metype=29, sil_type=1, sil=2)

    def check(snaps, nicrc):
        s = snaps[-1]
        assert (int(s[0x1B0001]["sil"]), int(s[0x1B0001]["sil_type"])) == (2, 3)
        assert (int(s[0x1B0002]["sil"]), int(s[0x1B0002]["sil_type"])) == (2, 1)
    S["sil_type_unknown"] = ([None], 0, [b.step()], check)

    # ADS-B version 0: NACp and SIL from the position's ME type (11: NACp 8, SIL 2); not any more after a version 2 status
    b = B()
    b.half(T0, 0x1C0001, 50.0, 8.0, 0, 11).ops(T0 + 100, 0x1C0001, 2).half(T0 + 20000, 0x1C0001, 50.0, 8.0, 1, 13)
    b.rec(T0, 0x1C0002, source=S4, msgtype=20, metype=11)  # not an extended squitter: nothing filled in

    def check(snaps, nicrc):
        e = snaps[-1][0x1C0001]
        assert (int(e["nac_p"]), int(e["sil"]), int(e["sil_type"])) == (8, 2, 1)
        assert upd(e, "nac_p") == T0 and upd(e, "sil") == T0
        assert src(snaps[-1][0x1C0002], "nac_p") == 0 and src(snaps[-1][0x1C0002], "sil") == 0
    S["v0_nacp_sil"] = ([None], 0, [b.step()], check)

    # NIC / Rc: every ME type x version x NIC supplement A / B / C.  An operational status sets version, A and C; an even
    # and an odd half of the ME type with B decode globally: both halves carry the same NIC / Rc
    b = B()
    for k, (me, v, na, nb, nc) in enumerate(NIC_CASES):
        a = nic_addr(k)
        b.ops(T0, a, v, acc_valid=4 | 8, nic_a=na, nic_c=nc)
        b.half(T0 + 100, a, 50.0, 8.0, 0, me, nic_b_valid=1, nic_b=nb).half(T0 + 500, a, 50.0, 8.0, 1, me, nic_b_valid=1, nic_b=nb)

    def check(snaps, nicrc):
        assert len(nicrc) == 3 * len(NIC_CASES) and all(tuple(nicrc[3 * k + 2])[2] == 1 for k in range(len(NIC_CASES)))
        got = {c: tuple(int(x) for x in nicrc[3 * k + 2])[:2] for k, c in enumerate(NIC_CASES)}
        # every combination against the table typed from track.c:690-892
        assert sorted(NIC_RC) == [0] + list(range(5, 23))
        for (me, v, na, nb, nc), pair in got.items():
            assert pair == NIC_RC[me][v][4 * na + 2 * nb + nc], (me, v, na, nb, nc)
        # spot values read off track.c:690-892
        assert got[(11, 2, 1, 1, 0)] == (9, 75) and got[(11, 2, 1, 0, 0)] == (8, 186) and got[(11, 1, 1, 0, 0)] == (9, 75)
        assert got[(13, 2, 1, 0, 0)] == (6, 0) and got[(13, 2, 0, 1, 0)] == (6, 556) and got[(13, 1, 1, 0, 0)] == (6, 1112)
        assert got[(8, 2, 0, 0, 1)] == (6, 926) and got[(8, 2, 1, 0, 1)] == (7, 371) and got[(8, 1, 1, 0, 1)] == (0, 0)
        assert got[(16, 0, 1, 1, 0)] == (3, 18520) and got[(16, 2, 1, 0, 0)] == (2, 14816) and got[(7, 2, 1, 0, 1)] == (8, 186)
        assert got[(0, 2, 1, 1, 1)] == (0, 0) and got[(20, 0, 0, 0, 0)] == (11, 8) and got[(17, 1, 0, 0, 0)] == (1, 37040)
        e = snaps[-1][nic_addr(NIC_CASES.index((11, 2, 1, 1, 0)))]
        assert (int(e["nic"]), int(e["rc"]), int(e["cpr_even_nic"]), int(e["cpr_odd_rc"])) == (9, 75, 9, 75)
    S["nic_rc_table"] = ([None], 0, [b.step()], check)

    # a global decode takes the worse half; a decode relative to the aircraft's position takes the minimum of the half's
    # and the stored NIC and of the half's and the stored Rc (track.c:470-473, as written)
    b = B()
    b.half(T0, 0x1D0001, 50.0, 8.0, 0, 11).half(T0 + 400, 0x1D0001, 50.0, 8.0, 1, 13)          # global: (min 8 6, max 186 926)
    b.half(T0 + 11000, 0x1D0001, 50.0, 8.0, 0, 9).half(T0 + 22000, 0x1D0001, 50.0, 8.0, 1, 14)  # local: (6, 8) then (5, 8)

    def check(snaps, nicrc):
        assert [tuple(int(x) for x in r) for r in nicrc] == [(0, 0, 0), (6, 926, 1), (6, 8, 1), (5, 8, 1)]
        e = snaps[-1][0x1D0001]
        assert (int(e["nic"]), int(e["rc"]), int(e["cpr_even_nic"]), int(e["cpr_even_rc"])) == (5, 8, 11, 8)
    S["nic_relative_minimum"] = ([None], 0, [b.step()], check)

    # the derived geometric altitude.  A: baro and delta from ADS-B, no geometric altitude: derived, and the validity is
    # the combination (baro's stale time, 15 s).  B: a fresh ADS-B geometric altitude against a later Mode S baro: not
    # derived; 60 s later the geometric altitude is stale and the later baro and delta win: derived.  C: same sources,
    # baro later than the geometric altitude but the delta earlier: not derived
    b = B()
    sq = dict(crc=0, source=ip.ADSB, msgtype=17)
    b.rec(T0, 0x1E0001, metype=19, geom_delta_valid=1, geom_delta=250).alt(T0 + 100, 0x1E0001, 10000, **sq)
    b.rec(T0, 0x1E0002, metype=20, altitude_geom_valid=1, altitude_geom=9000).rec(T0 + 10, 0x1E0002, metype=19, geom_delta_valid=1, geom_delta=-50)
    for k in range(3):
        b.alt(T0 + 20 + k, 0x1E0002, 10000)
    b.rec(T0, 0x1E0003, metype=19, geom_delta_valid=1, geom_delta=75).rec(T0 + 10, 0x1E0003, metype=20, altitude_geom_valid=1, altitude_geom=9000)
    b.alt(T0 + 20, 0x1E0003, 10000, **sq)
    early = b.step()
    b.rec(T0 + 60010, 0x1E0002, metype=19, geom_delta_valid=1, geom_delta=-50).alt(T0 + 60020, 0x1E0002, 10100)

    def check(snaps, nicrc):
        a, bb, c = snaps[0][0x1E0001], snaps[0][0x1E0002], snaps[0][0x1E0003]
        assert int(a["alt_geom"]) == 10250 and src(a, "altitude_geom") == ip.ADSB and upd(a, "altitude_geom") == T0 + 100
        assert int(a["altitude_geom_stale"]) == T0 + 100 + 15000 and int(a["altitude_geom_expires"]) == T0 + 70000
        assert int(bb["alt_geom"]) == 9000 and int(c["alt_geom"]) == 9000 and upd(c, "altitude_geom") == T0 + 10
        bb = snaps[1][0x1E0002]
        assert int(bb["alt_geom"]) == 10050 and src(bb, "altitude_geom") == S4 and upd(bb, "altitude_geom") == T0 + 60020
    S["derived_geom"] = ([None], 0, [early, b.step()], check)

    # expiry: 70 s after their update squawk and altitude go (and altitude_baro_reliable with the altitude); nac_v,
    # alert, spi and emergency have no EXPIRE line and keep their source
    b = B()
    b.rec(T0, 0x1F0001, squawk_valid=1, squawk=0x1200, nac_v_valid=1, nac_v=2, alert_valid=1, alert=1, spi_valid=1, spi=1,
          emergency_valid=1, emergency=4, altitude_baro_valid=1, altitude_baro=5000)
    b.rec(T0 + 60000, 0x1F0001, category_valid=1, category=0xA3)

    def check(snaps, nicrc):
        e = snaps[1][0x1F0001]
        assert src(e, "squawk") == ip.ADSB and src(e, "altitude_baro") == ip.ADSB and int(e["altitude_baro_reliable"]) == 10
        e = snaps[2][0x1F0001]
        assert src(e, "squawk") == 0 and src(e, "altitude_baro") == 0 and int(e["altitude_baro_reliable"]) == 0
        assert [src(e, k) for k in ("nac_v", "alert", "spi", "emergency")] == [ip.ADSB] * 4
        assert int(e["category"]) == 0xA3 and int(e["squawk"]) == 0x1200
        assert not pkg.capi.aircraft_valid(e, "nac_v", T0 + 70000) and pkg.capi.aircraft_valid(e, "nac_v", T0 + 69999)
    S["expire_asymmetries"] = ([None], 0, [b.step(), ("expire", T0 + 69999), ("expire", T0 + 70000)], check)

    # the signal ring: ten levels above zero and one of zero, which is not stored, wrap at eight
    b = B()
    for k in range(11):
        b.rec(T0 + k, 0x200001, source=S4, msgtype=11, signal=0.0 if k == 4 else 0.01 * (k + 1))

    def check(snaps, nicrc):
        e = snaps[-1][0x200001]
        want = [0.01 * (k + 1) for k in range(11) if k != 4]
        assert [float(x) for x in e["signal_level"]] == [want[8], want[9]] + want[2:8] and int(e["signal_next"]) == 2
        assert int(e["messages"]) == 11
    S["signal_ring"] = ([None], 0, [b.step()], check)

    # ---- accept_data's refusals, member by member (track.c:170-196 with the intervals of :108-143).  Per member five
    # aircraft, each told ADS-B version 2 by an operational status 5 s before (so that no record fills in a version 0
    # NACp / SIL), each with value 0 from ADS-B at T0 and then one record with value 1:
    #   0. from a lesser source 1 s later: refused;   1. at the interval's last millisecond: refused;
    #   2. at its first millisecond outside: accepted;   3. from ADS-B, 1 ms before T0: older than `updated`, refused;
    #   4. from ADS-B 1 s later: accepted.
    # The members of msd_pos_feed ride along (pos_streams.refusal_family): their sources and times are the table's too
    b = B()
    lesser = dict(source=S4, msgtype=20, crc=0x123456)
    for k, (member, stale, fields, values, read) in enumerate(TRK_MEMBERS):
        last, first = trk_refusal_offsets(member, stale)
        for case, (dt, who) in enumerate(((1000, lesser), (last, lesser), (first, lesser), (-1, {}), (1000, {}))):
            a = trk_refusal_addr(k, case)
            b.ops(T0 - 5000, a, 2).rec(T0, a, **fields(values[0])).rec(T0 + dt, a, **fields(values[1]), **who)
    ps.refusal_family(b)

    def check(snaps, nicrc):
        s = snaps[-1]
        for k, (member, stale, fields, values, read) in enumerate(TRK_MEMBERS):
            last, first = trk_refusal_offsets(member, stale)
            assert (last, first) == ((15000, 15001) if member == "altitude_baro" else (14999, 15000) if member in ("squawk", "airground") else (59999, 60000))
            want = [(0, ip.ADSB, 0), (0, ip.ADSB, 0), (1, S4, first), (0, ip.ADSB, 0), (1, ip.ADSB, 1000)]
            for case, (v, source, dt) in enumerate(want):
                e = s[trk_refusal_addr(k, case)]
                assert (read(e), src(e, member), upd(e, member)) == (values[v], source, T0 + dt), (member, case)
        for member in ps.REFUSAL_MEMBERS:
            want = [(0, ip.ADSB, 0), (0, ip.ADSB, 0), (1, S4 if member in POS_MEMBER_VALUES else ip.TISB, 60000), (0, ip.ADSB, 0),
                    (1, ip.ADSB, 1000)]
            for case, (v, source, dt) in enumerate(want):
                e = s[ps.refusal_addr(member, case)]
                assert (src(e, member), upd(e, member)) == (source, T0 + dt), (member, case)
                if member in POS_MEMBER_VALUES:
                    assert int(e[member]) == POS_MEMBER_VALUES[member][v], (member, case)
        # a refused CPR half leaves the NIC / Rc of the half before it: ME type 11 at version 0 is (8, 186), the TIS-B
        # halves' ME type 13 is (6, 926)
        for case, want in enumerate(((8, 186), (8, 186), (6, 926), (8, 186), (8, 186))):
            e = s[ps.refusal_addr("cpr_even", case)]
            assert (int(e["cpr_even_nic"]), int(e["cpr_even_rc"])) == want, case
    S["refusals"] = ([None, dict(ps.HOME, max_range_m=150 * ps.NM)], 0, [b.step()], check)

    # altitude_to_feet (track.c:978-987): metres are divided by 0.3048 in double and truncated towards zero.  381 m are
    # exactly 1250 ft; 235 m and 997 m are 770.9974 and 3270.9974 ft (the fraction 380 / 381, the closest a whole number of
    # metres comes to the next foot from below); 16 777 217 m is not a float: a division in float gives 55 043 360;
    # 654 553 015 m is the largest value whose feet fit an int.  A unit that is neither feet nor metres gives 0
    metric = [(3048, 10000), (381, 1250), (235, 770), (997, 3270), (-235, -770), (-997, -3270), (-1, -3), (-381, -1250),
              (16777217, 55043362), (-16777217, -55043362), (654553015, 2147483645)]
    small = 8  # the barometric altitude gets the first eight: its gate multiplies the jump by 600 in int
    b = B()
    for k, (raw, feet) in enumerate(metric):
        if k < small:
            b.rec(T0, 0x210000 + k, altitude_baro_valid=1, altitude_baro=raw, altitude_baro_unit=1)
        b.rec(T0, 0x218000 + k, altitude_geom_valid=1, altitude_geom=raw, altitude_geom_unit=1)
    b.rec(T0, 0x21F000, altitude_baro_valid=1, altitude_baro=5000, altitude_baro_unit=2, altitude_geom_valid=1,
          altitude_geom=6000, altitude_geom_unit=2)

    def check(snaps, nicrc):
        s = snaps[-1]
        for k, (raw, feet) in enumerate(metric):
            if k < small:
                assert int(s[0x210000 + k]["alt_baro"]) == feet and src(s[0x210000 + k], "altitude_baro") == ip.ADSB, raw
            assert int(s[0x218000 + k]["alt_geom"]) == feet and src(s[0x218000 + k], "altitude_geom") == ip.ADSB, raw
        e = s[0x21F000]
        assert (int(e["alt_baro"]), int(e["alt_geom"]), src(e, "altitude_baro"), src(e, "altitude_geom")) == (0, 0, ip.ADSB, ip.ADSB)
    S["metric_altitudes"] = ([None], 0, [b.step()], check)

    # the version is kept per source (track.c:1032-1054): a TIS-B operational status sets tisb_version, an ADS-R one
    # adsr_version, a Mode S reply none.  The version 0 rule for NACp / SIL looks at the message's source's version: a
    # TIS-B position of ME type 11 fills in NACp 8 while tisb_version is 0 and nothing after a TIS-B version 2 status,
    # whatever adsb_version says
    b = B()
    b.ops(T0, 0x240001, 2, source=ip.TISB, msgtype=18).ops(T0 + 10, 0x240001, 1, source=ip.ADSR, msgtype=18)
    b.half(T0 + 20, 0x240001, 50.0, 8.0, 0, 11, source=ip.TISB, msgtype=18)
    b.ops(T0, 0x240002, 2).half(T0 + 20, 0x240002, 50.0, 8.0, 0, 11, source=ip.TISB, msgtype=18)
    b.rec(T0, 0x240003, source=S4, msgtype=20, crc=0x123456, opstatus=1 | (2 << 1))  # (no reply carries one: the dummy takes it)

    def check(snaps, nicrc):
        e = snaps[-1][0x240001]
        assert [int(e[k]) for k in ("adsb_version", "tisb_version", "adsr_version")] == [-1, 2, 1]
        assert src(e, "nac_p") == 0 and src(e, "sil") == 0
        e = snaps[-1][0x240002]
        assert [int(e[k]) for k in ("adsb_version", "tisb_version", "adsr_version")] == [2, 0, -1]
        assert (src(e, "nac_p"), int(e["nac_p"]), int(e["sil"]), int(e["sil_type"])) == (ip.TISB, 8, 2, 1)
        e = snaps[-1][0x240003]
        assert [int(e[k]) for k in ("adsb_version", "tisb_version", "adsr_version")] == [-1, -1, -1]
    S["version_arms"] = ([None], 0, [b.step()], check)

    # combine_validity with one source only (track.c:200-215: `*to = *from`, the stale interval included).
    # A: the barometric altitude comes from a record without a source (SOURCE_INVALID, with crc 0: reliable 10), the delta
    # from ADS-B 100 ms later: the derived altitude's validity is the delta's, stale after 60 s.
    # B1, B2: the delta expires (source gone, `updated` stays), an ADS-B altitude 100 ms later derives the geometric
    # altitude from it and the old delta: the validity is the altitude's and stale after 15 s; so a geometric altitude from
    # Mode S 14 999 ms later is refused (B1), 15 000 ms later it is accepted, and is itself stale 15 s later (B2)
    b = B()
    b.rec(T0, 0x250001, source=ip.INVALID, altitude_baro_valid=1, altitude_baro=10000)
    b.rec(T0 + 100, 0x250001, metype=19, geom_delta_valid=1, geom_delta=250)
    for a in (0x250002, 0x250003):
        b.rec(T0, a, metype=19, geom_delta_valid=1, geom_delta=-75).rec(T0 + 10, a, category_valid=1, category=0xA3)
    first = b.step()
    for a, dt in ((0x250002, 14999), (0x250003, 15000)):
        b.alt(T0 + 70100, a, 20000, crc=0, source=ip.ADSB, msgtype=17)
        b.rec(T0 + 70100 + dt, a, altitude_geom_valid=1, altitude_geom=5000, **lesser)

    def check(snaps, nicrc):
        e = snaps[0][0x250001]
        assert (src(e, "altitude_baro"), int(e["altitude_baro_reliable"]), int(e["alt_geom"])) == (0, 10, 10250)
        assert (src(e, "altitude_geom"), upd(e, "altitude_geom")) == (ip.ADSB, T0 + 100)
        assert (int(e["altitude_geom_stale"]), int(e["altitude_geom_expires"]), int(e["altitude_geom_stale_15s"])) == (T0 + 60100, T0 + 70100, 0)
        assert src(snaps[1][0x250002], "geom_delta") == 0 and upd(snaps[1][0x250002], "geom_delta") == T0
        e = snaps[2][0x250002]
        assert (int(e["alt_geom"]), src(e, "altitude_geom"), upd(e, "altitude_geom")) == (19925, ip.ADSB, T0 + 70100)
        assert (int(e["altitude_geom_stale"]), int(e["altitude_geom_expires"]), int(e["altitude_geom_stale_15s"])) == (T0 + 85100, T0 + 140100, 1)
        e = snaps[2][0x250003]
        assert (int(e["alt_geom"]), src(e, "altitude_geom"), upd(e, "altitude_geom")) == (5000, S4, T0 + 85100)
        assert (int(e["altitude_geom_stale"]), int(e["altitude_geom_expires"]), int(e["altitude_geom_stale_15s"])) == (T0 + 100100, T0 + 155100, 1)
    S["combine_single_source"] = ([None], 0, [first, ("expire", T0 + 70000), b.step()], check)

    # the gate's remaining arms.  A: crc 0 counts 10 except from MLAT (track.c:1121): 1.  B: an altitude 2^31 ms + 100 s
    # old: (int) trackDataAge is negative there and :1110 takes abs() of its hundredth; the altitude has long expired, so
    # the jump is taken and the reliability starts again at 1
    b = B()
    b.rec(T0, 0x260001, source=ip.MLAT, msgtype=17, crc=0, altitude_baro_valid=1, altitude_baro=10000)
    b.alt(T0, 0x260002, 10000).alt(T0 + (1 << 31) + 100000, 0x260002, 20000)

    def check(snaps, nicrc):
        e = snaps[-1][0x260001]
        assert (int(e["alt_baro"]), int(e["altitude_baro_reliable"]), src(e, "altitude_baro")) == (10000, 1, ip.MLAT)
        e = snaps[-1][0x260002]
        assert (int(e["alt_baro"]), int(e["altitude_baro_reliable"]), upd(e, "altitude_baro")) == (20000, 1, T0 + (1 << 31) + 100000)
    S["baro_gate_arms"] = ([None], 0, [b.step()], check)

    # pos_streams' surface movement codes, seen in the table: the speed kept as gs, valid also where it is 0
    receivers, fp, steps = ps.scenarios(pkg)["surface_movement_codes"]

    def check(snaps, nicrc):
        for k, gs in enumerate(ps.MOVEMENT_GS):
            e = snaps[-1][0x230000 + k]
            assert (int(e["gs"]), src(e, "gs"), upd(e, "gs")) == (gs, ip.ADSB, T0 + 40000), ps.MOVEMENT_CODES[k]
        assert [r[2] for r in nicrc] == [0] * 12 + [0, 1, 0, 1]
    S["surface_movement_codes"] = (receivers, fp, steps, check)

    # pos_streams' reliable_sides: bad data at 3 / 1 takes the position and both counters, at 3 / 2 it leaves 2 / 1
    receivers, fp, steps = ps.scenarios(pkg)["reliable_sides"]

    def check(snaps, nicrc):
        a, bb = snaps[-1][0x410001], snaps[-1][0x410002]
        assert (int(a["pos_reliable_odd"]), int(a["pos_reliable_even"]), src(a, "position")) == (0, 0, 0)
        assert (int(bb["pos_reliable_odd"]), int(bb["pos_reliable_even"]), src(bb, "position")) == (2, 1, ip.ADSB)
        assert src(a, "cpr_odd") == 0 and src(a, "cpr_even") == 0 and src(bb, "cpr_odd") == 0 and src(bb, "cpr_even") == 0
    S["reliable_sides"] = (receivers, fp, steps, check)
    return S


def mixed_stream(pkg, n=2000, seed=11):
    """pos_streams.mixed_stream's 40 aircraft on two receivers, its records dressed as the demodulator's sources dress
    them: squitters with crc 0, altitudes, NIC supplements, rates and geometric deltas, operational status with accuracy
    and HRD / TAH, identification; in between DF4 / 5 / 20 / 21 replies with altitude, squawk, flight status, Comm-B
    registers, and DF11 with nothing but a signal level.  -> (receivers, msgs, fields, receiver)."""
    rng = np.random.default_rng(seed)
    receivers, m, f, r = ps.mixed_stream(pkg, n)
    m, f = m.copy(), f.copy()
    alt = {}
    for i in range(n):
        if m["msgtype"][i] == 32 or f["addr"][i] == 0:
            continue
        a = int(f["addr"][i])
        base = alt.setdefault(a, int(rng.integers(20, 380)) * 100)
        m["signalLevel"][i] = 0.0 if rng.uniform() < 0.05 else rng.uniform(1e-4, 0.5)
        f["addrtype"][i] = int(rng.integers(0, 3))
        u = rng.uniform()
        if m["msgtype"][i] == 17:
            m["crc"][i] = 0
            if f["cpr_valid"][i]:
                f["metype"][i] = int(rng.choice([9, 10, 11, 12, 13, 16, 20])) if f["cpr_type"][i] else int(rng.choice([5, 6, 7, 8]))
                f["nic_b_valid"][i], f["nic_b"][i] = 1, int(rng.integers(0, 2))
                if f["cpr_type"][i]:
                    jump = 4000 if rng.uniform() < 0.05 else int(rng.integers(-2, 3)) * 25
                    f["altitude_baro_valid"][i], f["altitude_baro"][i] = 1, base + jump
                    f["airground"][i] = ia.AG_AIRBORNE if u < 0.8 else ia.AG_UNCERTAIN
                else:
                    f["airground"][i] = ia.AG_GROUND
                    f["heading_valid"][i], f["heading_type"][i], f["heading_raw"][i] = 1, ia.TRACK_OR_HEADING, int(rng.integers(0, 128))
            elif f["velocity_valid"][i]:
                f["baro_rate_valid"][i], f["baro_rate"][i] = int(u < 0.6), int(rng.integers(-30, 30)) * 64
                f["geom_rate_valid"][i], f["geom_rate"][i] = int(u >= 0.5), int(rng.integers(-30, 30)) * 64
                f["geom_delta_valid"][i], f["geom_delta"][i] = 1, int(rng.integers(-20, 20)) * 25
                f["nac_v_valid"][i], f["nac_v"][i] = 1, int(rng.integers(0, 5))
                if u < 0.2:  # subtype 3: airspeed and heading instead of the velocity
                    f["velocity_valid"][i], f["heading_valid"][i] = 0, 1
                    f["heading_type"][i], f["heading_raw"][i] = ia.MAGNETIC_OR_TRUE, int(rng.integers(0, 1024))
            elif f["opstatus"][i]:
                f["opstatus"][i] = int(f["opstatus"][i]) | (int(rng.choice([0, 2, 3])) << 23) | (int(rng.choice([0, 1, 3])) << 26)
                f["acc_valid"][i] = int(rng.integers(0, 64))
                for k in ("nic_a", "nic_c", "nic_baro"):
                    f[k][i] = int(rng.integers(0, 2))
                f["nac_p"][i], f["gva"][i], f["sda"][i] = int(rng.integers(0, 12)), int(rng.integers(0, 4)), int(rng.integers(0, 4))
                f["sil"][i], f["sil_type"][i] = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        elif m["msgtype"][i] == 21:  # the stream's tas / ias replies: DF21 with squawk, flight status and a register
            m["crc"][i] = a & 0xFFFFFF
            f["squawk_valid"][i], f["squawk"][i] = 1, int(rng.choice([0x1200, 0x7000, 0x2345]))
            f["alert_valid"][i], f["alert"][i], f["spi_valid"][i], f["spi"][i] = 1, int(u < 0.1), 1, int(u > 0.95)
            f["airground"][i] = int(rng.choice([ia.AG_AIRBORNE, ia.AG_UNCERTAIN]))
            if u < 0.5:
                f["commb_format"][i], f["commb_valid"][i] = 8, 1 | 4
                f["roll_q"][i], f["track_rate_q"][i] = int(rng.integers(-200, 200)), int(rng.integers(-100, 100))
                f["heading_valid"][i], f["heading_type"][i], f["heading_raw"][i] = 1, ia.GROUND_TRACK, int(rng.integers(0, 2048))
            else:
                f["commb_format"][i], f["commb_valid"][i], f["mach_raw"][i] = 9, 8, int(rng.integers(50, 220))
                f["heading_valid"][i], f["heading_type"][i], f["heading_raw"][i] = 1, ia.MAGNETIC, int(rng.integers(0, 2048))
                f["baro_rate_valid"][i], f["baro_rate"][i] = 1, int(rng.integers(-30, 30)) * 32
        # every tenth record of an aircraft becomes a short reply or an identification instead
        v = rng.uniform()
        if v < 0.04 and not f["cpr_valid"][i]:
            keep = (int(f["addr"][i]), int(f["source"][i]), int(f["addrtype"][i]))
            f[i] = np.zeros((), dtype=f.dtype)
            f["addr"][i], f["addrtype"][i] = keep[0], keep[2]
            kind = int(rng.integers(0, 4))
            if kind == 0:    # DF4: altitude, flight status
                m["msgtype"][i], f["source"][i], m["crc"][i] = 4, S4, a & 0xFFFFFF
                f["altitude_baro_valid"][i], f["altitude_baro"][i] = 1, base + int(rng.integers(-1, 2)) * 100
                f["airground"][i], f["alert_valid"][i], f["spi_valid"][i] = ia.AG_UNCERTAIN, 1, 1
            elif kind == 1:  # DF11: the address, nothing else
                m["msgtype"][i], f["source"][i], m["crc"][i] = 11, ip.MODE_S, 0
                f["airground"][i] = ia.AG_UNCERTAIN
            elif kind == 2:  # DF20 with BDS 4,0
                m["msgtype"][i], f["source"][i], m["crc"][i] = 20, S4, a & 0xFFFFFF
                f["altitude_baro_valid"][i], f["altitude_baro"][i] = 1, base
                f["commb_format"][i], f["nav_valid"][i] = 7, 1 | 4 | 8 | 16 | 64
                f["nav_mcp_altitude"][i], f["nav_fms_altitude"][i], f["nav_qnh_raw"][i] = base, base + 1000, 2132
                f["nav_modes"][i], f["nav_altitude_source"][i] = int(rng.integers(0, 64)), int(rng.integers(0, 5))
            else:            # identification, or target state and status
                m["msgtype"][i], f["source"][i], m["crc"][i] = 17, keep[1], 0
                if rng.uniform() < 0.5:
                    f["metype"][i], f["callsign_valid"][i], f["callsign"][i] = 4, 1, b"FLT%04d " % (a % 10000)
                    f["category_valid"][i], f["category"][i] = 1, 0xA0 + int(rng.integers(1, 6))
                else:
                    f["metype"][i], f["mesub"][i], f["nav_valid"][i] = 29, 1, 2 | 32 | 4 | 16
                    f["nav_heading_raw"][i], f["nav_mcp_altitude"][i], f["nav_qnh_raw"][i] = int(rng.integers(0, 512)), base, 267
                    f["emergency_valid"][i], f["emergency"][i] = 1, int(rng.integers(0, 2))
                    f["acc_valid"][i], f["nac_p"][i], f["nic_baro"][i] = 1 | 2, int(rng.integers(0, 12)), 1
                    f["sil"][i], f["sil_type"][i] = int(rng.integers(0, 4)), int(rng.choice([1, 2, 3]))
    return receivers, m, f, r


RANDOM_SEED = 3  # chosen on the CPU (profiles/tracker_stream_coverage.md): the second reading alone meets RANDOM_MIN there
RANDOM_MIN = 20  # accepted and refused updates of every member
# record index -> times its position was drawn again, as settle_random_stream found them for RANDOM_SEED
RANDOM_DRAWS = {
    **dict.fromkeys([59, 90, 150, 170, 216, 267, 292, 335, 339, 350, 357, 363, 376, 450, 469, 474, 494, 496, 499, 511, 520, 543, 619,
                     632, 645, 721, 728, 739, 740, 750, 782, 797, 808, 812, 880, 902, 949, 954, 957, 1007, 1008, 1048, 1061, 1071,
                     1079, 1084, 1087, 1098, 1101, 1106, 1120, 1184, 1218, 1225, 1237, 1240, 1295, 1301, 1313, 1316, 1334, 1343,
                     1364, 1425, 1435, 1457, 1485, 1492, 1503, 1561, 1573, 1575, 1593, 1594, 1598, 1605, 1610, 1626, 1655, 1659,
                     1674, 1730, 1756, 1758, 1762, 1780, 1787, 1796, 1809, 1816, 1847, 1862, 1870, 1880, 1881, 1899, 1905, 1916,
                     1919, 1945, 1947, 1955, 1967, 1976, 1982, 1994, 2026, 2060, 2061, 2084, 2102, 2105, 2111, 2117, 2125, 2137,
                     2144, 2146, 2148, 2156, 2162, 2175, 2206, 2215, 2224, 2256, 2301, 2306, 2327, 2335, 2394, 2398, 2405, 2443,
                     2449, 2459, 2470, 2473, 2488, 2491, 2501, 2503, 2505, 2516, 2532, 2547, 2563, 2609, 2617, 2618, 2632, 2667,
                     2703, 2715, 2719, 2742, 2777, 2780, 2830, 2843, 2861, 2873, 2879, 2891, 2895, 2900, 2905, 2910, 2911, 2915,
                     2927, 2959, 2961, 2975, 2980, 2981, 3024, 3036, 3065, 3067, 3081, 3082, 3093, 3094, 3119, 3133, 3141, 3206,
                     3210, 3236, 3312, 3323, 3401, 3404, 3414, 3418, 3420, 3461, 3466, 3483, 3495, 3501, 3508, 3525, 3572, 3583,
                     3605, 3632, 3634, 3641, 3642, 3657, 3662, 3702, 3753, 3760, 3765, 3774, 3796, 3800, 3802, 3815, 3823, 3865,
                     3866, 3871, 3904, 3919], 1),
    **dict.fromkeys([96, 158, 206, 285, 354, 355, 464, 608, 629, 847, 874, 914, 1038, 1133, 1233, 1276, 1354, 1484, 1532, 1744, 1818,
                     1876, 1933, 1934, 2028, 2071, 2075, 2138, 2159, 2316, 2389, 2446, 2663, 2720, 2982, 3030, 3204, 3334, 3335,
                     3352, 3408, 3415, 3547, 3579, 3633, 3710, 3733, 3817, 3944], 2),
    **dict.fromkeys([642, 770, 1291, 1791, 1852, 2237, 2985, 3054, 3281, 3790, 3867], 3),
    **dict.fromkeys([103, 517, 519, 687, 1180, 2140, 2172, 3274, 3342], 4),
    **dict.fromkeys([3302], 5),
}
RANDOM_SQUAWKS = (0x1200, 0x7000, 0x2345)
AIS = b"@ABCDEFGHIJKLMNOPQRSTUVWXYZ[\\]^_ !\"#$%&'()*+,-./0123456789:;<=>?"  # the 64 characters a callsign can carry
# the reference's arithmetic is undefined beyond these (int overflow in the gate's delta * 600, (int) of a double past
# INT_MAX in altitude_to_feet): a drawn altitude stays inside, everything else takes the whole range of its type
BARO_FEET_MAX, BARO_METRES_MAX, GEOM_METRES_MAX = 1_700_000, 518_000, 654_553_015


def random_stream(pkg, n=4000, seed=RANDOM_SEED, draws=None):
    """A drawn stream for the whole tracker stack: the flights of pos_streams.mixed_stream -- 48 aircraft on three
    receivers, their CPR halves, velocities and surface movements, plausible so that the device's libm and the host's
    decide every gate alike -- and everything else of a record drawn independently of everything else: which members it
    carries, their values over the whole range of their types (altitudes: as far as the reference's arithmetic is
    defined), the message type, the crc, the source (three in five keep the flight's ADS-B or TIS-B, the others take any
    of the eight).  One record in ten carries a time up to 90 s behind the stream's; one in twelve is a Mode A/C reply on
    one of three codes that half of the drawn squawks use too; DF11 and address 0 are mixed in.
    draws: {record index: times drawn again} for the positions that settle_random_stream moved by a few metres because
    a range, a bearing or a gate came closer to a limit than range_streams' margins (default: RANDOM_DRAWS, the seed's).
    -> (receivers, msgs, fields, receiver), in stream order."""
    rng = np.random.default_rng(seed)
    draws = RANDOM_DRAWS if draws is None else draws

    def jitter(i):  # 22 m at most, times how often the record has been drawn (far out a bearing needs more to leave an edge)
        return tuple(draws[i] * np.random.default_rng([seed, i, draws[i]]).uniform(-2e-4, 2e-4, 2)) if i in draws else (0.0, 0.0)

    receivers, m, f, r = ps.mixed_stream(pkg, n, seed=seed, aircraft=48, third_receiver=True, jitter=jitter)
    m, f = m.copy(), f.copy()
    u1 = lambda: int(rng.integers(0, 256))          # noqa: E731
    u2 = lambda: int(rng.integers(0, 1 << 16))      # noqa: E731
    i2 = lambda: int(rng.integers(-1 << 15, 1 << 15))  # noqa: E731
    i4 = lambda: int(rng.integers(-1 << 31, 1 << 31))  # noqa: E731
    p = lambda x: rng.uniform() < x                 # noqa: E731
    base = {}
    for i in range(n):
        if p(1 / 12) and not f["cpr_valid"][i]:     # a Mode A/C reply, as msd_fields_mode_ac leaves it
            code = int(rng.choice(RANDOM_SQUAWKS))
            rx = int(r[i])
            f[i] = np.zeros((), dtype=f.dtype)
            m["msgtype"][i], m["msgbits"][i], m["addr"][i] = 32, 16, code
            f["addr"][i], f["source"][i], f["squawk_valid"][i], f["squawk"][i] = code | (1 << 24), ip.MODE_AC, 1, code
            r[i] = rx
            continue
        if m["msgtype"][i] == 32 or f["addr"][i] == 0:
            continue
        a = int(f["addr"][i])
        feet = base.setdefault(a, int(rng.integers(-10, 450)) * 100)
        if p(0.1):
            m["sysTimestampMsg"][i] -= int(rng.integers(1, 90001))
        if p(0.4):
            f["source"][i] = int(rng.integers(0, 8))
        if not f["cpr_valid"][i] and p(0.3):
            m["msgtype"][i] = int(rng.choice([4, 5, 11, 11, 17, 18, 20, 21]))
        m["crc"][i] = 0 if p(0.5) else int(rng.integers(1, 1 << 24))
        m["iid"][i], m["correctedbits"][i] = int(rng.choice([0, 0, 0, 5])), int(rng.choice([0, 0, 1, 2]))
        m["signalLevel"][i] = 0.0 if p(0.05) else rng.uniform(1e-4, 0.5)
        f["addrtype"][i] = u1()
        f["metype"][i] = (int(rng.integers(5, 23)) if p(0.7) else u1()) if f["cpr_valid"][i] or p(0.5) else f["metype"][i]
        if f["cpr_valid"][i]:
            f["nic_b_valid"][i], f["nic_b"][i] = int(p(0.7)), u1()
        if p(0.08):
            f["opstatus"][i] = int(rng.integers(0, 1 << 32)) | 1
        if p(0.3):
            unit = 0 if p(0.85) else 1 if p(0.7) else u1()
            top = BARO_METRES_MAX if unit == 1 else BARO_FEET_MAX
            value = int(rng.integers(-top, top + 1)) if p(0.3) else (feet + int(rng.integers(-12, 13)) * 25) * (3 if unit == 1 else 10) // 10
            f["altitude_baro_valid"][i], f["altitude_baro_unit"][i], f["altitude_baro"][i] = 1, unit, value
        if p(0.2):
            unit = 0 if p(0.85) else 1 if p(0.7) else u1()
            value = int(rng.integers(-GEOM_METRES_MAX, GEOM_METRES_MAX + 1)) if unit == 1 else i4()
            f["altitude_geom_valid"][i], f["altitude_geom_unit"][i], f["altitude_geom"][i] = 1, unit, value
        f["geom_delta_valid"][i], f["geom_delta"][i] = int(p(0.2)), i2()
        f["baro_rate_valid"][i], f["baro_rate"][i] = int(p(0.2)), i2()
        f["geom_rate_valid"][i], f["geom_rate"][i] = int(p(0.2)), i2()
        f["squawk_valid"][i], f["squawk"][i] = int(p(0.25)), int(rng.choice(RANDOM_SQUAWKS)) if p(0.5) else u2()
        f["emergency_valid"][i], f["emergency"][i] = int(p(0.15)), u1()
        f["heading_type"][i] = int(rng.integers(0, 6)) if p(0.85) else u1()
        f["commb_format"][i] = int(rng.choice([0, 7, 8, 9])) if p(0.8) else u1()
        # a heading has the bits its message carries (the text writers print no others): 11 in BDS 5,0 / 6,0, 10 in an
        # airborne velocity, 7 in a surface position
        bits = 11 if f["commb_format"][i] in (8, 9) else 10 if f["metype"][i] == 19 else 7
        f["heading_valid"][i], f["heading_raw"][i] = int(p(0.3)), u2() & ((1 << bits) - 1)
        f["commb_valid"][i] = (1 * p(0.15)) | (2 * p(0.05)) | (4 * p(0.15)) | (8 * p(0.15))
        f["roll_q"][i], f["track_rate_q"][i], f["mach_raw"][i], f["gs"][i] = i2(), i2(), u2(), u2()
        f["ias_valid"][i], f["ias"][i], f["tas_valid"][i], f["tas"][i] = int(p(0.1)), u2(), int(p(0.1)), u2()
        f["airground"][i] = int(rng.integers(0, 4)) if p(0.8) else u1()
        if p(0.15):
            f["callsign_valid"][i], f["callsign"][i] = 1, bytes(AIS[int(k)] for k in rng.integers(0, 64, 8))
        f["category_valid"][i], f["category"][i] = int(p(0.1)), u1()
        f["nav_valid"][i], f["nav_modes"][i], f["nav_heading_raw"][i], f["nav_qnh_raw"][i] = u1() if p(0.2) else 0, u1(), u2(), u2()
        f["nav_mcp_altitude"][i], f["nav_fms_altitude"][i] = i4(), i4()
        f["nav_altitude_source"][i] = u1() if p(0.15) else 0
        f["alert_valid"][i], f["alert"][i] = int(p(0.15)), int(p(0.5)) if p(0.8) else u1()
        f["spi_valid"][i], f["spi"][i] = int(p(0.15)), int(p(0.5)) if p(0.8) else u1()
        f["acc_valid"][i] = u1() if p(0.25) else 0
        for k in ("nac_p", "nic_baro", "nic_a", "nic_c", "gva", "sda", "sil", "nac_v"):
            f[k][i] = u1()
        f["nac_v_valid"][i] = int(p(0.15))
        f["sil_type"][i] = (int(rng.integers(1, 4)) if p(0.8) else u1()) if p(0.2) else 0
    return receivers, m, f, r


def settle_random_stream(pkg, n=4000, seed=RANDOM_SEED, rounds=100):
    """-> the draws with which the second reading of the range keeps range_streams' margins over whole_stack.steps_of's
    steps (what RANDOM_DRAWS records for RANDOM_SEED).  Not run by the tests: they assert the margins."""
    import indep_range as ir
    import range_streams as rs
    import whole_stack as ws
    draws = {}
    for _ in range(rounds):
        receivers, m, f, r = random_stream(pkg, n, seed, draws)
        t = ir.RangeTracker(receivers, 8, polar=True)
        rs.run(t, [s for s in ws.steps_of(m, f, r)[0] if s[0] != "match"])
        close = [k for k, (rm, bm, gm) in t.by_record.items() if rm < 2 * rs.RANGE_MARGIN or bm < 2 * rs.BEARING_MARGIN or gm < 2 * rs.GATE_MARGIN]
        if not close:
            return draws
        for k in close:
            draws[k] = draws.get(k, 0) + 1
    raise AssertionError("no draw keeps the margins")


class Counting(im.Tracker):
    """The second reading of the table with Mode A/C matching, counting accept_data's verdicts per member."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.accepted, self.refused = {}, {}

    def feed(self, a, rx, m, f):
        for k, d in a.v.items():  # (combine_validity's `*to = *from` copies a name along: put them back)
            d.name = k
        return super().feed(a, rx, m, f)

    def accept(self, d, source):
        ok = super().accept(d, source)
        tally = self.accepted if ok else self.refused
        tally[d.name] = tally.get(d.name, 0) + 1
        return ok


def wide_stream(pkg, aircraft, records, receivers=1, skipped_every=0, replies=False):
    """pos_streams.wide_stream with what the table reads: squitters with crc 0 and a signal level, a barometric altitude
    that climbs 25 ft per record with a 5000 ft jump every 97th record of the stream, ME types 9 to 13 and the NIC
    supplement B by aircraft, air / ground.  replies: of every ten records of the stream one each becomes a DF4 (altitude),
    DF5 (squawk), DF11, DF20 (altitude, BDS 5,0) and DF21 (squawk, BDS 6,0) reply of the same aircraft, so that half the
    stream is squitters (every fifth one an airborne velocity instead of a position) and half is replies.  No Python loop
    over the records."""
    rx, m, f, r = ps.wide_stream(pkg, aircraft, records, receivers, skipped_every)
    i = np.arange(records)
    a, k = i % aircraft, i // aircraft
    on = f["cpr_valid"] == 1
    m["signalLevel"] = np.where(i % 5 == 0, 0.0, 1e-3 * (1 + i % 89))
    f["metype"] = np.where(on, 9 + (a + k // 7) % 5, 0)
    f["nic_b_valid"], f["nic_b"] = on, on & (a % 2 == 1)
    f["altitude_baro_valid"] = on
    f["altitude_baro"] = np.where(on, 5000 + 25 * k + np.where(i % 97 == 0, 5000, 0), 0)
    f["airground"] = np.where(on, np.where(i % 11 == 0, 3, 2), 0)
    if replies:
        kind = (k + 3 * a) % 10  # 0..4 squitters, 5 DF4, 6 DF5, 7 DF11, 8 DF20, 9 DF21
        reply = on & (kind >= 5)
        vel = on & (kind == 4)
        for name in ("cpr_valid", "cpr_type", "cpr_odd", "cpr_lat", "cpr_lon", "nic_b_valid", "nic_b"):
            f[name][reply | vel] = 0
        f["metype"][reply] = 0
        f["metype"][vel], f["velocity_valid"][vel], f["altitude_baro_valid"][vel], f["altitude_baro"][vel] = 19, 1, 0, 0
        f["ew_vel"][vel], f["ns_vel"][vel] = (100 + a % 300)[vel], (200 - a % 400)[vel]
        f["baro_rate_valid"][vel], f["baro_rate"][vel], f["geom_delta_valid"][vel], f["geom_delta"][vel] = 1, 1500, 1, 125
        m["msgtype"][reply] = np.array([4, 5, 11, 20, 21])[kind[reply] - 5]
        m["crc"][reply & (kind != 7)] = (0x100000 + a)[reply & (kind != 7)]
        f["source"][reply] = np.where(kind[reply] == 7, ip.MODE_S, S4)
        f["airground"][reply] = 3
        squawk, noalt = reply & ((kind == 6) | (kind == 9)), reply & ((kind == 6) | (kind == 7) | (kind == 9))
        f["altitude_baro_valid"][noalt], f["altitude_baro"][noalt] = 0, 0
        f["squawk_valid"][squawk], f["squawk"][squawk] = 1, (0x1000 + (a & 0x777))[squawk]
        f["alert_valid"][reply & (kind != 7)], f["spi_valid"][reply & (kind != 7)] = 1, 1
        b50, b60 = reply & (kind == 8), reply & (kind == 9)
        f["commb_format"][b50], f["commb_valid"][b50], f["roll_q"][b50], f["track_rate_q"][b50] = 8, 1 | 4, -37, 12
        f["heading_valid"][b50], f["heading_type"][b50], f["heading_raw"][b50] = 1, ia.GROUND_TRACK, (a % 2048)[b50]
        f["tas_valid"][b50], f["tas"][b50] = 1, 420
        f["commb_format"][b60], f["commb_valid"][b60], f["mach_raw"][b60] = 9, 8, 190
        f["heading_valid"][b60], f["heading_type"][b60], f["heading_raw"][b60] = 1, ia.MAGNETIC, (a % 2048)[b60]
        f["ias_valid"][b60], f["ias"][b60] = 1, 280
    return rx, m, f, r


# ---- runners -------------------------------------------------------------------------------------------------------
def by_addr(snap):
    return {int(e["addr"]) | (int(e["receiver"]) << 32): e for e in snap}


def run_library(tracker, steps, pieces=None, every_step=True):
    """steps through a table capi.PositionTracker -> (POSITION_DTYPE rows, NICRC_DTYPE rows, [snapshot after each step])"""
    rows, nic, snaps = [], [], []
    for s in steps:
        if s[0] == "expire":
            tracker.expire(s[1])
        else:
            _, m, f, r = s
            k = pieces or max(len(m), 1)
            for i in range(0, len(m), k):
                o, q = tracker.update_nicrc(m[i:i + k], f[i:i + k], r[i:i + k])
                rows.append(o), nic.append(q)
        if every_step:
            snaps.append(tracker.snapshot())
    if not every_step:
        snaps.append(tracker.snapshot())
    return np.concatenate(rows), np.concatenate(nic), snaps


def run_model(pkg, receivers, filter_persistence, steps):
    """-> (rows, nicrc, [snapshot dicts after each step]) from the second reading"""
    t = ia.Tracker(receivers, filter_persistence or 8)
    rows, nic, snaps = [], [], []
    for s in steps:
        if s[0] == "expire":
            t.expire(s[1])
        else:
            o, q = t.update(s[1], s[2], s[3])
            rows += o
            nic += q
        snaps.append(t.snapshot(pkg.capi.AC_MEMBERS))
    return rows, nic, snaps


def entry_as_dict(e):
    """an AIRCRAFT_DTYPE entry under the second reading's names and value types"""
    d = {}
    for k in e.dtype.names:
        if k == "pad":
            assert not e[k].any()
        elif k in ("track", "mag_heading", "true_heading"):
            assert int(e[k]["pad"]) == 0
            d[k] = (int(e[k]["kind"]), int(e[k]["raw"]), int(e[k]["ew"]), int(e[k]["ns"]))
        elif k in ("updated", "source"):
            d[k] = [int(x) for x in e[k]]
        elif k == "signal_level":
            d[k] = [float(x) for x in e[k]]
        elif k == "callsign":
            d[k] = bytes(e[k])
        elif k in ("lat", "lon"):
            d[k] = float(e[k])
        else:
            d[k] = int(e[k])
    return d


def differences(snap, model):
    """field by field: [(addr, member, library, second reading)]"""
    out = []
    if len(snap) != len(model):
        return [("aircraft", len(snap), len(model))]
    for e, w in zip(snap, model):
        g = entry_as_dict(e)
        assert set(g) == set(w), set(g) ^ set(w)
        out += [(hex(w["addr"]), k, g[k], w[k]) for k in g if g[k] != w[k]]
    return out
