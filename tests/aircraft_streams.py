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
         "v0_nacp_sil", "nic_rc_table", "nic_relative_minimum", "derived_geom", "expire_asymmetries", "signal_ring"]
NIC_CASES = [(me, v, a, b, c) for me in [0] + list(range(5, 23)) for v in (0, 1, 2) for a in (0, 1) for b in (0, 1) for c in (0, 1)]


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
