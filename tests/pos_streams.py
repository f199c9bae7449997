"""Constructed record streams for the position tracker's tests (test_positions_model.py on the CPU,
test_gpu_positions.py on the GPU): a builder that writes msd_message / msd_fields rows the way the field decoder would
have left them, the named scenarios of the issue, a 2000-record mixed stream, and runners for the three
implementations (the GPU object, the host twin, the second reading of tests/indep_positions.py).  For the machinery
around the per-record logic (tests/test_gpu_positions_machinery.py): wide_stream, a vectorised stream of any length, and
chain_scenario, five aircraft in one probe chain that runs across the end of the table.

A scenario is (receivers, filter_persistence, steps); a step is ("update", msgs, fields, receiver) or ("expire", now_ms).
Every scenario keeps every plausibility gate at least 1 m from its limit (asserted on the twin by the tests)."""
import numpy as np

import indep_positions as ip

T0 = 1_600_000_000_000  # ms: a wall clock, as readsb's sysTimestampMsg is
NM = 1852.0
HOME = dict(lat=52.0, lon=4.0, latlon_valid=1)


class Builder:
    def __init__(self, pkg):
        self.pkg, self.m, self.f, self.r = pkg, [], [], []

    def rec(self, t, addr, rx=0, source=ip.ADSB, msgtype=17, **kw):
        m = np.zeros((), dtype=self.pkg.capi.MESSAGE_DTYPE)
        f = np.zeros((), dtype=self.pkg.capi.FIELDS_DTYPE)
        m["sysTimestampMsg"], m["msgtype"], m["addr"], m["msgbits"] = t, msgtype, addr & 0xFFFFFF, 112
        f["addr"], f["source"] = addr, source
        for k, v in kw.items():
            f[k] = v
        self.m.append(m), self.f.append(f), self.r.append(rx)
        return self

    def pos(self, t, addr, lat, lon, odd, surface=False, movement=0, **kw):
        y, x = ip.cpr_encode(lat, lon, odd, surface)
        return self.rec(t, addr, cpr_valid=1, cpr_type=0 if surface else 1, cpr_odd=odd, cpr_lat=y, cpr_lon=x,
                        movement=movement, metype=7 if surface else 11, **kw)

    def raw(self, t, addr, y, x, odd, **kw):
        return self.rec(t, addr, cpr_valid=1, cpr_type=1, cpr_odd=odd, cpr_lat=y, cpr_lon=x, metype=11, **kw)

    def vel(self, t, addr, ew, ns, **kw):
        return self.rec(t, addr, velocity_valid=1, ew_vel=ew, ns_vel=ns, metype=19, **kw)

    def opstatus(self, t, addr, version, **kw):
        return self.rec(t, addr, opstatus=1 | (version << 1), metype=31, **kw)

    def step(self):
        out = ("update", np.array(self.m, dtype=self.pkg.capi.MESSAGE_DTYPE), np.array(self.f, dtype=self.pkg.capi.FIELDS_DTYPE),
               np.array(self.r, dtype=np.uint32))
        self.m, self.f, self.r = [], [], []
        return out


def scenarios(pkg):
    S = {}
    B = lambda: Builder(pkg)  # noqa: E731

    # even / odd pair inside and just outside 10 s (no receiver location: the late half decodes nothing)
    b = B()
    b.pos(T0, 0x100001, 51.5, 3.5, 0).pos(T0 + 10000, 0x100001, 51.5, 3.5, 1)
    b.pos(T0, 0x100002, 51.5, 3.5, 0).pos(T0 + 10001, 0x100002, 51.5, 3.5, 1)
    S["pair_10s"] = ([None], 0, [b.step()])

    # the same with the demodulator's clock, which starts at 0: position_valid.updated == 0 is then "recent" and the
    # unpaired half is tried relative to (0, 0) (track.c:466)
    b = B()
    b.pos(1000, 0x100003, 0.3, 0.4, 0).pos(12000, 0x100003, 0.3, 0.4, 1).pos(13000, 0x100004, 51.5, 3.5, 0)
    S["clock_from_zero"] = ([None], 0, [b.step()])

    # surface: 25 s with gs > 25 kt or unknown, 50 s with gs <= 25 kt (movement 48 = 24.5 kt, 49 = 25.5 kt)
    b = B()
    for k, (gap, mov) in enumerate(((25000, 49), (25001, 49), (50000, 48), (50001, 48), (25001, 0), (25000, 0))):
        a = 0x200000 + k
        b.pos(T0, a, 52.3, 4.76, 0, surface=True, movement=mov).pos(T0 + gap, a, 52.3, 4.76, 1, surface=True, movement=mov)
    S["surface_windows"] = ([HOME], 0, [b.step()])

    # surface movement read by version: 3 is 0.1875 kt as v0 and 0.1979 kt as v2 -- both slow; and a surface pair
    # without any reference
    b = B()
    b.opstatus(T0, 0x210000, 2).pos(T0 + 100, 0x210000, 52.3, 4.76, 0, surface=True, movement=3)
    b.pos(T0 + 40000, 0x210000, 52.3, 4.76, 1, surface=True, movement=3)
    b.pos(T0, 0x210001, 52.3, 4.76, 0, surface=True, rx=1).pos(T0 + 1000, 0x210001, 52.3, 4.76, 1, surface=True, rx=1)
    S["surface_version_and_no_reference"] = ([HOME, None], 0, [b.step()])

    # type mismatch between the halves; source mismatch (ADS-B against TIS-B)
    b = B()
    b.pos(T0, 0x300001, 52.3, 4.76, 0).pos(T0 + 500, 0x300001, 52.3, 4.76, 1, surface=True)
    b.pos(T0, 0x300002, 52.3, 4.76, 0).pos(T0 + 500, 0x300002, 52.3, 4.76, 1, source=ip.TISB)
    b.pos(T0 + 900, 0x300002, 52.3, 4.76, 0, source=ip.TISB)      # a lesser source while ADS-B is fresh: not accepted
    b.pos(T0 + 60000, 0x300002, 52.3, 4.76, 0, source=ip.TISB)    # stale by now: accepted, but 59.5 s from its odd half
    b.pos(T0 + 60400, 0x300002, 52.3, 4.76, 1, source=ip.TISB)    # both TIS-B: global
    S["type_and_source_mismatch"] = ([None], 0, [b.step()])

    # global failure -> pos_reliable decrement -> position invalidated; with more good pairs first it survives one
    b = B()
    for a, good in ((0x400001, 1), (0x400002, 4)):
        t = T0
        for k in range(good):
            b.pos(t, a, 50.0 + 0.001 * k, 8.0, 0).pos(t + 400, a, 50.0 + 0.001 * k, 8.0, 1)
            t += 1000
        b.pos(t, a, 40.0, 20.0, 0).pos(t + 400, a, 40.0, 20.0, 1)       # implausible: both halves dropped
        b.pos(t + 12000, a, 50.01, 8.0, 0).pos(t + 12400, a, 50.01, 8.0, 1)  # the bad odd half is 11.6 s old by now
    S["global_failure"] = ([None], 3, [b.step()])

    # local, relative to the aircraft's last position, within 10 minutes and after them
    b = B()
    b.pos(T0, 0x500001, 48.0, 11.0, 0).pos(T0 + 500, 0x500001, 48.0, 11.0, 1)
    b.pos(T0 + 30000, 0x500001, 48.05, 11.05, 0).pos(T0 + 300000, 0x500001, 48.4, 11.4, 1)
    b.pos(T0 + 300000 + 599999, 0x500001, 48.5, 11.5, 0).pos(T0 + 1600000, 0x500001, 48.6, 11.6, 1)
    S["aircraft_relative"] = ([None], 0, [b.step()])

    # receiver-relative for each --max-range branch: 0, <= 180 NM, between, >= 360 NM; inside and outside the limit
    rx = [dict(HOME, max_range_m=0.0), dict(HOME, max_range_m=150 * NM), dict(HOME, max_range_m=250 * NM),
          dict(HOME, max_range_m=400 * NM)]
    b = B()
    for r in range(4):
        b.pos(T0, 0x600000 + r, 52.5, 5.0, 0, rx=r)       # about 40 NM away
        b.pos(T0, 0x610000 + r, 52.0, 7.5, 1, rx=r)       # about 129 NM: outside 360 - 250 = 110 NM
        b.pos(T0, 0x620000 + r, 53.0, 9.0, 0, rx=r).pos(T0 + 300, 0x620000 + r, 53.0, 9.0, 1, rx=r)  # global, 190 NM
    S["receiver_relative"] = (rx, 0, [b.step()])

    # speed check with gs, tas, ias and none: a jump of about 5.6 km in 10 s passes at 700 kt (none) and fails at
    # 100 kt; the odd half is 10.1 s old by then, so only the local decode is tried
    b = B()
    for k, kw in enumerate((dict(), dict(velocity_valid=1, ew_vel=60, ns_vel=80), dict(tas_valid=1, tas=100),
                            dict(ias_valid=1, ias=80), dict(velocity_valid=1, ew_vel=600, ns_vel=800))):
        a = 0x700000 + k
        b.pos(T0, a, 45.0, 9.0, 0).pos(T0 + 500, a, 45.0, 9.0, 1)
        if kw:
            b.rec(T0 + 600, a, metype=19, **kw)
        b.pos(T0 + 10600, a, 45.05, 9.0, 0)
        b.pos(T0 + 11100, a, 45.05, 9.0, 1)   # the global decode of the new pair meets the same check
    S["speed_check"] = ([None], 0, [b.step()])

    # timestamps running backwards: every member has its own `updated`, so an older odd half is accepted while the odd
    # member is new, an older even half is not, and a good global decode older than the position is skipped (-2)
    b = B()
    b.pos(T0 + 5000, 0x800001, 47.0, 8.0, 0).pos(T0 + 4000, 0x800001, 47.0, 8.0, 1).pos(T0 + 3000, 0x800001, 47.0, 8.0, 0)
    b.pos(T0 + 5500, 0x800001, 47.0, 8.0, 1).pos(T0 + 5200, 0x800001, 47.001, 8.0, 0)
    S["backwards"] = ([None], 0, [b.step()])

    # expiry and TTL: a one-message aircraft goes after 60 s, the others after 10 minutes; a position expires after
    # 70 s and takes pos_reliable with it; Mode A/C records and address 0 are skipped
    steps = []
    b = B()
    b.pos(T0, 0x900001, 47.0, 8.0, 0).pos(T0 + 300, 0x900001, 47.0, 8.0, 1).pos(T0, 0x900002, 47.0, 8.0, 0)
    b.rec(T0, 0x001234, msgtype=32, source=ip.MODE_AC).rec(T0, 0, msgtype=11, source=ip.MODE_S)
    steps += [b.step(), ("expire", T0 + 60000), ("expire", T0 + 60001), ("expire", T0 + 70300)]
    b.pos(T0 + 80000, 0x900001, 47.2, 8.2, 0).pos(T0 + 80400, 0x900001, 47.2, 8.2, 1).pos(T0 + 80500, 0x900002, 47.0, 8.0, 1)
    steps += [b.step(), ("expire", T0 + 80400 + 600000), ("expire", T0 + 80400 + 600001), ("expire", T0 + 80500 + 600001)]
    b.pos(T0 + 900000, 0x900001, 47.2, 8.2, 0)
    steps += [b.step()]
    S["expiry_and_ttl"] = ([None], 0, steps)

    # accept_data's refusals for the six members msd_pos_feed accepts (refusal_family below)
    b = B()
    refusal_family(b)
    S["refusals"] = ([None, dict(HOME, max_range_m=150 * NM)], 0, [b.step()])

    # the speed check of a surface target.  Without any valid speed: 100 kt x 4 / 3 = 133 kt = 68.42 m/s; the position
    # is 30 s old, so the limit is 100 m + 31 s x 68.42 m/s = 2221 m: 1800 m north passes, 2350 m fails (with the
    # airborne default of 700 kt, clamped to the surface's 150 kt, the limit were 2492 m and it would pass).  With gs
    # valid -- movement 48 is 24.5 kt, stored as 24 --: 24 x 4 / 3 = 32 kt = 16.46 m/s, the position is 60 s old (the
    # pairing window of a slow target is 50 s): 100 m + 61 s x 16.46 m/s = 1104 m: 850 m passes, 1350 m fails
    b = B()
    for k, (mov, gap, north) in enumerate(((0, 30000, 1800.0), (0, 30000, 2350.0), (48, 60000, 850.0), (48, 60000, 1350.0))):
        a = 0x220000 + k
        b.pos(T0, a, 52.3, 4.76, 0, surface=True, movement=mov).pos(T0 + 400, a, 52.3, 4.76, 1, surface=True, movement=mov)
        b.pos(T0 + 400 + gap, a, 52.3 + north / M_PER_DEG, 4.76, 0, surface=True, movement=mov)
    S["surface_speed_check"] = ([HOME], 0, [b.step()])

    # the surface movement codes at the steps of the table's upper half (mode_s.c:216-259): 93 is 69.5 kt, 94 71 kt,
    # 108 99 kt, 109 102.5 kt, 123 172.5 kt, 124 180 kt, 125 and 127 are 0 kt ("reserved") -- and 0 kt is a valid speed
    # of at most 25 kt, so those two pair their halves across 40 s and the others do not
    b = B()
    for k, mov in enumerate(MOVEMENT_CODES):
        a = 0x230000 + k
        b.pos(T0, a, 52.3, 4.76, 0, surface=True, movement=mov).pos(T0 + 40000, a, 52.3, 4.76, 1, surface=True, movement=mov)
    S["surface_movement_codes"] = ([HOME], 0, [b.step()])

    # --max-range in the global decode: without a receiver location the limit is not applied (receiver 0); with one a
    # pair 190 NM away is bad data and one 40 NM away is not (receiver 1; there single halves are tried relative to the
    # receiver, within 100 NM: the far one fails, the near one decodes)
    b = B()
    b.pos(T0, 0x630000, 53.0, 9.0, 0, rx=0).pos(T0 + 300, 0x630000, 53.0, 9.0, 1, rx=0)
    b.pos(T0, 0x630001, 53.0, 9.0, 0, rx=1).pos(T0 + 300, 0x630001, 53.0, 9.0, 1, rx=1)
    b.pos(T0, 0x630002, 52.5, 5.0, 0, rx=1).pos(T0 + 300, 0x630002, 52.5, 5.0, 1, rx=1)
    S["global_max_range"] = ([dict(max_range_m=100 * NM), dict(HOME, max_range_m=100 * NM)], 0, [b.step()])

    # a negative --max-range is not "none": doLocalCPR takes it for a limit below 180 NM, and `range_limit > 0` then
    # leaves the range check out: the single half decodes relative to the receiver
    b = B()
    b.pos(T0, 0x640000, 52.5, 5.0, 0)
    S["negative_max_range"] = ([dict(HOME, max_range_m=-1.0)], 0, [b.step()])

    # the speed check is for sources no better than the position's.  A and B have a TIS-B position at 50 N 8 E; 20 s
    # later (too late to pair with the first halves) an even half from 52 N -- 222 km away, beyond the 100 NM of a decode
    # relative to the aircraft: -1 -- and its odd half, a global pair: from ADS-B it is taken unchecked (A), from TIS-B
    # it is 222 km in 20 s and bad data (B).  C and D the same for the local decode, 50.5 N, 56 km away, where 933 kt
    # allow 10.4 km: ADS-B taken (C), TIS-B refused (D)
    b = B()
    for k, (src, lat, pair_) in enumerate(((ip.ADSB, 52.0, True), (ip.TISB, 52.0, True), (ip.ADSB, 50.5, False), (ip.TISB, 50.5, False))):
        a = 0x650000 + k
        b.pos(T0, a, 50.0, 8.0, 0, source=ip.TISB).pos(T0 + 400, a, 50.0, 8.0, 1, source=ip.TISB)
        b.pos(T0 + 20000, a, lat, 8.0, 0, source=src)
        if pair_:
            b.pos(T0 + 20400, a, lat, 8.0, 1, source=src)
    S["higher_source_skips_speed_check"] = ([None], 0, [b.step()])

    # pos_reliable_odd and _even part ways: three global decodes on odd halves make 3 / 1 (A) and one more on an even half
    # 3 / 2 (B); bad data then costs one each: 2 / 0 takes A's position away (and both counters), 2 / 1 leaves B's
    b = B()
    for k, a in enumerate((0x410001, 0x410002)):
        b.pos(T0, a, 50.0, 8.0, 0)
        for j in range(3):
            b.pos(T0 + 400 * (j + 1), a, 50.0, 8.0, 1)
        if k:
            b.pos(T0 + 1600, a, 50.0, 8.0, 0)
        b.pos(T0 + 2000, a, 40.0, 20.0, 0)
    S["reliable_sides"] = ([None], 8, [b.step()])

    # the global airborne decode refuses a pair of which only the odd half's latitude is out of range (cpr.c:188-196).
    # Even YZ = 0, odd YZ = 99328 = 131072 x 97 / 128: j = floor(-60 x 97 / 128 + 0.5) = floor(-44.97) = -45, so the even
    # latitude is 6 x (15 + 0) = 90 exactly -- in range -- and the odd one 360 / 59 x (14 + 97 / 128) = 90.048: bad data.
    # Odd YZ = 31744 = 131072 x 31 / 128: j = -15, the even latitude is 6 x 45 = 270 -> -90, in range, the odd one
    # 360 / 59 x (44 + 31 / 128) = 269.95, which is below 270 and stays: bad data
    b = B()
    b.raw(T0, 0x420001, 0, 0, 0).raw(T0 + 400, 0x420001, 99328, 0, 1)
    b.raw(T0, 0x420002, 0, 0, 0).raw(T0 + 400, 0x420002, 31744, 0, 1)
    S["odd_latitude_alone_out_of_range"] = ([None], 0, [b.step()])
    return S


# What the later scenarios are named for, derived by hand in their comments: the rows' results and the counters that tell.
# test_positions_model.py asserts them on the host twin, test_gpu_positions.py on the device.
KNOWN = {
    "surface_speed_check": ([-1, 0, 1] + [-1, 0, -1] + [-1, 0, 1] + [-1, 0, -1], dict(cpr_local_speed_checks=2, cpr_surface=12)),
    "surface_movement_codes": ([-1, -1] * 6 + [-1, 0] * 2, dict(cpr_global_ok=2)),
    "global_max_range": ([-1, 0] + [-1, -2] + [2, 0], dict(cpr_global_range_checks=1, cpr_local_range_checks=1)),
    "negative_max_range": ([2], dict(cpr_local_range_checks=0, cpr_local_receiver_relative=1)),
    "higher_source_skips_speed_check": ([-1, 0, -1, 0] + [-1, 0, -1, -2] + [-1, 0, 1] + [-1, 0, -1],
                                        dict(cpr_global_speed_checks=1, cpr_local_speed_checks=1, cpr_local_range_checks=2)),
    "reliable_sides": ([-1, 0, 0, 0, -2] + [-1, 0, 0, 0, 0, -2], dict(cpr_global_bad=2)),
    "odd_latitude_alone_out_of_range": ([-1, -2, -1, -2], dict(cpr_global_bad=2, cpr_global_range_checks=0, cpr_global_speed_checks=0)),
}


def known(name, out, st):
    results, counters = KNOWN[name] if name != "refusals" else ([x for case in REFUSAL_RESULTS for x in case], dict(
        cpr_local_receiver_relative=5, cpr_local_aircraft_relative=1, cpr_global_skipped=1, cpr_global_ok=1, cpr_local_speed_checks=0))
    assert [int(x) for x in out["result"]] == results, name
    assert {k: st[k] for k in counters} == counters, name


M_PER_DEG = 6371e3 * np.pi / 180  # greatcircle's metres per degree of latitude
MOVEMENT_CODES = (93, 94, 108, 109, 123, 124, 125, 127)
MOVEMENT_GS = (69, 71, 99, 102, 172, 180, 0, 0)  # (uint32) of the knots above: what the table keeps as gs
# refusal_family: per member the address of its five aircraft's first, what the ADS-B record at T0 and the others carry
# (value A, value B), and what tells them apart in the table entry
REFUSAL_MEMBERS = ("gs", "ias", "tas", "cpr_even", "cpr_odd", "position")
REFUSAL_CASES = (("inside", 1000, False), ("last_ms", 59999, False), ("first_ms_outside", 60000, True), ("older", -1, False),
                 ("equal_source", 1000, True))


def refusal_addr(member, case):
    return 0xA00000 + 0x100 * REFUSAL_MEMBERS.index(member) + case


def refusal_family(b):
    """accept_data (track.c:170-196) for gs, ias, tas, the CPR halves and the position, all stale after 60 s: per member
    five aircraft with an ADS-B value at T0 and then one record each --
      0. a lesser source 1 s later: refused;  1. the same 59 999 ms later: refused;  2. 60 000 ms later: accepted;
      3. the same source, 1 ms before T0: older than `updated`, refused;  4. the same source 1 s later: accepted.
    gs, ias, tas and the CPR halves are on receiver 0 (no location: a single half decodes nothing, -1, and a refused half
    is NOT_TRIED); the position's aircraft are on receiver 1 (52 N 4 E, --max-range 150 NM): the odd half at T0 decodes
    relative to the receiver (2), a TIS-B even half then decodes relative to the aircraft and the position's accept_data
    decides (refused: -1, accepted: 1); the ADS-B even half pairs with the odd one: 1 ms older than the position it is
    a good decode that is skipped (-2), 1 s later it is the position (0).  REFUSAL_RESULTS has the rows' results."""
    lesser = dict(source=ip.MODE_S_CHECKED, msgtype=20)
    for case, (_, dt, _) in enumerate(REFUSAL_CASES):
        same = case >= 3
        a = refusal_addr("gs", case)
        b.vel(T0, a, 300, 400)  # 500 kt
        b.vel(T0 + dt, a, 60, 80) if same else b.rec(T0 + dt, a, commb_valid=2, gs=100, **lesser)
        a = refusal_addr("ias", case)
        b.rec(T0, a, ias_valid=1, ias=250)
        b.rec(T0 + dt, a, ias_valid=1, ias=180, **({} if same else lesser))
        a = refusal_addr("tas", case)
        b.rec(T0, a, tas_valid=1, tas=420)
        b.rec(T0 + dt, a, tas_valid=1, tas=390, **({} if same else lesser))
        for odd, member in ((0, "cpr_even"), (1, "cpr_odd")):
            a = refusal_addr(member, case)
            b.pos(T0, a, 51.5, 3.5, odd)
            b.pos(T0 + dt, a, 51.6, 3.5, odd, source=ip.ADSB if same else ip.TISB)
            if not same:
                b.f[-1]["metype"] = 13  # the table tells by the NIC / Rc whether the half was stored
        a = refusal_addr("position", case)
        b.pos(T0, a, 52.5, 5.0, 1, rx=1)
        b.pos(T0 + dt, a, 52.5, 5.0, 0, rx=1, source=ip.ADSB if same else ip.TISB)
    return b


#                   gs      ias       tas       cpr_even  cpr_odd   position     (first record, second record) per case
REFUSAL_RESULTS = [[-3, -3, -3, -3, -3, -3, -1, -3, -1, -3, 2, -1],    # a lesser source inside the interval
                   [-3, -3, -3, -3, -3, -3, -1, -3, -1, -3, 2, -1],    # at its last millisecond
                   [-3, -3, -3, -3, -3, -3, -1, -1, -1, -1, 2, 1],     # at the first outside
                   [-3, -3, -3, -3, -3, -3, -1, -3, -1, -3, 2, -2],    # older than `updated`
                   [-3, -3, -3, -3, -3, -3, -1, -1, -1, -1, 2, 0]]     # an equal source


def mixed_stream(pkg, n=2000, seed=7, aircraft=40, third_receiver=False, jitter=None):
    """n records of 40 aircraft on two receivers: straight flights with a position every 400 to 600 ms alternating even
    and odd, velocities, airspeeds, operational status, a few surface targets, jumps to implausible places, Mode A/C
    records and address 0 in between; in time order.  third_receiver: a third one, in Sydney, takes every third aircraft.
    jitter(i) -> (dlat, dlon) moves the position that record i carries (range_streams.settle's way of keeping a margin).
    -> (receivers, msgs, fields, receiver)."""
    rng = np.random.default_rng(seed)
    rxs = [dict(lat=52.0, lon=4.0, latlon_valid=1, max_range_m=300 * NM), dict(lat=48.0, lon=11.0, latlon_valid=1)]
    if third_receiver:
        rxs.append(dict(lat=-33.9, lon=151.2, latlon_valid=1, max_range_m=200 * NM))
    b = Builder(pkg)
    planes = []
    for k in range(aircraft):
        r = k % len(rxs)
        planes.append(dict(addr=0x3C0000 + 97 * k + (1 << 24 if k % 13 == 0 else 0), rx=r, lat=rxs[r]["lat"] + rng.uniform(-1.5, 1.5),
                           lon=rxs[r]["lon"] + rng.uniform(-2, 2), vlat=rng.uniform(-2e-6, 2e-6), vlon=rng.uniform(-3e-6, 3e-6),
                           surface=k % 10 == 9, odd=int(rng.integers(0, 2)), source=ip.TISB if k % 13 == 0 else ip.ADSB))
    t = T0
    while len(b.m) < n:
        t += int(rng.integers(5, 40))
        p = planes[int(rng.integers(0, len(planes)))]
        dt = t - T0
        lat, lon = p["lat"] + p["vlat"] * dt, p["lon"] + p["vlon"] * dt
        u = rng.uniform()
        kw = dict(rx=p["rx"], source=p["source"])
        if p["surface"]:
            lat, lon = p["lat"] + p["vlat"] * dt * 0.02, p["lon"] + p["vlon"] * dt * 0.02
        if u < 0.70:
            p["odd"] ^= 1
            if rng.uniform() < 0.04:
                k = 0.1 if rng.uniform() < 0.5 else 1.0                          # bad data, near (speed) or far (range)
                lat, lon = lat + k * rng.uniform(3, 6), lon - k * rng.uniform(3, 6)
            if jitter:
                lat, lon = lat + jitter(len(b.m))[0], lon + jitter(len(b.m))[1]
            b.pos(t, p["addr"], lat, lon, p["odd"], surface=p["surface"], movement=int(rng.integers(0, 60)) if p["surface"] else 0, **kw)
        elif u < 0.85:
            b.vel(t, p["addr"], int(p["vlon"] * 2.4e8), int(p["vlat"] * 3.6e8), **kw)
        elif u < 0.90:
            b.rec(t, p["addr"], tas_valid=1, tas=int(rng.integers(100, 500)), msgtype=21, **dict(kw, source=ip.MODE_S))
        elif u < 0.93:
            b.rec(t, p["addr"], ias_valid=1, ias=int(rng.integers(100, 400)), msgtype=21, **dict(kw, source=ip.MODE_S))
        elif u < 0.96:
            b.opstatus(t, p["addr"], int(rng.integers(0, 3)), **kw)
        elif u < 0.98:
            b.rec(t, 0x7000 + int(rng.integers(0, 8)), msgtype=32, source=ip.MODE_AC, rx=p["rx"])
        else:
            b.rec(t, 0, msgtype=0, source=ip.MODE_S, rx=p["rx"])
    _, m, f, r = b.step()
    return rxs, m[:n], f[:n], r[:n]


def cpr_encode_array(lat, lon, odd):
    """indep_positions.cpr_encode (airborne) over arrays."""
    table = np.array(ip.NL_TABLE)
    dlat = 360.0 / np.where(odd, 59.0, 60.0)
    yz = np.floor(131072 * np.mod(lat, dlat) / dlat + 0.5)
    rlat = dlat * (yz / 131072 + np.floor(lat / dlat))
    nl = 59 - np.searchsorted(table, np.abs(rlat), side="right")
    dlon = 360.0 / np.maximum(nl - odd, 1)
    xz = np.floor(131072 * np.mod(lon, dlon) / dlon + 0.5)
    return yz.astype(np.int64) & 0x1FFFF, xz.astype(np.int64) & 0x1FFFF


def wide_stream(pkg, aircraft, records, receivers=1, skipped_every=0, seed=1):
    """records airborne position squitters, round robin over `aircraft` aircraft (addresses 0x100000 + a, aircraft a on
    receiver a % receivers, no receiver has a location), even and odd alternating, 500 ms between two positions of one
    aircraft, each flying straight at up to about 450 kt: nearly every record is a global decode with a speed check, whose
    limit of 500 m + 1.5 s x 933 kt stays about 1100 m from the at most 120 m flown.  skipped_every = k > 0 turns every
    k-th record into one the tracker skips, in turn a Mode A/C record (msgtype 32) and address 0; the aircraft whose
    record that was pairs its next half with one 1.5 s old.  In time order, no Python loop over the records.
    -> (receivers, msgs, fields, receiver)."""
    rng = np.random.default_rng(seed)
    lat0, lon0 = rng.uniform(-60, 60, aircraft), rng.uniform(-180, 180, aircraft)
    vlat, vlon = rng.uniform(-1.5e-6, 1.5e-6, aircraft), rng.uniform(-1.5e-6, 1.5e-6, aircraft)  # degrees per ms
    i = np.arange(records)
    a, k = i % aircraft, i // aircraft
    t = T0 + k * 500 + (a * 500) // aircraft
    odd = (k & 1).astype(np.int64)
    dt = (k * 500).astype(np.float64)
    y, x = cpr_encode_array(lat0[a] + vlat[a] * dt, lon0[a] + vlon[a] * dt, odd)
    m = np.zeros(records, dtype=pkg.capi.MESSAGE_DTYPE)
    f = np.zeros(records, dtype=pkg.capi.FIELDS_DTYPE)
    m["sysTimestampMsg"], m["msgtype"], m["msgbits"], m["addr"] = t, 17, 112, 0x100000 + a
    f["addr"], f["source"], f["metype"] = 0x100000 + a, ip.ADSB, 11
    f["cpr_valid"], f["cpr_type"], f["cpr_odd"], f["cpr_lat"], f["cpr_lon"] = 1, 1, odd, y, x
    if skipped_every:
        skipped = i % skipped_every == skipped_every - 1
        ac = skipped & ((i // skipped_every) % 2 == 0)
        zero = skipped & ~ac
        m["msgtype"][ac], f["source"][ac] = 32, ip.MODE_AC
        m["msgtype"][zero], m["addr"][zero], f["addr"][zero], f["source"][zero] = 11, 0, 0, ip.MODE_S
        for name in ("metype", "cpr_valid", "cpr_type", "cpr_odd", "cpr_lat", "cpr_lon"):
            f[name][skipped] = 0
    return [None] * receivers, m, f, (a % receivers).astype(np.uint32)


def chain_addresses(pkg, capacity=64):
    """Five addresses of receiver 0 with the home slots capacity - 1 (three), 0 and 1: inserted into an empty table they
    occupy capacity - 1, 0, 1, 2, 3, one probe chain across the table's end."""
    want = [capacity - 1] * 3 + [0, 1]
    got = [None] * 5
    a = 0x480000
    while None in got:
        s = pkg.capi.pos_home_slot(0, a, capacity)
        for j in range(5):
            if got[j] is None and want[j] == s:
                got[j] = a
                break
        a += 1
    return got


CHAIN_VARIANTS = ("whole", "two_calls", "reversed")
CHAIN_ALIVE = {"whole": [5, 5, 3, 3], "two_calls": [2, 5, 5, 3, 3], "reversed": [5, 5, 3, 3]}  # aircraft after each step


def chain_place(j):
    return 50.0 + 0.5 * j, 8.0 + 0.3 * j


def chain_scenario(pkg, capacity=64, variant="whole"):
    """The aircraft of chain_addresses: the first and third of the three that wrap and the one at home in slot 1 survive,
    the two between them are heard once and leave from the middle of the chain.
      1. at T0 a good even / odd pair for the survivors and one record for the others (two_calls: the first two aircraft
         in one call, the rest in the next; reversed: the five in the opposite order);
      2. at T0 + 61000 an even half per survivor: its odd half is 60.6 s old, so it decodes relative to the position of
         step 1, through the speed check against that position, and becomes the position;
      3. expiry at T0 + 61001: the others are more than 60 s old, the survivors move into the other table;
      4. at T0 + 61400 the survivors' odd halves: global against the even half that was stored before the rebuild,
         through the speed check against the position that was."""
    assert variant in CHAIN_VARIANTS
    addrs = chain_addresses(pkg, capacity)
    order = [4, 3, 2, 1, 0] if variant == "reversed" else [0, 1, 2, 3, 4]
    survivors = [j for j in order if j in (0, 2, 4)]
    b = Builder(pkg)

    def first(js):
        for j in js:
            b.pos(T0 + j, addrs[j], *chain_place(j), 0)
        for j in js:
            if j in survivors:
                b.pos(T0 + 400 + j, addrs[j], *chain_place(j), 1)
        return b.step()

    steps = [first(order[:2]), first(order[2:])] if variant == "two_calls" else [first(order)]
    for j in survivors:
        b.pos(T0 + 61000, addrs[j], *chain_place(j), 0)
    steps += [b.step(), ("expire", T0 + 61001)]
    for j in survivors:
        b.pos(T0 + 61400, addrs[j], *chain_place(j), 1)
    steps.append(b.step())
    return [None], 0, steps


# ---- runners -------------------------------------------------------------------------------------------------------
def run_library(tracker, steps, pieces=None):
    """steps through a capi.PositionTracker -> POSITION_DTYPE rows of all update steps, in order; pieces: cut every
    update into calls of that many records."""
    outs = []
    for s in steps:
        if s[0] == "expire":
            tracker.expire(s[1])
            continue
        _, m, f, r = s
        k = pieces or max(len(m), 1)
        for i in range(0, len(m), k):
            outs.append(tracker.update(m[i:i + k], f[i:i + k], r[i:i + k]))
    return np.concatenate(outs) if outs else np.zeros(0)


def run_model(receivers, filter_persistence, steps):
    t = ip.Tracker(receivers, filter_persistence or 8)
    rows = []
    for s in steps:
        if s[0] == "expire":
            t.expire(s[1])
        else:
            rows += t.update(s[1], s[2], s[3])
    return rows, t.get_stats()


def rows_of(out):
    """POSITION_DTYPE -> comparable tuples with the coordinates as bit patterns."""
    return [(int(o["decoded"]), int(o["relative"]), int(o["surface"]), int(o["result"]),
             int(o["lat"].view(np.uint64)), int(o["lon"].view(np.uint64))) for o in out]


def rows_of_model(rows):
    return [(d, rel, s, res, int(np.float64(lat).view(np.uint64)), int(np.float64(lon).view(np.uint64)))
            for d, rel, s, res, lat, lon in rows]
