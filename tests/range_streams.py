"""Constructed record streams for the receiver range's tests (test_range_model.py on the CPU, test_gpu_range.py on the
GPU), built with pos_streams.Builder: the named scenarios of the issue, a 2000-record mixed stream over four receivers,
and one runner for the three implementations (the GPU object, the host twin, the second reading of tests/indep_range.py).

A scenario is (receivers, filter_persistence, steps, polar); a step is ("update", msgs, fields, receiver),
("expire", now_ms), ("set_receiver", index, dict), ("take",) -- a read with MSD_RANGE_TAKE_LONGEST -- or ("reset",).

Every scenario keeps, on the second reading, every plausibility gate at least 1 m from its limit, every evaluated range
at least 0.05 m from the nearest integer (and from --max-range) and every bearing at least 0.01 degrees from a bucket edge
-- fifty and a thousand times the contract's figures.  settle() sees to that: a scenario is a function of a jitter per
aircraft -- per record where an aircraft moves --, a small offset of its position drawn from a generator seeded with the
scenario's name, the key and the number of times the key has been drawn; the second reading runs over the candidate and
reports its margins per aircraft and per record, and those that came closer are drawn again.  The tests assert the three
margins on the host object."""
import math
import zlib

import numpy as np

import indep_positions as ip
import indep_range as ir
from pos_streams import HOME, NM, T0, Builder, chain_addresses, chain_place

RANGE_MARGIN, BEARING_MARGIN, GATE_MARGIN = 0.05, 0.01, 1.0
M_PER_DEG = 6371e3 * math.pi / 180
RECORD = 1 << 30  # a jitter key's first member that says "the record with this index", not a receiver


def offset(rx, azimuth_deg, metres):
    """A place `metres` from the receiver in the compass direction `azimuth_deg` (flat-earth: good enough to aim with)."""
    a = math.radians(azimuth_deg)
    return (rx["lat"] + metres * math.cos(a) / M_PER_DEG,
            rx["lon"] + metres * math.sin(a) / (M_PER_DEG * math.cos(math.radians(rx["lat"]))))


def pair(b, t, addr, lat, lon, **kw):
    return b.pos(t, addr, lat, lon, 0, **kw).pos(t + 400, addr, lat, lon, 1, **kw)


def run(tr, steps, pieces=None):
    """steps through a capi.PositionTracker or an ir.RangeTracker -> one observation per step: (the rows of range_read,
    the distances, the position rows of an update step as comparable tuples)."""
    seen = []
    for s in steps:
        rows = []
        if s[0] == "update":
            _, m, f, r = s
            k = pieces or max(len(m), 1)
            for i in range(0, len(m), k):
                rows += positions(tr.update(m[i:i + k], f[i:i + k], r[i:i + k]))
        elif s[0] == "expire":
            tr.expire(s[1])
        elif s[0] == "set_receiver":
            tr.set_receiver(s[1], **s[2])
        elif s[0] == "take":
            rows = read_rows(tr.range_read(take_longest=True))
        elif s[0] == "reset":
            tr.reset()
        seen.append((read_rows(tr.range_read()), [int(d) for d in tr.range_distances()], rows))
    return seen


def pb_of(tr, scenario, now_ms):
    """The two protobuf outputs of a table tracker with the range and aircraft.pb enabled: (range_pb() per receiver,
    aircraft_pb(now_ms) per receiver); of the second reading: the same from its arrays, the snapshot of `scenario`'s host
    table and indep_range_pb.Writer."""
    return tr.range_pb(), tr.aircraft_pb(now_ms)


def pb_of_model(pkg, m, snapshot, now_ms):
    import indep_range_pb
    w = indep_range_pb.Writer(pkg.capi.AC, len(m.rx))
    dist = {k: getattr(a, "distance", 0) for k, a in m.aircraft.items()}
    return [ir.polar_range_pb(r.polar) for r in m.range], w.files(snapshot, now_ms, dist)[0]


def read_rows(rows):
    if isinstance(rows, np.ndarray):
        return [(tuple(int(v) for v in r["polar_range"]), int(r["longest_m"]), int(r["longest_nm"]), int(r["evaluated"]))
                for r in rows]
    return rows


def positions(out):
    bits = lambda v: int(np.float64(v).view(np.uint64))  # noqa: E731
    if isinstance(out, np.ndarray):
        return [(int(o["decoded"]), int(o["relative"]), int(o["surface"]), int(o["result"]), bits(o["lat"]), bits(o["lon"]))
                for o in out]
    return [(d, rel, s, res, bits(lat), bits(lon)) for d, rel, s, res, lat, lon in out]


def model(scenario, capacity=None):
    receivers, fp, steps, polar = scenario
    return ir.RangeTracker(receivers, fp or 8, capacity, polar=polar)


def settle(name, build, rounds=200):
    """build(jitter) -> scenario, jitter(key) -> (dlat, dlon) within +-0.01 degrees; a key is (receiver, addr) for an
    aircraft that sits still or (RECORD, i) for the i-th record of the scenario's updates.  Draws again, from a generator
    seeded with (name, key, draw number), every aircraft and every record whose margins on the second reading are below
    the module's figures."""
    draws = {}

    def jitter(key):
        g = np.random.default_rng([zlib.crc32(name.encode()), key[0], key[1], draws.get(key, 0)])
        return tuple(g.uniform(-0.01, 0.01, 2))

    for _ in range(rounds):
        scenario = build(jitter)
        t = model(scenario)
        run(t, scenario[2])
        close = [k if by is t.by_aircraft else (RECORD, k) for by in (t.by_aircraft, t.by_record)
                 for k, (rm, bm, gm) in by.items() if rm < RANGE_MARGIN or bm < BEARING_MARGIN or gm < GATE_MARGIN]
        if not close:
            return scenario
        for k in close:
            draws[k] = draws.get(k, 0) + 1
    raise AssertionError(f"{name}: no draw keeps the margins")


_cache = {}


def scenarios(pkg):
    if "scenarios" not in _cache:
        _cache["scenarios"] = _scenarios(pkg)
    return _cache["scenarios"]


def _scenarios(pkg):
    S = {}
    B = lambda: Builder(pkg)  # noqa: E731

    # 1. one even / odd pair: the first half alone decodes nothing, the second evaluates one range
    def one_pair(jit):
        b, a = B(), 0xA00001
        d = jit((0, a))
        lat, lon = 52.3 + d[0], 4.5 + d[1]
        steps = [b.pos(T0, a, lat, lon, 0).step(), b.pos(T0 + 400, a, lat, lon, 1).step()]
        return [HOME], 0, steps, True
    S["one_pair"] = settle("one_pair", one_pair)

    # 2. no receiver location: nothing is evaluated; msd_pos_set_receiver mid-stream: later records count
    def no_location(jit):
        b = B()
        p = {a: (52.3 + 0.1 * k + jit((0, a))[0], 4.5 + jit((0, a))[1]) for k, a in enumerate((0xA00011, 0xA00012))}
        pair(b, T0, 0xA00011, *p[0xA00011])
        steps = [b.step(), ("set_receiver", 0, HOME)]
        pair(b, T0 + 1000, 0xA00012, *p[0xA00012])
        steps += [b.step(), ("set_receiver", 0, dict(lat=0.0, lon=0.0, latlon_valid=0))]  # the arrays stay
        pair(b, T0 + 2000, 0xA00011, *p[0xA00011])
        pair(b, T0 + 2000, 0xA00012, *p[0xA00012])                     # decoded, no location: distance back to 0
        steps += [b.step(), ("set_receiver", 0, HOME)]
        pair(b, T0 + 3000, 0xA00011, *p[0xA00011])
        steps += [b.step()]
        return [None], 0, steps, True
    S["no_location"] = settle("no_location", no_location)

    # 3. a decoded position from TIS-B resets an earlier distance and touches no array: ADS-B goes stale after 60 s, the
    # TIS-B even half then decodes relative to the aircraft's position, the odd half makes a TIS-B pair
    def non_adsb(jit):
        b, a = B(), 0xA00021
        d = jit((0, a))
        lat, lon = 51.7 + d[0], 3.2 + d[1]
        pair(b, T0, a, lat, lon)
        steps = [b.step()]
        b.pos(T0 + 61000, a, lat, lon, 0, source=ip.TISB)
        steps += [b.step()]
        b.pos(T0 + 61400, a, lat, lon, 1, source=ip.TISB)
        steps += [b.step()]
        return [HOME], 0, steps, True
    S["non_adsb"] = settle("non_adsb", non_adsb)

    # 4. receiver-relative decode at pos_reliable 0 / 0: the position expires (the counters with it), velocities keep the
    # aircraft alive, and more than ten minutes after the position a single half decodes relative to the receiver --
    # decoded, nothing evaluated, distance 0 --; the other half then makes a global pair, which is evaluated
    def relative_0_0(jit):
        b, a = B(), 0xA00031
        d = jit((0, a))
        lat, lon = 52.4 + d[0], 4.9 + d[1]
        pair(b, T0, a, lat, lon)
        steps = [b.step(), ("expire", T0 + 100000)]
        b.vel(T0 + 400000, a, 100, 100)
        b.pos(T0 + 601000, a, lat, lon, 0)
        steps += [b.step()]
        b.pos(T0 + 601400, a, lat, lon, 1)
        steps += [b.step()]
        return [dict(HOME, max_range_m=150 * NM)], 0, steps, True
    S["relative_0_0"] = settle("relative_0_0", relative_0_0)

    # 6. longest: without a limit, and with one -- an aircraft that flies out through --max-range on aircraft-relative
    # decodes (single halves 11 s apart, which doLocalCPR does not hold against the receiver's limit) keeps raising its
    # bucket and its distance but not `longest` --; a read that takes `longest` leaves the polar range alone
    def longest(limit_m):
        def build(jit):
            b, a, a2 = B(), 0xA00041, 0xA00042
            d, d2 = jit((0, a)), jit((0, a2))
            lat, lon = offset(HOME, 70, 98e3)
            pair(b, T0, a2, 52.2 + d2[0], 4.3 + d2[1])
            pair(b, T0, a, lat + d[0], lon + d[1])
            steps = [b.step()]
            for k in range(1, 4):
                lat, lon = offset(HOME, 70, 98e3 + 3e3 * k)
                b.pos(T0 + 400 + 11000 * k, a, lat + d[0], lon + d[1], 0)
            steps += [b.step(), ("take",)]
            pair(b, T0 + 40000, a2, 52.2 + d2[0], 4.3 + d2[1])
            steps += [b.step()]
            return [dict(HOME, max_range_m=limit_m)], 0, steps, True
        return build
    S["longest_no_limit"] = settle("longest_no_limit", longest(0.0))
    S["longest_limit"] = settle("longest_limit", longest(100e3))

    # 7. more than one wavefront: 65 aircraft interleaved across three receivers with different locations
    rx3 = [HOME, dict(lat=48.0, lon=11.0, latlon_valid=1), dict(lat=-33.9, lon=151.2, latlon_valid=1, max_range_m=300 * NM)]

    def three_receivers(jit):
        b = B()
        for half in (0, 1):
            for k in range(65):
                r, a = k % 3, 0xA10000 + 7 * k
                d = jit((r, a))
                lat, lon = offset(rx3[r], 5.5 * k + 1, 20e3 + 4e3 * k)
                b.pos(T0 + 400 * half + k, a, lat + d[0], lon + d[1], half, rx=r)
        return rx3, 0, [b.step()], True
    S["three_receivers"] = settle("three_receivers", three_receivers)
    # 11. the same without MSD_RANGE_POLAR: distances and longest work, the buckets stay 0
    S["three_receivers_no_polar"] = S["three_receivers"][:3] + (False,)

    # 8. last record wins: one aircraft, 300 records, out and back along one bearing: the distance is the last record's,
    # the bucket keeps the maximum
    def out_and_back(jit):
        b, a = B(), 0xA00051
        for k in range(300):
            d = jit((RECORD, k))
            lat, lon = offset(HOME, 123.0, 30e3 + 60.0 * (150 - abs(150 - k)))
            b.pos(T0 + 500 * k, a, lat + 0.02 * d[0], lon + 0.02 * d[1], k & 1)
        return [HOME], 0, [b.step()], True
    S["out_and_back"] = settle("out_and_back", out_and_back)

    # 9. table maintenance: pos_streams.chain_scenario's aircraft -- a probe chain across the end of a table of 64 slots,
    # two of them leaving from its middle at the expiry -- seen from a receiver with a location (the jitter moves the
    # receiver: the chain's places are fixed); then everything expires; then reset
    def chain(jit):
        addrs = chain_addresses(pkg, 64)
        d = jit((0, 0))
        b = B()
        for j in range(5):
            b.pos(T0 + j, addrs[j], *chain_place(j), 0)
        for j in (0, 2, 4):
            b.pos(T0 + 400 + j, addrs[j], *chain_place(j), 1)
        steps = [b.step()]
        for j in (0, 2, 4):
            b.pos(T0 + 61000, addrs[j], *chain_place(j), 0)
        steps += [b.step(), ("expire", T0 + 61001)]
        for j in (0, 2, 4):
            b.pos(T0 + 61400, addrs[j], *chain_place(j), 1)
        steps += [b.step(), ("expire", T0 + 61400 + 600001), ("reset",)]
        pair(b, T0, addrs[1], *chain_place(1))
        steps += [b.step()]
        return [dict(HOME, lat=HOME["lat"] + d[0], lon=HOME["lon"] + d[1])], 0, steps, True
    S["chain"] = settle("chain", chain)

    # 10. contention: 4096 records of 512 aircraft in one receiver and one bucket
    def contention(jit):
        b = B()
        for rep in range(4):
            for half in (0, 1):
                for k in range(512):
                    a = 0xA20000 + k
                    d = jit((0, a))
                    lat, lon = offset(HOME, 200.0, 50e3 + 150.0 * k)
                    b.pos(T0 + 1000 * rep + 400 * half + k // 8, a, lat + 0.05 * d[0], lon + 0.05 * d[1], half)
        return [HOME], 0, [b.step()], True
    S["contention"] = settle("contention", contention)

    # 12. --max-range nearer to a range than the next whole metre: the range margin is the distance to the limit.  The
    # pair is decoded while the receiver has no limit (a global decode is held against --max-range, and that gate must stay
    # 1 m away); then the limit is set 0.3 m beyond where the aircraft's even half will decode, 11 s later and so relative
    # to the aircraft, which the limit does not gate: within the limit, 0.3 m from it and about 0.5 m from a whole metre
    S["limit_beside_the_range"] = limit_beside_the_range(pkg)[0]
    return S


def limit_beside_the_range(pkg):
    """-> (scenario, the third record's range, the limit).  The place is searched for along a meridian: the aircraft sits
    still, so what its halves decode to is known in advance."""
    a = 0xA00071
    for k in range(100000):
        lat, lon = 52.3 + 1e-5 * k, 4.5
        ye, xe = ip.cpr_encode(lat, lon, 0)
        yo, xo = ip.cpr_encode(lat, lon, 1)
        ranges, ok = [], True
        for fflag in (1, 0):  # the pair's decode is the odd half's, the late half's its own
            p = ip.decode_airborne(ye, xe, yo, xo, fflag)[1:]
            rng = ip.greatcircle(HOME["lat"], HOME["lon"], *p)
            ok = ok and edge_distance_ok(ir.get_bearing(HOME["lat"], HOME["lon"], *p))
            ranges.append(rng)
        frac = ranges[1] - math.floor(ranges[1])
        if ok and 0.45 <= frac <= 0.55 and abs(ranges[0] - ir.c_round(ranges[0])) >= 0.35:  # the pair's own margin stays larger
            break
    else:
        raise AssertionError("no such place")
    limit = ranges[1] + 0.3
    b = Builder(pkg)
    pair(b, T0, a, lat, lon)
    steps = [b.step(), ("set_receiver", 0, dict(HOME, max_range_m=limit))]
    b.pos(T0 + 11400, a, lat, lon, 0)
    steps += [b.step()]
    return ([HOME], 0, steps, True), ranges[1], limit


def edge_distance_ok(bearing):
    return ir.edge_distance(bearing) >= 10 * BEARING_MARGIN


def below_one_metre(pkg, polar=True):
    """13. An aircraft 0.4 m from the receiver: the receiver is put 0.4 m south of where the pair decodes.  The range is
    0 m, and below 1 m the bearing says nothing: the bearing margin is reported as 0, which is why this scenario is not
    one of those the device is held to (the contract covers streams whose margins stay above its figures)."""
    a, lat, lon = 0xA00081, 52.3, 4.5
    ye, xe = ip.cpr_encode(lat, lon, 0)
    yo, xo = ip.cpr_encode(lat, lon, 1)
    plat, plon = ip.decode_airborne(ye, xe, yo, xo, 1)[1:]
    b = Builder(pkg)
    pair(b, T0, a, lat, lon)
    return [dict(lat=plat - 0.4 / M_PER_DEG, lon=plon, latlon_valid=1)], 0, [b.step()], polar


def bucket_wrap(pkg):
    """5. Two aircraft just either side of the direction in which getBearing jumps from 360 to 0 both land in bucket 0;
    two more on each side of an edge 2.5 + 5k, about 0.02 degrees apart, land in different buckets.  The places are searched
    for: each aircraft sits still, so its two global decodes (from the even and from the odd half) are known in advance,
    and a place is taken when both keep the margins.  -> (scenario, [(bearing, bucket) per aircraft])."""
    def decodes(lat, lon):
        ye, xe = ip.cpr_encode(lat, lon, 0)
        yo, xo = ip.cpr_encode(lat, lon, 1)
        return [ip.decode_airborne(ye, xe, yo, xo, f)[1:] for f in (0, 1)]

    def find(az0, step, want):
        for k in range(200000):
            lat, lon = offset(HOME, az0 + k * step, 180e3)
            ok = True
            for p in decodes(lat, lon):
                rng = ip.greatcircle(HOME["lat"], HOME["lon"], *p)
                bearing = ir.get_bearing(HOME["lat"], HOME["lon"], *p)
                ok = ok and abs(rng - ir.c_round(rng)) >= RANGE_MARGIN and want(bearing)
            if ok:
                return lat, lon
        raise AssertionError("no such place")

    # where the bearing wraps: scan the compass for the largest jump
    samples = [ir.get_bearing(HOME["lat"], HOME["lon"], *offset(HOME, az, 180e3)) for az in range(360)]
    wrap = max(range(360), key=lambda az: abs(samples[az] - samples[az - 1]))
    rising = samples[(wrap + 1) % 360] > samples[wrap]  # the bearing grows with the compass direction, or falls
    edge_az = next(az for az in range(360) if (samples[az - 1] - 92.5) * (samples[az] - 92.5) < 0 and abs(samples[az] - samples[az - 1]) < 5)
    places = [
        find(wrap - 1.0, 0.001, lambda v: (0.3 < v < 2.0) if not rising else (358.0 < v < 359.7)),
        find(wrap - 1.0, 0.001, lambda v: (358.0 < v < 359.7) if not rising else (0.3 < v < 2.0)),
        find(edge_az - 1.0, 0.0002, lambda v: 0.010 <= 92.5 - v <= 0.0125),
        find(edge_az - 1.0, 0.0002, lambda v: 0.010 <= v - 92.5 <= 0.0125),
    ]
    b = Builder(pkg)
    for k, (lat, lon) in enumerate(places):
        pair(b, T0 + k, 0xA00061 + k, lat, lon)
    seen = []
    for lat, lon in places:
        p = decodes(lat, lon)[1]
        bearing = ir.get_bearing(HOME["lat"], HOME["lon"], *p)
        seen.append((bearing, int(ir.c_round(bearing / 5)) % 72))
    return ([HOME], 0, [b.step()], True), seen


def mixed_stream(pkg, n=2000, seed=11):
    """14. n records of 48 aircraft on four receivers -- one without a location, one with --max-range --: straight flights
    with a position every few hundred ms alternating even and odd, velocities, airspeeds, operational status, TIS-B
    aircraft, Mode A/C records and address 0 in between, an expiry in the middle; in time order."""
    rxs = [dict(lat=52.0, lon=4.0, latlon_valid=1, max_range_m=300 * NM), dict(lat=48.0, lon=11.0, latlon_valid=1), None,
           dict(lat=-33.9, lon=151.2, latlon_valid=1)]

    def build(jit):
        rng = np.random.default_rng(seed)
        b = Builder(pkg)
        planes = []
        for k in range(48):
            r = k % 4
            base = rxs[r] or dict(lat=10.0, lon=10.0)
            a = 0x3D0000 + 89 * k
            planes.append(dict(addr=a, rx=r, lat=base["lat"] + rng.uniform(-1.5, 1.5), lon=base["lon"] + rng.uniform(-2, 2),
                               vlat=rng.uniform(-2e-6, 2e-6), vlon=rng.uniform(-3e-6, 3e-6), odd=int(rng.integers(0, 2)),
                               source=ip.TISB if k % 11 == 5 else ip.ADSB))
        t, steps = T0, []
        for i in range(n):
            if i == n // 2:
                steps += [b.step(), ("expire", t)]
            t += int(rng.integers(5, 40))
            p = planes[int(rng.integers(0, len(planes)))]
            dt = t - T0
            u = rng.uniform()
            kw = dict(rx=p["rx"], source=p["source"])
            if u < 0.72:
                p["odd"] ^= 1
                d = jit((RECORD, i))
                b.pos(t, p["addr"], p["lat"] + p["vlat"] * dt + 0.02 * d[0], p["lon"] + p["vlon"] * dt + 0.02 * d[1], p["odd"], **kw)
            elif u < 0.86:
                b.vel(t, p["addr"], int(p["vlon"] * 2.4e8), int(p["vlat"] * 3.6e8), **kw)
            elif u < 0.91:
                b.rec(t, p["addr"], tas_valid=1, tas=int(rng.integers(100, 500)), msgtype=21, **dict(kw, source=ip.MODE_S))
            elif u < 0.95:
                b.opstatus(t, p["addr"], int(rng.integers(0, 3)), **kw)
            elif u < 0.98:
                b.rec(t, 0x7000 + int(rng.integers(0, 8)), msgtype=32, source=ip.MODE_AC, rx=p["rx"])
            else:
                b.rec(t, 0, msgtype=0, source=ip.MODE_S, rx=p["rx"])
        steps.append(b.step())
        return rxs, 0, steps, True
    if ("mixed", n, seed) not in _cache:
        _cache["mixed", n, seed] = settle(f"mixed{seed}", build)
    return _cache["mixed", n, seed]


def known_answers(name, seen):
    """What a scenario is named for, on the observations of run(): so that three readings cannot agree on a stream that
    never reaches the rule in question."""
    nonzero = lambda row: [v for v in row[0] if v]  # noqa: E731
    if name == "one_pair":
        assert seen[0][0] == [((0,) * 72, 0, 0, 0)] and seen[0][1] == [0]          # the first half alone: nothing
        (row,), (d,) = seen[1][0], seen[1][1]
        assert row[3] == 1 and nonzero(row) == [d] and row[1] == d and row[2] == d // 1852 and 40000 < d < 60000
    elif name == "no_location":
        assert seen[0][0] == [((0,) * 72, 0, 0, 0)] and seen[0][1] == [0]          # decoded, no location
        assert seen[2][0][0][3] == 1 and seen[2][1][0] == 0 and seen[2][1][1] > 0   # after set_receiver
        assert seen[4][0] == seen[2][0] and seen[4][1] == [0, 0]                    # location gone: arrays kept, distances 0
        assert seen[6][0][0][3] == 3 and seen[6][1][0] > 0 and seen[6][1][1] == 0
    elif name == "non_adsb":
        assert seen[0][1][0] > 0 and seen[1][1] == [0] and seen[2][1] == [0]
        assert seen[1][2][0][:2] == (1, 1) and seen[2][2][0][:2] == (1, 0)          # aircraft-relative, then a TIS-B pair
        assert seen[0][0] == seen[1][0] == seen[2][0] and seen[0][0][0][3] == 1
    elif name == "relative_0_0":
        assert seen[0][1][0] > 0 and seen[0][0][0][3] == 1
        assert seen[2][2][-1][:2] == (1, 2) and seen[2][1] == [0] and seen[2][0][0][3] == 1  # receiver-relative at 0 / 0
        assert seen[3][2][0][:2] == (1, 0) and seen[3][1][0] > 0 and seen[3][0][0][3] == 2   # the global pair
    elif name in ("longest_no_limit", "longest_limit"):
        row, (far, near) = seen[1][0][0], seen[1][1]
        assert row[3] == 5 and max(row[0]) == far > 106000 and [r[:2] for r in seen[1][2]] == [(1, 1)] * 3
        if name == "longest_limit":
            assert 97000 < row[1] < 100000 < far                                    # beyond --max-range: not the longest
        else:
            assert row[1] == far
        assert seen[2][2] == [row] and seen[2][0][0] == (row[0], 0, 0, 5)           # taken: longest zeroed, the rest kept
        assert near <= seen[3][0][0][1] <= near + 2 and max(seen[3][0][0][0]) == far and seen[3][0][0][3] == 7
    elif name in ("three_receivers", "three_receivers_no_polar"):
        rows, dist, _ = seen[0]
        assert [r[3] for r in rows] == [22, 22, 21] and len(dist) == 65 and all(dist)
        assert [r[1] for r in rows] == [max(dist[:22]), max(dist[22:44]), max(dist[44:])]
        if name == "three_receivers":
            assert [len(nonzero(r)) for r in rows] == [22, 22, 21]
        else:
            assert all(not nonzero(r) for r in rows)
    elif name == "out_and_back":
        (row,), (d,) = seen[0][0], seen[0][1]
        assert row[3] == 299 and nonzero(row) == [row[1]] and 38900 < row[1] < 39200 and 30000 < d < 30200
    elif name == "chain":
        assert len(seen[0][1]) == 5 and sorted(bool(d) for d in seen[0][1]) == [False, False, True, True, True]
        assert len(seen[2][1]) == 3 and all(seen[2][1]) and seen[2][0] == seen[1][0]    # the expiry: distances move, arrays stay
        assert seen[3][0][0][3] == 9
        assert seen[4][1] == [] and seen[4][0] == seen[3][0]                              # everything gone but the arrays
        assert seen[5][0] == [((0,) * 72, 0, 0, 0)] and seen[5][1] == []                  # reset
        assert seen[6][0][0][3] == 1 and seen[6][1][0] > 0                                # still enabled
    elif name == "limit_beside_the_range":
        assert seen[0][0][0][3] == 1 and seen[2][0][0][3] == 2 and seen[2][2][0][:2] == (1, 1)   # the late half: aircraft-relative
        assert seen[2][0][0][1] == max(seen[0][1][0], seen[2][1][0])                             # within the limit: it counts
    elif name == "contention":
        (row,), dist = seen[0][0], seen[0][1]
        assert row[3] == 3584 and len(dist) == 512 and nonzero(row) == [max(dist)] and row[1] == max(dist)
