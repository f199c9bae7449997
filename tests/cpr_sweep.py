"""The reference's recorded CPR answers (tests/golden/cpr/*.npz, written by tests/golden/make_cpr_records.py) as record
streams for the position tracker, and the POSITION_DTYPE rows those streams must give: test_cpr_sweep.py holds the host
twin to them, test_gpu_cpr_sweep.py the device.  The expected rows come from the files alone; the only arithmetic done here
is indep_positions.greatcircle for the range gate, and a case whose distance lies within 1 m of its limit is not allowed
(asserted, cap zero: the contract of modes_hip.h is 1e-3 m and the suite keeps 1 m).

Every case is an aircraft of its own, address 0x100000 + case index, with records at T0 + 400 k, written as
pos_streams.Builder.pos / raw leaves them (msgtype 17, 112 bits, cpr_valid, metype 11 airborne or 7 surface).

cpr_reference.npz, by its `kind` column:
  0  airborne pair: receiver 0, which has no location; two ADS-B records, the half that fflag names second.  The first
     row is result -1.  The second is the recorded answer: 0 -> decoded, relative 0, the recorded patterns; -1 -> -1
     (the local attempt that follows has no reference); -2 -> -2.
  1  surface pair: the same with cpr_type 0 on a receiver at the case's reference with max_range_m = 0 (no range gate);
     one receiver per distinct reference.
  2, surface == 0   one record on a receiver at the case's reference with max_range_m = 180 NM: recorded 0 -> decoded,
     relative 2, result 2 with the recorded patterns unless greatcircle(reference, answer) > 180 NM, then -1; -1 -> -1.
  2, surface == 1   NOT REACHABLE, left out (16 575 cases): the tracker decodes a surface half relative only to the
     aircraft's own last position, never to a receiver, and that position is always itself a CPR result -- it cannot be
     set to the file's arbitrary reference.  The chained family covers surface-relative decodes instead.

cpr_chained.npz: per case three records on receiver 0: the place's airborne pair with source TIS-B at T0 and T0 + 400,
odd half second (row: decoded, relative 0, P's patterns), then the third half with source ADS-B at T0 + 800.  The two
stored halves then differ in source, so no global decode is tried, and 7 > 5 means no speed check: the third half is
decoded relative to exactly P with the 100 NM limit as the only gate.  Recorded 0 within 100 NM of P -> decoded,
relative 1, result 1 with the recorded patterns; recorded 0 further away -> -1; recorded -1 -> -1."""
import os

import numpy as np

import indep_positions as ip
import pos_streams as ps

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.path.join(HERE, "golden", "cpr", "cpr_reference.npz")
CHAINED = os.path.join(HERE, "golden", "cpr", "cpr_chained.npz")
ADDR0 = 0x100000
NM = 1852.0
RECEIVER_RANGE_M = NM * 180
AIRCRAFT_RANGE_M = NM * 100
UNREACHABLE = 16575  # kind 2 with surface == 1 in cpr_reference.npz
KIND_CHAINED = 3
COUNTERS = ("cpr_surface", "cpr_airborne", "cpr_global_ok", "cpr_global_bad", "cpr_global_skipped", "cpr_global_range_checks",
            "cpr_global_speed_checks", "cpr_local_ok", "cpr_local_aircraft_relative", "cpr_local_receiver_relative",
            "cpr_local_skipped", "cpr_local_range_checks", "cpr_local_speed_checks", "aircraft")


def load(path):
    g = np.load(path)
    return {k: g[k] for k in g.files}


def beyond(reflat, reflon, lat_bits, lon_bits, limit):
    """greatcircle(reference, answer) > limit per case; no distance may lie within 1 m of the limit."""
    lat, lon = lat_bits.view(np.float64), lon_bits.view(np.float64)
    d = np.array([ip.greatcircle(float(a), float(b), float(c), float(e)) for a, b, c, e in zip(reflat, reflon, lat, lon)])
    near = np.abs(d - limit) < 1.0
    assert not near.any(), ("cases within 1 m of the range limit", np.flatnonzero(near)[:5], d[near][:5])
    return d > limit


def records(pkg, case, k, source, airborne, odd, cprlat, cprlon):
    """whole record arrays, one entry per element of the arguments"""
    n = len(case)
    m, f = np.zeros(n, dtype=pkg.capi.MESSAGE_DTYPE), np.zeros(n, dtype=pkg.capi.FIELDS_DTYPE)
    m["sysTimestampMsg"], m["msgtype"], m["msgbits"], m["addr"] = ps.T0 + 400 * k, 17, 112, ADDR0 + case
    f["addr"], f["source"], f["metype"] = ADDR0 + case, source, np.where(airborne, 11, 7)
    f["cpr_valid"], f["cpr_type"], f["cpr_odd"], f["cpr_lat"], f["cpr_lon"] = 1, airborne, odd, cprlat, cprlon
    return m, f


def rows(pkg, surface, result, relative, lat_bits, lon_bits):
    """the expected rows: result >= 0 is a decoded position"""
    w = np.zeros(len(result), dtype=pkg.capi.POSITION_DTYPE)
    ok = result >= 0
    w["decoded"], w["relative"], w["surface"], w["result"] = ok, np.where(ok, relative, 0), surface, result
    zero = np.uint64(0)
    w["lat"], w["lon"] = np.where(ok, lat_bits, zero).view(np.float64), np.where(ok, lon_bits, zero).view(np.float64)
    return w


def in_case_order(sweep, order):
    """the stream with its records in `order`, which keeps every case's own records in order"""
    out = dict(sweep)
    for key in ("m", "f", "r", "case", "kind", "want"):
        out[key] = sweep[key][order]
    return out


def shuffled(sweep, seed=1090):
    """a fixed shuffle of the cases: one wavefront of walkers then holds every kind and every outcome side by side"""
    key = np.random.default_rng(seed).permutation(int(sweep["case"].max()) + 1)
    return in_case_order(sweep, np.lexsort((sweep["m"]["sysTimestampMsg"], key[sweep["case"]])))


def reference_stream(pkg, g=None):
    """-> dict: receivers, m, f, r (file order), case and kind per record, want (rows), counters"""
    g = g or load(REFERENCE)
    ints, refs, res = g["ints"], g["refs"], g["result"]
    kind, fflag, surf = ints[:, 0], ints[:, 5], ints[:, 6]
    idx = np.arange(len(res))
    pair, rel = idx[kind <= 1], idx[(kind == 2) & (surf == 0)]
    assert int(((kind == 2) & (surf == 1)).sum()) == UNREACHABLE and len(pair) + len(rel) + UNREACHABLE == len(res)

    # receivers: 0 has no location, then one per distinct reference of the surface pairs, then of the relative cases
    receivers, rx = [None], np.zeros(len(res), dtype=np.uint32)
    for cases, max_range in ((idx[kind == 1], 0.0), (rel, RECEIVER_RANGE_M)):
        uniq, inv = np.unique(refs[cases], axis=0, return_inverse=True)
        rx[cases] = len(receivers) + inv.reshape(-1)
        receivers += [dict(lat=float(a), lon=float(b), latlon_valid=1, max_range_m=max_range) for a, b in uniq]

    # pairs: the half that fflag names comes second
    ff = fflag[pair]
    first = records(pkg, pair, 0, ip.ADSB, kind[pair] == 0, 1 - ff, np.where(ff, ints[pair, 1], ints[pair, 3]),
                    np.where(ff, ints[pair, 2], ints[pair, 4]))
    second = records(pkg, pair, 1, ip.ADSB, kind[pair] == 0, ff, np.where(ff, ints[pair, 3], ints[pair, 1]),
                     np.where(ff, ints[pair, 4], ints[pair, 2]))
    single = records(pkg, rel, 0, ip.ADSB, np.ones(len(rel), dtype=bool), fflag[rel], ints[rel, 1], ints[rel, 2])
    far = beyond(refs[rel, 0], refs[rel, 1], g["lat_bits"][rel], g["lon_bits"][rel], RECEIVER_RANGE_M) & (res[rel] == 0)
    rel_result = np.where((res[rel] == 0) & ~far, 2, -1)
    want = [rows(pkg, kind[pair] == 1, np.full(len(pair), -1), 0, g["lat_bits"][pair], g["lon_bits"][pair]),
            rows(pkg, kind[pair] == 1, res[pair], 0, g["lat_bits"][pair], g["lon_bits"][pair]),
            rows(pkg, np.zeros(len(rel), dtype=bool), rel_result, 2, g["lat_bits"][rel], g["lon_bits"][rel])]
    case = np.concatenate([pair, pair, rel])
    k = np.concatenate([np.zeros(len(pair), dtype=np.int64), np.ones(len(pair), dtype=np.int64), np.zeros(len(rel), dtype=np.int64)])
    order = np.lexsort((k, case))  # file order
    pres = res[pair]
    counters = dict.fromkeys(COUNTERS, 0)
    counters.update(cpr_surface=2 * int((kind == 1).sum()), cpr_airborne=2 * int((kind == 0).sum()) + len(rel),
                    cpr_global_ok=int((pres == 0).sum()), cpr_global_bad=int((pres == -2).sum()),
                    cpr_global_skipped=int((pres == -1).sum()), cpr_local_ok=int((rel_result == 2).sum()),
                    cpr_local_receiver_relative=int((rel_result == 2).sum()), cpr_local_range_checks=int(far.sum()),
                    cpr_local_skipped=len(pair) + int((pres == -1).sum()) + int((rel_result == -1).sum()),
                    aircraft=len(pair) + len(rel))
    sweep = dict(receivers=receivers, m=np.concatenate([first[0], second[0], single[0]]),
                 f=np.concatenate([first[1], second[1], single[1]]), r=rx[case], case=case, kind=kind[case].astype(np.int64),
                 want=np.concatenate(want), counters=counters, cases=len(pair) + len(rel))
    return in_case_order(sweep, order)


def chained_stream(pkg, g=None):
    g = g or load(CHAINED)
    pairs, third, res = g["pairs"], g["third"], g["result"]
    n = len(res)
    case, place = np.arange(n), third[:, 0]
    air = np.ones(n, dtype=bool)
    first = records(pkg, case, 0, ip.TISB, air, 0, pairs[place, 0], pairs[place, 1])
    second = records(pkg, case, 1, ip.TISB, air, 1, pairs[place, 2], pairs[place, 3])
    last = records(pkg, case, 2, ip.ADSB, third[:, 4] == 0, third[:, 3], third[:, 1], third[:, 2])
    plat, plon = g["p_lat_bits"][place], g["p_lon_bits"][place]
    far = beyond(plat.view(np.float64), plon.view(np.float64), g["lat_bits"], g["lon_bits"], AIRCRAFT_RANGE_M) & (res == 0)
    result = np.where((res == 0) & ~far, 1, -1)
    none = np.zeros(n, dtype=bool)
    want = [rows(pkg, none, np.full(n, -1), 0, plat, plon), rows(pkg, none, np.zeros(n, dtype=np.int64), 0, plat, plon),
            rows(pkg, third[:, 4] == 1, result, 1, g["lat_bits"], g["lon_bits"])]
    k = np.repeat(np.arange(3), n)
    counters = dict.fromkeys(COUNTERS, 0)
    ok = int((result == 1).sum())
    counters.update(cpr_surface=int((third[:, 4] == 1).sum()), cpr_airborne=2 * n + int((third[:, 4] == 0).sum()),
                    cpr_global_ok=n, cpr_local_ok=ok, cpr_local_aircraft_relative=ok, cpr_local_range_checks=int(far.sum()),
                    cpr_local_skipped=n + n - ok, aircraft=n)
    sweep = dict(receivers=[None], m=np.concatenate([first[0], second[0], last[0]]),
                 f=np.concatenate([first[1], second[1], last[1]]), r=np.zeros(3 * n, dtype=np.uint32), case=np.tile(case, 3),
                 kind=np.full(3 * n, KIND_CHAINED), want=np.concatenate(want), counters=counters, cases=n,
                 half_cell_refusals=int((res == -1).sum()))
    return in_case_order(sweep, np.lexsort((k, sweep["case"])))


def mismatches(sweep, got, limit=10):
    """rows compared field by field, the coordinates as uint64 -> [(case, kind, got, want)], at most `limit`"""
    want = sweep["want"]
    assert len(got) == len(want)
    bad = np.zeros(len(want), dtype=bool)
    for name in ("decoded", "relative", "surface", "result"):
        bad |= got[name] != want[name]
    for name in ("lat", "lon"):
        bad |= np.ascontiguousarray(got[name]).view(np.uint64) != np.ascontiguousarray(want[name]).view(np.uint64)
    return int(bad.sum()), [(int(sweep["case"][i]), int(sweep["kind"][i]), ps.rows_of(got[i:i + 1])[0], ps.rows_of(want[i:i + 1])[0])
                            for i in np.flatnonzero(bad)[:limit]]


def run(pkg, sweep, host, capacity, pieces=None):
    """the stream through one position tracker -> rows, statistics"""
    t = pkg.capi.PositionTracker(capacity=capacity, receivers=sweep["receivers"], host=host)
    k = pieces or len(sweep["m"])
    out = np.concatenate([t.update(sweep["m"][i:i + k], sweep["f"][i:i + k], sweep["r"][i:i + k]) for i in range(0, len(sweep["m"]), k)])
    st = t.stats()
    t.close()
    return out, st
