"""aircraft_streams.random_stream through one tracker with everything enabled -- the aircraft table, Mode A/C matching,
the reduced Beast output's verdicts, SBS, aircraft.pb, the VRS list and the receiver range --, and the second readings of
all of them over the same steps.  test_aircraft_model.py holds the host object to the second readings, test_gpu_aircraft_
table.py the device to the host object's bytes.

The stream is cut into CUTS update steps; after each one comes what trackPeriodicUpdate does, an expiry and a Mode A/C
match at the latest time so far.  A tracker is observed after every step (the snapshot, the hits, every receiver's codes,
the range rows and distances) and the writers write once at the end, a second after the stream's latest time."""
import numpy as np

import aircraft_streams as acs
import indep_range as ir
import indep_range_pb
import indep_reduce as ired
import indep_sbs as isbs
import indep_vrs as iv
import modeac_streams as mas
import range_streams as rs
import reduce_streams

CUTS = 8
INTERVAL_MS = 1000
SBS_KW = dict(gnss=True, utc_offset_ms=7200000)


def steps_of(m, f, r, cuts=CUTS):
    steps, latest, last = [], 0, 0
    edges = [len(m) * k // cuts for k in range(cuts + 1)]
    for a, b in zip(edges[:-1], edges[1:]):
        steps.append(("update", m[a:b], f[a:b], r[a:b]))
        latest = max(latest, int(m["sysTimestampMsg"][a:b].max()))
        tracked = (m["msgtype"][a:b] != 32) & (f["addr"][a:b] != 0)
        if tracked.any():
            last = int(m["sysTimestampMsg"][a:b][tracked][-1])  # messageNow(): the last tracked message's time
        steps += [("expire", latest), ("match", latest, last)]
    return steps, latest + 1000


def tracker(pkg, receivers, host, capacity=1024):
    return pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, host=host, table=True, modeac=True,
                                    reduce_interval_ms=INTERVAL_MS, sbs=True, pb=True, vrs=True, range=True, polar=True)


def run_library(t, steps, now, pieces=None):
    """-> dict of everything the tracker delivers, as bytes or as comparable Python values"""
    rows, nic, fwd, sbs, obs = [], [], [], [], []
    for s in steps:
        if s[0] == "expire":
            t.expire(s[1])
        elif s[0] == "match":
            t.modeac_match(s[1], s[2])
        else:
            _, m, f, r = s
            k = pieces or len(m)
            for i in range(0, len(m), k):
                o, q, w, row = t.update_sbs(m[i:i + k], f[i:i + k], r[i:i + k], forward=True)
                rows.append(o), nic.append(q), fwd.append(w), sbs.append(row)
        o = mas.observe(t, t.nrx)
        o["range"] = (rs.read_rows(t.range_read()), [int(d) for d in t.range_distances()])
        obs.append(o)
    m, f, _ = reduce_streams.records(steps)
    out = dict(rows=np.concatenate(rows), nic=np.concatenate(nic), fwd=np.concatenate(fwd), sbs=np.concatenate(sbs), obs=obs)
    out["sbs_wire"] = t.sbs_wire(m, f, out["sbs"], now_ms=now, **SBS_KW)
    out["reduce_wire"] = t.reduce_wire(m, out["fwd"])
    out["pb"], out["range_pb"], out["vrs"] = t.aircraft_pb(now), t.range_pb(), t.vrs(now)
    out["stats"], out["margins"] = t.stats(), t.range_margins()
    if t.host:
        out["pb_margin"] = t.pb_margin
    return out


def same_bytes(got, want):
    """two run_library results of trackers that promise the same bytes"""
    for k in ("rows", "nic", "fwd", "sbs"):
        assert got[k].tobytes() == want[k].tobytes(), (k, [i for i in range(len(want[k])) if got[k][i] != want[k][i]][:5])
    assert len(got["obs"]) == len(want["obs"])
    for i, (g, w) in enumerate(zip(got["obs"], want["obs"])):
        assert g["snap_raw"].tobytes() == w["snap_raw"].tobytes(), (i, "snapshot")
        assert g["hits_raw"].tobytes() == w["hits_raw"].tobytes(), (i, "hits")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g["codes"], w["codes"])), (i, "codes")
        assert g["range"] == w["range"], (i, "range")
    for k in ("sbs_wire", "reduce_wire"):
        assert got[k][0] == want[k][0] and (got[k][1] == want[k][1]).all(), k
    for k in ("pb", "range_pb", "vrs"):
        assert got[k] == want[k], k


def run_models(pkg, receivers, steps, now, host, margins=True):
    """The second readings over the same steps, compared with the host object's run_library result `host` on the way (the
    writers' second readings read that result's last snapshot).  -> the counting table reading."""
    import pos_streams as ps
    import sbs_streams as ss
    m, f, r = reduce_streams.records(steps)
    # the table with Mode A/C matching: rows, NIC / Rc, every step's snapshot, hits and codes
    t = acs.Counting(receivers, 8)
    rows, nic, i = [], [], 0
    for s in steps:
        if s[0] == "expire":
            t.expire(s[1])
        elif s[0] == "match":
            t.match_ac(s[1], s[2])
        else:
            o, q = t.update(s[1], s[2], s[3])
            rows += o
            nic += q
        g = host["obs"][i]
        assert acs.differences(g["snap_raw"], t.snapshot(pkg.capi.AC_MEMBERS)) == [], i
        assert [(int(h["receiver"]), int(h["addr"]), int(h["mode_a_hit"]), int(h["mode_c_hit"])) for h in g["hits_raw"]] == t.hits(), i
        for k in range(len(receivers)):
            want = t.codes_of(k)
            assert [tuple(int(v) for v in c) for c in g["codes"][k]] == [tuple(c) for c in want], (i, k)
        i += 1
    assert ps.rows_of(host["rows"]) == ps.rows_of_model(rows)
    assert [(int(q["nic"]), int(q["rc"]), int(q["set"])) for q in host["nic"]] == nic
    # the verdicts
    red = ired.Tracker(receivers, 8, INTERVAL_MS)
    fwd = []
    for s in steps:
        if s[0] == "expire":
            red.expire(s[1])
        elif s[0] == "update":
            fwd += red.update(s[1], s[2], s[3])[2]
    assert [int(x) for x in host["fwd"]] == fwd
    assert host["reduce_wire"][0] == reduce_streams.stream_of(pkg, m, fwd)[0]
    # SBS: the rows and the text
    sb = isbs.Tracker(receivers, 8)
    srows = []
    for s in steps:
        if s[0] == "expire":
            sb.expire(s[1])
        elif s[0] == "update":
            srows += sb.update_sbs(s[1], s[2], s[3])[2]
    ss.same_rows(host["sbs"], srows)
    want, ends = isbs.stream(m, f, srows, now_ms=now, **SBS_KW)
    assert host["sbs_wire"][0] == want and (host["sbs_wire"][1] == ends).all()
    # the range after every step, and the two protobuf outputs with the distances
    rt = ir.RangeTracker(receivers, 8, polar=True)
    i = 0
    for s in steps:
        if s[0] == "expire":
            rt.expire(s[1])
        elif s[0] == "update":
            rt.update(s[1], s[2], s[3])
        assert host["obs"][i]["range"] == (rt.range_read(), rt.range_distances()), i
        i += 1
    # (the bearing's margin is 5 |q - floor(q) - 0.5| there and |k - round(k)| x 5 with k = (bearing - 2.5) / 5 here: the
    # same distance but for the rounding of a few double operations on numbers below 360)
    want = rt.range_margins()
    if margins:  # (the device's margins are its own libm's)
        assert host["margins"]["min_range_margin_m"] == want["min_range_margin_m"]
        assert abs(host["margins"]["min_bearing_margin_deg"] - want["min_bearing_margin_deg"]) < 1e-9
    snapshot = host["obs"][-1]["snap_raw"]
    w = indep_range_pb.Writer(pkg.capi.AC, len(receivers))
    dist = {k: getattr(a, "distance", 0) for k, a in rt.aircraft.items()}
    assert host["pb"] == w.files(snapshot, now, dist)[0]
    assert host["range_pb"] == [ir.polar_range_pb(x.polar) for x in rt.range]
    assert host["vrs"] == iv.documents(snapshot, pkg.capi.AC, len(receivers), now)[0]
    return t
