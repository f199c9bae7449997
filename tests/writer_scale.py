"""The three shapes at which the tracker's stream writers are held to the host twin past one round of their scan
(msd_block_scan_impl.h: block_sums_scan walks the workgroups' sums 256 at a time, so past 65 536 records or items every
offset rests on what it carries from round to round), for tests/test_gpu_writer_scale.py on the GPU and
tests/test_writer_scale_model.py on the twin alone.  run_a / run_b / run_c drive one tracker -- the GPU object or the
twin, the same calls -- and return what its writers left; shape_a / shape_b / shape_c say on the twin's output that the
shape is what it is meant to be.  Streams come from aircraft_streams.wide_stream: no Python loop over records."""
import numpy as np

import aircraft_streams as acs

WT = 256  # a workgroup of the writers

# A: records past one round -- 263 172 records are 1 029 workgroups (five rounds) for the reduced Beast and the SBS
# writer, 65 793 aircraft and 3 receivers are 258 workgroups of items (two rounds) for aircraft.pb and the VRS list
A_AIRCRAFT, A_RECEIVERS = WT * WT + WT + 1, 3
# B: items past two rounds, many files -- 517 workgroups of items for aircraft.pb (an aircraft or a file head each), 521
# for VRS (a head and a tail per document): three rounds, through scan_kernel<4>
B_AIRCRAFT, B_RECEIVERS = 2 * WT * WT + WT + 1, 1024
# C: receivers past one round, hardly any aircraft -- 65 536 receivers (the most a tracker takes), on eight of them 300
# aircraft: 258 workgroups of nearly nothing but heads, and the range's 4 718 592 polar entries, 72 rounds
C_AIRCRAFT, C_RECORDS, C_RECEIVERS = 300, 1200, 1 << 16
C_USED = (0, 1, 255, 256, 257, 32767, 65534, 65535)
RANGE_BUCKETS = 72


def rounds(items):
    """rounds of block_sums_scan over the workgroups of `items` lanes"""
    return (-(-items // WT) + WT - 1) // WT


def stream_a(pkg):
    return acs.wide_stream(pkg, aircraft=A_AIRCRAFT, records=4 * A_AIRCRAFT, receivers=A_RECEIVERS, skipped_every=17, replies=True)


def stream_b(pkg):
    return acs.wide_stream(pkg, aircraft=B_AIRCRAFT, records=4 * B_AIRCRAFT, receivers=B_RECEIVERS, replies=True)


def stream_c(pkg):
    _, m, f, _ = acs.wide_stream(pkg, C_AIRCRAFT, C_RECORDS, replies=True)
    r = np.array(C_USED, dtype=np.uint32)[(np.arange(C_RECORDS) % C_AIRCRAFT) % len(C_USED)]  # an aircraft stays where it is
    return [None] * C_RECEIVERS, m, f, r


def messages_total(nrx):
    """a count per receiver for aircraft.pb's head: 0, one-byte and ten-byte varints"""
    return (np.arange(nrx, dtype=np.uint64) * np.uint64(0x0040201008040201)) ^ (np.arange(nrx, dtype=np.uint64) >> np.uint64(3))


def _now(m):
    return int(m["sysTimestampMsg"][-1])


def run_a(pkg, stream, host):
    receivers, m, f, r = stream
    t = pkg.capi.PositionTracker(capacity=1 << 17, receivers=receivers, host=host, table=True, sbs=True, pb=True, vrs=True,
                                 reduce_interval_ms=1000)
    now = _now(m)
    out = {}
    rows = t.update_sbs(m, f, r, nicrc=True, forward=True)
    out["rows"] = rows
    out["reduce_wire"] = t.reduce_wire(m, rows[2])
    out["sbs_wire"] = t.sbs_wire(m, f, rows[3], now_ms=now, gnss=True)
    out["aircraft_pb"] = t.aircraft_pb_stream(now)
    out["pb_margin"] = t.pb_margin
    out["vrs"] = t.vrs_stream(now)
    for part in range(8):
        out["vrs %d of 8" % part] = t.vrs_stream(now, part=part, n_parts=8)
    out["snapshot"] = (t.snapshot(),)
    out["live"], out["stats"] = t.live(), t.stats()
    t.close()
    return out


def run_b(pkg, stream, host):
    receivers, m, f, r = stream
    t = pkg.capi.PositionTracker(capacity=1 << 18, receivers=receivers, host=host, table=True, pb=True, vrs=True)
    now = _now(m)
    out = {}
    out["rows"] = t.update_nicrc(m, f, r)
    out["aircraft_pb"] = t.aircraft_pb_stream(now, messages_total=messages_total(len(receivers)))
    out["pb_margin"] = t.pb_margin
    out["vrs"] = t.vrs_stream(now)
    out["snapshot"] = (t.snapshot(),)
    out["live"], out["stats"] = t.live(), t.stats()
    t.close()
    return out


def run_c(pkg, stream, host):
    receivers, m, f, r = stream
    t = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, host=host, table=True, pb=True, vrs=True, range=True,
                                 polar=True)
    now = _now(m)
    out = {}
    out["rows"] = t.update_nicrc(m, f, r)
    out["aircraft_pb"] = t.aircraft_pb_stream(now)
    out["pb_margin"] = t.pb_margin
    out["vrs"] = t.vrs_stream(now)
    out["range_pb"] = t.range_pb_stream()
    out["range_read"] = (t.range_read(),)
    out["range_margins"] = t.range_margins()
    out["snapshot"] = (t.snapshot(),)
    out["live"], out["stats"] = t.live(), t.stats()
    t.close()
    return out


COMPARED = {"a": ["rows", "reduce_wire", "sbs_wire", "aircraft_pb", "vrs"] + ["vrs %d of 8" % p for p in range(8)] + ["snapshot"],
            "b": ["rows", "aircraft_pb", "vrs", "snapshot"],
            "c": ["rows", "aircraft_pb", "vrs", "range_pb", "range_read", "snapshot"]}


def first_difference(name, got, want):
    """None, or where the GPU object's output `name` leaves the twin's: the part of the tuple and, for a stream, the
    first differing byte and the receiver row or record it lies in"""
    assert len(got) == len(want), name
    ends = None  # of a (stream, ends) or (stream, receiver rows) pair
    if isinstance(want[0], bytes):
        ends = (want[1]["end"] if want[1].dtype.names else want[1]).astype(np.uint64)
    for k, (a, b) in enumerate(zip(got, want)):
        if a is None and b is None:
            continue
        if isinstance(b, bytes):
            if a == b:
                continue
            x, y = np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)
            n = min(len(x), len(y))
            d = np.flatnonzero(x[:n] != y[:n])
            at = int(d[0]) if d.size else n
            row = None if ends is None else int(np.searchsorted(ends, at, side="right"))
            return "%s[%d]: %d and %d bytes, first difference at byte %d (row %s): %s / %s" % (
                name, k, len(x), len(y), at, row, x[at:at + 16].tobytes().hex(), y[at:at + 16].tobytes().hex())
        if a.dtype != b.dtype or a.shape != b.shape:
            return "%s[%d]: %s %s and %s %s" % (name, k, a.dtype, a.shape, b.dtype, b.shape)
        if a.tobytes() != b.tobytes():
            rows = a.reshape(len(a), -1).view(np.uint8) if a.dtype.names is None else a.view(np.uint8).reshape(len(a), -1)
            other = b.reshape(len(b), -1).view(np.uint8) if b.dtype.names is None else b.view(np.uint8).reshape(len(b), -1)
            i = int(np.flatnonzero((rows != other).any(axis=1))[0])
            return "%s[%d]: first difference in row %d of %d: %s / %s" % (name, k, i, len(a), a[i], b[i])
    return None


def _lengths(ends):
    return np.diff(np.concatenate([[0], ends.astype(np.int64)]))


def _common(pkg, out, aircraft, gate=True):
    assert out["live"] == aircraft == len(out["snapshot"][0])
    for name in ("aircraft_pb", "vrs"):
        stream, rx = out[name]
        assert int(rx["aircraft"].sum()) == out["live"], name
        assert int(rx["end"][-1]) == len(stream) and (np.diff(rx["end"].astype(np.int64)) > 0).all(), name
    if gate:
        assert out["stats"]["min_gate_margin_m"] >= 1.0, out["stats"]["min_gate_margin_m"]


def shape_a(pkg, stream, out):
    """on the twin's output: everyone is live and written, the eight VRS parts share the aircraft out, both record
    writers have both outcomes, and the comparison carries no margin"""
    receivers, m, f, r = stream
    n = len(m)
    assert n == 4 * A_AIRCRAFT == 263172 and rounds(n) == 5 and rounds(A_AIRCRAFT + A_RECEIVERS) == 2
    _common(pkg, out, A_AIRCRAFT)
    whole = out["vrs"][1]["aircraft"].astype(np.int64)
    parts = sum(out["vrs %d of 8" % p][1]["aircraft"].astype(np.int64) for p in range(8))
    assert (parts == whole).all() and all(out["vrs %d of 8" % p][1]["aircraft"].sum() > 0 for p in range(8))
    for name in ("reduce_wire", "sbs_wire"):
        stream_, ends = out[name]
        assert len(ends) == n and int(ends[-1]) == len(stream_) < 1 << 32, name
    # both outcomes in both record writers: 247 692 records with a verdict, of them 164 100 seen twice and so written by
    # the reduced Beast writer; 81 273 records without an SBS line
    verdict = out["rows"][2]
    both = pkg.capi.REDUCE_FORWARD | pkg.capi.REDUCE_SEEN_TWICE
    written = _lengths(out["reduce_wire"][1]) > 0
    silent = int((_lengths(out["sbs_wire"][1]) == 0).sum())
    assert (int((verdict != 0).sum()), int(written.sum()), silent) == (247692, 164100, 81273)
    assert (written == (verdict & both == both)).all()
    assert out["pb_margin"] >= pkg.capi.PB_RSSI_MARGIN_ULPS, out["pb_margin"]


def shape_b(pkg, stream, out):
    receivers, m, f, r = stream
    assert len(receivers) == B_RECEIVERS and len(m) == 4 * B_AIRCRAFT
    # aircraft.pb's items are the aircraft and a head per file, VRS's the aircraft and a head and a tail per document
    assert -(-(B_AIRCRAFT + B_RECEIVERS) // WT) == 518 and -(-(B_AIRCRAFT + 2 * B_RECEIVERS) // WT) == 522
    assert rounds(B_AIRCRAFT + B_RECEIVERS) == rounds(B_AIRCRAFT + 2 * B_RECEIVERS) == 3
    _common(pkg, out, B_AIRCRAFT)
    assert (out["aircraft_pb"][1]["aircraft"] >= B_AIRCRAFT // B_RECEIVERS).all()  # every file has its share
    assert out["pb_margin"] >= pkg.capi.PB_RSSI_MARGIN_ULPS, out["pb_margin"]


def shape_c(pkg, stream, out):
    receivers, m, f, r = stream
    assert len(receivers) == C_RECEIVERS and set(r.tolist()) == set(C_USED)
    assert rounds(C_AIRCRAFT + C_RECEIVERS) == 2 and rounds(C_RECEIVERS * RANGE_BUCKETS) == 72
    _common(pkg, out, C_AIRCRAFT)
    for name in ("aircraft_pb", "vrs"):
        used = np.flatnonzero(out[name][1]["aircraft"])
        assert used.tolist() == list(C_USED), name
    stream_, ends = out["range_pb"]
    # (an untouched receiver's entries: 32 00, then 71 of four bytes)
    assert len(ends) == C_RECEIVERS and int(ends[-1]) == len(stream_) == (2 + 4 * (RANGE_BUCKETS - 1)) * C_RECEIVERS
    # no receiver has a location: the range evaluates nothing and its margins stay infinite -- no libm margin to carry
    assert int(out["range_read"][0]["evaluated"].sum()) == 0
    assert all(v == float("inf") for v in out["range_margins"].values()), out["range_margins"]
    assert out["pb_margin"] >= pkg.capi.PB_RSSI_MARGIN_ULPS, out["pb_margin"]
