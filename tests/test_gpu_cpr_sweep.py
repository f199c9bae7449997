"""msd_cpr_impl.h as hipcc compiles it for the device, held to the reference's recorded answers through the product path:
the streams of tests/cpr_sweep.py (69 464 answers of cpr_reference.npz, of which 52 889 are reachable, and the chained
family of cpr_chained.npz) go through the tracker's walk kernel and the rows must equal the rows expected from the files
-- not merely the twin's --, in file order and shuffled so that one wavefront holds airborne, surface and relative
decodes and every outcome side by side.  The statistics equal the twin's.  The same coordinates then go through the
writers (SBS's %1.5f, VRS's %f, aircraft.pb's doubles) on the device and on the host object and are compared by bytes.
test_cpr_sweep.py holds the twin to the same expected rows on the CPU."""
import numpy as np
import pytest

import cpr_sweep as cs
import pos_streams as ps

pytestmark = pytest.mark.gpu
CAPACITY = {"reference": 1 << 17, "chained": 1 << 16}


@pytest.fixture(scope="module")
def sweeps(pkg):
    """every stream in both orders with the twin's rows and statistics of it, computed once"""
    out = {}
    for name, make in (("reference", cs.reference_stream), ("chained", cs.chained_stream)):
        s = make(pkg)
        for order, stream in (("file", s), ("shuffled", cs.shuffled(s))):
            rows, st = cs.run(pkg, stream, True, CAPACITY[name])
            assert cs.mismatches(stream, rows)[0] == 0 and st["min_gate_margin_m"] >= 1.0
            out[name, order] = (stream, rows, st)
    return out


@pytest.mark.parametrize("order", ["file", "shuffled"])
@pytest.mark.parametrize("name", ["reference", "chained"])
def test_rows_equal_the_recorded_answers(pkg, torch_cuda, sweeps, name, order):
    stream, _, hst = sweeps[name, order]
    got, st = cs.run(pkg, stream, False, CAPACITY[name])
    n, bad = cs.mismatches(stream, got)
    assert n == 0, (n, bad)
    assert {k: st[k] for k in cs.COUNTERS} == {k: hst[k] for k in cs.COUNTERS} == stream["counters"]
    print("%s, %s order: %d records, min_gate_margin_m gpu %.17g twin %.17g" % (name, order, len(got), st["min_gate_margin_m"],
                                                                               hst["min_gate_margin_m"]))
    assert st["min_gate_margin_m"] >= 1.0


def test_cut_without_regard_to_cases_or_wavefronts(pkg, torch_cuda, sweeps):
    """the shuffled reference stream in calls of 4093 records, a prime: pairs are cut between their halves"""
    stream, hrows, hst = sweeps["reference", "shuffled"]
    whole, wst = cs.run(pkg, stream, False, CAPACITY["reference"])
    cut, cst = cs.run(pkg, stream, False, CAPACITY["reference"], pieces=4093)
    assert cut.tobytes() == whole.tobytes(), cs.mismatches(dict(stream, want=whole), cut)
    assert cs.mismatches(stream, cut)[0] == 0
    assert {k: cst[k] for k in cs.COUNTERS} == {k: wst[k] for k in cs.COUNTERS} == {k: hst[k] for k in cs.COUNTERS}


def first_difference(got, want, ends, hends):
    """two streams of pieces that end at `ends` -> None, or the first piece that differs with both readings of it"""
    if got == want and np.array_equal(ends, hends):
        return None
    a = [0] + [int(e) for e in ends]
    b = [0] + [int(e) for e in hends]
    for i in range(len(hends)):
        x, y = got[a[i]:a[i + 1]], want[b[i]:b[i + 1]]
        if x != y:
            k = [j for j in range(max(len(x), len(y))) if j >= len(x) or j >= len(y) or x[j] != y[j]][0]
            return (i, k, x[max(k - 60, 0):k + 60], y[max(k - 60, 0):k + 60])
    return ("lengths", len(got), len(want))


def write(pkg, stream, host, capacity, **kw):
    t = pkg.capi.PositionTracker(capacity=capacity, receivers=stream["receivers"], host=host, table=True, sbs=True, **kw)
    out = dict(rows=t.update_sbs(stream["m"], stream["f"], stream["r"]))
    out["sbs"] = t.sbs_wire(stream["m"], stream["f"], out["rows"][3], now_is_received=True)
    if kw.get("vrs"):
        out["vrs"] = t.vrs_stream(ps.T0 + 1000)
    if kw.get("pb"):
        out["pb"] = t.aircraft_pb_stream(ps.T0 + 1000)
        if host:
            assert t.pb_margin >= pkg.capi.PB_RSSI_MARGIN_ULPS, t.pb_margin
    t.close()
    return out


def same_writes(stream, got, want):
    pos, nicrc, _, trk = got["rows"]
    hpos, hnicrc, _, htrk = want["rows"]
    n, bad = cs.mismatches(stream, pos)
    assert n == 0, (n, bad)
    assert pos.tobytes() == hpos.tobytes() and nicrc.tobytes() == hnicrc.tobytes()
    assert trk.tobytes() == htrk.tobytes(), [(i, trk[i], htrk[i]) for i in range(len(trk)) if trk[i].tobytes() != htrk[i].tobytes()][:5]
    assert first_difference(got["sbs"][0], want["sbs"][0], got["sbs"][1], want["sbs"][1]) is None  # a piece is a record's line
    for what in ("vrs", "pb"):
        if what in want:
            (g, grx), (h, hrx) = got[what], want[what]
            assert first_difference(g, h, grx["end"], hrx["end"]) is None, what
            assert grx.tobytes() == hrx.tobytes(), what


def test_writers_on_the_recorded_coordinates(pkg, torch_cuda, sweeps):
    """every coordinate the reference answered, printed by the device's decimal printers: SBS lines, the VRS list and
    aircraft.pb of a table tracker equal the host object's by bytes"""
    stream = sweeps["reference", "file"][0]
    want = write(pkg, stream, True, CAPACITY["reference"], pb=True, vrs=True)
    sbs, vrs, pb = want["sbs"][0], want["vrs"][0], want["pb"][0]
    lats = set(part.split(b",", 1)[0] for part in vrs.split(b'"Lat":')[1:])
    print("twin: SBS %d bytes in %d lines, VRS %d bytes with %d Lat of %d values, aircraft.pb %d bytes"
          % (len(sbs), sbs.count(b"\r\n"), len(vrs), vrs.count(b'"Lat":'), len(lats), len(pb)))
    assert sbs.count(b"\r\n") >= 30000 and len(sbs) > 3000000
    assert vrs.count(b'"Lat":') >= 20000 and len(lats) >= 10000 and vrs.count(b'"Long":-') >= 5000
    assert len(pb) > 2000000 and int(want["pb"][1]["with_positions"].sum()) >= 20000
    same_writes(stream, write(pkg, stream, False, CAPACITY["reference"], pb=True, vrs=True), want)


def test_sbs_on_the_chained_coordinates(pkg, torch_cuda, sweeps):
    """the third halves add tens of thousands of relative positions, many negative and many next to +-180"""
    stream = sweeps["chained", "shuffled"][0]
    want = write(pkg, stream, True, CAPACITY["chained"])
    sbs = want["sbs"][0]
    print("twin: SBS %d bytes in %d lines, %d next to +-180" % (len(sbs), sbs.count(b"\r\n"), sbs.count(b",179.9") + sbs.count(b",-179.9")
                                                               + sbs.count(b",-180.")))
    assert sbs.count(b"\r\n") >= 50000 and sbs.count(b",-") >= 20000
    assert sbs.count(b",179.9") >= 1000 and sbs.count(b",-179.9") >= 1000 and sbs.count(b",-180.") >= 200
    same_writes(stream, write(pkg, stream, False, CAPACITY["chained"]), want)
