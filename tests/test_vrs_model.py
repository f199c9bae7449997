"""The VRS output's host object (msd_pos_host_vrs_enable, msd_pos_host_vrs: a plain sequential writer over the exported
entries, snprintf with the reference's format strings) on the CPU: the host object == the second reading of
tests/indep_vrs.py == documents written out by hand, and every document is JSON.  The GPU is held against the host object
in test_gpu_vrs.py."""
import json

import pytest

import aircraft_streams as acs
import indep_positions as ip
import vrs_streams as vs

T0 = vs.T0  # 1600000000000


def twin(pkg, receivers, capacity=2048, vrs=True):
    return pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, host=True, table=True, vrs=vrs)


def fed(pkg, builder, receivers=(None,)):
    t = twin(pkg, list(receivers), 64)
    _, m, f, r = builder.step()
    t.update_nicrc(m, f, r)
    return t


@pytest.fixture(scope="module")
def host_runs(pkg):
    out = {}
    for name, make in vs.TABLES.items():
        sc = make(pkg)
        t = twin(pkg, sc[0])
        out[name] = (sc, vs.run(t, sc))
        t.close()
    return out


def objects(doc):
    return {int(a["Icao"], 16) & 0xFF: a for a in json.loads(doc.decode("ascii"))["acList"]}


def test_empty_documents(pkg):
    t = twin(pkg, [None, None], 64)
    assert t.vrs(0) == [b'{"acList":[]}\n'] * 2 and t.vrs(T0, 7, 8) == [b'{"acList":[]}\n'] * 2
    stream, rx = t.vrs_stream(T0)
    assert len(stream) == 28 and rx["end"].tolist() == [14, 28] and not rx["aircraft"].any() and not rx["reserved"].any()
    t.close()


def test_minimal_aircraft_by_hand(pkg):
    """two all-call replies and nothing else: a signal level never written prints 255 * 9e-5 / 8 as 0; the aircraft is
    written up to 5000 ms after it was seen and not one millisecond later; it is in part 0 of 8 (0x0D6 >> 8) alone"""
    b = acs.Builder(pkg)
    vs.two(b, T0, 0x4840D6, source=ip.MODE_S, msgtype=11)
    t = fed(pkg, b)
    want = b'{"acList":[{"Sig":0,"Icao":"4840D6","Mlat":false,"Tisb":false,"Gnd":false,"Trt":1,"Cmsgs":2}]}\n'
    assert t.vrs(T0 + 1) == [want] and t.vrs(T0 + 5001) == [want] and t.vrs(T0 + 5002) == [b'{"acList":[]}\n']
    assert t.vrs(T0) == [b'{"acList":[]}\n']  # seen one millisecond after now: the difference wraps
    assert t.vrs(T0 + 1, 0, 8) == [want] and t.vrs(T0 + 1, 1, 8) == [b'{"acList":[]}\n']
    assert t.vrs(T0 + 1, 0xD6, 2048) == [want] and t.vrs(T0 + 1, 0xD7, 2048) == [b'{"acList":[]}\n']
    t.close()


def test_two_aircraft_by_hand(pkg):
    """a velocity, a squawk, an altitude heard three times and a callsign with a quote, in address order with one comma.
    Sig: two levels of 0.25 and six of 1e-5 are 255 * 0.50007 / 8 = 15.94; gs = sqrt(100^2 + 100^2 + 0.5) = 141.4"""
    b = acs.Builder(pkg)
    vs.two(b, T0, 0x4840D7, signal=0.25, velocity_valid=1, ew_vel=-100, ns_vel=100, metype=19)
    for k in range(3):
        b.alt(T0 + k, 0x4840D6, -975)
    b.rec(T0 + 3, 0x4840D6, source=vs.S4, msgtype=21, squawk_valid=1, squawk=0x0123, callsign_valid=1, callsign=b'A"B     ')
    t = fed(pkg, b)
    want = (b'{"acList":[{"Sig":0,"Icao":"4840D6","Alt":-975,"Call":"A\\"B     ","Mlat":false,"Tisb":false,"Sqk":"0123",'
            b'"Gnd":false,"Trt":1,"Cmsgs":4},'
            b'{"Sig":16,"Icao":"4840D7","Mlat":false,"Tisb":false,"Spd":141,"SpdTyp":0,"Trak":315,"TrkH":false,'
            b'"Gnd":false,"Trt":3,"Cmsgs":2}]}\n')
    assert t.vrs(T0 + 1000) == [want]
    t.close()


@pytest.mark.parametrize("name", list(vs.TABLES))
def test_table_against_the_second_reading(pkg, host_runs, name):
    sc, got = host_runs[name]
    model = vs.run_model(pkg, lambda rx: twin(pkg, rx, vrs=False), sc)
    assert len(got) == len(model) == len(sc[2]) > 0
    for (stream, rx), (docs, counts) in zip(got, model):
        assert vs.split(stream, rx) == docs
        assert [int(x) for x in rx["aircraft"]] == counts and not rx["reserved"].any()
        for doc, n in zip(docs, counts):
            assert len(json.loads(doc.decode("ascii"))["acList"]) == n and doc.endswith(b"]}\n")
        longest = max([len(o) for doc in docs for o in doc[11:-3].split(b"},{")] + [0])
        assert longest + 3 <= pkg.capi.VRS_AIRCRAFT_MAX


def test_parts_against_the_second_reading(pkg):
    sc = vs.parts_table(pkg)
    t = twin(pkg, sc[0])
    t.update_nicrc(*sc[1][0][1:])
    snap = t.snapshot()
    for n_parts in (1, 2, 8, 2048):
        seen = []
        for part in range(n_parts):
            docs = t.vrs(T0 + 100, part, n_parts)
            assert docs == vs.iv.documents(snap, pkg.capi.AC, 2, T0 + 100, part, n_parts)[0]
            for r, doc in enumerate(docs):
                for a in json.loads(doc)["acList"]:
                    addr = int(a["Icao"], 16)
                    assert (addr & 2047) * n_parts // 2048 == part
                    seen.append((r, addr))
        assert sorted(seen) == sorted((r, 0x4B0000 + 0x1000 * r + low) for r in range(2) for low in vs.PART_LOWS)
    t.close()


def test_counts_and_commas(pkg, host_runs):
    T = vs.TILE
    (stream, rx), = host_runs["counts"][1]
    assert [int(x) for x in rx["aircraft"]] == [1, 0, T - 1, T, T + 1, 2 * T + 1, 0]
    docs = vs.split(stream, rx)
    assert docs[1] == docs[6] == b'{"acList":[]}\n' and docs[0].count(b"},{") == 0 and docs[5].count(b"},{") == 2 * T
    (stream, rx), = host_runs["comma"][1]
    assert [int(x) for x in rx["aircraft"]] == vs.COMMA_COUNTS
    for doc, n in zip(vs.split(stream, rx), vs.COMMA_COUNTS):
        assert doc.startswith(b'{"acList":[{' if n else b'{"acList":[]') and doc.count(b",{") == max(n - 1, 0)
        assert all((int(a["Icao"], 16) & 2047) >> 8 == vs.PART for a in json.loads(doc)["acList"])


def test_staleness_is_the_opposite_of_aircraft_pb(pkg, host_runs):
    sc, ((stream, rx),) = host_runs["stale"]
    assert sorted(objects(stream)) == [1, 4]
    t = pkg.capi.PositionTracker(capacity=64, receivers=[None], host=True, table=True, vrs=True, pb=True)
    t.update_nicrc(*sc[1][0][1:])
    import indep_aircraft_pb as ipb
    pb = [a["addr"] & 0xFF for a in ipb.read_file(t.aircraft_pb(sc[2][0][1])[0])["aircraft"]]
    assert pb == [1, 2, 3, 4] and t.vrs(sc[2][0][1]) == [stream]
    t.close()


def test_kinds_print_what_their_branch_says(pkg, host_runs):
    (stream, rx), = host_runs["kinds"][1]
    ac = objects(stream)
    assert len(ac) == 28 == int(rx["aircraft"][0])
    assert "Alt" not in ac[1] and ac[2]["Alt"] == -975 and ac[3]["GAlt"] == -1200 and "Alt" not in ac[3]
    assert ac[4]["Alt"] == 12000 and ac[4]["GAlt"] == 12125
    assert ac[5]["TAlt"] == 36000 and ac[5]["InHg"] == 29.92 and ac[6]["TAlt"] == -500 and "TAlt" not in ac[7]
    assert ac[7]["InHg"] == 29.91 and ac[7]["TTrk"] == 359 and "InHg" not in ac[6]
    assert (ac[8]["Spd"], ac[8]["SpdTyp"], ac[8]["Trak"], ac[8]["TrkH"], ac[8]["Sig"]) == (141, 0, 315, False, 16)
    assert (ac[9]["Spd"], ac[9]["SpdTyp"]) == (280, 2) and (ac[10]["Spd"], ac[10]["SpdTyp"]) == (421, 3)
    assert not {"Spd", "SpdTyp", "Trak", "TrkH", "Vsi", "Sqk", "Call", "Lat"} & set(ac[11])
    assert (ac[12]["Trak"], ac[12]["TrkH"]) == (359, False) and (ac[13]["Trak"], ac[13]["TrkH"]) == (351, True)
    assert (ac[14]["Trak"], ac[14]["TrkH"]) == (180, True)
    assert (ac[15]["Vsi"], ac[15]["VsiT"]) == (-2048, 1) and (ac[16]["Vsi"], ac[16]["VsiT"]) == (-64, 0)
    assert "Vsi" not in ac[17] and ac[17]["Sqk"] == "7700"
    assert [ac[k]["Gnd"] for k in (18, 19, 20, 21)] == [False, True, False, True]
    assert [ac[k]["Trt"] for k in (22, 23, 24, 25)] == [1, 3, 4, 5]
    assert ac[26]["Lat"] < -33 and ac[26]["Long"] < -70 and ac[26]["PosTime"] == T0 + 400 and not ac[26]["Tisb"]
    assert ac[27]["Tisb"] is True and "Lat" not in ac[27] and "PosTime" not in ac[27]
    assert ac[28]["Tisb"] is True and abs(ac[28]["Lat"] - 50.0) < 1e-3 and not ac[28]["Mlat"]
    assert b'"Lat":-33.' in stream and b'"Long":-70.' in stream


def test_escapes(pkg, host_runs):
    (stream, rx), = host_runs["escapes"][1]
    calls = [a["Call"] for a in json.loads(stream)["acList"]]
    assert calls == ['AB"CD   ', "EF\\GH   ", "\x01\x1f\x7f\x80\xff   ", "ABC", "12345678", '""\\\\\xfe\xfd\xfc\xfb', ""]
    assert b'"Call":"AB\\"CD   "' in stream and b'"Call":"EF\\\\GH   "' in stream and b'"Call":"ABC"' in stream
    assert b'"Call":"\\u0001\\u001f\x7f\\u0080\\u00ff   "' in stream and b'"Call":""' in stream


def test_bounds(pkg, host_runs):
    (stream, rx), = host_runs["bounds"][1]
    ac = json.loads(stream)["acList"]
    assert [a["Sig"] for a in ac[:7]] == [956250000, 4271250000, 0, 0, 0, 0, 0] and ac[6]["Icao"] == "4F0006"
    wide = ac[7]
    assert wide["Sig"] == 3825000000 and wide["Alt"] == -99900 and wide["GAlt"] == wide["TAlt"] == -(1 << 31)
    assert wide["Vsi"] == -32768 and wide["InHg"] == 1571.8 and wide["Call"] == "\xff" * 8 and wide["Sqk"] == "ffff" and wide["TTrk"] == 65535
    assert wide["Lat"] < -89 and wide["Long"] < -179 and wide["Trak"] == 359
    obj = stream[stream.index(b',{"Sig":3825000000'):-3]
    assert 330 < len(obj) <= pkg.capi.VRS_AIRCRAFT_MAX


def test_refused_and_repeated_calls(pkg, host_runs):
    sc, want = host_runs["expiring"]
    t = twin(pkg, sc[0])
    got = vs.run(t, sc, refuse=True)
    t.close()
    assert [(s, r.tobytes()) for s, r in got] == [(s, r.tobytes()) for s, r in want]
    assert [int(r["aircraft"].sum()) for _, r in want] == [40, 40, 14, 8]
