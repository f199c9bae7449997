"""aircraft.pb's host object (msd_pos_host_pb_enable, msd_pos_host_aircraft_pb: a plain sequential encoder over the
exported entries) on the CPU: the host object == the second reading of tests/indep_aircraft_pb.py (a wire reader and
writer over a field table, with the selection and written-state rules) == files written out by hand.  The GPU is held
against the host object in test_gpu_aircraft_pb.py."""
import numpy as np
import pytest

import aircraft_streams as acs
import indep_aircraft_pb as ipb
import indep_positions as ip
import pb_streams as pbs

T0 = pbs.T0  # 1600000000000


def twin(pkg, receivers, capacity=1024, pb=True):
    return pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, host=True, table=True, pb=pb)


def fed(pkg, builder, receivers=(None,)):
    t = twin(pkg, list(receivers), 64)
    _, m, f, r = builder.step()
    t.update_nicrc(m, f, r)
    return t


def test_empty_and_header_only_files(pkg):
    t = twin(pkg, [None, None], 64)
    assert t.aircraft_pb(0) == [b"", b""] and t.aircraft_pb(999) == [b"", b""]  # now = 0, messages = 0: zero bytes
    stream, rx = t.aircraft_pb_stream(999)
    assert stream == b"" and rx["end"].tolist() == [0, 0] and not rx["aircraft"].any() and t.pb_margin == float("inf")
    # now = 1600000005 = 0x5F5E1005: 05 20 78 7A 05 in groups of seven from the low end; messages = 300 = 0xAC 0x02
    head = bytes.fromhex("08 85 A0 F8 FA 05")
    assert t.aircraft_pb(T0 + 5999, [300, 0]) == [head + bytes.fromhex("10 AC 02"), head]
    assert t.aircraft_pb(1000, [0, 1 << 63]) == [b"\x08\x01", b"\x08\x01\x10" + b"\x80" * 9 + b"\x01"]
    t.close()


def test_minimal_aircraft(pkg):
    """two all-call replies and nothing else: addr, messages, seen, the rssi of a signal level never written, and an empty
    valid_source"""
    b = acs.Builder(pkg)
    pbs.two(b, T0, 0x4840D6, source=ip.MODE_S, msgtype=11)
    t = fed(pkg, b)
    want = bytes.fromhex(
        "7A 16"                    # aircraft (15), 22 bytes
        "08 D6 81 A1 02"           # addr 0x4840D6
        "50 02"                    # messages 2
        "58 81 80 BA BB C8 2E"     # seen 1600000000001
        "65 33 F4 45 C2"           # rssi (float)(10 * log10(9e-5 / 8)) = -49.488476
        "BA 09 00")                # valid_source (151), empty
    assert t.aircraft_pb(999) == [want]
    head = bytes.fromhex("08 DA A0 F8 FA 05")  # now = 1600000090
    # seen + 90000 == now_ms stays, one millisecond later the aircraft is gone
    assert t.aircraft_pb(T0 + 90001) == [head + want] and t.aircraft_pb(T0 + 90002, [5]) == [head + b"\x10\x05"]
    t.close()


def test_negative_values_and_an_omitted_latitude(pkg):
    """a barometric altitude of -975 ft as a ten-byte varint, a roll of -35.15625 degrees, lat == 0.0 not written"""
    b = acs.Builder(pkg)
    pbs.two(b, T0 + 10, 0x4840D7, signal=0.5, source=pbs.S4, msgtype=20, commb_format=8, commb_valid=1, roll_q=-200,
            altitude_baro_valid=1, altitude_baro=-975)
    t = fed(pkg, b)
    want = bytes.fromhex(
        "7A 2D"
        "08 D7 81 A1 02"
        "28 B1 F8 FF FF FF FF FF FF FF 01"  # alt_baro -975, sign-extended to 64 bits
        "50 02"
        "58 8B 80 BA BB C8 2E"              # seen 1600000000011
        "65 52 7D 10 C1"                    # rssi of two levels of 0.5 and six of 1e-5: -9.030596
        "ED 01 00 A0 0C C2"                 # roll (29): (-200 & 511) * 45 / 256 - 90 = -35.15625
        "BA 09 06 A8 06 04 E8 06 04")       # valid_source: altitude (101) = 4, roll (109) = 4 (Mode S, checked)
    assert t.aircraft_pb(999) == [want]
    d = ipb.read_file(want)["aircraft"][0]
    assert d["alt_baro"] == -975 and d["roll"] == -35.15625 and "lat" not in d and "lon" not in d
    t.close()


@pytest.mark.parametrize("name", list(pbs.TABLES))
def test_table_against_the_second_reading(pkg, name):
    sc = pbs.TABLES[name](pkg)
    t = twin(pkg, sc[0])
    got = pbs.run(t, sc)
    t.close()
    model = pbs.run_model(pkg, lambda rx: twin(pkg, rx, pb=False), sc)
    assert len(got) == len(model) == len(sc[2])
    for (stream, rx, margin), (files, rows, model_margin) in zip(got, model):
        assert pbs.split(stream, rx) == files
        assert [(int(x["aircraft"]), int(x["with_positions"]), int(x["tisb_positions"])) for x in rx] == rows
        assert margin == model_margin and not rx["reserved"].any()
        for f, row in zip(files, rows):  # and every file reads back: ascending fields, no zero scalar, nothing left out
            assert len(ipb.read_file(f)["aircraft"]) == row[0]
        entries = [a for f in files for a in ipb.read(ipb.UPDATE, f).get("aircraft", [])]
        assert max([len(a) + 3 for a in entries] + [0]) <= pkg.capi.PB_AIRCRAFT_MAX


def test_mixed_stream_against_the_second_reading(pkg):
    receivers, m, f, r = acs.mixed_stream(pkg)
    t0 = int(m["sysTimestampMsg"].min())
    sc = (receivers, [("update", m, f, r), ("expire", t0 + 61000)],
          [(0, t0 + 45000, [2000, 1]), (0, t0 + 46000, None), (1, t0 + 120000, None)])
    t = twin(pkg, receivers)
    got = pbs.run(t, sc)
    t.close()
    model = pbs.run_model(pkg, lambda rx: twin(pkg, rx, pb=False), sc)
    for (stream, rx, margin), (files, rows, model_margin) in zip(got, model):
        assert pbs.split(stream, rx) == files and margin == model_margin >= pkg.capi.PB_RSSI_MARGIN_ULPS
    assert int(got[0][1]["aircraft"].sum()) >= 35 and int(got[0][1]["with_positions"].sum()) >= 30
    flights = [a.get("flight") for a in ipb.read_file(pbs.split(got[2][0], got[2][1])[0])["aircraft"]]
    assert any(flights)  # attached at the first writes, long expired at the last


def test_convenience_returns_one_file_per_receiver(pkg):
    sc = pbs.TABLES["three"](pkg)
    t = twin(pkg, sc[0])
    t.update_nicrc(*sc[1][0][1:])
    files = t.aircraft_pb(T0 + 5000, [7, 8, 9])
    assert len(files) == 3 and [ipb.read_file(f)["messages"] for f in files] == [7, 8, 9]
    assert [len(ipb.read_file(f)["aircraft"]) for f in files] == [3, 0, 2]
    t.close()
