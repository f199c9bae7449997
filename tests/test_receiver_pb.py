"""receiver.pb (msd_receiver_pb, modes_hip.h "receiver.pb"): the bytes against hand-written ones and against the Python
protobuf writer of tests/indep_aircraft_pb.py over the Receiver message of readsb.proto, from both libraries."""
import errno
import math
import struct

import pytest

import indep_aircraft_pb as ipb

RECEIVER = [(1, "s", "version"), (2, "f", "refresh"), (3, "d", "latitude"), (4, "d", "longitude"), (5, "u", "altitude"),
            (6, "u", "antenna_serial"), (7, "u", "antenna_flags"), (8, "u", "antenna_gps_sats"), (9, "u", "antenna_gps_hdop"),
            (14, "u", "antenna_reserved"), (15, "u", "history")]  # readsb.proto, message Receiver


def c_round(x):
    """libm's round: halves away from zero"""
    return math.copysign(math.floor(abs(x) + 0.5), x)


def second_reading(**info):
    v = dict(info)
    acc = v.pop("location_accuracy", 0)
    lat, lon = v.get("latitude", 0.0), v.get("longitude", 0.0)
    if acc == 1 and (lat != 0.0 or lon != 0.0):  # net_io.c:2367-2374
        v["latitude"], v["longitude"] = c_round(lat * 100) / 100, c_round(lon * 100) / 100
    if isinstance(v.get("version"), str):
        v["version"] = v["version"].encode()
    return ipb.write(RECEIVER, v)


@pytest.fixture(params=[False, True], ids=["libmodes_hip", "libmsd_host"])
def pb(pkg, request):
    return lambda **info: pkg.capi.receiver_pb(host=request.param, **info)


def test_bytes_by_hand(pb):
    got = pb(version="msd 1", refresh=1000.0, latitude=52.5, longitude=-4.25, altitude=12, history=1)
    by_hand = (b"\x0a\x05msd 1" + b"\x15" + struct.pack("<f", 1000.0) + b"\x19" + struct.pack("<d", 52.5)
               + b"\x21" + struct.pack("<d", -4.25) + b"\x28\x0c" + b"\x78\x01")
    assert got == by_hand == second_reading(version="msd 1", refresh=1000.0, latitude=52.5, longitude=-4.25, altitude=12, history=1)
    every = dict(version="v", refresh=250.0, latitude=1.0, longitude=2.0, altitude=300, antenna_serial=0xFFFFFFFF,
                 antenna_flags=128, antenna_gps_sats=9, antenna_gps_hdop=12, antenna_reserved=16384, history=120)
    got = pb(**every)
    assert got == second_reading(**every)
    assert got.endswith(b"\x30\xff\xff\xff\xff\x0f" + b"\x38\x80\x01" + b"\x40\x09" + b"\x48\x0c" + b"\x70\x80\x80\x01" + b"\x78\x78")
    assert ipb.read(RECEIVER, got)["history"] == 120


def test_version_empty_and_null_and_all_zero(pb):
    assert pb() == b"" == pb(version=None) == pb(version="") == pb(location_accuracy=1)  # all zero: zero bytes
    assert pb(version="", history=1) == pb(version=None, history=1) == b"\x78\x01"
    assert pb(refresh=-0.0, latitude=-0.0) == b""  # -0.0 is omitted
    assert pb(latitude=float("nan")) == b"\x19" + struct.pack("<d", float("nan"))  # NaN is written


@pytest.mark.parametrize("accuracy", [0, 1, 2])
def test_location_accuracy(pb, accuracy):
    """52.125 x 100 and -4.375 x 100 are exact ties (away from zero: 52.13, -4.38); their neighbours lie on either side"""
    below, above = math.nextafter(52.125, 0.0), math.nextafter(52.125, 90.0)
    for lat, lon, r_lat, r_lon in ((52.125, -4.375, 52.13, -4.38), (below, -4.375, 52.12, -4.38), (above, 0.0, 52.13, 0.0),
                                   (0.0, -4.374999, 0.0, -4.37), (0.004, 0.0, 0.0, 0.0)):
        got = pb(latitude=lat, longitude=lon, location_accuracy=accuracy, history=3)
        assert got == second_reading(latitude=lat, longitude=lon, location_accuracy=accuracy, history=3)
        w_lat, w_lon = (r_lat, r_lon) if accuracy == 1 else (lat, lon)  # 0 and 2 write the location as given
        want = b"".join(tag + struct.pack("<d", x) for tag, x in ((b"\x19", w_lat), (b"\x21", w_lon)) if x != 0) + b"\x78\x03"
        assert got == want, (lat, lon)
    # (0, 0) is no location: nothing to round, nothing written
    assert pb(location_accuracy=accuracy, history=1) == b"\x78\x01"


def test_history_1_and_120(pb):
    assert pb(history=1) == b"\x78\x01" and pb(history=120) == b"\x78\x78" and pb(history=128) == b"\x78\x80\x01"


def test_refusals(pkg, pb):
    info = dict(version="msd", refresh=1000.0, history=7)
    whole = pb(**info)
    assert len(whole) == 5 + 5 + 2
    for cap in (0, 1, len(whole) - 1):
        with pytest.raises(pkg.MsdError) as e:
            pb(cap=cap, **info)
        assert e.value.code == -errno.ENOSPC and pkg.capi.receiver_pb.needed == len(whole)
    assert pb(cap=len(whole), **info) == pb(cap=len(whole) + 9, **info) == whole
    with pytest.raises(pkg.MsdError) as e:
        pb(reserved=1)
    assert e.value.code == -errno.EINVAL
    lib = pkg.capi.lib()
    assert lib.msd_receiver_pb(None, None, 0, None) == -errno.EINVAL
