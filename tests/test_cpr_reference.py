"""msd_cpr_impl.h as the host twin compiles it (libmsd_host.so: msd_cpr_host_airborne / _surface / _relative) against
what the reference's own cpr.c answered on the cases of tests/golden/make_cpr_records.py, recorded in
tests/golden/cpr/cpr_reference.npz: result codes equal, latitude and longitude equal as 64-bit patterns.  The second
reading's decoders (tests/indep_positions.py) are held to the same file.  Both are held in the same way to the chained
family of tests/golden/cpr/cpr_chained.npz: an airborne pair's answer P and a third half's answer relative to P."""
import os

import numpy as np
import pytest

import indep_positions as ip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cpr", "cpr_reference.npz")


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def bits(x):
    return int(np.float64(x).view(np.uint64))


def run(decoders, golden):
    bad = []
    for i in range(len(golden["result"])):
        kind, a, b, c, d, fflag, surface = (int(x) for x in golden["ints"][i])
        reflat, reflon = (float(x) for x in golden["refs"][i])
        if kind == 0:
            r, lat, lon = decoders[0](a, b, c, d, fflag)
        elif kind == 1:
            r, lat, lon = decoders[1](reflat, reflon, a, b, c, d, fflag)
        else:
            r, lat, lon = decoders[2](reflat, reflon, a, b, fflag, surface)
        want = (int(golden["result"][i]), int(golden["lat_bits"][i]), int(golden["lon_bits"][i]))
        got = (r, bits(lat), bits(lon)) if r >= 0 else (r, 0, 0)
        if got != want:
            bad.append((i, kind, got, want))
    return bad


def test_the_file_covers_what_it_says(golden):
    kinds, res = golden["ints"][:, 0], golden["result"]
    assert len(res) > 20000
    for kind in (0, 1, 2):
        assert ((kinds == kind) & (res == 0)).sum() > 2000
    assert ((kinds == 0) & (res == -1)).sum() > 100 and ((kinds == 1) & (res == -1)).sum() > 100  # zone crossings
    assert ((kinds == 2) & (res == -1)).sum() > 100


def test_host_twin_equals_the_reference_bit_for_bit(pkg, golden):
    bad = run([lambda *a: pkg.capi.cpr_host("airborne", *a), lambda *a: pkg.capi.cpr_host("surface", *a),
               lambda *a: pkg.capi.cpr_host("relative", *a)], golden)
    assert not bad, (len(bad), bad[:5])


def test_second_reading_equals_the_reference_bit_for_bit(golden):
    bad = run([ip.decode_airborne, ip.decode_surface, ip.decode_relative], golden)
    assert not bad, (len(bad), bad[:5])


# ---- the chained family (cpr_chained.npz): an airborne pair fixes P, a third half is decoded relative to P ----
CHAINED = os.path.join(os.path.dirname(GOLDEN), "cpr_chained.npz")


@pytest.fixture(scope="module")
def chained():
    g = np.load(CHAINED)
    return {k: g[k] for k in g.files}


def run_chained(airborne, relative, g):
    bad = []
    P = []
    for k in range(len(g["pairs"])):
        r, lat, lon = airborne(*(int(x) for x in g["pairs"][k]), 1)
        if (r, bits(lat), bits(lon)) != (0, int(g["p_lat_bits"][k]), int(g["p_lon_bits"][k])):
            bad.append((k, "pair", (r, bits(lat), bits(lon)), (0, int(g["p_lat_bits"][k]), int(g["p_lon_bits"][k]))))
        P.append((float(g["p_lat_bits"][k:k + 1].view(np.float64)[0]), float(g["p_lon_bits"][k:k + 1].view(np.float64)[0])))
    for i in range(len(g["result"])):
        place, cprlat, cprlon, fflag, surface = (int(x) for x in g["third"][i])
        r, lat, lon = relative(P[place][0], P[place][1], cprlat, cprlon, fflag, surface)
        want = (int(g["result"][i]), int(g["lat_bits"][i]), int(g["lon_bits"][i]))
        got = (r, bits(lat), bits(lon)) if r >= 0 else (r, 0, 0)
        if got != want:
            bad.append((i, "third", got, want))
    return bad


def test_the_chained_file_covers_what_it_says(chained):
    third, res = chained["third"], chained["result"]
    assert 10000 < len(res) <= 30000 and os.path.getsize(CHAINED) <= os.path.getsize(GOLDEN)
    surface = third[:, 4] == 1
    for s in (surface, ~surface):
        assert (s & (res == 0)).sum() > 2000 and (s & (res == -1)).sum() > 200  # -1: beyond the half cell
    plat = chained["p_lat_bits"].view(np.float64)[third[:, 0]]
    plon = chained["p_lon_bits"].view(np.float64)[third[:, 0]]
    lon = chained["lon_bits"].view(np.float64)
    near = np.abs(np.abs(plat)[:, None] - np.array(ip.NL_TABLE)[None, :]).min(axis=1)
    assert ((near < 3e-3) & (res == 0)).sum() > 2000
    # every transition latitude in both hemispheres with a P closer to it than 1.5e-4 degrees: a place at most 1e-4 away
    # (make_cpr_records.CHAIN_STEPS) and half a latitude cell of 4.7e-5 for the rounding, which may also carry P across
    table = np.array(ip.NL_TABLE)
    for sign in (1, -1):
        d = (sign * plat[res == 0])[:, None] - table[None, :]
        assert (np.abs(d) < 1.5e-4).any(axis=0).all(), sign
        assert ((d > 0) & (d < 1.5e-4)).sum() > 1000 and ((d < 0) & (d > -1.5e-4)).sum() > 1000, sign  # both sides
    # across +-180: eastwards decodeCPRrelative folds rlon > 180 and then refuses the answer, now 360 degrees from the
    # reference; westwards nothing folds and the answer lies below -180
    assert ((res == 0) & (lon < -180)).sum() > 200 and ((res == 0) & (lon < -180) & surface).sum() > 50
    east = [i for i in np.flatnonzero((res == -1) & (plon > 179)) if folds_then_refuses(plat[i], plon[i], *third[i, 1:])]
    assert len(east) > 200 and surface[east].sum() > 50


def folds_then_refuses(reflat, reflon, cprlat, cprlon, fflag, surface):
    """cpr.c's decodeCPRrelative up to its longitude, to tell which way a refused case went: the latitude passes, the
    longitude is beyond 180 and folded, and the last test refuses it"""
    import math
    dlat = (90.0 if surface else 360.0) / (59.0 if fflag else 60.0)
    flat, flon = cprlat / 131072.0, cprlon / 131072.0
    rlat = dlat * (math.floor(reflat / dlat) + math.floor(0.5 + ip.mod_double(reflat, dlat) / dlat - flat) + flat)
    if rlat < -90 or rlat > 90 or abs(rlat - reflat) > dlat / 2:
        return False
    dlon = ip.dlon_func(rlat, fflag, surface)
    rlon = dlon * (math.floor(reflon / dlon) + math.floor(0.5 + ip.mod_double(reflon, dlon) / dlon - flon) + flon)
    return rlon > 180 and abs(rlon - 360 - reflon) > dlon / 2


def test_host_twin_equals_the_chained_answers_bit_for_bit(pkg, chained):
    bad = run_chained(lambda *a: pkg.capi.cpr_host("airborne", *a), lambda *a: pkg.capi.cpr_host("relative", *a), chained)
    assert not bad, (len(bad), bad[:5])


def test_second_reading_equals_the_chained_answers_bit_for_bit(chained):
    bad = run_chained(ip.decode_airborne, ip.decode_relative, chained)
    assert not bad, (len(bad), bad[:5])
