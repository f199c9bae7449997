#!/usr/bin/env python3
"""Regenerates tests/golden/cpr/cpr_reference.npz: what the reference's own cpr.c answers on a set of inputs.

Where the reference tree is present (where oracle/oracle.py looks for it) its cpr.c is compiled, as it lies there,
together with the small driver below into a temporary directory; the driver reads cases from stdin and prints result
codes and the 64-bit patterns of lat / lon.  Only the recorded inputs and outputs are stored, no reference source.
The file has a directory of its own: tests/test_golden.py takes every *.npz directly under tests/golden for a capture
fixture of make_golden.py.
tests/test_cpr_reference.py checks libmsd_host.so's msd_cpr_host_* against the file bit for bit.

Cases (kind 0 airborne, 1 surface, 2 relative):
  random        3000 of each kind with random 17-bit words (and random references / flags)
  encoded       positions all over the globe encoded with tests/indep_positions.cpr_encode and decoded in every kind
  transitions   every NL transition latitude of cpr.c:82-143, approached from both sides in both hemispheres, each
                half on its own side as well (zone-crossing pairs: result -1)
  poles, wrap   latitudes at and next to +-90, longitudes at and next to +-180
  quadrants     surface pairs around a reference in each of the four longitude quadrants and both hemispheres, and
                the encodes-to-zero latitudes (cpr.c:264-280)

A second file, tests/golden/cpr/cpr_chained.npz, holds the chained family (chained() below): an airborne pair encoded at a
place, decodeCPRairborne's answer P for it, and decodeCPRrelative's answer for a third half -- either parity, airborne
or surface -- encoded at the place plus an offset and decoded against exactly P.  It is what the position tracker can be
given for its aircraft-relative decode (tests/cpr_sweep.py).
  places        every NL transition latitude +-1e-6 and +-3e-3 in both hemispheres at longitudes 0.3 and +-179.9995; +-89.99,
                +-87, 0 and +-1e-7 against +-180, +-179.99999, 0 and 90; 150 random places.  A place at or 1e-6 from a
                transition whose halves round to different sides of it has no P: it is moved away from the transition
                (from +-87 towards the equator) by up to 1e-4 degrees until its pair decodes.
  offsets       CHAIN_OFFSETS: nothing, either side of the surface half cell of 0.75 degrees, either side of the 100 NM
                limit, just inside the airborne half cell
A run leaves a file whose recorded arrays have not changed as it is, byte for byte, and refuses to change cpr_reference.npz.
"""
import os
import pathlib
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
import __graft_entry__ as g  # noqa: E402
import indep_positions as ip  # noqa: E402

DRIVER = r"""
#include <stdio.h>
#include <string.h>
#include <stdint.h>
#include "cpr.h"
int main(void) {
    int kind, a, b, c, d, fflag, surface;
    double reflat, reflon;
    while (scanf("%d %d %d %d %d %d %d %lf %lf", &kind, &a, &b, &c, &d, &fflag, &surface, &reflat, &reflon) == 9) {
        double lat = 0, lon = 0;
        uint64_t ulat, ulon;
        int r;
        if (kind == 0) r = decodeCPRairborne(a, b, c, d, fflag, &lat, &lon);
        else if (kind == 1) r = decodeCPRsurface(reflat, reflon, a, b, c, d, fflag, &lat, &lon);
        else r = decodeCPRrelative(reflat, reflon, a, b, fflag, surface, &lat, &lon);
        if (r < 0) lat = lon = 0;
        memcpy(&ulat, &lat, 8);
        memcpy(&ulon, &lon, 8);
        printf("%d %llu %llu\n", r, (unsigned long long)ulat, (unsigned long long)ulon);
    }
    return 0;
}
"""


def cases():
    rng = np.random.default_rng(1090)
    out = []

    def pair(lat, lon, surface, lat_odd=None, lon_odd=None):
        e = ip.cpr_encode(lat, lon, 0, surface)
        o = ip.cpr_encode(lat if lat_odd is None else lat_odd, lon if lon_odd is None else lon_odd, 1, surface)
        return e[0], e[1], o[0], o[1]

    def add_all(lat, lon, reflat=None, reflon=None, lat_odd=None):
        reflat = lat if reflat is None else reflat
        reflon = lon if reflon is None else reflon
        for fflag in (0, 1):
            out.append((0, *pair(lat, lon, False, lat_odd), fflag, 0, 0.0, 0.0))
            out.append((1, *pair(lat, lon, True, lat_odd), fflag, 1, reflat, reflon))
            for surface in (0, 1):
                y, x = ip.cpr_encode(lat, lon, fflag, bool(surface))
                out.append((2, y, x, 0, 0, fflag, surface, reflat, reflon))

    for kind in (0, 1, 2):
        for _ in range(3000):
            w = rng.integers(0, 1 << 17, 4)
            out.append((kind, int(w[0]), int(w[1]), int(w[2]), int(w[3]), int(rng.integers(0, 2)), int(rng.integers(0, 2)),
                        float(rng.uniform(-90, 90)), float(rng.uniform(-180, 180))))
    for _ in range(1500):
        lat, lon = float(rng.uniform(-89.9, 89.9)), float(rng.uniform(-180, 180))
        add_all(lat, lon, lat + float(rng.uniform(-1, 1)), lon + float(rng.uniform(-1, 1)))
    for t in ip.NL_TABLE:
        for sign in (1, -1):
            for eps in (1e-9, 1e-6, 1e-4, 3e-3):
                for lon in (0.3, -97.1, 151.7):
                    add_all(sign * (t - eps), lon)
                    add_all(sign * (t + eps), lon)
                    add_all(sign * (t - eps), lon, lat_odd=sign * (t + eps))  # the halves on different sides
                    add_all(sign * (t + eps), lon, lat_odd=sign * (t - eps))
    for lat in (90.0, -90.0, 89.999, -89.999, 87.0, -87.0, 86.9999, 0.0, 1e-7, -1e-7):
        for lon in (180.0, -180.0, 179.99999, -179.99999, 0.0, 90.0, -90.0, 45.0, -135.0):
            add_all(lat, lon)
    for reflat in (50.0, -50.0, 10.0, -10.0, 46.0, -46.0, 89.0, -89.0):
        for reflon in (-170.0, -100.0, -45.0, -10.0, 10.0, 45.0, 100.0, 170.0):
            for dlat, dlon in ((0.0, 0.0), (0.2, -0.3), (-0.4, 0.1), (10.0, 20.0), (-44.0, 44.0), (46.0, -46.0)):
                lat = max(-90.0, min(90.0, reflat + dlat))
                add_all(lat, ((reflon + dlon + 180.0) % 360.0) - 180.0, reflat, reflon)
            for fflag in (0, 1):  # latitudes that encode to zero
                out.append((1, 0, 5, 0, 7, fflag, 1, reflat, reflon))
    return out


CHAIN_OFFSETS = ((0.0, 0.0), (0.01, -0.01), (-0.3, 0.4), (0.74, 0.0), (-0.76, 0.2), (1.4, -1.0), (-1.6, 0.9), (0.0, 1.6),
                 (2.9, 0.0))
CHAIN_LIMIT_M = 1852.0 * 100
CHAIN_RANDOM_PLACES = 150


def chained_places():
    """-> (lat, lon, the offsets this place gets, the direction away from its transition latitude).  All edge places with
    all nine offsets would be 57 000 cases, so every edge place gets (0, 0) and three of the other eight offsets in
    rotation: the twelve places around one transition latitude see each offset at least four times.  The random places,
    which are the ones thinned to the size cap, get all nine."""
    rng = np.random.default_rng(1091)
    edges = []
    for t in ip.NL_TABLE:
        for sign in (1, -1):
            for eps in (1e-6, -1e-6, 3e-3, -3e-3):
                for lon in (0.3, 179.9995, -179.9995):
                    edges.append((sign * (t + eps), lon, sign * eps))
    for lat in (89.99, -89.99, 87.0, -87.0, 0.0, 1e-7, -1e-7):
        for lon in (180.0, -180.0, 179.99999, -179.99999, 0.0, 90.0):
            edges.append((lat, lon, -1e-6 * np.sign(lat) if abs(lat) == 87.0 else 0.0))  # 87 is a transition itself
    out = [(lat, lon, (0,) + tuple(1 + (3 * k + i) % 8 for i in range(3)), away) for k, (lat, lon, away) in enumerate(edges)]
    for _ in range(CHAIN_RANDOM_PLACES):
        out.append((float(rng.uniform(-89.0, 89.0)), float(rng.uniform(-180.0, 180.0)), tuple(range(len(CHAIN_OFFSETS))), 0.0))
    return out


CHAIN_STEPS = (0, 10, 25, 50, 100)  # x 1e-6 degrees: a CPR latitude cell is 4.6e-5 degrees, so the last cannot straddle


def ask(exe, cs):
    """cases (kind, a, b, c, d, fflag, surface, reflat, reflon) -> result, lat bits, lon bits as the driver answers"""
    text = "".join("%d %d %d %d %d %d %d %r %r\n" % c for c in cs)
    res = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    assert len(res) == 3 * len(cs)
    return (np.array(res[0::3], dtype=np.int32), np.array([int(x) for x in res[1::3]], dtype=np.uint64),
            np.array([int(x) for x in res[2::3]], dtype=np.uint64))


def chained(exe):
    """The chained family -> the arrays of cpr/cpr_chained.npz.
      pairs     (places, 4) int32: even lat, even lon, odd lat, odd lon of an airborne pair encoded at the place
      p_lat_bits, p_lon_bits    decodeCPRairborne(pair, fflag = 1): P.  Places whose pair does not decode (the halves
                round to different sides of a transition latitude) have no P and are left out.
      third     (cases, 5) int32: place index, cprlat, cprlon, fflag, surface of a third half encoded at place + offset
      result, lat_bits, lon_bits    decodeCPRrelative(P.lat, P.lon, third half)
    A case whose answer lies within 1 m of the tracker's 100 NM limit from P is left out here, not in the tests."""
    places = chained_places()

    def pairs_of(places):
        out = []
        for lat, lon, _, _ in places:
            e, o = ip.cpr_encode(lat, lon, 0, False), ip.cpr_encode(lat, lon, 1, False)
            out.append((0, e[0], e[1], o[0], o[1], 1, 0, 0.0, 0.0))
        return out

    # a place 1e-6 from a transition whose halves round to different sides of it is moved away from the transition, in
    # the steps of CHAIN_STEPS, until its pair decodes
    tries = [pairs_of([(lat + np.sign(away) * step * 1e-6, lon, o, away) for lat, lon, o, away in places]) for step in CHAIN_STEPS]
    answers = [ask(exe, t)[0] for t in tries]
    for k, (lat, lon, o, away) in enumerate(places):
        if abs(away) == 1e-6:
            step = [s for s, a in zip(CHAIN_STEPS, answers) if a[k] == 0][0]
            places[k] = (lat + np.sign(away) * step * 1e-6, lon, o, away)
    pairs = pairs_of(places)
    pres, plat, plon = ask(exe, pairs)
    keep = np.flatnonzero(pres == 0)
    cs, near = [], 0
    for new, k in enumerate(keep):
        lat, lon, offsets, _ = places[k]
        reflat, reflon = float(plat[k:k + 1].view(np.float64)[0]), float(plon[k:k + 1].view(np.float64)[0])
        for o in offsets:
            tlat = max(-90.0, min(90.0, lat + CHAIN_OFFSETS[o][0]))
            tlon = ((lon + CHAIN_OFFSETS[o][1] + 180.0) % 360.0) - 180.0
            for fflag in (0, 1):
                for surface in (0, 1):
                    y, x = ip.cpr_encode(tlat, tlon, fflag, bool(surface))
                    cs.append((new, (2, y, x, 0, 0, fflag, surface, reflat, reflon)))
    res, lat, lon = ask(exe, [c for _, c in cs])
    ok = np.ones(len(cs), dtype=bool)
    for i, (_, c) in enumerate(cs):
        if res[i] == 0:
            d = ip.greatcircle(c[7], c[8], float(lat[i:i + 1].view(np.float64)[0]), float(lon[i:i + 1].view(np.float64)[0]))
            if abs(d - CHAIN_LIMIT_M) < 1.0:
                ok[i], near = False, near + 1
    third = np.array([(new, c[1], c[2], c[5], c[6]) for new, c in cs], dtype=np.int32)[ok]
    print("chained:", len(places), "places,", len(keep), "with a pair that decodes;", len(third), "cases,", near,
          "left out within 1 m of the range limit;", {int(k): int((res[ok] == k).sum()) for k in np.unique(res[ok])})
    return dict(pairs=np.array([pairs[k][1:5] for k in keep], dtype=np.int32), p_lat_bits=plat[keep], p_lon_bits=plon[keep],
                third=third, result=res[ok], lat_bits=lat[ok], lon_bits=lon[ok])


def same_arrays(path, arrays):
    if not os.path.exists(path):
        return False
    old = np.load(path)
    return sorted(old.files) == sorted(arrays) and all(
        old[k].dtype == arrays[k].dtype and old[k].shape == arrays[k].shape and old[k].tobytes() == arrays[k].tobytes()
        for k in arrays)


def write(name, arrays, must_be_unchanged=False):
    """A file whose arrays are what is recorded already is left as it is, byte for byte (a zip archive carries the time
    it was written)."""
    path = os.path.join(HERE, "cpr", name)
    if same_arrays(path, arrays):
        print("cpr/" + name, "holds these answers already: left unchanged")
        return
    assert not (must_be_unchanged and os.path.exists(path)), "cpr/" + name + " would change"
    np.savez_compressed(path, **arrays)
    print("cpr/" + name, "written:", os.path.getsize(path), "bytes")


def main():
    O = g.load_oracle()
    if not os.path.isdir(O.REF_DIR):
        raise SystemExit("the reference tree is not there: nothing to record")
    cs = cases()
    os.makedirs(os.path.join(HERE, "cpr"), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        (tmp / "driver.c").write_text(DRIVER)
        exe = str(tmp / "driver")
        subprocess.check_call(["gcc", "-O2", "-I" + O.REF_DIR, str(tmp / "driver.c"), os.path.join(O.REF_DIR, "cpr.c"),
                               "-o", exe, "-lm"])
        result, lat, lon = ask(exe, cs)
        chain = chained(exe)
    ints = np.array([c[:7] for c in cs], dtype=np.int32)
    refs = np.array([c[7:] for c in cs], dtype=np.float64)
    print("reference:", len(cs), "cases;", {int(k): int((result == k).sum()) for k in np.unique(result)})
    write("cpr_reference.npz", dict(ints=ints, refs=refs, result=result, lat_bits=lat, lon_bits=lon), must_be_unchanged=True)
    assert len(chain["third"]) <= 30000
    write("cpr_chained.npz", chain)
    assert os.path.getsize(os.path.join(HERE, "cpr", "cpr_chained.npz")) <= os.path.getsize(os.path.join(HERE, "cpr", "cpr_reference.npz"))


if __name__ == "__main__":
    main()
