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


def main():
    O = g.load_oracle()
    if not os.path.isdir(O.REF_DIR):
        raise SystemExit("the reference tree is not there: nothing to record")
    cs = cases()
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        (tmp / "driver.c").write_text(DRIVER)
        exe = str(tmp / "driver")
        subprocess.check_call(["gcc", "-O2", "-I" + O.REF_DIR, str(tmp / "driver.c"), os.path.join(O.REF_DIR, "cpr.c"),
                               "-o", exe, "-lm"])
        text = "".join("%d %d %d %d %d %d %d %r %r\n" % c for c in cs)
        res = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    assert len(res) == 3 * len(cs)
    ints = np.array([c[:7] for c in cs], dtype=np.int32)
    refs = np.array([c[7:] for c in cs], dtype=np.float64)
    result = np.array(res[0::3], dtype=np.int32)
    lat = np.array([int(x) for x in res[1::3]], dtype=np.uint64)
    lon = np.array([int(x) for x in res[2::3]], dtype=np.uint64)
    os.makedirs(os.path.join(HERE, "cpr"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "cpr", "cpr_reference.npz"), ints=ints, refs=refs, result=result, lat_bits=lat,
                        lon_bits=lon)
    print("cpr/cpr_reference.npz written:", len(cs), "cases;", {int(k): int((result == k).sum()) for k in np.unique(result)})


if __name__ == "__main__":
    main()
