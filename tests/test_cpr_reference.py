"""msd_cpr_impl.h as the host twin compiles it (libmsd_host.so: msd_cpr_host_airborne / _surface / _relative) against
what the reference's own cpr.c answered on the cases of tests/golden/make_cpr_records.py, recorded in
tests/golden/cpr/cpr_reference.npz: result codes equal, latitude and longitude equal as 64-bit patterns.  The second
reading's decoders (tests/indep_positions.py) are held to the same file."""
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
