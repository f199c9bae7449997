"""`msd_replay --positions --aircraft` on the generator's positions scene: behind the message lines, one line per
aircraft of the table's snapshot, with the place the scene put the aircraft at.

Tolerance, from CPR itself: an airborne position is rounded to the nearest of 2^17 steps per cell, so a decoded coordinate
is at most half a step from the truth -- 0.5 * (360 / 59) / 2^17 degrees of latitude, 0.5 * (360 / max(NL(lat) - 1, 1)) /
2^17 of longitude --, and the tool prints six decimals: half of 1e-6 more.  The tool runs with --clock-start-ms, as
DESIGN.md 4.10 "The clock" tells a caller of the tracker to: on the demodulator's clock from zero a lone first half is
decoded relative to (0, 0) and one aircraft of this scene keeps that false track (tests/test_gpu_positions_end_to_end.py)."""
import os
import subprocess

import pytest

import indep_positions as ip

pytestmark = pytest.mark.gpu
N_AIRCRAFT = 8
START_MS = 1_600_000_000_000


@pytest.fixture(scope="module")
def scene(pkg, torch_cuda, tmp_path_factory):
    cfg = pkg.siggen.make_cfg(seed=77, n_aircraft=N_AIRCRAFT, positions=True)
    iq = pkg.siggen.generate(cfg, 6 * pkg.CHUNK)
    path = tmp_path_factory.mktemp("aircraft") / "scene.uc8"
    iq.tofile(path)
    truth = {a: (lat, lon) for a, lat, lon in (pkg.siggen.aircraft_position(cfg, k) for k in range(N_AIRCRAFT))}
    return str(path), truth


def tool(pkg, *args):
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "msd_replay")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


def test_one_line_per_aircraft_at_the_scenes_place(pkg, torch_cuda, scene):
    path, truth = scene
    res = tool(pkg, "--ifile", path, "--iformat", "uc8", "--fix", "--positions", "--aircraft", "--clock-start-ms", str(START_MS))
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    first = next(i for i, l in enumerate(lines) if l.startswith("aircraft "))
    assert first > 300 and all(l.startswith("aircraft ") for l in lines[first:]) and not any(l.startswith("aircraft ") for l in lines[:first])
    rows = [l[len("aircraft "):].split(",") for l in lines[first:]]
    assert all(len(r) == 8 for r in rows)
    addrs = [int(r[0], 16) for r in rows]
    assert addrs == sorted(set(addrs))                    # one line per aircraft, in address order
    # the message lines name the same aircraft: every DF17 frame's address (bytes 1..3) has its line
    squitters = {int(l[3:9], 16) for l in lines[:first] if l.startswith("*8d")}
    assert squitters <= set(addrs) and set(truth) <= set(addrs)
    per_aircraft = {int(r[0], 16): r for r in rows}
    for a, (lat, lon) in truth.items():
        r = per_aircraft[a]
        assert int(r[1]) >= 10 and r[6] != "" and r[7] != "", r
        tlat = 0.5 * (360.0 / 59) / 131072 * (1 + 1e-9) + 0.5e-6
        tlon = 0.5 * (360.0 / max(ip.nl(lat) - 1, 1)) / 131072 * (1 + 1e-9) + 0.5e-6
        assert abs(float(r[6]) - lat) <= tlat and abs(float(r[7]) - lon) <= tlon, (hex(a), r, lat, lon)


def test_aircraft_without_positions_is_refused(pkg, torch_cuda, scene):
    res = tool(pkg, "--ifile", scene[0], "--iformat", "uc8", "--aircraft")
    assert res.returncode != 0 and "--positions" in res.stderr and res.stdout == ""
