"""End to end on the GPU: a generated capture in which every DF17 frame is an airborne position squitter of an aircraft
standing at a known place (siggen's positions scene) goes through the demodulator with the field decode
(msd_collect_fields), the records and fields the project's own decoder produced go back to the device and through
msd_pos_update, and `msd_replay --positions` prints the same coordinates for the same capture.

Tolerance, from CPR itself and not from a run: an airborne position is encoded in 17 bits per cell, rounded to the
nearest step, so a decoded coordinate is at most half a step from the truth -- in latitude 0.5 * (360 / 59) / 2^17
degrees (the odd format's larger cell; 2.6 m), in longitude 0.5 * (360 / max(NL(lat) - 1, 1)) / 2^17 degrees at the
aircraft's latitude.  Both get a factor 1 + 1e-9 for the double arithmetic on either side.

The demodulator's clock starts at 0, so position_valid.updated == 0 counts as recent during the first ten minutes
(track.c:466) and a lone first half is tried relative to (0, 0), as the reference would with such a clock.  For the
scene's 0xf49550 (53.956 N, 51.620 W) that decode lands close to (0, 0), inside the range limit, and is taken; every
later global decode of that aircraft then fails the speed check against it and the aircraft-relative decode carries
the false track on (the host twin shows the same: 0 global decodes of 40 positions, 39 of 40 for the other seven).
The tracker test therefore does what DESIGN.md 4.10 "The clock" tells a caller to do and adds a wall-clock start time
to sysTimestampMsg; then a lone first half is skipped, every one of the scene's aircraft must get global decodes, and
each is held to the tolerance.  The tool has no such option and is compared on the zero clock, line by line."""
import os
import subprocess

import numpy as np
import pytest

import indep_positions as ip

pytestmark = pytest.mark.gpu
N_AIRCRAFT = 8
START_MS = 1_600_000_000_000      # a wall clock: far more than ten minutes after position_valid.updated == 0


@pytest.fixture(scope="module")
def scene(pkg, torch_cuda, tmp_path_factory):
    cfg = pkg.siggen.make_cfg(seed=77, n_aircraft=N_AIRCRAFT, positions=True)
    n = 6 * pkg.CHUNK
    iq = pkg.siggen.generate(cfg, n)
    path = tmp_path_factory.mktemp("pos") / "scene.uc8"
    iq.tofile(path)
    dem = pkg.Demodulator(fmt=pkg.FMT_UC8, nfix_crc=1, max_batch_samples=8 * pkg.CHUNK, decode_fields=True)
    d_iq = torch_cuda.from_numpy(iq).to("cuda:0")
    dem.launch_device(d_iq.data_ptr(), n, last=True)
    msgs, fields = dem.collect_fields()
    dem.close()
    truth = {a: (lat, lon) for a, lat, lon in (pkg.siggen.aircraft_position(cfg, k) for k in range(N_AIRCRAFT))}
    return str(path), msgs, fields, truth


def tolerances(lat):
    return (0.5 * (360.0 / 59) / 131072 * (1 + 1e-9),
            0.5 * (360.0 / max(ip.nl(lat) - 1, 1)) / 131072 * (1 + 1e-9))


def test_decoder_fields_through_the_tracker_with_device_records(pkg, torch_cuda, scene):
    _, msgs, fields, truth = scene
    msgs = msgs.copy()
    msgs["sysTimestampMsg"] += START_MS
    assert len(msgs) > 300 and int(fields["cpr_valid"].sum()) > 200
    dm = torch_cuda.from_numpy(msgs.view(np.uint8).copy()).to("cuda:0")
    df = torch_cuda.from_numpy(fields.view(np.uint8).copy()).to("cuda:0")
    torch_cuda.cuda.synchronize()
    gpu = pkg.capi.PositionTracker(capacity=64)
    twin = pkg.capi.PositionTracker(capacity=64, host=True)
    got = gpu.update_device(dm.data_ptr(), df.data_ptr(), len(msgs))
    want = twin.update(msgs, fields)
    assert twin.stats()["min_gate_margin_m"] >= 1.0
    assert got.tobytes() == want.tobytes()
    glob = (got["decoded"] == 1) & (got["relative"] == 0)
    assert int(glob.sum()) > 100
    assert N_AIRCRAFT // 10 == 0                         # the generator's silent tenth never sends DF17: here, nobody
    seen = set()
    for i in np.flatnonzero(glob):
        addr = int(fields["addr"][i])
        if addr not in truth:
            continue                                     # a repaired or colliding frame under another address
        lat, lon = truth[addr]
        tlat, tlon = tolerances(lat)
        assert abs(got["lat"][i] - lat) <= tlat and abs(got["lon"][i] - lon) <= tlon, (hex(addr), got[i], lat, lon)
        seen.add(addr)
    print("global decodes per aircraft:", {hex(a): int((glob & (fields["addr"] == a)).sum()) for a in truth})
    assert seen == set(truth), sorted(hex(a) for a in seen)
    gpu.close()
    twin.close()


def test_replay_tool_prints_the_same_coordinates(pkg, torch_cuda, scene):
    path, msgs, fields, _ = scene
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "msd_replay")
    res = subprocess.run([exe, "--ifile", path, "--iformat", "uc8", "--fix", "--positions"], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(msgs)
    twin = pkg.capi.PositionTracker(capacity=1 << 16, host=True)
    want = twin.update(msgs, fields)
    twin.close()
    with_pos = 0
    for line, m, p in zip(lines, msgs, want):
        raw = "*" + bytes(m["msg"][:m["msgbits"] // 8]).hex() + ";"
        expect = raw + ("%.6f,%.6f" % (p["lat"], p["lon"]) if p["decoded"] else "")
        assert line == expect
        with_pos += int(p["decoded"])
    assert with_pos > 100
