"""`msd_replay --positions --lat --lon --stats-range --stats-range-pb FILE --aircraft --aircraft-pb FILE` on a small
constructed capture -- a Beast file of DF17 airborne positions, eight aircraft around the receiver, an even and an odd
squitter each, encoded here bit by bit --, in a fresh child process, against the Python objects fed the tool's own --raw
output one record per call as the tool feeds them: the range lines are the device object's and the host object's rows, the
polar-range file their range_pb, and aircraft.pb carries every aircraft's distance.  The host object's margins are
asserted; the places are drawn by range_streams.settle as every range stream's are."""
import os
import subprocess

import numpy as np
import pytest

import indep_positions as ip
import indep_range_pb
import range_streams as rs
from avr_streams import df17
from remote_decode import frame
from test_range_model import assert_margins

pytestmark = pytest.mark.gpu
NOW_MS = 1_600_000_000_000
HOME = rs.HOME
ADDRS = [0x4B1000 + 0x111 * k for k in range(8)]


def airborne_position(addr, y, x, odd):
    """DF17 type 11: TC 5 bits, SS 2, NICsb 1, altitude 12 (Q bit set), T 1, F 1, CPR latitude 17, CPR longitude 17."""
    me = 11 << 51 | 0xC38 << 36 | odd << 34 | y << 17 | x
    return df17(addr, me.to_bytes(7, "big"))


def places(pkg):
    """Eight places 30 to 170 km out in eight directions whose two decodes keep the margins: the scenario the second
    reading settles is the tool's stream -- every squitter at NOW_MS, evens first."""
    def build(jit):
        b = rs.Builder(pkg)
        for odd in (0, 1):
            for k, a in enumerate(ADDRS):
                d = jit((0, a))
                lat, lon = rs.offset(HOME, 45.0 * k + 7, 30e3 + 20e3 * k)
                b.pos(NOW_MS, a, lat + d[0], lon + d[1], odd)
        return [HOME], 0, [b.step()], True
    scenario = rs.settle("replay_tool", build)
    f = scenario[2][0][2]
    return scenario, [(int(f["cpr_lat"][i]), int(f["cpr_lon"][i]), int(f["cpr_odd"][i]), int(f["addr"][i])) for i in range(len(f))]


def test_tool_prints_and_writes_the_objects_range(pkg, torch_cuda, tmp_path):
    scenario, cpr = places(pkg)
    data = b""
    for y, x, odd, addr in cpr:
        data += frame(ord("3"), airborne_position(addr, y, x, odd), ts=12345, signal=0x60)
    path = tmp_path / "positions.beast"
    path.write_bytes(data)
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "msd_replay")
    polar_path, pb_path = tmp_path / "polar.pb", tmp_path / "aircraft.pb"
    res = subprocess.run([exe, "--beast-in", str(path), "--now-ms", str(NOW_MS), "--positions", "--lat", str(HOME["lat"]), "--lon",
                          str(HOME["lon"]), "--stats-range", "--stats-range-pb", str(polar_path), "--aircraft", "--aircraft-pb",
                          str(pb_path), "--stats"], capture_output=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.decode().splitlines()
    raw = [x for x in lines if x.startswith("*")]
    assert len(raw) == 16 and sum(1 for x in raw if not x.endswith(";")) == 8  # the eight odd halves decode
    # the tool's own messages through the Python objects, one record per call
    msgs = np.zeros(16, dtype=pkg.capi.MESSAGE_DTYPE)
    for i, x in enumerate(raw):
        b = bytes.fromhex(x[1:].split(";")[0])
        msgs["msg"][i][:14] = np.frombuffer(b, dtype=np.uint8)
        msgs["msgbits"][i], msgs["msgtype"][i], msgs["sysTimestampMsg"][i] = 112, 17, NOW_MS
        msgs["addr"][i], msgs["timestampMsg"][i] = int.from_bytes(b[1:4], "big"), 12345
        msgs["signalLevel"][i] = (0x60 / 255.0) * (0x60 / 255.0)  # net_io.c:1563-1565
    fields = np.array([pkg.capi.decode_fields(msgs[i]) for i in range(16)], dtype=pkg.capi.FIELDS_DTYPE)
    assert [int(a) for a in fields["addr"]] == ADDRS * 2 and (fields["cpr_valid"] == 1).all() and (fields["source"] == ip.ADSB).all()
    dev, host = [pkg.capi.PositionTracker(capacity=1 << 16, receivers=[HOME], host=h, table=True, pb=True, range=True)
                 for h in (False, True)]
    for t in (dev, host):
        for i in range(16):
            t.update_nicrc(msgs[i:i + 1], fields[i:i + 1])
    assert_margins(host)
    m = rs.model(scenario)
    rs.run(m, scenario[2])
    row, = rs.read_rows(dev.range_read())
    assert [row] == rs.read_rows(host.range_read()) == m.range_read() and row[3] == 8 and sum(1 for v in row[0] if v) == 8
    assert [x for x in lines if x.startswith("range ")] == ["range longest_m,%d,longest_nm,%d,evaluated,8" % (row[1], row[2])]
    assert [x for x in lines if x.startswith("range-bucket ")] == ["range-bucket %d,%d" % (b, v) for b, v in enumerate(row[0])]
    assert polar_path.read_bytes() == dev.range_pb()[0] == host.range_pb()[0] == rs.ir.polar_range_pb(row[0])
    want, = host.aircraft_pb(NOW_MS, [16])
    assert host.pb_margin >= pkg.capi.PB_RSSI_MARGIN_ULPS
    got = pb_path.read_bytes()
    assert got == want == dev.aircraft_pb(NOW_MS, [16])[0]
    seen = indep_range_pb.distance_places(got)
    assert [a for a, _, _, _ in seen] == ADDRS and [d for _, d, _, _ in seen] == m.range_distances() == list(dev.range_distances())
    assert all(d > 29000 for _, d, _, _ in seen) and max(d for _, d, _, _ in seen) == row[1]
    dev.close(), host.close()


def test_stats_range_needs_a_location(pkg, torch_cuda, tmp_path):
    path = tmp_path / "empty.beast"
    path.write_bytes(b"")
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "msd_replay")
    res = subprocess.run([exe, "--beast-in", str(path), "--positions", "--stats-range"], capture_output=True, timeout=120)
    assert res.returncode == 2 and b"--lat --lon" in res.stderr
    res = subprocess.run([exe, "--beast-in", str(path), "--positions", "--lat", "52", "--lon", "4", "--stats-range-pb", str(tmp_path / "x")],
                         capture_output=True, timeout=120)
    assert res.returncode == 2 and b"--stats-range" in res.stderr
