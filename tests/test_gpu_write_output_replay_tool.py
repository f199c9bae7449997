"""`msd_replay --positions --aircraft --write-output DIR` on a golden capture repeated three times over 61 s of message
time: the directory holds receiver.pb, history_0.pb .. history_2.pb and aircraft.pb and nothing else, and each is the
file the host object writes when the test follows the tool's cadence through capi on the tool's own messages -- the
once-per-second expiry, aircraft.pb every second, a history file every 30 s with receiver.pb behind it, one more aircraft.pb
after the last message.  Without --write-output the tool prints what it printed before."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import indep_aircraft_pb as ipb
import indep_history as ih
from helpers import FIELDS, load_golden
from test_receiver_pb import RECEIVER

pytestmark = pytest.mark.gpu
START_MS = 1_600_000_000_000
CAPTURE = "uc8_fix_exact_multiple"  # what tests/test_gpu_aircraft_pb_replay_tool.py replays
GAP_BUFFERS = 559                   # 559 buffers of 131 072 samples at 2.4 MHz: 30.53 s from one copy's start to the next's
HOME = dict(lat=52.25, lon=4.5)


def tool(pkg, *args):
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "msd_replay")
    return subprocess.run([exe, *args], capture_output=True, timeout=120)


@pytest.fixture(scope="module")
def capture(pkg, tmp_path_factory):
    meta, z = load_golden(CAPTURE)
    iq = pkg.siggen.generate(pkg.siggen.make_cfg(seed=meta["seed"], fmt=pkg.FMT_UC8, **meta["gen"]), meta["nsamples"], nthreads=4)
    assert hashlib.sha256(iq.tobytes()).hexdigest() == meta["iq_sha256"]
    msgs = np.zeros(len(z["addr"]), dtype=pkg.capi.MESSAGE_DTYPE)
    for k in FIELDS + ("msg",):
        msgs[k] = z[k]
    d = tmp_path_factory.mktemp("write_output")
    iq.tofile(d / "capture.uc8")
    return iq, msgs, d


def raw_lines(stdout):
    return [x.split(b";")[0] for x in stdout.splitlines() if x.startswith(b"*")]


def test_the_directory_is_the_host_objects(pkg, torch_cuda, capture):
    iq, _, d = capture
    capi = pkg.capi
    # three copies of the capture, the second and third 30.53 s and 61.06 s in; silence (127, 127) between them
    per = GAP_BUFFERS * capi.CHUNK
    one = iq.view(np.uint8).ravel()  # I and Q, a byte each
    nsamples = 2 * per + one.size // 2
    long_iq = np.full(2 * nsamples, 127, dtype=np.uint8)
    for k in range(3):
        long_iq[2 * k * per:2 * k * per + one.size] = one
    path = d / "long.uc8"
    long_iq.tofile(path)
    out = d / "out"
    out.mkdir()
    res = tool(pkg, "--ifile", str(path), "--iformat", "uc8", "--fix", "--positions", "--aircraft", "--clock-start-ms", str(START_MS),
               "--lat", str(HOME["lat"]), "--lon", str(HOME["lon"]), "--stats", "--write-output", str(out))
    assert res.returncode == 0, res.stderr[-2000:]
    # the tool's own messages, from the library on the same samples
    dem = pkg.Demodulator(fmt=pkg.FMT_UC8, nfix_crc=1, max_batch_samples=64 * capi.CHUNK)
    d_iq = torch_cuda.from_numpy(long_iq).to("cuda:0")
    msgs = capi.replay_device(dem, d_iq.data_ptr(), nsamples, 64 * capi.CHUNK)
    dem.close()
    del d_iq
    assert raw_lines(res.stdout) == [b"*" + bytes(m["msg"][:m["msgbits"] // 8]).hex().encode() for m in msgs]
    tm = msgs.copy()
    tm["sysTimestampMsg"] += START_MS
    times = [int(t) for t in tm["sysTimestampMsg"]]
    assert times == sorted(times) and times[-1] - times[0] > 60000
    fields = np.array([capi.decode_fields(msgs[i]) for i in range(len(msgs))], dtype=capi.FIELDS_DTYPE)
    # the cadence (readsb.c:410-428 on the message clock), through capi on the host object
    got_receiver = ipb.read(RECEIVER, (out / "receiver.pb").read_bytes())
    info = dict(version=got_receiver["version"], refresh=1000.0, latitude=HOME["lat"], longitude=HOME["lon"], location_accuracy=2)
    assert len(info["version"]) > 0
    t = capi.PositionTracker(capacity=1 << 16, receivers=[dict(HOME, latlon_valid=1)], host=True, table=True, pb=True)
    want = {"receiver.pb": capi.receiver_pb(history=1, **info)}
    next_update = next_full = next_history = 0
    history_next, full, margin = 0, False, float("inf")
    for i, now in enumerate(times):
        if now >= next_update:
            t.expire(now)
            next_update = now + 1000
        if now >= next_full:
            want["aircraft.pb"], = t.aircraft_pb(now, [i])
            margin = min(margin, t.pb_margin)
            next_full = now + 1000
        if now >= next_history:
            want["history_%d.pb" % history_next], = t.history_pb(now)
            if not full:
                want["receiver.pb"] = capi.receiver_pb(history=history_next + 1, **info)
                full = history_next == 119
            history_next = (history_next + 1) % 120
            next_history = now + 30000
        t.update_nicrc(tm[i:i + 1], fields[i:i + 1])
    want["aircraft.pb"], = t.aircraft_pb(times[-1], [len(msgs)])
    margin = min(margin, t.pb_margin)
    assert margin >= capi.PB_RSSI_MARGIN_ULPS and t.stats()["min_gate_margin_m"] >= 1e-3
    t.close()
    # the same names -- no temporary file is left -- and the same bytes
    assert sorted(os.listdir(out)) == sorted(want) == ["aircraft.pb", "history_0.pb", "history_1.pb", "history_2.pb", "receiver.pb"]
    for name in sorted(want):
        assert (out / name).read_bytes() == want[name], name
    assert got_receiver["history"] == 3 == sum(n.startswith("history_") for n in want)
    assert (got_receiver["latitude"], got_receiver["longitude"], got_receiver["refresh"]) == (HOME["lat"], HOME["lon"], 1000.0)
    # the first history file is written before the first message reaches the tracker; the second has the first copy's
    # positions, 30.5 s old, to draw trails from
    assert ih.read_file(want["history_0.pb"]) == dict(now=START_MS // 1000, history=[])
    second = ih.read_file(want["history_1.pb"])
    assert second["now"] == min(x for x in times if x >= times[0] + 30000) // 1000 and len(second["history"]) >= 1
    assert all("lat" in h and "lon" in h for h in second["history"])
    assert len(ipb.read_file(want["aircraft.pb"])["aircraft"]) >= 3
    stat = [x for x in res.stderr.decode().splitlines() if x.startswith("write-output ")]
    assert stat == ["write-output aircraft_pb,4,history,3,receiver_pb,4"]


def test_without_the_option_nothing_changes(pkg, torch_cuda, capture):
    """the same run with and without --write-output prints the same lines: the pinned messages, and one expiry at the
    first message, which has nobody to remove"""
    _, msgs, d = capture
    args = ["--ifile", str(d / "capture.uc8"), "--iformat", "uc8", "--fix", "--positions", "--aircraft", "--clock-start-ms", str(START_MS)]
    plain = tool(pkg, *args)
    assert plain.returncode == 0, plain.stderr[-2000:]
    assert raw_lines(plain.stdout) == [b"*" + bytes(m["msg"][:m["msgbits"] // 8]).hex().encode() for m in msgs]
    out = d / "short"
    out.mkdir()
    with_dir = tool(pkg, *args, "--write-output", str(out), "--write-output-every", "0.01")
    assert with_dir.returncode == 0, with_dir.stderr[-2000:]
    assert (with_dir.stdout, with_dir.stderr) == (plain.stdout, plain.stderr)
    assert sorted(os.listdir(out)) == ["aircraft.pb", "history_0.pb", "receiver.pb"]
    assert ipb.read(RECEIVER, (out / "receiver.pb").read_bytes())["refresh"] == 100.0  # at least 0.1 s


def test_write_output_needs_the_table(pkg, torch_cuda, capture):
    res = tool(pkg, "--ifile", str(capture[2] / "capture.uc8"), "--iformat", "uc8", "--positions", "--write-output", str(capture[2]))
    assert res.returncode == 2 and b"--aircraft" in res.stderr
