"""`msd_replay --positions --aircraft --aircraft-pb FILE` on a golden capture: FILE reads back with the second reading of
tests/indep_aircraft_pb.py, and it is the host object's file on the tool's own --raw output -- the capture's pinned
messages, which the tool's lines are compared with first, the clock moved, one record per call as the tool feeds them,
now = the last message's time, `messages` = the tool's count.  Refused without --aircraft."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import indep_aircraft_pb as ipb
from helpers import FIELDS, load_golden

pytestmark = pytest.mark.gpu
START_MS = 1_600_000_000_000
CAPTURE = "uc8_fix_exact_multiple"


def tool(pkg, *args):
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "msd_replay")
    return subprocess.run([exe, *args], capture_output=True, timeout=120)


@pytest.fixture(scope="module")
def capture(pkg, tmp_path_factory):
    meta, z = load_golden(CAPTURE)
    iq = pkg.siggen.generate(pkg.siggen.make_cfg(seed=meta["seed"], fmt=pkg.FMT_UC8, **meta["gen"]), meta["nsamples"], nthreads=4)
    assert hashlib.sha256(iq.tobytes()).hexdigest() == meta["iq_sha256"]
    d = tmp_path_factory.mktemp("pb")
    iq.tofile(d / "capture.uc8")
    msgs = np.zeros(len(z["addr"]), dtype=pkg.capi.MESSAGE_DTYPE)
    for k in FIELDS + ("msg",):
        msgs[k] = z[k]
    return str(d / "capture.uc8"), msgs, d


def test_file_is_the_host_objects(pkg, torch_cuda, capture):
    path, msgs, d = capture
    out = d / "aircraft.pb"
    res = tool(pkg, "--ifile", path, "--iformat", "uc8", "--fix", "--positions", "--aircraft", "--clock-start-ms", str(START_MS), "--stats",
               "--aircraft-pb", str(out))
    assert res.returncode == 0, res.stderr[-2000:]
    raw = [x.split(b";")[0] for x in res.stdout.splitlines() if x.startswith(b"*")]
    assert raw == [b"*" + bytes(m["msg"][:m["msgbits"] // 8]).hex().encode() for m in msgs]  # the tool's own messages
    fields = np.array([pkg.capi.decode_fields(msgs[i]) for i in range(len(msgs))], dtype=pkg.capi.FIELDS_DTYPE)
    tm = msgs.copy()
    tm["sysTimestampMsg"] += START_MS
    t = pkg.capi.PositionTracker(capacity=1 << 16, host=True, table=True, pb=True)
    for i in range(len(msgs)):
        t.update_nicrc(tm[i:i + 1], fields[i:i + 1])
    want, = t.aircraft_pb(int(tm["sysTimestampMsg"][-1]), [len(msgs)])
    assert t.pb_margin >= pkg.capi.PB_RSSI_MARGIN_ULPS
    t.close()
    got = out.read_bytes()
    d = ipb.read_file(got)
    assert d["now"] == int(tm["sysTimestampMsg"][-1]) // 1000 and d["messages"] == len(msgs) and len(d["aircraft"]) >= 3
    assert all("rssi" in a and a["messages"] >= 2 for a in d["aircraft"])
    assert got == want
    stat = [x for x in res.stderr.decode().splitlines() if x.startswith("aircraft.pb ")]
    assert stat and stat[0].startswith("aircraft.pb aircraft,%d," % len(d["aircraft"])) and stat[0].endswith(",bytes,%d" % len(got))


def test_aircraft_pb_needs_the_table(pkg, torch_cuda, capture):
    res = tool(pkg, "--ifile", capture[0], "--iformat", "uc8", "--positions", "--aircraft-pb", str(capture[2] / "no.pb"))
    assert res.returncode == 2 and b"--aircraft" in res.stderr
