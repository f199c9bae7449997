"""`msd_replay --positions --aircraft --vrs-out FILE [--vrs-parts N]` on a short constructed capture: FILE is the Python
API's parts 0 .. N-1 concatenated -- the host object's and the device object's, fed the tool's own --raw output, the clock
moved, one record per call as the tool feeds them, now = the last message's time --, N defaults to readsb's 8, and
`--vrs-parts 1` is one JSON document.  Refused without --aircraft, and with a part count that is no power of two."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

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
    d = tmp_path_factory.mktemp("vrs")
    iq.tofile(d / "capture.uc8")
    msgs = np.zeros(len(z["addr"]), dtype=pkg.capi.MESSAGE_DTYPE)
    for k in FIELDS + ("msg",):
        msgs[k] = z[k]
    return str(d / "capture.uc8"), msgs, d


def api_parts(pkg, msgs, host, n_parts):
    fields = np.array([pkg.capi.decode_fields(msgs[i]) for i in range(len(msgs))], dtype=pkg.capi.FIELDS_DTYPE)
    tm = msgs.copy()
    tm["sysTimestampMsg"] += START_MS
    t = pkg.capi.PositionTracker(capacity=1 << 16, host=host, table=True, vrs=True)
    for i in range(len(msgs)):
        t.update_nicrc(tm[i:i + 1], fields[i:i + 1])
    out = b"".join(t.vrs(int(tm["sysTimestampMsg"][-1]), part, n_parts)[0] for part in range(n_parts))
    t.close()
    return out


def test_file_is_the_python_apis_parts(pkg, torch_cuda, capture):
    path, msgs, d = capture
    common = ("--ifile", path, "--iformat", "uc8", "--fix", "--positions", "--aircraft", "--clock-start-ms", str(START_MS), "--stats")
    res = tool(pkg, *common, "--vrs-out", str(d / "eight.json"))
    assert res.returncode == 0, res.stderr[-2000:]
    raw = [x.split(b";")[0] for x in res.stdout.splitlines() if x.startswith(b"*")]
    assert raw == [b"*" + bytes(m["msg"][:m["msgbits"] // 8]).hex().encode() for m in msgs]  # the tool's own messages
    eight = (d / "eight.json").read_bytes()
    assert eight == api_parts(pkg, msgs, True, 8) == api_parts(pkg, msgs, False, 8)
    docs = eight.splitlines()
    assert len(docs) == 8 and sum(len(json.loads(x)["acList"]) for x in docs) >= 3
    stat = [x for x in res.stderr.decode().splitlines() if x.startswith("vrs ")]
    assert stat == ["vrs parts,8,aircraft,%d,bytes,%d" % (sum(len(json.loads(x)["acList"]) for x in docs), len(eight))]
    res = tool(pkg, *common, "--vrs-out", str(d / "one.json"), "--vrs-parts", "1")
    assert res.returncode == 0, res.stderr[-2000:]
    one = (d / "one.json").read_bytes()
    assert one == api_parts(pkg, msgs, True, 1)
    whole = json.loads(one)["acList"]  # one JSON document
    assert sorted(a["Icao"] for a in whole) == sorted(a["Icao"] for x in docs for a in json.loads(x)["acList"])
    assert all(a["Cmsgs"] >= 2 and "Sig" in a for a in whole)


def test_vrs_out_needs_the_table_and_a_power_of_two(pkg, torch_cuda, capture):
    res = tool(pkg, "--ifile", capture[0], "--iformat", "uc8", "--positions", "--vrs-out", str(capture[2] / "no.json"))
    assert res.returncode == 2 and b"--vrs-out goes with --positions --aircraft" in res.stderr
    res = tool(pkg, "--ifile", capture[0], "--iformat", "uc8", "--positions", "--aircraft", "--vrs-out", str(capture[2] / "no.json"),
               "--vrs-parts", "6")
    assert res.returncode == 2 and b"--vrs-parts" in res.stderr and not (capture[2] / "no.json").exists()
