"""`msd_replay --modeac --positions --aircraft --match-modeac` on a generated capture with Mode S frames and Mode A/C
replies: the tool's `modeac` and `modeac-code` lines against the host twin fed the same messages -- the tool's own
message lines, decoded again on the host -- with expiry and a match wherever a message's time reaches next_update, as
trackPeriodicUpdate does.  Integer values: the lines are compared as text."""
import os
import subprocess

import numpy as np
import pytest

import indep_modeac as im

pytestmark = pytest.mark.gpu
START_MS = 1_600_000_000_000


@pytest.fixture(scope="module")
def capture(pkg, torch_cuda, tmp_path_factory):
    n = 24 * pkg.CHUNK + 333  # 1.3 s at 2.4 MHz: the periodic step runs at the first message and once more
    iq = pkg.siggen.generate(pkg.siggen.make_cfg(seed=606, msgs_per_sec=5000, ac_per_sec=600, n_aircraft=80), n)
    path = tmp_path_factory.mktemp("modeac") / "capture.uc8"
    iq.tofile(path)
    dem = pkg.Demodulator(nfix_crc=1, mode_ac=1, max_batch_samples=32 * pkg.CHUNK, message_capacity=1 << 17, decode_fields=True)
    dem.launch_device(torch_cuda.from_numpy(iq).to("cuda:0").data_ptr(), n, last=True)
    msgs, fields = dem.collect_fields()
    return str(path), msgs, fields


def tool(pkg, *args):
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "msd_replay")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


def twin_lines(pkg, msgs, fields):
    """what the tool does, on the host twin: one record per call, the periodic step in front of it"""
    t = pkg.capi.PositionTracker(capacity=1 << 16, host=True, table=True, modeac=True)
    next_update = last = 0
    for i in range(len(msgs)):
        m, f = msgs[i:i + 1].copy(), fields[i:i + 1].copy()
        m["sysTimestampMsg"] += START_MS
        now = int(m["sysTimestampMsg"][0])
        if now >= next_update:
            t.expire(now)
            t.modeac_match(now, last)
            next_update = now + 1000
        if int(m["msgtype"][0]) != 32 and int(f["addr"][0]) != 0:
            last = now
        t.update(m, f)
    hits, codes = t.modeac_hits(), t.modeac_codes(0)
    t.close()
    lines = ["modeac %06x,%d,%d" % (int(h["addr"]), int(h["mode_a_hit"]), int(h["mode_c_hit"])) for h in hits
             if h["mode_a_hit"] or h["mode_c_hit"]]
    for i in np.nonzero(codes["count"])[0]:
        match = int(codes["match"][i])
        lines.append("modeac-code %04x,%d,%d,%s" % (im.index_to_mode_a(int(i)), int(codes["count"][i]), int(codes["age"][i]),
                                                     "ffffffff" if match == 0xFFFFFFFF else "%06x" % match if match else ""))
    return lines, codes


def test_modeac_lines_are_the_twins(pkg, torch_cuda, capture):
    path, msgs, fields = capture
    base = ["--ifile", path, "--iformat", "uc8", "--fix", "--modeac", "--positions", "--aircraft", "--clock-start-ms", str(START_MS)]
    res = tool(pkg, *base, "--match-modeac")
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    got = [l for l in lines if l.startswith("modeac")]
    assert lines[-len(got):] == got and lines[-len(got) - 1].startswith("aircraft ")  # behind the aircraft lines
    assert sum(1 for l in lines if l.startswith("*")) == len(msgs)
    want, codes = twin_lines(pkg, msgs, fields)
    assert got == want
    replies = int((msgs["msgtype"] == 32).sum())
    assert replies > 50 and int(codes["count"].sum()) == replies and sum(1 for l in got if l.startswith("modeac-code ")) > 5
    assert (codes["lastcount"] != 0).any() and (codes["lastcount"] != codes["count"]).any()  # matched once in mid-stream
    # without the option the tool's output is what it was: the same lines less the modeac ones
    plain = tool(pkg, *base)
    assert plain.returncode == 0 and plain.stdout.splitlines() == lines[:-len(got)]
