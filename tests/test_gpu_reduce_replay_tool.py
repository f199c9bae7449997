"""`msd_replay --positions --aircraft --beast-reduce-out FILE` on the generator's positions scene and on a Beast file
made from its messages: FILE is the host twin's reduced stream on the same records -- the tool's own messages, decoded
again on the host, one record per call as the tool feeds them --, and at --beast-reduce-interval 0 with --net-verbatim
it is the tool's --beast output restricted to the records whose verdict says forward.  Bytes are compared as bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import indep_reduce as ir
import reduce_streams as rs

pytestmark = pytest.mark.gpu
START_MS = 1_600_000_000_000
NOW_MS = 4321


@pytest.fixture(scope="module")
def scene(pkg, torch_cuda, tmp_path_factory):
    cfg = pkg.siggen.make_cfg(seed=77, n_aircraft=8, positions=True)
    n = 6 * pkg.CHUNK
    iq = pkg.siggen.generate(cfg, n)
    d = tmp_path_factory.mktemp("reduce")
    path = d / "scene.uc8"
    iq.tofile(path)
    dem = pkg.Demodulator(nfix_crc=1, max_batch_samples=8 * pkg.CHUNK, message_capacity=1 << 16)
    dem.launch_device(torch_cuda.from_numpy(iq).to("cuda:0").data_ptr(), n, last=True)
    msgs = dem.collect()
    assert len(msgs) > 300
    # the same messages as a Beast file: what msd_accept_beast makes of it is the second input
    host = C.CDLL(pkg.capi.HOST_LIB_PATH)
    host.msd_beast_frame_out.restype = C.c_size_t
    host.msd_beast_frame_out.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    buf, data = (C.c_uint8 * 64)(), bytearray()
    for i in range(len(msgs)):
        data += bytes(buf[:host.msd_beast_frame_out(msgs[i:i + 1].ctypes.data, 0, buf)])
    beast = d / "scene.beast"
    beast.write_bytes(bytes(data))
    remote = pkg.Demodulator(nfix_crc=1).accept_beast(bytes(data), NOW_MS)
    assert len(remote) > 300
    return str(path), msgs, str(beast), remote, d


def tool(pkg, *args):
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "msd_replay")
    return subprocess.run([exe, *args], capture_output=True, timeout=120)


def twin_stream(pkg, msgs, interval_ms, verbatim=False, net_only=False):
    """what the tool does, on the host twin: the fields of msd_decode_fields, the clock moved, one record per call"""
    fields = np.array([pkg.capi.decode_fields(msgs[i]) for i in range(len(msgs))], dtype=pkg.capi.FIELDS_DTYPE)
    tm = msgs.copy()
    tm["sysTimestampMsg"] += START_MS
    t = pkg.capi.PositionTracker(capacity=1 << 16, host=True, table=True, reduce_interval_ms=interval_ms)
    fwd = np.concatenate([t.update_reduce(tm[i:i + 1], fields[i:i + 1], nicrc=False)[2] for i in range(len(msgs))])
    out, ends = t.reduce_wire(msgs, fwd, verbatim=verbatim, net_only=net_only)
    t.close()
    return out, ends, fwd


@pytest.mark.parametrize("source", ["ifile", "beast-in"])
@pytest.mark.parametrize("interval,extra", [(None, []), ("1", ["--net-only"]), ("15.5", ["--net-verbatim"])])
def test_file_is_the_twins_stream(pkg, torch_cuda, scene, source, interval, extra):
    path, msgs, beast, remote, d = scene
    out = d / ("%s_%s.bin" % (source, interval))
    base = ["--ifile", path, "--iformat", "uc8", "--fix"] if source == "ifile" else ["--beast-in", beast, "--now-ms", str(NOW_MS), "--fix"]
    args = base + ["--positions", "--aircraft", "--clock-start-ms", str(START_MS), "--stats", "--beast-reduce-out", str(out)] + extra
    if interval:
        args += ["--beast-reduce-interval", interval]
    res = tool(pkg, *args)
    assert res.returncode == 0, res.stderr[-2000:]
    recs = msgs if source == "ifile" else remote
    ms = 125 if interval is None else min(int(float(interval) * 1000 + 0.5), 15000)  # the default, and the cap of 15 s
    want, ends, fwd = twin_stream(pkg, recs, ms, verbatim="--net-verbatim" in extra, net_only="--net-only" in extra)
    assert out.read_bytes() == want
    sent = int(np.count_nonzero(np.diff(np.concatenate([[0], ends]))))
    line = [l for l in res.stderr.decode().splitlines() if l.startswith("reduce ")]
    assert line == ["reduce forwarded,%d,of,%d,bytes,%d" % (sent, len(recs), len(want))]
    if source == "ifile":  # the scene's records spread over 0.3 s: some are forwarded, some are not
        assert 0 < sent < len(recs)


def test_interval_zero_verbatim_is_the_beast_output_of_the_forwarded_records(pkg, torch_cuda, scene):
    path, msgs, beast, remote, d = scene
    base = ["--ifile", path, "--iformat", "uc8", "--fix", "--net-verbatim"]
    out = d / "zero.bin"
    res = tool(pkg, *base, "--positions", "--aircraft", "--clock-start-ms", str(START_MS), "--beast-reduce-out", str(out),
               "--beast-reduce-interval", "0")
    assert res.returncode == 0, res.stderr[-2000:]
    full = tool(pkg, *base, "--beast")
    assert full.returncode == 0
    _, _, fwd = twin_stream(pkg, msgs, 0, verbatim=True)
    every, ends = rs.stream_of(pkg, msgs, np.full(len(msgs), ir.FORWARD, dtype=np.uint8), verbatim=True)
    assert full.stdout == every  # with --net-verbatim every record has a frame: ends cuts the output into records
    starts = np.concatenate([[0], ends[:-1]])
    want = b"".join(full.stdout[int(starts[i]):int(ends[i])] for i in range(len(msgs)) if fwd[i] & ir.FORWARD)
    assert out.read_bytes() == want and 0 < len(want) <= len(every)


def test_reduce_out_needs_the_table(pkg, torch_cuda, scene):
    res = tool(pkg, "--ifile", scene[0], "--iformat", "uc8", "--positions", "--beast-reduce-out", str(scene[4] / "no.bin"))
    assert res.returncode != 0 and b"--aircraft" in res.stderr
