"""`msd_replay --positions --aircraft --sbs-out FILE` on the generator's positions scene: FILE is the host twin's SBS
stream on the same records -- the tool's own messages, decoded again on the host, the clock moved, one record per call as
the tool feeds them, fields 9-10 the message's own time --, with --gnss, --net-only and --utc-offset, beside
--beast-reduce-out, and refused without --aircraft.  Bytes are compared as bytes."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
START_MS = 1_600_000_000_000


@pytest.fixture(scope="module")
def scene(pkg, torch_cuda, tmp_path_factory):
    cfg = pkg.siggen.make_cfg(seed=77, n_aircraft=8, positions=True)
    n = 6 * pkg.CHUNK
    iq = pkg.siggen.generate(cfg, n)
    d = tmp_path_factory.mktemp("sbs")
    path = d / "scene.uc8"
    iq.tofile(path)
    dem = pkg.Demodulator(nfix_crc=1, max_batch_samples=8 * pkg.CHUNK, message_capacity=1 << 16)
    dem.launch_device(torch_cuda.from_numpy(iq).to("cuda:0").data_ptr(), n, last=True)
    msgs = dem.collect()
    assert len(msgs) > 300
    return str(path), msgs, d


def tool(pkg, *args):
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "msd_replay")
    return subprocess.run([exe, *args], capture_output=True, timeout=120)


def twin_stream(pkg, msgs, reduce_ms=None, **kw):
    """what the tool does, on the host twin -> (bytes, ends, verdicts or None)"""
    fields = np.array([pkg.capi.decode_fields(msgs[i]) for i in range(len(msgs))], dtype=pkg.capi.FIELDS_DTYPE)
    tm = msgs.copy()
    tm["sysTimestampMsg"] += START_MS
    t = pkg.capi.PositionTracker(capacity=1 << 16, host=True, table=True, sbs=True, reduce_interval_ms=reduce_ms)
    res = [t.update_sbs(tm[i:i + 1], fields[i:i + 1], nicrc=False, forward=reduce_ms is not None) for i in range(len(msgs))]
    trk = np.concatenate([x[3] for x in res])
    off = kw.get("utc_offset_ms", 0)
    out, ends = t.sbs_wire(tm, fields, trk, now_is_received=True, now_ms=max(-off, 0), **kw)
    fwd = np.concatenate([x[2] for x in res]) if reduce_ms is not None else None
    t.close()
    return out, ends, fwd


@pytest.mark.parametrize("extra,kw", [([], {}), (["--gnss"], dict(gnss=True)), (["--net-only"], dict(net_only=True)),
                                      (["--net-verbatim", "--utc-offset", "-18000"], dict(verbatim=True, utc_offset_ms=-18000000)),
                                      (["--utc-offset", "19800"], dict(utc_offset_ms=19800000))])
def test_file_is_the_twins_stream(pkg, torch_cuda, scene, extra, kw):
    path, msgs, d = scene
    out = d / ("sbs_%s.txt" % "_".join(x.strip("-") for x in extra))
    res = tool(pkg, "--ifile", path, "--iformat", "uc8", "--fix", "--positions", "--aircraft", "--clock-start-ms", str(START_MS),
               "--stats", "--sbs-out", str(out), *extra)
    assert res.returncode == 0, res.stderr[-2000:]
    want, ends, _ = twin_stream(pkg, msgs, **kw)
    got = out.read_bytes()
    assert got == want
    lines = int(np.count_nonzero(np.diff(np.concatenate([[0], ends]))))
    stat = [x for x in res.stderr.decode().splitlines() if x.startswith("sbs ")]
    assert stat == ["sbs lines,%d,of,%d,bytes,%d" % (lines, len(msgs), len(want))]
    assert 0 < lines <= len(msgs) and got.count(b"\r\n") == lines and got.startswith(b"MSG,")
    if not extra:  # positions decode in this scene, and the dates are the moved clock's
        assert any(x.split(b",")[14] for x in got.split(b"\r\n")[:-1]) and b",2020/09/13,12:26:4" in got


def test_beside_the_reduced_output(pkg, torch_cuda, scene):
    path, msgs, d = scene
    sbs, red = d / "both.txt", d / "both.bin"
    res = tool(pkg, "--ifile", path, "--iformat", "uc8", "--fix", "--positions", "--aircraft", "--clock-start-ms", str(START_MS),
               "--sbs-out", str(sbs), "--beast-reduce-out", str(red))
    assert res.returncode == 0, res.stderr[-2000:]
    want, _, fwd = twin_stream(pkg, msgs, reduce_ms=125)
    assert sbs.read_bytes() == want
    t = pkg.capi.PositionTracker(capacity=64, host=True, table=True, reduce_interval_ms=125)
    assert red.read_bytes() == t.reduce_wire(msgs, fwd)[0]
    t.close()


def test_sbs_out_needs_the_table(pkg, torch_cuda, scene):
    res = tool(pkg, "--ifile", scene[0], "--iformat", "uc8", "--positions", "--sbs-out", str(scene[2] / "no.txt"))
    assert res.returncode == 2 and b"--aircraft" in res.stderr
