"""msd_replay --avr-in: an AVR text file through msd_accept_avr, read in --avr-chunk pieces.  Its --raw, --net-raw and
--beast output is byte-identical to what the twin path accepts (msd_avr_reader_feed and the checker of
tests/remote_decode.py per piece), written by the same formatters, and its --stats counters are the twin's."""
import ctypes as C
import os
import random
import subprocess

import pytest

import avr_streams as A
from remote_decode import Checker

pytestmark = pytest.mark.gpu


def tool(pkg):
    return os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "msd_replay")


def expected_output(pkg, recs, fmt, mlat):
    host = C.CDLL(os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "libmsd_host.so"))
    host.msd_avr_line_out.restype = C.c_size_t
    host.msd_avr_line_out.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    host.msd_beast_frame_out.restype = C.c_size_t
    host.msd_beast_frame_out.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    out, count = bytearray(), 0
    for i in range(len(recs)):
        r = recs[i:i + 1].copy()
        buf = (C.c_uint8 * 64)()
        if fmt == "raw":  # displayModesMessage --raw (mode_s.c:1786-1798)
            ts = int(r["timestampMsg"][0])
            out += (b"@%012X" % ts if mlat and ts else b"*") + bytes(r["msg"][0][: int(r["msgbits"][0]) // 8]).hex().encode() + b";\n"
            count += 1
            continue
        n = host.msd_avr_line_out(r.ctypes.data, mlat, 0, buf) if fmt == "net-raw" else \
            host.msd_beast_frame_out(r.ctypes.data, 0, buf)
        out += bytes(buf[:n])
        count += n > 0
    return bytes(out), count


def parse_stats(text):
    st = {}
    for line in text.splitlines():
        parts = line.split()
        if len(parts) >= 2 and parts[1].isdigit():
            v = [int(x) for x in parts[1:]]
            st[parts[0]] = v if len(v) > 1 else v[0]
    return st


@pytest.mark.parametrize("nfix,fmt,mlat", [(1, "raw", 0), (0, "net-raw", 1), (2, "beast", 1), (1, "raw", 1)])
@pytest.mark.parametrize("chunk", [61, 65536])
def test_replay_tool_avr_in_matches_the_twin(pkg, oracle, torch_cuda, tmp_path, nfix, fmt, mlat, chunk):
    rng = random.Random(31 * nfix + mlat)
    data = A.corrupt(rng, A.mixed_prefix_stream(rng, 1500, [rng.randrange(1, 1 << 24) for _ in range(12)]), 0.004)
    data += b"q" * 700 + b"\n" + A.star(A.df17(9)) + A.star(A.df17(10))[:-1]  # a long line; the last one stays incomplete
    path = tmp_path / "in.avr"
    path.write_bytes(data)
    reader, chk = A.Reader(pkg, 1, mlat), Checker(pkg, oracle, nfix, 1)
    recs = [chk.frames(reader.feed(part), 1234) for part in A.chunked(data, chunk)]
    recs = recs[0] if len(recs) == 1 else __import__("numpy").concatenate(recs)
    assert len(recs) > 300
    flag = {0: "--no-fix", 1: "--fix", 2: "--aggressive"}[nfix]
    args = [tool(pkg), "--avr-in", str(path), "--avr-chunk", str(chunk), "--now-ms", "1234", flag, "--stats", "--modeac"]
    if mlat:
        args.append("--mlat")
    if fmt != "raw":
        args.append("--" + fmt)
    res = subprocess.run(args, capture_output=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    want_out, want_count = expected_output(pkg, recs, fmt, mlat)
    assert res.stdout == want_out
    got = parse_stats(res.stderr.decode())
    want = dict(chk.stats, messages=want_count, **{"avr_" + k: v for k, v in reader.stats.items()})
    for k, v in want.items():
        assert got[k] == v, (k, got[k], v)
    assert got["avr_long_lines"] == 1 and got["avr_dropped_lines"] > 0
