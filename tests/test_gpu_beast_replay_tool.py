"""msd_replay --beast-in: a Beast file through msd_accept_beast, read in --beast-chunk pieces.  Its --raw, --net-raw and
--beast output is byte-identical to what the checker of tests/remote_decode.py accepts, written by the same formatters,
and its --stats counters are the checker's (h).  The AddressSanitizer + UBSan build of the tool (scripts/sanitize.sh
asan; the host side of the Beast input, msd_frames.cpp, instrumented) runs the corrupted corpora without a report."""
import ctypes as C
import os
import random
import subprocess

import pytest

from remote_decode import Checker
from test_gpu_beast_ingest import corrupted_corpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tool(pkg):
    return os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "msd_replay")


def expected_output(pkg, recs, fmt):
    host = C.CDLL(os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "libmsd_host.so"))
    host.msd_avr_line_out.restype = C.c_size_t
    host.msd_avr_line_out.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    host.msd_beast_frame_out.restype = C.c_size_t
    host.msd_beast_frame_out.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    out = bytearray()
    for i in range(len(recs)):
        r = recs[i:i + 1].copy()
        if fmt == "raw":  # displayModesMessage --raw (mode_s.c:1786-1798)
            out += b"*" + bytes(r["msg"][0][: int(r["msgbits"][0]) // 8]).hex().encode() + b";\n"
        elif fmt == "net-raw":
            buf = (C.c_uint8 * 64)()
            out += bytes(buf[: host.msd_avr_line_out(r.ctypes.data, 0, 0, buf)])
        else:
            buf = (C.c_uint8 * 64)()
            out += bytes(buf[: host.msd_beast_frame_out(r.ctypes.data, 0, buf)])
    return bytes(out)


def parse_stats(text):
    st = {}
    for line in text.splitlines():
        parts = line.split()
        if len(parts) >= 2 and parts[1].isdigit():
            v = [int(x) for x in parts[1:]]
            st[parts[0]] = v if len(v) > 1 else v[0]
    return st


def checker_stats_as_tool_prints(chk, recs, fmt):
    """The remote counters, and `messages`: what the tool wrote -- every accepted message with --raw, the ones
    modesQueueOutput forwards (no two-bit repairs without --net-verbatim, net_io.c:1263-1290) with --net-raw / --beast."""
    want = dict(chk.stats)
    want["messages"] = len(recs) if fmt == "raw" else int((recs["correctedbits"] < 2).sum())
    return want


@pytest.mark.parametrize("nfix,fmt,chunk,frames", [
    (1, "raw", 65536, 3000), (0, "net-raw", 4096, 3000), (2, "beast", 7, 600), (1, "raw", 1, 60),
])
def test_replay_tool_beast_in_matches_the_checker(pkg, oracle, torch_cuda, tmp_path, nfix, fmt, chunk, frames):
    rng = random.Random(31 * nfix + chunk)
    data = corrupted_corpus(rng, frames)
    path = tmp_path / "in.beast"
    path.write_bytes(data)
    chk = Checker(pkg, oracle, nfix, 0)
    recs = chk.beast(data, 1234)
    assert len(recs) > 0
    flag = {0: "--no-fix", 1: "--fix", 2: "--aggressive"}[nfix]
    args = [tool(pkg), "--beast-in", str(path), "--beast-chunk", str(chunk), "--now-ms", "1234", flag, "--stats"]
    if fmt != "raw":
        args.append("--" + fmt)
    res = subprocess.run(args, capture_output=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout == expected_output(pkg, recs, fmt)
    got = parse_stats(res.stderr.decode())
    for k, v in checker_stats_as_tool_prints(chk, recs, fmt).items():
        assert got[k] == v, (k, got[k], v)


@pytest.fixture(scope="module")
def asan_build(pkg):
    out = os.path.join(ROOT, "build", "san_asan")
    subprocess.check_call(["bash", os.path.join(ROOT, "scripts", "sanitize.sh"), "asan", out], stdout=subprocess.DEVNULL)
    assert "__asan_report" in subprocess.check_output(["nm", os.path.join(out, "msd_frames.o")], text=True)
    return out


@pytest.mark.parametrize("nfix", [0, 1, 2])
def test_beast_in_under_address_sanitizer(pkg, torch_cuda, asan_build, tmp_path, nfix):
    """The corrupted corpora of test (b), in pieces that cut frames, escapes and garbage runs, through the instrumented
    tool: no report, and the output of the ordinary build."""
    data = corrupted_corpus(random.Random(100 * nfix + 1), 3000)
    path = tmp_path / "in.beast"
    path.write_bytes(data)
    flag = {0: "--no-fix", 1: "--fix", 2: "--aggressive"}[nfix]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=66:protect_shadow_gap=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=66")
    for chunk in ("4093", "65536"):
        args = ["--beast-in", str(path), "--beast-chunk", chunk, "--now-ms", "5", flag, "--stats", "--modeac"]
        want = subprocess.run([tool(pkg)] + args, capture_output=True, timeout=600)
        assert want.returncode == 0, want.stderr[-2000:]
        got = subprocess.run([os.path.join(asan_build, "msd_replay")] + args, capture_output=True, timeout=900, env=env)
        text = (got.stdout + got.stderr).decode(errors="replace")
        assert got.returncode == 0 and "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
        assert got.stdout == want.stdout and got.stdout.count(b";") > 100
        assert parse_stats(got.stderr.decode()) == parse_stats(want.stderr.decode())
