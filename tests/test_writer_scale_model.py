"""The streams of tests/test_gpu_writer_scale.py on the host twin alone: that each shape is what the GPU test means it to
be -- everyone live and written, the scan of every writer past one round, both outcomes in both record writers, the
gate and rssi margins far away -- so that a checkout without a GPU notices if wide_stream changes under them.  And the
comparison of that test, on outputs made wrong on purpose."""
import numpy as np
import pytest

import writer_scale as ws


@pytest.fixture(scope="module")
def c_out(pkg):
    stream = ws.stream_c(pkg)
    return stream, ws.run_c(pkg, stream, True)


@pytest.mark.parametrize("shape", ["a", "b"])
def test_shape(pkg, shape):
    stream = getattr(ws, "stream_" + shape)(pkg)
    out = getattr(ws, "run_" + shape)(pkg, stream, True)
    getattr(ws, "shape_" + shape)(pkg, stream, out)
    # measured on the twin: a gate margin of 956 m (a) and 957 m (b) against the 1 m asked for, an rssi margin of
    # 981 302 (a) and 555 370 ulps (b) against the 8 asked for
    assert out["stats"]["min_gate_margin_m"] > 900.0 and out["pb_margin"] > 1e5


def test_shape_c(pkg, c_out):
    stream, out = c_out
    ws.shape_c(pkg, stream, out)


def test_rounds():
    assert [ws.rounds(n) for n in (1, 256, 65536, 65537, 131072, 131073)] == [1, 1, 1, 2, 2, 3]


def test_the_comparison_names_the_first_difference(pkg, c_out):
    """first_difference on the twin's own output of shape c, and on copies with one byte, one row, one length changed"""
    _, out = c_out
    for name in ws.COMPARED["c"]:
        assert ws.first_difference(name, out[name], out[name]) is None
    stream, rx = out["aircraft_pb"]
    at = int(rx["end"][255]) + 1  # a byte of receiver 256's file
    bad = bytearray(stream)
    bad[at] ^= 1
    bad[-1] ^= 1
    msg = ws.first_difference("aircraft_pb", (bytes(bad), rx), out["aircraft_pb"])
    assert "first difference at byte %d (row 256)" % at in msg, msg
    msg = ws.first_difference("aircraft_pb", (stream[:-1], rx), out["aircraft_pb"])
    assert "first difference at byte %d (row %d)" % (len(stream) - 1, len(rx) - 1) in msg, msg
    rows = rx.copy()
    rows["aircraft"][257] += 1
    msg = ws.first_difference("aircraft_pb", (stream, rows), out["aircraft_pb"])
    assert "aircraft_pb[1]: first difference in row 257 of 65536" in msg, msg
    ends = out["range_pb"][1].copy()
    ends[300:] -= np.uint64(4)  # what a carry lost between two rounds would look like
    msg = ws.first_difference("range_pb", (out["range_pb"][0], ends), out["range_pb"])
    assert "range_pb[1]: first difference in row 300 of 65536" in msg, msg
