"""msd_avr_reader_feed (libmsd_host.so), the host twin of msd_accept_avr, against the stream rules of
include/modes_hip.h restated in Python (avr_streams.Model): known answers, the edge cases of the line cutting, and
independence of how a stream is cut into calls.  No GPU needed."""
import ctypes as C
import random

import numpy as np
import pytest

import avr_streams as A

CHUNKS = (1, 2, 7, 255, 256, 257, 4096)


def run(pkg, chunks, mode_ac, keep):
    """Feed the chunks to the reader and to the model; both record lists and both counter sets."""
    rd, md = A.Reader(pkg, mode_ac, keep), A.Model(mode_ac, keep)
    got, want = [], []
    for part in chunks:
        recs = rd.feed(part)
        mine = md.feed(part)
        assert len(recs) == len(mine)
        got += [(bytes(r["msg"][: int(r["msgbits"]) // 8]), int(r["timestampMsg"]), float(r["signalLevel"])) for r in recs]
        want += mine
        for r in recs:
            assert not any(r["msg"][int(r["msgbits"]) // 8:]) and r["sysTimestampMsg"] == 0
    assert got == want
    assert rd.stats == md.stats
    st = rd.stats
    assert st["lines"] == st["frames"] + st["dropped_lines"] + st["long_lines"]
    return got, st, rd


def test_known_answers_for_the_five_prefixes(pkg):
    data, mode_ac = A.edge_streams()["five prefixes"]
    a, b, c = A.df17(0x4840D6), A.df17(0xABCDEF), A.df4(0x4840D6)
    ts = 0x0123456789AB
    got, st, _ = run(pkg, [data], mode_ac, 1)
    lvl = lambda v: (v / 255.0) * (v / 255.0)
    assert got == [(a, 0, 0.0), (b, 0, 0.0), (a, ts, 0.0), (c, ts, 0.0), (b, ts, lvl(0x80)),
                   (a, ts, lvl(-1)), (a, ts, lvl((7 << 4) | -1)),  # signal digits that are none: hexval gives -1
                   (a, 0, 0.0)]                                    # a timestamp digit that is none: 0
    assert st == dict(lines=12, frames=8, dropped_lines=4, long_lines=0)
    got0, _, _ = run(pkg, [data], mode_ac, 0)
    assert [g[0] for g in got0] == [g[0] for g in got] and all(g[1] == 0 for g in got0)
    assert [g[2] for g in got0] == [g[2] for g in got]


def test_record_fields_are_those_of_parse_line(pkg):
    """The reader hands on msd_avr_parse_line's record unchanged: msgtype, crc, addr as wire_message fills them."""
    rd = A.Reader(pkg, 1, 0)
    recs = rd.feed(A.star(A.df17(0x4840D6)) + A.star(A.df4(0x4840D6)) + b"*7700;\n")
    assert list(recs["msgtype"]) == [17, 4, 32] and list(recs["msgbits"]) == [112, 56, 16]
    assert list(recs["addr"]) == [0x4840D6, 0x4840D6, 0x7700 | (1 << 24)] and list(recs["crc"]) == [0, 0x4840D6, 0]
    one = np.zeros(1, dtype=pkg.capi.MESSAGE_DTYPE)
    rd.host.msd_avr_parse_line.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    assert rd.host.msd_avr_parse_line(A.star(A.df17(0x4840D6))[:-1], 1, 0, one.ctypes.data) == 1
    assert one[0].tobytes() == recs[0].tobytes()


@pytest.mark.parametrize("name", sorted(A.edge_streams()))
def test_edge_streams_whole(pkg, name):
    data, mode_ac = A.edge_streams()[name]
    _, st, rd = run(pkg, [data], mode_ac, 1)
    assert st["frames"] > 0
    if name == "256 and 257":
        # 256 bytes of white space and a message: accepted; 257: long, whatever it holds
        assert st == dict(lines=8, frames=4, dropped_lines=2, long_lines=2)
    if name == "long run":
        assert st == dict(lines=4, frames=2, dropped_lines=0, long_lines=2)
    if name == "mode a/c off":
        assert st["frames"] == 1 and st["dropped_lines"] == 2
    if name == "mode a/c on":
        assert st["frames"] == 3 and st["dropped_lines"] == 2
    if name == "no newline at the end":
        assert rd.st.len == len(A.star(A.df17(0xABCDEF))) - 1 and not rd.st.discard


def test_discard_state_is_a_flag_and_no_bytes(pkg):
    rd = A.Reader(pkg, 0, 0)
    assert len(rd.feed(b"x" * 256)) == 0 and rd.st.len == 256 and rd.st.discard == 0
    assert len(rd.feed(b"x")) == 0 and rd.st.len == 0 and rd.st.discard == 1
    assert len(rd.feed(A.star(A.df17(1))[:-1])) == 0 and rd.st.len == 0 and rd.st.discard == 1
    assert len(rd.feed(b"\n" + A.star(A.df17(1)))) == 1 and rd.st.discard == 0
    assert rd.stats == dict(lines=2, frames=1, dropped_lines=0, long_lines=1)


@pytest.mark.parametrize("name", sorted(A.edge_streams()))
def test_chunk_independence(pkg, name):
    data, mode_ac = A.edge_streams()[name]
    whole = run(pkg, [data], mode_ac, 1)[:2]
    for size in CHUNKS:
        assert run(pkg, A.chunked(data, size), mode_ac, 1)[:2] == whole, size
    rng = random.Random(len(data))
    for _ in range(5):
        assert run(pkg, A.random_cuts(rng, data), mode_ac, 1)[:2] == whole


@pytest.mark.parametrize("keep", [0, 1])
def test_corrupted_mixed_stream_in_every_chunking(pkg, keep):
    rng = random.Random(41 + keep)
    data = A.corrupt(rng, A.mixed_prefix_stream(rng, 600, [1, 0x4840D6, 0xABCDEF]), 0.03)
    data += b" " * 255 + A.corrupt(rng, A.mixed_prefix_stream(rng, 50, [7]), 0.3)
    whole = run(pkg, [data], 1, keep)[:2]
    assert whole[1]["frames"] > 100 and whole[1]["dropped_lines"] > 10
    for size in CHUNKS:
        assert run(pkg, A.chunked(data, size), 1, keep)[:2] == whole, size
    for _ in range(5):
        assert run(pkg, A.random_cuts(rng, data), 1, keep)[:2] == whole
