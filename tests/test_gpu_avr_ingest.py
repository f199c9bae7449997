"""msd_accept_avr on the GPU against its twin path on a second context -- msd_avr_reader_feed, then one
msd_accept_frames per call over the records that call completed, with the same now_ms -- and against the checker of
tests/remote_decode.py over the twin's records: the records field by field, every remote counter (but the diagnostic
tile_rewalks), msd_avr_stats, and the ICAO filter afterwards (the probe call of the Beast tests)."""
import ctypes as C
import errno
import random

import numpy as np
import pytest

import avr_streams as A
from remote_decode import Checker, assert_same_records, assert_same_stats, frame

pytestmark = pytest.mark.gpu


def remote(dem):
    st = dem.remote_stats()
    st.pop("tile_rewalks")
    return st


class Pair:
    """The context under test and the twin path beside it."""

    def __init__(self, pkg, oracle, nfix=1, mode_ac=0, keep=False, orc=None, fmt=None):
        kw = dict(fmt=pkg.FMT_UC8 if fmt is None else fmt, nfix_crc=nfix, mode_ac=mode_ac, message_capacity=1 << 19,
                  max_batch_samples=4 * pkg.CHUNK)
        self.dem, self.twin = pkg.Demodulator(**kw), pkg.Demodulator(**kw)
        self.reader = A.Reader(pkg, mode_ac, keep)
        self.chk = Checker(pkg, oracle, nfix, mode_ac, oracle=orc)
        self.keep = keep

    def close(self):
        self.dem.close()
        self.twin.close()

    def call(self, part, now_ms, device=None):
        """One call on both sides; returns the accepted records."""
        recs = self.reader.feed(bytes(part))
        want = self.twin.accept_frames(recs, now_ms)
        assert_same_records(want, self.chk.frames(recs, now_ms))
        got = self.dem.accept_avr(part if device is None else device, now_ms, keep_timestamp=self.keep)
        assert_same_records(got, want)
        return got

    def feed(self, chunks, now_ms):
        n = 0
        for part in chunks:
            n += len(self.call(part, now_ms))
        self.same_state()
        return n

    def same_state(self):
        assert_same_stats(remote(self.dem), remote(self.twin))
        assert_same_stats(remote(self.dem), self.chk.stats)
        assert self.dem.avr_stats() == self.reader.stats
        st = self.dem.avr_stats()
        assert st["lines"] == st["frames"] + st["dropped_lines"] + st["long_lines"]

    def probe(self, now_ms, rng, decoys=64):
        """One DF4 per address the checker has seen added and a few random ones: the three filters answer alike."""
        addrs = sorted(self.chk.known) + [rng.randrange(1 << 24) for _ in range(decoys)]
        data = b"".join(frame(ord("2"), A.df4(a)) for a in addrs)
        want = self.chk.beast(data, now_ms)
        assert_same_records(self.dem.accept_beast(data, now_ms), want)
        assert_same_records(self.twin.accept_beast(data, now_ms), want)


@pytest.fixture
def make(pkg, oracle, torch_cuda):
    made = []

    def f(**kw):
        made.append(Pair(pkg, oracle, **kw))
        return made[-1]

    yield f
    for p in made:
        p.close()


@pytest.fixture(scope="module")
def capture_lines(pkg, oracle):
    """A replayed synthetic capture's messages as AVR lines, as the raw output writes them (computed once)."""
    cfg = pkg.siggen.make_cfg(seed=1090)
    iq = pkg.siggen.generate(cfg, 12 * pkg.CHUNK + 777)
    msgs, _ = oracle.Oracle(oracle.FMT_UC8, 58, 1, 0).replay(iq)
    assert len(msgs) > 300
    return b"".join(oracle.avr_line(m) for m in msgs), len(msgs)


@pytest.fixture(scope="module")
def consts(pkg):
    L = C.CDLL(pkg.capi.LIB_PATH)
    for n in ("msd_avr_span_bytes", "msd_avr_lookback_bytes", "msd_avr_piece_bytes"):
        getattr(L, n).restype = C.c_uint32
    return L.msd_avr_span_bytes(), L.msd_avr_lookback_bytes(), L.msd_avr_piece_bytes()


# (a) a replayed capture as AVR lines: whole, chunked, at random cuts; host and device input
@pytest.mark.parametrize("chunking", ["whole", "device", "1", "31", "256", "257", "4096", "random", "random-device"])
def test_replayed_capture(make, capture_lines, chunking, torch_cuda):
    data, nmsgs = capture_lines
    rng = random.Random(7)
    p = make()
    if chunking in ("whole", "device"):
        dev = None
        if chunking == "device":
            dev = torch_cuda.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
            torch_cuda.cuda.synchronize()
        got = p.call(data, 5, device=dev)
        p.same_state()
        assert len(got) > nmsgs // 2 and p.dem.avr_stats()["frames"] == nmsgs
    elif chunking == "random-device":
        dev = torch_cuda.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
        torch_cuda.cuda.synchronize()
        pos = 0
        for part in A.random_cuts(rng, data):
            p.call(part, 5, device=dev[pos:pos + len(part)])
            pos += len(part)
        p.same_state()
        assert p.dem.avr_stats()["frames"] == nmsgs
    else:
        head = data[:2048] if chunking == "1" else data
        chunks = A.random_cuts(rng, head) if chunking == "random" else A.chunked(head, int(chunking))
        assert p.feed(chunks, 5) > 0
    p.probe(6, rng)


# (b) the reader test's streams, so that every state crosses call boundaries
@pytest.mark.parametrize("name", sorted(A.edge_streams()))
def test_edge_streams(make, name):
    data, mode_ac = A.edge_streams()[name]
    rng = random.Random(len(name))
    for chunks in ([data], A.chunked(data, 1) if len(data) < 3000 else A.chunked(data, 255), A.chunked(data, 256),
                   A.chunked(data, 257), A.random_cuts(rng, data, (1, 2, 7, 31, 255, 256, 257, 300))):
        p = make(mode_ac=mode_ac, keep=True)
        p.feed(chunks, 9)
        assert p.dem.avr_stats()["frames"] > 0
    # the newline as the first and as the last byte of a call, on the last pair
    p.feed([b"*8D48", b"\n", b"\n" + A.star(A.df17(5)), A.star(A.df17(6))[:-1], b"\n"], 10)
    p.probe(11, rng)


def test_discard_flag_crosses_calls(make):
    p = make()
    ok = A.star(A.df17(0x4840D6))
    p.feed([b"x" * 256, b"x", ok[:-1], b"", b"y" * 5000, b"\n" + ok, b" " * 257, b"\n", ok, b" " * 256, b"\n" + ok], 3)
    assert p.dem.avr_stats() == dict(lines=6, frames=3, dropped_lines=1, long_lines=2)


# (c) lines across every internal boundary: the workgroup's span, its look-back, the mask words and the threads' bytes
# inside it, and the seam between the kept bytes and the new ones
def test_lines_across_the_kernels_boundaries(make, consts):
    span, lookback, _ = consts
    rng = random.Random(11)
    a, b = A.df17(0x4840D6), A.df4(0x4840D6)

    def fill_to(out, target):
        """Lines (valid ones, mostly behind white space so that they stay few; empty, junk) up to exactly `target` bytes."""
        while len(out) < target:
            left = target - len(out)
            line = rng.choice([A.star(a), b"\n", b"junk\n"] + [A.padded(b, rng.randrange(100, 257), rng)] * 5)
            out += line if len(line) <= left else b" " * (left - 1) + b"\n"
        assert len(out) == target

    body = bytearray()
    fill_to(body, span - 40)
    body += A.star(a)                      # a plain line across the first span's end
    fill_to(body, 2 * span - 130)
    body += A.padded(a, 256, rng)          # the longest accepted line across the second
    fill_to(body, 3 * span - 200)
    body += A.padded(a, 257, rng) + A.star(b)  # an overlong one across the third, a valid one right behind it
    fill_to(body, 4 * span - 256 - 1)
    body += A.padded(b, 256)               # ends with the span: its start is the first byte the look-back must reach
    body += A.padded(a, 256) + A.star(a)
    body = bytes(body)
    shifts = list(range(0, 66)) + [lookback - 257, lookback - 256, 255, 256, 257, lookback, span - 1]
    p = make()
    for d in shifts:  # every stream ends with a newline: the pair starts each one in the same state
        data = (b" " * (d - 1) + b"\n" if d else b"") + body
        assert p.feed([data], 1) > 10
    # the seam: the same stream behind every length of kept bytes, in a piece that spans workgroups
    line = A.star(a)[:-1]
    start = body.index(b"\n", span) + 1  # a line start
    for keepn in (1, 15, 16, 17, 63, 64, 65, 255, 256):
        kept = line[:keepn] if keepn < len(line) else b" " * (keepn - len(line)) + line
        rest = line[keepn:] + b"\n" + body[start:]
        assert len(kept) == keepn
        before = p.dem.avr_stats()
        p.feed([body[:start] + kept, rest], 2)
        after = p.dem.avr_stats()
        assert after["long_lines"] - before["long_lines"] == 1 and after["frames"] - before["frames"] > 10


# (d) corrupted text under the three --fix levels
@pytest.mark.parametrize("nfix", [0, 1, 2])
def test_corrupted_text(make, capture_lines, nfix):
    rng = random.Random(100 + nfix)
    data = A.corrupt(rng, capture_lines[0], 0.01)
    # bit errors too, so that the repair levels differ: flip one hex digit's low bit in some lines
    out = bytearray(data)
    for _ in range(300):
        i = rng.randrange(len(out))
        if out[i] in b"02468ACE":
            out[i] += 1
    p = make(nfix=nfix, mode_ac=nfix % 2)
    p.feed(A.random_cuts(rng, bytes(out)), 1000)
    st = p.dem.avr_stats()
    assert st["dropped_lines"] > 0 and st["frames"] > capture_lines[1] // 2
    assert p.chk.stats["remote_rejected_bad"] > 0
    if nfix:
        assert p.chk.stats["remote_accepted"][1] > 0
    p.probe(1001, rng)


# (e) the five prefixes, with and without MSD_AVR_KEEP_TIMESTAMP
@pytest.mark.parametrize("keep", [False, True])
def test_mixed_prefixes(make, keep):
    rng = random.Random(21)
    data = A.mixed_prefix_stream(rng, 1500, [rng.randrange(1, 1 << 24) for _ in range(20)])
    p = make(mode_ac=1, keep=keep)
    got = np.concatenate([p.call(part, 4) for part in A.random_cuts(rng, data)])
    p.same_state()
    assert len(got) > 500 and (got["msgbits"] == 16).any() and (got["signalLevel"] > 0).any()
    assert bool((got["timestampMsg"] != 0).any()) == keep
    p.probe(5, rng)


# (f) '<' lines with the flag and Beast frames of the same messages: the same records
def test_signal_lines_match_the_beast_path(make):
    rng = random.Random(22)
    p = make(mode_ac=1, keep=True)
    addrs = [rng.randrange(1, 1 << 24) for _ in range(10)]
    avr, beast = bytearray(), bytearray()
    for _ in range(400):
        a = rng.choice(addrs)
        body = rng.choice([A.df17(a), A.df4(a), bytes([0x12, 0x34])])
        ts, sig = rng.randrange(1 << 48), rng.randrange(256)
        avr += b"<%012X%02X" % (ts, sig) + body.hex().encode() + b";\n"
        beast += frame({2: ord("1"), 7: ord("2"), 14: ord("3")}[len(body)], body, ts, sig)
    got = p.call(bytes(avr), 9)
    assert len(got) > 300 and (got["timestampMsg"] != 0).all()
    fresh = make(mode_ac=1)  # a context that has seen nothing, as p's had not
    assert_same_records(got, fresh.dem.accept_beast(bytes(beast), 9))
    assert_same_stats(remote(p.dem), remote(fresh.dem))


# (g) the filter is shared, both ways
def test_avr_adds_reach_the_gpu_resolve_path(pkg, oracle, torch_cuda):
    import mag_scenes as ms
    Cn = pkg.CHUNK
    rng = random.Random(8)
    known = rng.sample(range(1, 1 << 24), 40)
    strangers = rng.sample(range(1, 1 << 24), 20)
    orc = oracle.Oracle(oracle.FMT_MAG16, 58, 1, 0)
    p = Pair(pkg, oracle, orc=orc, fmt=pkg.FMT_MAG16)
    try:
        data = b"".join(A.star(A.df17(a)) for a in known)
        assert len(p.call(data, 0)) == len(known)
        assert all(orc.filter_test(a) for a in known)
        sc = ms.Scene(8 * Cn - 5, seed=8)  # two batches of four buffers, both resolved on the GPU
        sample = 1000
        for k in range(400):
            a = known[k % len(known)] if k % 3 else strangers[k % len(strangers)]
            sc.frame(sample, df=4 if k % 2 else 5, addr=a, accept=a in known)
            sample += 2500
        want, wstats = orc.replay(sc.mag, cap=1 << 16)
        d = torch_cuda.from_numpy(sc.mag.view(np.uint8).copy()).to("cuda:0")
        got = pkg.replay_device(p.dem, d.data_ptr(), sc.n, 4 * Cn)
        assert p.dem.timing()["resolve_passes"] > 0
        assert len(want) > 200 and {int(m["msgtype"]) for m in want} == {4, 5}
        for f in ("timestampMsg", "sysTimestampMsg", "signalLevel", "addr", "msgtype", "correctedbits", "score", "crc",
                  "bestphase"):
            assert np.array_equal(got[f], want[f]), f
        assert np.array_equal(got["msg"], want["msg"])
        assert p.dem.stats()["demod_rejected_unknown_icao"] == wstats["demod_rejected_unknown_icao"] > 0
    finally:
        p.close()


def test_a_call_that_completes_no_line_still_expires(make):
    rng = random.Random(5)
    p = make()
    a, b = 0x111111, 0x222222
    replies = A.star(A.df4(a)) + A.star(A.df4(b))
    # the flips happen in calls that carry nothing, or a piece of a line only
    for now, data in ((0, A.star(A.df17(a)) + replies), (30000, b""), (70000, A.star(A.df17(b)) + replies),
                      (140000, b"*20000"), (200000, b"5"), (200001, b"30"), (200002, b"\n" + replies)):
        p.feed([data], now)
    p.probe(200003, rng)
    assert p.chk.stats["remote_rejected_unknown_icao"] > 0


# (h) one call longer than a piece
def test_a_call_longer_than_one_piece(make, consts):
    rng = random.Random(9)
    a = [A.df17(rng.randrange(1, 1 << 24)) for _ in range(8)]
    block = bytearray()
    for k in range(100):  # mostly white space and overlong lines, so that the checker's per-record Python stays short
        block += A.padded(rng.choice(a + [A.df4(1)]), rng.randrange(150, 257), rng)
        block += b"z" * rng.randrange(257, 900) + b"\n" + b" " * rng.randrange(600, 2000) + b"\n"
    block = bytes(block)
    data = block * (consts[2] // len(block) + 4)
    assert consts[2] < len(data) < consts[2] + (1 << 20)
    p = make()
    assert p.feed([data], 77) > 3000
    assert p.dem.avr_stats()["long_lines"] > 0
    p.probe(78, rng)


# (i) error codes and msd_reset
def test_busy_invalid_and_reset(pkg, make, torch_cuda):
    p = make()
    dem = p.dem
    ok = A.star(A.df17(0x4840D6))
    iq = np.full(2 * pkg.CHUNK * 2, 127, dtype=np.uint8)
    d = torch_cuda.from_numpy(iq).to("cuda:0")
    dem.launch_device(d.data_ptr(), 2 * pkg.CHUNK, last=True)
    with pytest.raises(pkg.MsdError) as e:
        dem.accept_avr(ok, 0)
    assert f"{-errno.EBUSY}" in str(e.value)
    dem.collect()
    L = pkg.capi.lib()
    assert L.msd_accept_avr(dem._h, ok, len(ok), 0, 2, 0, None, None) == -errno.EINVAL
    assert L.msd_accept_avr(dem._h, None, 5, 0, 0, 0, None, None) == -errno.EINVAL
    assert L.msd_get_avr_stats(dem._h, None) == -errno.EINVAL
    assert dem.avr_stats() == dict(lines=0, frames=0, dropped_lines=0, long_lines=0)
    assert len(dem.accept_avr(ok + ok[:-1], 0)) == 1  # one line kept without its newline
    assert dem.avr_stats()["lines"] == 1
    pkg.capi.lib().msd_reset(dem._h)
    assert dem.avr_stats() == dict(lines=0, frames=0, dropped_lines=0, long_lines=0)
    assert len(dem.accept_avr(b"\n", 0)) == 0  # the kept line is gone: this is an empty line
    assert dem.avr_stats() == dict(lines=1, frames=0, dropped_lines=1, long_lines=0)
    dem.accept_avr(b"x" * 300, 0)
    pkg.capi.lib().msd_reset(dem._h)
    assert len(dem.accept_avr(ok, 0)) == 1  # and so is the discard flag
