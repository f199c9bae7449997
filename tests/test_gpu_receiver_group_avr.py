"""msd_group_accept_avr on the GPU: every receiver of a group call against code that has its own CPU tests -- its stream
through avr_streams.Model (the stream rule of include/modes_hip.h in Python) with that receiver's Mode A/C switch and the
entry's timestamp flag, the records that yields through a remote_decode.Checker of that receiver.  Every comparison is
exact: the records of every call per receiver, every remote counter except the diagnostic tile_rewalks, msd_avr_stats,
and the filter afterwards (a probe call: one DF4 line per address any checker saw added, plus decoys)."""
import ctypes as C
import errno
import random

import numpy as np
import pytest

import avr_streams as A
from remote_decode import Checker, assert_same_records, assert_same_stats, frame
from test_gpu_avr_ingest import capture_lines  # noqa: F401  (the module-scoped fixture)
from test_gpu_receiver_group import OracleReceiver, same, uc8_scene
from test_remote_decode_model import df11, df20
from test_wire_readers import flipped

pytestmark = pytest.mark.gpu


def records(pkg, recs):
    """Model.feed's (payload, timestamp, level) tuples as the records msd_avr_parse_line leaves"""
    out = np.zeros(len(recs), dtype=pkg.capi.MESSAGE_DTYPE)
    for k, (pay, ts, level) in enumerate(recs):
        out["msg"][k, :len(pay)] = np.frombuffer(pay, dtype=np.uint8)
        out["msgbits"][k], out["timestampMsg"][k], out["signalLevel"][k] = 8 * len(pay), ts, level
    return out


class Rig:
    """A group, and per receiver a Model and a Checker; call() feeds all three and compares."""

    def __init__(self, pkg, oracle, K, nfix=1, flags=0, levels=None, modeac=None, refs=None):
        self.pkg, self.K = pkg, K
        self.g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, nfix_crc=nfix, flags=flags)
        self.levels = levels or [nfix] * K
        self.modeac = modeac or [0] * K
        for r in range(K):
            if self.levels[r] != nfix:
                self.g.set_receiver_options(r, nfix_crc=self.levels[r])
            if self.modeac[r]:
                self.g.set_receiver_mode_ac(r, 1)
        self.oracle, self.refs = oracle, refs
        self.model = [A.Model(self.modeac[r], False) for r in range(K)]
        self.chk = [self.checker(r) for r in range(K)]

    def checker(self, r):
        return Checker(self.pkg, self.oracle, self.levels[r], self.modeac[r], oracle=self.refs[r].orc if self.refs else None)

    def remote(self, r):
        st = self.g.remote_stats(r)
        st.pop("tile_rewalks")
        return st

    def call(self, chunks, now_ms, keep=False, device=None):
        """chunks: [(receiver, bytes)]; now_ms and keep one value or one per entry.  Returns {receiver: records}."""
        n = len(chunks)
        nows = [now_ms] * n if isinstance(now_ms, int) else list(now_ms)
        keeps = [keep] * n if isinstance(keep, bool) else list(keep)
        ent, n, data = self.g.avr_entries(chunks, nows)
        for i in range(n):
            ent[i].flags = self.pkg.capi.AVR_KEEP_TIMESTAMP if keeps[i] else 0
        if device is not None:
            data = device.from_numpy(np.frombuffer(data + b"\0", dtype=np.uint8).copy()).to("cuda:0")
        got = self.g.accept_avr(data, None, entries=(ent, n))
        rank = {r: i for i, (r, _) in enumerate(chunks)}
        rx = [int(r) for r in got["receiver"]]
        assert all(rank[a] <= rank[b] for a, b in zip(rx[:-1], rx[1:])), "delivery is by entry, in entry order"
        out = {}
        for (r, part), now, k in zip(chunks, nows, keeps):
            self.model[r].keep = k
            recs = self.model[r].feed(part) if len(part) else []  # an empty entry leaves the kept line alone
            out[r] = got["m"][got["receiver"] == r]
            assert_same_records(out[r], self.chk[r].frames(records(self.pkg, recs), now))
        return out

    def beast(self, chunks, now_ms):
        got = self.g.accept_beast(chunks, now_ms)
        out = {}
        for r, part in chunks:
            out[r] = got["m"][got["receiver"] == r]
            assert_same_records(out[r], self.chk[r].beast(part, now_ms))
        return out

    def check_stats(self):
        for r in range(self.K):
            assert_same_stats(self.remote(r), self.chk[r].stats)
            assert self.g.avr_stats(r) == self.model[r].stats, r

    def probe(self, now_ms, rng, decoys=32):
        """One DF4 line per address any checker saw added and a few random ones, to every receiver: each receiver's
        filter must answer as its own checker's."""
        addrs = sorted(set().union(*[c.known for c in self.chk])) + [rng.randrange(1 << 24) for _ in range(decoys)]
        data = b"".join(A.star(A.df4(a)) for a in addrs)
        out = self.call([(r, data) for r in range(self.K)], now_ms)
        self.check_stats()
        return out

    def close(self):
        self.g.close()


@pytest.fixture
def rig(pkg, oracle, torch_cuda):
    made = []

    def f(K, **kw):
        made.append(Rig(pkg, oracle, K, **kw))
        return made[-1]

    yield f
    for r in made:
        r.close()


@pytest.fixture(scope="module")
def consts(pkg):
    L = C.CDLL(pkg.capi.LIB_PATH)
    for n in ("msd_avr_span_bytes", "msd_avr_lookback_bytes"):
        getattr(L, n).restype = C.c_uint32
    return L.msd_avr_span_bytes(), L.msd_avr_lookback_bytes()


def cut(data, sizes):
    """data in chunks of the given sizes, the last size repeated"""
    out, pos, i = [], 0, 0
    while pos < len(data):
        k = sizes[min(i, len(sizes) - 1)]
        out.append(data[pos:pos + k])
        pos += k
        i += 1
    return out


def corrupted_text(rng, text, nlines):
    """as test_gpu_avr_ingest.test_corrupted_text: character substitutions, bit errors in hex digits; one long line"""
    lines = text.split(b"\n")
    at = rng.randrange(len(lines) - nlines)
    out = bytearray(A.corrupt(rng, b"\n".join(lines[at:at + nlines]) + b"\n", 0.01))
    for _ in range(nlines // 3):
        i = rng.randrange(len(out))
        if out[i] in b"02468ACE":
            out[i] += 1
    at = out.index(b"\n", len(out) // 2) + 1
    return bytes(out[:at]) + b"z" * rng.randrange(257, 600) + b"\n" + bytes(out[at:])


ST = A.star
OK, OK2 = A.star(A.df17(0x4840D6)), A.star(A.df17(0xABCDEF))


# 1. K = 4, different corrupted corpora, each stream cut differently, entry order rotated, empty entries and calls that
# omit a receiver, at every group repair level
@pytest.mark.parametrize("nfix", [0, 1, 2])
def test_corrupted_text_cut_differently(pkg, oracle, rig, capture_lines, nfix):
    K = 4
    R = rig(K, nfix=nfix)
    data = [corrupted_text(random.Random(10 * nfix + r), capture_lines[0], 300) for r in range(K)]
    want = [A.Model(0, False) for _ in range(K)]
    for r in range(K):  # what every stream holds, before the group sees it: frames, dropped and long lines, bad frames, adds
        recs = want[r].feed(data[r])
        pre = Checker(pkg, oracle, nfix)
        assert len(recs) > 100 and len(pre.frames(records(pkg, recs), 0)) > 50
        assert want[r].stats["dropped_lines"] > 0 and want[r].stats["long_lines"] > 0
        assert pre.stats["remote_rejected_bad"] > 0 and pre.known
    plans = [[1] * 60 + [4096], [44, 45] * 15 + [4095], [4097, 4095, 4096], [7, 100, 2, 4096, 1, 4097]]
    queues = [cut(data[r], plans[r]) for r in range(K)]
    c = 0
    while any(queues):
        chunks = []
        for k in range(K):
            r = (k + c) % K  # rotated entry order
            if c % 5 == 3 and r == c % K:
                continue  # this call omits the receiver; its bytes wait
            chunks.append((r, queues[r].pop(0) if queues[r] else b""))  # an exhausted stream: an empty entry
        R.call(chunks, 1000 + c)
        c += 1
    assert c > 40
    R.check_stats()
    assert [m.stats for m in R.model] == [m.stats for m in want]
    assert len({tuple(sorted(ch.known)) for ch in R.chk}) > 1  # different filters
    R.probe(2000, random.Random(nfix))


# 2. an address learnt by receiver 0 is known to receiver 0 only, and only from its add on
def test_isolation(rig):
    X = 0x4840D6
    R = rig(2)
    sq, rp = ST(A.df17(X)), ST(A.df4(X))
    a = R.call([(0, rp + sq + rp), (1, rp)], 5)  # the reply in front of the squitter is rejected
    assert [int(m["msgtype"]) for m in a[0]] == [17, 4] and len(a[1]) == 0
    b = R.call([(1, rp), (0, rp)], 6)
    assert len(b[0]) == 1 and len(b[1]) == 0
    R.check_stats()
    assert R.remote(0)["remote_rejected_unknown_icao"] == 1 and R.remote(0)["remote_accepted"][0] == 3
    assert R.remote(1)["remote_rejected_unknown_icao"] == 2 and sum(R.remote(1)["remote_accepted"]) == 0


# 3. bytes of one entry never complete, start or discard a line of a neighbouring one
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("second", ["completes", "newline"])
def test_neighbouring_segments(rig, swap, second):
    R = rig(2)
    head, rest = OK[:20], OK[20:]
    nxt = rest + OK2 if second == "completes" else b"\n" + OK2
    first = [(0, OK2 + head), (1, nxt)]
    a = R.call(first[::-1] if swap else first, 1)
    assert [int(m["addr"]) for m in a[0]] == [0xABCDEF]  # the fragment is kept, not completed by the neighbour's bytes
    assert [int(m["addr"]) for m in a[1]] == [0xABCDEF]  # ... whose first line is dropped, or empty
    assert R.g.avr_stats(0) == dict(lines=1, frames=1, dropped_lines=0, long_lines=0)
    assert R.g.avr_stats(1) == dict(lines=2, frames=1, dropped_lines=1, long_lines=0)
    b = R.call([(1, head), (0, rest)][::-1] if swap else [(1, head), (0, rest)], 2)
    assert [int(m["addr"]) for m in b[0]] == [0x4840D6] and len(b[1]) == 0  # completed by its own next chunk only
    assert [int(m["addr"]) for m in R.call([(1, rest)], 3)[1]] == [0x4840D6]
    R.check_stats()


def test_discarding_is_the_entrys_own(rig):
    R = rig(3)
    a = R.call([(0, OK + b"x" * 300), (1, OK[:10]), (2, b"y" * 200)], 1)  # 0 is left inside an overlong line
    assert len(a[0]) == 1
    b = R.call([(0, b"x" * 5 + OK[:-1] + b"\n" + OK), (1, OK[10:] + OK2), (2, b"y" * 57)], 2)
    assert len(b[0]) == 1 and len(b[1]) == 2  # 0 discards up to its first newline; its neighbour is not discarding
    assert R.g.avr_stats(0) == dict(lines=3, frames=2, dropped_lines=0, long_lines=1)
    assert R.g.avr_stats(1) == dict(lines=2, frames=2, dropped_lines=0, long_lines=0)
    c = R.call([(2, b"\n" + OK), (0, b"")], 3)  # 200 kept + 57 new bytes passed 256 without a newline
    assert len(c[2]) == 1 and R.g.avr_stats(2) == dict(lines=2, frames=1, dropped_lines=0, long_lines=1)
    R.check_stats()


# 4. lines on the kernels' boundaries: spans, 64-byte mask words, the look-back clipped at s0, the 256 / 257 edge
def test_boundaries(rig, consts):
    span, lookback = consts
    rng = random.Random(4)
    R = rig(3)
    a, b = A.df17(0x4840D6), A.df4(0x4840D6)

    def fill_to(out, target):
        while len(out) < target:
            left = target - len(out)
            line = rng.choice([ST(a), b"\n", b"junk\n"] + [A.padded(b, rng.randrange(100, 257), rng)] * 5)
            out += line if len(line) <= left else b" " * (left - 1) + b"\n"
        assert len(out) == target

    body = bytearray()
    fill_to(body, span - 40)
    body += ST(a)                          # across the first span's end
    fill_to(body, 2 * span - 130)
    body += A.padded(a, 256, rng)          # the longest accepted line across a span seam
    fill_to(body, 3 * span - 200)
    body += A.padded(a, 257, rng) + ST(b)  # an overlong one across a seam, a valid one right behind it
    fill_to(body, 4 * span - 257)
    body += A.padded(b, 256) + A.padded(a, 256) + ST(a)  # ends with the span: the first byte the look-back must reach
    body = bytes(body)
    m = A.Model(0, False)
    assert len(m.feed(body)) > 20 and m.stats["long_lines"] == 1 and m.stats["dropped_lines"] > 0
    # shifted so that newline, start, ';' and prefix fall on either side of span and mask-word boundaries
    shifts = [0, 1, 2, 17, 18, 19, 44, 45, 46, 62, 63, 64, 65, lookback - 257, lookback - 256, lookback, span - 1]
    for k in range(0, len(shifts), 3):
        chunks = [(r, (b" " * (d - 1) + b"\n" if d else b"") + body) for r, d in enumerate(shifts[k:k + 3])]
        assert all(len(v) > 10 for v in R.call(chunks, 1).values())
    # the 256 / 257 edge measured from s0: a kept line, then the rest of a line of exactly 256 and of 257 bytes
    for keepn in (1, 63, 64, 65, 200, 255):
        l256, l257 = A.padded(a, 256), A.padded(a, 257)
        R.call([(0, l256[:keepn]), (1, l257[:keepn]), (2, ST(a)[:min(keepn, 20)])], 2)
        before = [R.g.avr_stats(r) for r in range(3)]
        out = R.call([(0, l256[keepn:] + body), (1, l257[keepn:] + body), (2, ST(a)[min(keepn, 20):] + body)], 2)
        after = [R.g.avr_stats(r) for r in range(3)]
        assert len(out[0]) == len(out[1]) + 1 == len(out[2])
        assert [after[r]["long_lines"] - before[r]["long_lines"] for r in range(3)] == [1, 2, 1]
    # entries of 4095, 4096 and 4097 bytes behind kept lines of 0, 1 and 256 bytes
    for kept in (0, 1, 256):
        for r, size in enumerate((span - 1, span, span + 1)):
            if kept:
                R.call([(r, (b" " * 300 + ST(a) + b" " * 256)[-kept:])], 3)
        chunks = []
        for r, size in enumerate((span - 1, span, span + 1)):
            part = bytearray(ST(b) if kept else b"")
            fill_to(part, size - len(ST(a)) + 7)
            chunks.append((r, bytes(part) + ST(a)[:-7]))
        assert all(len(x) == size for (_, x), size in zip(chunks, (span - 1, span, span + 1)))
        assert all(len(v) > 3 for v in R.call(chunks, 3).values())
        R.call([(r, ST(a)[-7:]) for r in range(3)], 3)
    R.check_stats()
    R.probe(4, rng)


# 5. one receiver's entries through the group equal msd_accept_avr on a context fed the same calls
def test_same_as_a_context(pkg, rig, capture_lines):
    rng = random.Random(5)
    data = corrupted_text(rng, capture_lines[0], 300)
    R = rig(2)
    dem = pkg.Demodulator(fmt=pkg.FMT_UC8, nfix_crc=1, message_capacity=1 << 16, max_batch_samples=4 * pkg.CHUNK)
    try:
        for k, part in enumerate(cut(data, [3, 4096, 45, 257, 4097, 1, 2000])):
            got = R.call([(1, part)], 50 + k, keep=bool(k % 2))
            assert_same_records(got[1], dem.accept_avr(part, 50 + k, keep_timestamp=bool(k % 2)))
        assert R.model[1].stats["frames"] > 100
        known = sorted(R.chk[1].known) + [rng.randrange(1 << 24) for _ in range(32)]
        probe = b"".join(ST(A.df4(x)) for x in known)
        assert_same_records(R.call([(1, probe)], 99)[1], dem.accept_avr(probe, 99))
        st = dem.remote_stats()
        st.pop("tile_rewalks")
        assert st == R.remote(1)
        assert dem.avr_stats() == R.g.avr_stats(1)
    finally:
        dem.close()


# 6. each receiver's own repair level and Mode A/C switch, the timestamp flag per entry; '<' lines against Beast frames
def test_per_receiver_options(pkg, rig):
    rng = random.Random(6)
    levels, modeac = [0, 1, 2, 1], [0, 1, 0, 1]
    R = rig(4, levels=levels, modeac=modeac)
    parts = []
    for k in range(60):
        a = 0x500000 + k
        good = A.df17(a)
        ts = b"%012X" % (k + 1)
        parts += [ST(good), b":" + flipped(good, [rng.randrange(40, 112)]).hex().encode() + b";\n",
                  b"@" + ts + flipped(good, rng.sample(range(40, 112), 2)).hex().encode() + b";\n",
                  b"%" + ts + df11(a, 0).hex().encode() + b";\n",
                  b"<" + ts + b"%02X" % rng.randrange(256) + flipped(df11(a, 0), [rng.randrange(8, 32)]).hex().encode() + b";\n",
                  b"*%04X;\n" % rng.randrange(1 << 16)]
    data = b"".join(parts)
    keeps = [True, False, True, False]
    got = R.call([(r, data) for r in range(4)], 7, keep=keeps)
    R.check_stats()
    acc = [R.remote(r)["remote_accepted"] for r in range(4)]
    assert acc[0][1] == acc[0][2] == 0 and acc[1][1] > 0 and acc[1][2] == 0 and acc[2][2] > 0
    for r in range(4):
        nac = int(np.sum(got[r]["msgtype"] == 32))
        assert nac == (60 if modeac[r] else 0) and R.remote(r)["remote_received_modeac"] == nac
        assert R.g.avr_stats(r)["dropped_lines"] == (0 if modeac[r] else 60)
        assert bool((got[r]["timestampMsg"] != 0).any()) == keeps[r]
    again = R.call([(r, data) for r in range(4)], 8, keep=[not k for k in keeps])  # the flag is the entry's
    for r in range(4):
        assert bool((again[r]["timestampMsg"] != 0).any()) != keeps[r]
    # '<' lines on receiver 1 and the same messages as Beast frames on receiver 3 (same options, same history)
    avr, beast = bytearray(), bytearray()
    for _ in range(200):
        a = 0x500000 + rng.randrange(60)
        body = rng.choice([A.df17(a), A.df4(a), bytes([0x12, 0x34])])
        ts, sig = rng.randrange(1 << 48), rng.randrange(256)
        avr += b"<%012X%02X" % (ts, sig) + body.hex().encode() + b";\n"
        beast += frame({2: ord("1"), 7: ord("2"), 14: ord("3")}[len(body)], body, ts, sig)
    x = R.call([(1, bytes(avr))], 9, keep=True)[1]
    y = R.beast([(3, bytes(beast))], 9)[3]
    assert len(x) > 150 and (x["signalLevel"] > 0).any()
    assert_same_records(x, y)
    with pytest.raises(pkg.MsdError) as e:  # an AVR entry is history: the level is fixed
        R.g.set_receiver_options(0, nfix_crc=1)
    assert f"{-errno.EBUSY}" in str(e.value)
    R.g.set_receiver_options(0, nfix_crc=0, preamble_threshold=70)  # the current level is always allowed


# 7. Beast and AVR entries on one receiver: one set of remote counters, two framing states
def test_beast_and_avr_on_one_receiver(pkg, rig):
    R = rig(2)
    assert sum(R.remote(1)["remote_accepted"]) == 0
    R.call([(1, OK)], 0)
    assert R.remote(1)["remote_accepted"][0] == 1  # a group that has only ever seen AVR
    F = frame(ord("3"), A.df17(0x123456))
    R.call([(0, OK2 + OK[:17])], 1)            # left in mid-line ...
    R.beast([(0, F + F[:12])], 2)              # ... across a Beast call that is left in mid-frame
    a = R.call([(0, OK[17:] + OK2[:5])], 3)
    assert [int(m["addr"]) for m in a[0]] == [0x4840D6]
    b = R.beast([(0, F[12:] + frame(ord("2"), A.df4(0x4840D6)))], 4)
    assert [int(m["msgtype"]) for m in b[0]] == [17, 4]
    c = R.call([(0, OK2[5:] + ST(A.df4(0x123456)))], 5)  # an address learnt from Beast accepts an AVR reply
    assert [int(m["msgtype"]) for m in c[0]] == [17, 4]
    R.check_stats()
    st = R.remote(0)
    assert st["frames"] == 7 and st["remote_accepted"][0] == 7 and R.g.avr_stats(0)["frames"] == 4


# 8. one filter per receiver for AVR and IQ, both ways, with the resolve on the GPU and on the host
@pytest.mark.parametrize("stage", ["gpu", "host_resolve"])
def test_shared_filter_with_the_iq_path(pkg, oracle, rig, stage):
    rng = random.Random(7)
    flags = pkg.capi.CFG_HOST_RESOLVE if stage == "host_resolve" else 0
    refs = [OracleReceiver(oracle, oracle.FMT_UC8) for _ in range(2)]
    R = rig(2, flags=flags, refs=refs)
    known = rng.sample(range(1, 1 << 24), 20)
    others = rng.sample(range(1, 1 << 24), 20)
    R.call([(0, b"".join(ST(A.df17(a)) for a in known)), (1, b"".join(ST(A.df17(a)) for a in others))], 0)
    for buf in range(2):
        scene = uc8_scene([(1000 + 3000 * k, (4, 5)[k % 2], known[(k + 20 * buf) % 20]) for k in range(40)])
        got = R.g.submit(np.concatenate([scene, scene]), [0, 1])
        for r in range(2):
            same(got["m"][got["receiver"] == r], refs[r].feed(scene), f"buffer {buf} receiver {r}")
    s0, s1 = R.g.stats(0), R.g.stats(1)
    assert s0["demod_accepted"][0] >= 70 and sum(s1["demod_accepted"]) == 0 and s1["demod_rejected_unknown_icao"] >= 70
    if stage == "gpu":
        assert R.g.timing()["resolve_passes"] == 1 and R.g.timing()["resolve_fallback"] == 0  # no upload, no host resolve
    # the other way: addresses learnt from receiver 1's IQ make a later AVR reply acceptable on receiver 1 only
    fresh = rng.sample(range(1, 1 << 24), 20)
    sq = uc8_scene([(1000 + 3000 * k, 17, fresh[k % 20]) for k in range(40)])
    quiet = uc8_scene([])
    got = R.g.submit(np.concatenate([quiet, sq]), [0, 1])
    same(got["m"][got["receiver"] == 0], refs[0].feed(quiet))
    same(got["m"][got["receiver"] == 1], refs[1].feed(sq))
    learnt = [a for a in fresh if refs[1].orc.filter_test(a)]
    assert len(learnt) >= 15
    replies = b"".join(ST(A.df4(a)) + ST(df20(a)) for a in learnt)
    out = R.call([(0, replies), (1, replies)], 1)
    assert len(out[0]) == 0 and len(out[1]) == 2 * len(learnt)
    R.check_stats()


# 9. per-entry clocks across the 60 s flip; an entry that completes no line still expires; a zero-byte entry only expires
def test_clocks(rig):
    R = rig(3)
    a, b = 0x111111, 0x222222
    replies = ST(A.df4(a)) + ST(A.df4(b))
    steps = ((0, ST(A.df17(a)) + replies), (30000, b""), (70000, ST(A.df17(b)) + replies), (140000, b"*20000"),
             (200000, b"5"), (200001, b"30"))
    for k, (t0, data) in enumerate(steps):
        # receiver 0 crosses the flips in calls that carry nothing or a piece of a line; 1 gets the same bytes on a slow
        # clock; 2 the same clock as 0 with zero-byte entries only
        R.call([(0, data), (1, data), (2, data if k == 0 else b"")], [t0, k, t0])
    out = R.call([(r, (b"" if r == 2 else b"\n") + replies) for r in range(3)], [200002, 7, 200002])
    assert len(out[0]) == 0 and len(out[1]) == 2 and len(out[2]) == 0
    assert R.chk[0].stats["remote_rejected_unknown_icao"] > 0
    R.check_stats()
    R.probe([200003, 8, 200003], random.Random(9))


# 10. one receiver's active table fills up inside its entry; then an IQ buffer for that receiver
def test_full_active_table_and_the_hand_over(oracle, rig):
    rng = random.Random(10)
    refs = [OracleReceiver(oracle, oracle.FMT_UC8) for _ in range(2)]
    R = rig(2, refs=refs)
    addrs = rng.sample(range(1, 1 << 24), 6000)
    full = b"".join(ST(A.df17(a)) + ST(A.df4(rng.choice(addrs))) for a in addrs)
    R.call([(1, OK + OK2), (0, full)], 0)
    assert R.chk[0].stats["remote_rejected_unknown_icao"] > 0  # replies of aircraft the full table could not take
    R.check_stats()
    R.probe(1, rng)
    ins = [a for a in addrs[:30] if refs[0].orc.filter_test(a)]
    outs = [a for a in addrs[-400:] if not refs[0].orc.filter_test(a)][:10]
    assert ins and outs
    scene = uc8_scene([(1000 + 3000 * k, 4, (ins + outs)[k % len(ins + outs)]) for k in range(40)])
    got = R.g.submit(np.concatenate([scene, scene]), [0, 1])
    for r in range(2):
        same(got["m"][got["receiver"] == r], refs[r].feed(scene), f"receiver {r}")
    assert R.g.stats(0)["demod_accepted"][0] > 0 and R.g.stats(0)["demod_rejected_unknown_icao"] > 0
    R.probe(2, rng, decoys=4)


# 11. a wide call from device and from host memory
@pytest.mark.parametrize("where", ["device", "host"])
def test_wide_call(rig, torch_cuda, where):
    K = 64
    rng = random.Random(11)
    R = rig(K)
    dev = torch_cuda if where == "device" else None
    small = [b"", b"\n", b"*8D48", OK[:30], b";\n" + OK, b" " * 40]
    for c in range(3):
        chunks = []
        for r in range(K):
            if r % 8 == c:
                chunks.append((r, A.mixed_prefix_stream(rng, 40, [0x600000 + r, 0x600100 + r])[:-rng.randrange(1, 9)]))
            else:
                chunks.append((r, rng.choice(small)))
        rng.shuffle(chunks)
        R.call(chunks, 10 + c, device=dev)
    R.check_stats()
    assert sum(m.stats["frames"] for m in R.model) > 400 and sum(len(c.known) for c in R.chk) > 20
    R.probe(30, rng, decoys=4)


# 12. a call of two pieces: nine entries of nearly 1 MiB, mostly lines of blanks
def test_a_call_of_two_pieces(pkg, rig, torch_cuda):
    rng = random.Random(12)
    R = rig(9)
    big = []
    for r in range(9):
        head = A.mixed_prefix_stream(rng, 20, [0x700000 + r]) + b"q" * 300 + b"\n"
        tail = A.mixed_prefix_stream(rng, 20, [0x700000 + r, 0x700100 + r]) + ST(A.df17(r + 1))[:9]
        room = (1 << 20) - 8 - r - len(head) - len(tail)
        blanks = (b" " * 255 + b"\n") * (room // 256) + (b" " * (room % 256 - 1) + b"\n" if room % 256 else b"")
        big.append((r, head + blanks + tail))
        assert len(A.Model(0, False).feed(big[-1][1])) > 20  # real messages around the blanks
    assert sum(len(b) for _, b in big) > (8 << 20) and all(len(b) <= pkg.capi.GROUP_AVR_ENTRY_MAX for _, b in big)
    out = R.call(big, 20, device=torch_cuda)  # eight entries are the first piece, the ninth is the second
    assert all(len(v) > 0 for v in out.values())
    R.call([(r, ST(A.df17(r + 1))[9:]) for r in range(9)], 21)
    R.check_stats()
    assert all(m.stats["long_lines"] == 1 and m.stats["dropped_lines"] > 4000 for m in R.model)
    R.probe(30, rng, decoys=4)


# 13. arguments: every -EINVAL leaves the state untouched; n == 0; reset_receiver
def test_arguments_and_reset(pkg, rig):
    capi = pkg.capi
    R = rig(3, levels=[1, 2, 1], modeac=[0, 1, 0])
    L = capi._group_lib()
    R.call([(0, OK[:10]), (1, b"x" * 300), (2, OK2)], 3)  # a kept line, a discard flag, a known address
    data = np.frombuffer(OK + OK, dtype=np.uint8).copy()
    E = capi.GroupAvrEntry

    def raw(entries, n=None, ptr=data.ctypes.data, null_entries=False):
        arr = (E * max(len(entries), 1))(*entries)
        return L.msd_group_accept_avr(R.g._h, ptr, 0, None if null_entries else arr, len(entries) if n is None else n,
                                      None, None)

    bad = [
        [E(3, 0, 0, 4, 0, 9)],                                    # a receiver out of range
        [E(0, 0, 0, 4, 0, 9), E(0, 0, 4, 4, 0, 9)],               # the same receiver twice
        [E(0, 0, 0, 1, 0, 9), E(1, 0, 1, 1, 0, 9), E(2, 0, 2, 1, 0, 9), E(0, 0, 3, 1, 0, 9)],  # n > max_receivers
        [E(0, 2, 0, 4, 0, 9)],                                    # an unknown flag bit
        [E(0, 3, 0, 4, 0, 9)],
        [E(0, 0, 0, 4, 1, 9)],                                    # reserved
        [E(0, 0, 0, capi.GROUP_AVR_ENTRY_MAX + 1, 0, 9)],         # too long
        [E(0, 0, (1 << 64) - 2, 4, 0, 9)],                        # an offset that wraps
        [E(0, 0, (1 << 47) + 1, 0, 0, 9)],                        # an offset no address space has
        [E(1, 0, 0, 4, 0, 9), E(2, 1, 0, 4, 0, 9), E(0, 0, 0, 4, 7, 9)],  # a bad entry behind good ones
    ]
    for entries in bad:
        assert raw(entries) == -errno.EINVAL, [tuple(getattr(e, f) for f, _ in E._fields_) for e in entries]
    assert raw([E(0, 0, 0, 4, 0, 9)], ptr=None) == -errno.EINVAL
    assert raw([E(0, 0, 0, 4, 0, 9)], null_entries=True) == -errno.EINVAL
    assert raw([], ptr=None, null_entries=True) == 0  # n == 0
    assert len(R.g.accept_avr([], 9)) == 0
    R.check_stats()
    # nothing was touched: the kept line completes, the discard goes on, the filters and clocks did not move
    out = R.call([(0, OK[10:]), (1, OK[:-1] + b"\n" + OK), (2, ST(A.df4(0xABCDEF)))], 4)
    assert all(len(out[r]) == 1 for r in range(3))
    assert R.g.avr_stats(1) == dict(lines=2, frames=1, dropped_lines=0, long_lines=1)
    R.check_stats()
    # reset: the kept line, the discard flag and both sets of counters go, the options stay
    R.call([(0, OK[:10]), (1, b"x" * 300)], 5)
    for r in (0, 1):
        R.g.reset_receiver(r)
        assert R.g.avr_stats(r) == dict(lines=0, frames=0, dropped_lines=0, long_lines=0)
        assert all(v == 0 or v == [0, 0, 0] for v in R.g.remote_stats(r).values())
        R.model[r], R.chk[r] = A.Model(R.modeac[r], False), R.checker(r)
    assert R.g.receiver_options(1)["nfix_crc"] == 2 and R.g.receiver_mode_ac(1) == 1
    out = R.call([(0, OK[10:] + OK), (1, b"*7700;\n" + OK)], 6)  # no kept line to complete, nothing to discard
    assert len(out[0]) == 1 and [int(m["msgtype"]) for m in out[1]] == [32, 17]
    assert R.g.avr_stats(0) == dict(lines=2, frames=1, dropped_lines=1, long_lines=0)
    R.check_stats()
    R.g.set_receiver_options(0, nfix_crc=1)  # unchanged level: allowed
    R.g.reset_receiver(0)
    R.g.set_receiver_options(0, nfix_crc=0)  # after the reset the level may change again
