"""msd_group_accept_beast on the GPU: every receiver of a group call against a checker of its own
(tests/remote_decode.py's Checker, the CPU restatement the context path is held to).  Every comparison is exact: the
records of every call per receiver, every remote counter except the diagnostic tile_rewalks, and the filter afterwards
(a probe call: one DF4 per address the checker saw added, plus decoys)."""
import errno
import random

import numpy as np
import pytest

from remote_decode import Checker, assert_same_records, assert_same_stats, frame
from test_gpu_beast_ingest import corrupted_corpus, df17
from test_gpu_receiver_group import OracleReceiver, same, uc8_scene
from test_remote_decode_model import df4, df11, df20
from test_wire_readers import flipped

pytestmark = pytest.mark.gpu


class Rig:
    """A group and one checker per receiver; call() feeds both and compares."""

    def __init__(self, pkg, oracle, K, nfix=1, flags=0, levels=None, modeac=None, refs=None):
        self.pkg, self.K = pkg, K
        self.g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, nfix_crc=nfix, flags=flags)
        levels = levels or [nfix] * K
        modeac = modeac or [0] * K
        for r in range(K):
            if levels[r] != nfix:
                self.g.set_receiver_options(r, nfix_crc=levels[r])
            if modeac[r]:
                self.g.set_receiver_mode_ac(r, 1)
        self.chk = [Checker(pkg, oracle, levels[r], modeac[r], oracle=refs[r].orc if refs else None) for r in range(K)]

    def remote(self, r):
        st = self.g.remote_stats(r)
        st.pop("tile_rewalks")
        return st

    def call(self, chunks, now_ms, device=None):
        """chunks: [(receiver, bytes)]; now_ms an int or one per entry.  Returns {receiver: records}."""
        nows = [now_ms] * len(chunks) if isinstance(now_ms, int) else list(now_ms)
        if device is None:
            got = self.g.accept_beast(chunks, nows)
        else:
            ent, n, data = self.g.beast_entries(chunks, nows)
            dev = device.from_numpy(np.frombuffer(data + b"\0", dtype=np.uint8).copy()).to("cuda:0")
            got = self.g.accept_beast(dev, None, entries=(ent, n))
        rank = {r: i for i, (r, _) in enumerate(chunks)}
        rx = [int(r) for r in got["receiver"]]
        assert all(rank[a] <= rank[b] for a, b in zip(rx[:-1], rx[1:])), "delivery is by entry, in entry order"
        out = {}
        for (r, data), now in zip(chunks, nows):
            out[r] = got["m"][got["receiver"] == r]
            assert_same_records(out[r], self.chk[r].beast(data, now))
        return out

    def check_stats(self):
        for r in range(self.K):
            assert_same_stats(self.remote(r), self.chk[r].stats)

    def probe(self, now_ms, rng, decoys=32):
        """One DF4 per address any checker saw added and a few random ones, to every receiver: each receiver's filter
        must answer as its own checker's."""
        addrs = sorted(set().union(*[c.known for c in self.chk])) + [rng.randrange(1 << 24) for _ in range(decoys)]
        data = b"".join(frame(ord("2"), df4(a)) for a in addrs)
        self.call([(r, data) for r in range(self.K)], now_ms)
        self.check_stats()

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


def cut(data, sizes):
    """data in chunks of the given sizes, the last size repeated"""
    out, pos, i = [], 0, 0
    while pos < len(data):
        k = sizes[min(i, len(sizes) - 1)]
        out.append(data[pos:pos + k])
        pos += k
        i += 1
    return out


# 1. K = 4, different corrupted corpora, each stream cut differently, entry order rotated, empty entries and calls that
# omit a receiver, at every group repair level
@pytest.mark.parametrize("nfix", [0, 1, 2])
def test_corrupted_corpora_cut_differently(rig, nfix):
    K = 4
    R = rig(K, nfix=nfix)
    data = [corrupted_corpus(random.Random(10 * nfix + r), 300) for r in range(K)]
    plans = [[1] * 40 + [4096], [44, 45] * 15 + [4095], [4097, 4095, 4096], [7, 100, 2, 4096, 1, 4097]]
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
    assert all(ch.stats["remote_rejected_bad"] > 0 and ch.stats["other_frames"] > 0 for ch in R.chk)
    assert len({tuple(sorted(ch.known)) for ch in R.chk}) == K  # four different filters
    R.probe(2000, random.Random(nfix))


# 2. an address learnt by receiver 0 is known to receiver 0 only, and only from its add on
def test_isolation(rig):
    X = 0x4840D6
    R = rig(2)
    sq, rp = frame(ord("3"), df17(X)), frame(ord("2"), df4(X))
    a = R.call([(0, rp + sq + rp), (1, rp)], 5)  # the reply in front of the squitter is rejected
    assert [int(m["msgtype"]) for m in a[0]] == [17, 4] and len(a[1]) == 0
    b = R.call([(1, rp), (0, rp)], 6)
    assert len(b[0]) == 1 and len(b[1]) == 0
    R.check_stats()
    assert R.remote(0)["remote_rejected_unknown_icao"] == 1 and R.remote(0)["remote_accepted"][0] == 3
    assert R.remote(1)["remote_rejected_unknown_icao"] == 2 and sum(R.remote(1)["remote_accepted"]) == 0


# 3. bytes of one entry never complete, start or charge a frame of a neighbouring one
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("split", [10, 1])
def test_no_leakage_between_neighbouring_segments(rig, swap, split):
    R = rig(2)
    F = frame(ord("3"), df17(0xABCDEF))
    G = frame(ord("3"), df17(0x123456))
    rest = F[split:] + bytes([0x41] * 20)  # what would complete receiver 0's frame, then filler: a gap of 42 or 33 bytes
    first = [(0, G + F[:split]), (1, rest + G)]  # split = 1: the 0x1A is the last byte of receiver 0's entry
    a = R.call(first[::-1] if swap else first, 1)
    assert [int(m["addr"]) for m in a[0]] == [0x123456]  # the fragment is kept, not completed by the neighbour's bytes
    assert [int(m["addr"]) for m in a[1]] == [0x123456]
    assert R.remote(1)["remote_rejected_bad"] == len(rest) // 15 and R.remote(0)["remote_rejected_bad"] == 0
    second = [(0, F[split:]), (1, F[:split])]
    b = R.call(second[::-1] if swap else second, 2)
    assert [int(m["addr"]) for m in b[0]] == [0xABCDEF] and len(b[1]) == 0  # completed by its own next chunk only
    c = R.call([(1, F[split:])], 3)
    assert [int(m["addr"]) for m in c[1]] == [0xABCDEF]
    R.check_stats()


# 4. a group entry against a context fed the same chunks (and both against the checker)
def test_same_as_a_context(pkg, oracle, rig):
    rng = random.Random(4)
    data = corrupted_corpus(rng, 300)
    R = rig(2)
    dem = pkg.Demodulator(fmt=pkg.FMT_UC8, nfix_crc=1, message_capacity=1 << 16, max_batch_samples=4 * pkg.CHUNK)
    try:
        for k, part in enumerate(cut(data, [3, 4096, 45, 4097, 1, 2000])):
            got = R.call([(1, part)], 50 + k)
            assert_same_records(got[1], dem.accept_beast(part, 50 + k))
        known = sorted(R.chk[1].known) + [rng.randrange(1 << 24) for _ in range(32)]
        probe = b"".join(frame(ord("2"), df4(a)) for a in known)
        assert_same_records(R.call([(1, probe)], 99)[1], dem.accept_beast(probe, 99))
        st = dem.remote_stats()
        st.pop("tile_rewalks")
        assert st == R.remote(1)
    finally:
        dem.close()


# 5. an out-of-phase stream (tiles walked again) between two ordinary entries; entry sizes around the tile behind a kept frame
def test_tiles_and_rewalks(rig):
    rng = random.Random(5)
    R = rig(3)
    one = frame(ord("3"), df17(0x1A331A), ts=0x1A331A331A33, signal=0x1A)
    # 1000 frames, 8 tiles.  Following the scanner by hand over these bytes (seed 5), the true chain enters three of the
    # tiles at a 0x1A that is not on the tile's own chain, which starts inside a frame; 400 frames would need no re-walk
    hard = b"".join(one + bytes([0x41] * rng.randrange(3)) for _ in range(1000))
    assert len(hard) > 2 * 4096
    side = [corrupted_corpus(random.Random(50 + r), 100) for r in range(2)]
    R.call([(0, side[0]), (1, hard), (2, side[1])], 0)
    assert R.g.remote_stats(1)["tile_rewalks"] > 0 and R.chk[1].stats["remote_accepted"][0] == 1000
    R.check_stats()
    stream = corrupted_corpus(rng, 700)
    pos = 0
    for k in (1, 4095, 4096, 4097):
        head = frame(ord("3"), df17(0x777000 + k))[:12]  # leaves a kept frame in front of the next entry
        body = frame(ord("3"), df17(0x777000 + k))[12:] + stream[pos:pos + k]
        pos += k
        R.call([(0, head), (2, head)], k)
        R.call([(0, body[:k]), (2, body)], k)
        R.call([(0, body[k:])], k)
    R.check_stats()
    R.probe(5000, rng)


# 6. each receiver's own repair level and Mode A/C switch
def test_per_receiver_options(pkg, rig):
    rng = random.Random(6)
    levels, modeac = [0, 1, 2, 1], [0, 1, 0, 1]
    R = rig(4, levels=levels, modeac=modeac)
    parts = []
    for k in range(60):
        a = 0x500000 + k
        good = df17(a)
        parts += [frame(ord("3"), good), frame(ord("3"), flipped(good, [rng.randrange(40, 112)])),
                  frame(ord("3"), flipped(good, rng.sample(range(40, 112), 2))), frame(ord("2"), df11(a, 0)),
                  frame(ord("2"), flipped(df11(a, 0), [rng.randrange(8, 32)])),
                  frame(ord("1"), bytes([rng.randrange(256), rng.randrange(256)]), ts=k)]
    data = b"".join(parts)
    got = R.call([(r, data) for r in range(4)], 7)
    R.check_stats()
    acc = [R.remote(r)["remote_accepted"] for r in range(4)]
    assert acc[0][1] == acc[0][2] == 0 and acc[1][1] > 0 and acc[1][2] == 0 and acc[2][2] > 0
    for r in range(4):
        nac = int(np.sum(got[r]["msgtype"] == 32))
        assert nac == (60 if modeac[r] else 0) and R.remote(r)["remote_received_modeac"] == 60
    with pytest.raises(pkg.MsdError) as e:  # a Beast entry is history: the level is fixed
        R.g.set_receiver_options(0, nfix_crc=1)
    assert f"{-errno.EBUSY}" in str(e.value)
    R.g.set_receiver_options(0, nfix_crc=0, preamble_threshold=70)  # the current level is always allowed


# 7. one filter per receiver for both inputs, both ways, with the resolve on the GPU and on the host
@pytest.mark.parametrize("stage", ["gpu", "host_resolve"])
def test_shared_filter_with_the_iq_path(pkg, oracle, rig, stage):
    rng = random.Random(7)
    flags = pkg.capi.CFG_HOST_RESOLVE if stage == "host_resolve" else 0
    refs = [OracleReceiver(oracle, oracle.FMT_UC8) for _ in range(2)]
    R = rig(2, flags=flags, refs=refs)
    known = rng.sample(range(1, 1 << 24), 20)
    others = rng.sample(range(1, 1 << 24), 20)
    # Beast squitters on receiver 0 (receiver 1 hears other aircraft) ...
    R.call([(0, b"".join(frame(ord("3"), df17(a)) for a in known)),
            (1, b"".join(frame(ord("3"), df17(a)) for a in others))], 0)
    # ... make the replies of a later capture acceptable for receiver 0 and not for its neighbour: two buffers each
    for buf in range(2):
        scene = uc8_scene([(1000 + 3000 * k, (4, 5)[k % 2], known[(k + 20 * buf) % 20]) for k in range(40)])
        got = R.g.submit(np.concatenate([scene, scene]), [0, 1])
        for r in range(2):
            same(got["m"][got["receiver"] == r], refs[r].feed(scene), f"buffer {buf} receiver {r}")
    s0, s1 = R.g.stats(0), R.g.stats(1)
    assert s0["demod_accepted"][0] >= 70 and sum(s1["demod_accepted"]) == 0 and s1["demod_rejected_unknown_icao"] >= 70
    if stage == "gpu":
        assert R.g.timing()["resolve_passes"] == 1 and R.g.timing()["resolve_fallback"] == 0  # no upload, no host resolve
    # the other way: addresses learnt from receiver 1's IQ make a later Beast DF4 acceptable on receiver 1 only
    fresh = rng.sample(range(1, 1 << 24), 20)
    sq = uc8_scene([(1000 + 3000 * k, 17, fresh[k % 20]) for k in range(40)])
    quiet = uc8_scene([])
    got = R.g.submit(np.concatenate([quiet, sq]), [0, 1])
    same(got["m"][got["receiver"] == 0], refs[0].feed(quiet))
    same(got["m"][got["receiver"] == 1], refs[1].feed(sq))
    learnt = [a for a in fresh if refs[1].orc.filter_test(a)]
    assert len(learnt) >= 15
    replies = b"".join(frame(ord("2"), df4(a)) + frame(ord("3"), df20(a)) for a in learnt)
    out = R.call([(0, replies), (1, replies)], 1)
    assert len(out[0]) == 0 and len(out[1]) == 2 * len(learnt)
    R.check_stats()


# 8. per-entry clocks: one receiver crosses the 60 s flip twice and forgets, its neighbour in the same calls does not
def test_expiry_per_entry(rig):
    R = rig(2)
    a, b = 0x111111, 0x222222
    clocks = ((0, 0), (30000, 1), (70000, 2), (140000, 3), (200000, 4))
    adds = (a, None, b, None, None)
    out = None
    for (t0, t1), add in zip(clocks, adds):
        data = (frame(ord("3"), df17(add)) if add else b"") + frame(ord("2"), df4(a)) + frame(ord("2"), df4(b))
        out = R.call([(0, data), (1, data)], [t0, t1])
    assert len(out[0]) == 0 and len(out[1]) == 2  # the first forgot both aircraft, the second remembers them
    R.check_stats()
    R.probe([200001, 5], random.Random(8))


# 9. one receiver's active table fills up inside its entry; then an IQ buffer for that receiver (beyond the 6000-slot
# rule: resolved on the host against the filter the Beast call left, its snapshot handed over afterwards)
def test_full_active_table_and_the_hand_over(oracle, rig):
    rng = random.Random(9)
    refs = [OracleReceiver(oracle, oracle.FMT_UC8) for _ in range(2)]
    R = rig(2, refs=refs)
    addrs = rng.sample(range(1, 1 << 24), 6000)
    full = b"".join(frame(ord("3"), df17(a)) + frame(ord("2"), df4(rng.choice(addrs))) for a in addrs)
    R.call([(1, corrupted_corpus(rng, 100)), (0, full)], 0)
    assert R.chk[0].stats["remote_rejected_unknown_icao"] > 0  # replies of aircraft the full table could not take
    R.check_stats()
    R.probe(1, rng)
    ins = [a for a in addrs[:30] if refs[0].orc.filter_test(a)]
    outs = [a for a in addrs[-400:] if not refs[0].orc.filter_test(a)][:10]
    assert ins and outs
    scene = uc8_scene([(1000 + 3000 * k, 4, (ins + outs)[k % len(ins + outs)]) for k in range(40)])
    for _ in range(2):  # the second buffer meets the snapshot the first one's host resolve uploaded
        got = R.g.submit(np.concatenate([scene, scene]), [0, 1])
        for r in range(2):
            same(got["m"][got["receiver"] == r], refs[r].feed(scene), f"receiver {r}")
    assert R.g.stats(0)["demod_accepted"][0] > 0 and R.g.stats(0)["demod_rejected_unknown_icao"] > 0
    R.probe(2, rng)


# 10. a wide call from device and from host memory; a call of more than one piece
@pytest.mark.parametrize("where", ["device", "host"])
def test_wide_call(rig, torch_cuda, where):
    K = 64
    rng = random.Random(10)
    R = rig(K)
    dev = torch_cuda if where == "device" else None
    for c in range(2):
        chunks = []
        for r in range(K):
            if r % 8 == c:
                chunks.append((r, corrupted_corpus(rng, 100)))
            else:
                chunks.append((r, rng.choice([b"", b"\x1a", b"\x1a3\x00", bytes(rng.randrange(256) for _ in range(5))])))
        rng.shuffle(chunks)
        R.call(chunks, 10 + c, device=dev)
    R.check_stats()
    # ten entries of about 0.9 MiB, more than one piece (8 MiB): frames at both ends of long runs without a 0x1A
    big = []
    for r in range(10):
        run = bytes([0x40 + r]) * (450 << 10)
        big.append((r, corrupted_corpus(rng, 60) + run + corrupted_corpus(rng, 60) + run + frame(ord("3"), df17(r + 1))[:9]))
    assert sum(len(b) for _, b in big) > (8 << 20) and all(len(b) < (1 << 20) for _, b in big)
    R.call(big, 20, device=dev)
    R.call([(r, frame(ord("3"), df17(r + 1))[9:]) for r in range(10)], 21, device=dev)
    R.check_stats()
    R.probe(30, rng, decoys=8)


# 11. arguments: every -EINVAL leaves the state untouched; n == 0; reset_receiver
def test_arguments_and_reset(pkg, rig):
    capi = pkg.capi
    R = rig(3, levels=[1, 2, 1], modeac=[0, 1, 0])
    L = capi._group_lib()
    F = frame(ord("3"), df17(0xABCDEF))
    R.call([(0, F[:10]), (1, bytes([0x41] * 40) + F[:5]), (2, bytes([0x41] * 40))], 3)  # kept frames and a pending gap
    data = np.frombuffer(F + F, dtype=np.uint8).copy()
    E = capi.GroupBeastEntry

    def raw(entries, n=None, ptr=data.ctypes.data, null_entries=False):
        arr = (E * max(len(entries), 1))(*entries)
        return L.msd_group_accept_beast(R.g._h, ptr, 0, None if null_entries else arr, len(entries) if n is None else n,
                                        None, None)

    bad = [
        [E(3, 0, 0, 4, 0, 9)],                                    # a receiver out of range
        [E(0, 0, 0, 4, 0, 9), E(0, 0, 4, 4, 0, 9)],               # the same receiver twice
        [E(0, 0, 0, 1, 0, 9), E(1, 0, 1, 1, 0, 9), E(2, 0, 2, 1, 0, 9), E(0, 0, 3, 1, 0, 9)],  # n > max_receivers
        [E(0, 1, 0, 4, 0, 9)],                                    # flags
        [E(0, 0, 0, 4, 1, 9)],                                    # reserved
        [E(0, 0, 0, capi.GROUP_BEAST_ENTRY_MAX + 1, 0, 9)],       # too long
        [E(0, 0, (1 << 64) - 2, 4, 0, 9)],                        # an offset that wraps
        [E(0, 0, (1 << 47) + 1, 0, 0, 9)],                        # an offset no address space has
    ]
    for entries in bad:
        assert raw(entries) == -errno.EINVAL, [tuple(getattr(e, f) for f, _ in E._fields_) for e in entries]
    assert raw([E(0, 0, 0, 4, 0, 9)], ptr=None) == -errno.EINVAL
    assert raw([E(0, 0, 0, 4, 0, 9)], null_entries=True) == -errno.EINVAL
    assert raw([], ptr=None, null_entries=True) == 0  # n == 0
    assert len(R.g.accept_beast([], 9)) == 0
    R.check_stats()
    # nothing was touched: the kept frames complete, the pending gap is charged, the clocks did not move
    out = R.call([(0, F[10:]), (1, F[5:]), (2, F)], 4)
    assert all(len(out[r]) == 1 for r in range(3))
    assert R.remote(2)["remote_rejected_bad"] == 2 and R.remote(1)["remote_rejected_bad"] == 2
    R.check_stats()
    # reset: counters, kept frame and gap go, the options stay
    R.call([(1, F[:10] + b""), (2, bytes([0x41] * 29))], 5)
    R.g.reset_receiver(1)
    R.g.reset_receiver(2)
    zero = R.g.remote_stats(1)
    assert all(v == 0 or v == [0, 0, 0] for v in zero.values())
    assert R.g.receiver_options(1)["nfix_crc"] == 2 and R.g.receiver_mode_ac(1) == 1
    for r in (1, 2):
        R.chk[r] = Checker(pkg, R.chk[r].O, (1, 2, 1)[r], (0, 1, 0)[r])
    out = R.call([(1, F[10:] + F), (2, F)], 6)  # no kept frame to complete, no gap of 29 to charge
    assert len(out[1]) == 1 and len(out[2]) == 1 and R.remote(2)["remote_rejected_bad"] == 0
    R.check_stats()
    R.g.set_receiver_options(0, nfix_crc=1)  # unchanged level: allowed
    R.g.reset_receiver(0)
    R.g.set_receiver_options(0, nfix_crc=0)  # after the reset the level may change again


# 12. a call of two pieces: nine entries of just under 1 MiB, mostly filler without a 0x1A
def test_a_call_of_two_pieces(pkg, rig, torch_cuda):
    rng = random.Random(12)
    R = rig(9)
    big = []
    for r in range(9):
        head = corrupted_corpus(rng, 40)
        tail = corrupted_corpus(rng, 40) + frame(ord("3"), df17(r + 1))[:9]  # a frame cut across the call's end
        room = (1 << 20) - 8 - r - len(head) - len(tail)
        big.append((r, head + bytes([0x40 + r]) * room + tail))
    sizes = [len(b) for _, b in big]
    assert sum(sizes) > (8 << 20) >= sum(sizes[:8]) and all(s <= pkg.capi.GROUP_BEAST_ENTRY_MAX for s in sizes)
    out = R.call(big, 20, device=torch_cuda)  # eight entries are the first piece, the ninth is the second
    assert all(len(v) > 0 for v in out.values())
    out = R.call([(r, frame(ord("3"), df17(r + 1))[9:]) for r in range(9)], 21)
    assert all([int(m["addr"]) for m in out[r]] == [r + 1] for r in range(9))  # completed across the piece boundary too
    R.check_stats()
    assert all(ch.stats["garbage_bytes"] > 1000000 for ch in R.chk)  # the filler, charged to no frame
    R.probe(30, rng, decoys=4)
