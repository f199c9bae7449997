"""msd_group_accept_beast_wire / msd_group_accept_avr_wire on the GPU.  Two groups of one configuration get the same
bytes, one through the plain accept call; every entry's bytes of the wire call must equal libmsd_host.so's
msd_beast_frame_out / msd_avr_line_out over the plain group's records of that entry, nmessages their number, and
afterwards the two groups have equal counters and answer a probe alike (remote_out.Twin).  Every comparison is exact."""
import errno
import random

import numpy as np
import pytest

from remote_decode import frame
from remote_out import WIRE_AVR, WIRE_AVR_MLAT, WIRE_BEAST, Twin, ap, avr_stream, beast_stream, corpus, cut_at, es, pi
from test_gpu_receiver_group import uc8_scene
from test_wire_readers import flipped

pytestmark = pytest.mark.gpu
B = 256  # records per workgroup of the wire kernels: msd_wire_store::WT (msd_wire_store_impl.h)


@pytest.fixture
def twin(pkg, torch_cuda):
    made = []

    def f(K, **kw):
        made.append(Twin(pkg, K, **kw))
        return made[-1]

    yield f
    for t in made:
        t.close()


def stream(kind, items, rng=None):
    return beast_stream(items, rng) if kind == "beast" else avr_stream(items, rng)


def sq(addr, ts=0, sig=0x80):
    return (pi(bytes([0x8D]) + addr.to_bytes(3, "big") + b"\x20\x2C\xC3\x71\xC3\x2C\xE0"), ts, sig)


def reply(addr, ts=0, sig=0x80):
    return (ap(bytes([0x20, 0x00, 0x05, 0x30]), addr), ts, sig)


_parity = {}


# 1. parity: K = 4 at levels 0, 1, 2, 1, Mode A/C on for receiver 3, a corrupted corpus per receiver in three calls cut
# inside frames and lines
@pytest.mark.parametrize("stage", ["gpu", "host_resolve"])
@pytest.mark.parametrize("verbatim", [False, True])
@pytest.mark.parametrize("fmt", [WIRE_BEAST, WIRE_AVR, WIRE_AVR_MLAT])
@pytest.mark.parametrize("kind", ["beast", "avr"])
def test_parity(pkg, twin, kind, fmt, verbatim, stage):
    K = 4
    T = twin(K, levels=[0, 1, 2, 1], modeac=[0, 0, 0, 1], flags=pkg.capi.CFG_HOST_RESOLVE if stage == "host_resolve" else 0)
    if kind not in _parity:  # once per input
        _parity[kind] = [stream(kind, corpus(random.Random(100 + r), 300), random.Random(200 + r)) for r in range(K)]
    data = _parity[kind]
    parts = [cut_at(data[r], (len(data[r]) // 3 + 5 + r, 2 * len(data[r]) // 3 + 11 + r)) for r in range(K)]
    corrected = set()
    for c in range(3):
        order = [(c + k) % K for k in range(K)]
        want, _ = T.wire(kind, [(r, parts[r][c]) for r in order], 1000 + c, fmt, verbatim, keep=True)
        for m in want:
            corrected.update(int(x) for x in m["correctedbits"])
    assert corrected == {0, 1, 2}
    T.same_state(random.Random(1), 2000)


# 2. entry edges in one call: empty, half a frame, only rejected, only 2-bit repairs without verbatim, one record,
# and the first two shapes again so that one of them is last
@pytest.mark.parametrize("kind", ["beast", "avr"])
def test_entry_edges(twin, kind):
    rng = random.Random(2)
    T = twin(7, levels=[1, 1, 1, 2, 1, 1, 1])
    one = stream(kind, [sq(0xABCDEF)])
    rejected = stream(kind, [reply(rng.randrange(1 << 24)) for _ in range(5)])  # address/parity of unknown aircraft
    # (not every pair of flipped bits is repaired: the entry's records are those the plain group delivers)
    two_bits = stream(kind, [(flipped(sq(0x123450 + k)[0], rng.sample(range(40, 112), 2)), 0, 0x80) for k in range(12)])
    chunks = [(0, b""), (1, one[:9]), (2, rejected), (3, two_bits), (4, one), (5, b""), (6, one[:9])]
    want, got = T.wire(kind, chunks, 5, WIRE_BEAST, False)
    n2 = len(want[3])
    assert [len(m) for m in want] == [0, 0, 0, n2, 1, 0, 0] and n2 > 0
    assert [(len(b), nm) for _, b, nm in got] == [(0, 0), (0, 0), (0, 0), (0, n2), (len(got[4][1]), 1), (0, 0), (0, 0)]
    assert len(got[4][1]) > 0 and all(int(m["correctedbits"]) == 2 for m in want[3])
    want, got = T.wire(kind, [(1, one[9:]), (6, one[9:]), (3, two_bits)], 6, WIRE_AVR, True)  # the kept halves complete
    assert [nm for _, _, nm in got] == [1, 1, n2] and all(len(b) > 0 for _, b, _ in got)
    T.same_state(rng, 7)


# 3. lengths and the scan: doubled 0x1A in timestamp, signal and payload in runs, entries of B - 1, B, B + 1, 4 B + 1
# records and one record directly behind the longest
@pytest.mark.parametrize("kind,fmt", [("beast", WIRE_BEAST), ("avr", WIRE_BEAST), ("beast", WIRE_AVR_MLAT)])
def test_lengths_and_the_scan(twin, kind, fmt):
    rng = random.Random(3)
    sizes = [B - 1, B, B + 1, 4 * B + 1, 1]
    T = twin(len(sizes))

    def items(n, r):
        out, k = [], 0
        while len(out) < n:  # runs of 1..5 frames rich in 0x1A, then as many without
            run = rng.randrange(1, 6)
            dense = k % 2 == 0
            for _ in range(run):
                me = bytes([0x1A] * rng.randrange(1, 8)).ljust(7, b"\x33") if dense else b"\x20\x2C\xC3\x71\xC3\x2C\xE0"
                body = pi(bytes([0x8D]) + (0x1A0000 + r).to_bytes(3, "big") + me)
                out.append((body, rng.choice([0x1A1A1A1A1A1A, 0x1A331A331A33, 0x001A00001A00]) if dense else 0x112233445566,
                            0x1A if dense else 0x80))
            k += 1
        return out[:n]

    chunks = [(r, stream(kind, items(n, r))) for r, n in enumerate(sizes)]
    want, got = T.wire(kind, chunks, 9, fmt, False, keep=True)
    assert [len(m) for m in want] == sizes
    if fmt == WIRE_BEAST and kind == "beast":
        assert len({len(b) for _, b, _ in got}) == len(sizes) and got[0][1].count(b"\x1a\x1a") > 100
    T.same_state(rng, 10)


# 3b. the scan past one round: the wire kernels scan a piece's records, entry after entry, 256 sums a round
# (block_sums_scan, msd_block_scan_impl.h), so past 65 536 records every record's start and every entry's range rest on
# what the scan carries between its rounds.  One call, one piece, of 65 793 = 256 B + B + 1 accepted DF17 frames and one
# record behind them.  An entry takes at most 1 MiB (MSD_GROUP_BEAST_ENTRY_MAX, MSD_GROUP_AVR_ENTRY_MAX), which is
# fewer than 65 793 DF17 frames in either input, so three entries of 21 931 share them: the seams between the entries
# lie inside workgroups, the seam between the rounds inside the third entry.  A few hundred frames built once, half of
# them rich in 0x1A, are tiled -- no parity per record in Python.
@pytest.mark.parametrize("kind,fmt", [("beast", WIRE_BEAST), ("avr", WIRE_AVR_MLAT)])
def test_the_scan_past_one_round(pkg, twin, kind, fmt):
    rng = random.Random(33)
    each, tile = (B * B + B + 1) // 3, 300
    sizes = [each, each, each, 1]
    assert sum(sizes[:3]) == 256 * B + B + 1 and (sum(sizes) + B - 1) // B == 258
    T = twin(len(sizes))

    def items(r):
        out = []
        for k in range(tile):  # runs of five frames rich in 0x1A, then five without
            dense = (k // 5) % 2 == 0
            me = bytes([0x1A] * rng.randrange(1, 8)).ljust(7, b"\x33") if dense else b"\x20\x2C\xC3\x71\xC3\x2C\xE0"
            body = pi(bytes([0x8D]) + (0x1A0000 + r).to_bytes(3, "big") + me)
            out.append((body, rng.choice([0x1A1A1A1A1A1A, 0x1A331A331A33, 0x001A00001A00]) if dense else 0x112233445566 + k,
                        0x1A if dense else 0x80))
        return out

    chunks = []
    for r, n in enumerate(sizes):
        some = items(r)
        chunks.append((r, stream(kind, some) * (n // tile) + stream(kind, some[:n % tile])))
    limit = pkg.capi.GROUP_BEAST_ENTRY_MAX if kind == "beast" else pkg.capi.GROUP_AVR_ENTRY_MAX
    assert 23 * (B * B + B + 1) > limit >= max(len(b) for _, b in chunks)  # (23: the shortest Beast frame of a DF17)
    want, got = T.wire(kind, chunks, 9, fmt, False, keep=True)
    assert [len(m) for m in want] == sizes and [nm for _, _, nm in got] == sizes
    assert all(len(b) > 23 * each for _, b, _ in got[:3]) and len(got[3][1]) >= 23
    T.same_state(rng, 10)


# 4. kept state across calls: a frame / line split between two calls of one receiver shows in the second call's entry
# only, and another receiver that uses the same entry slot in between gets none of its bytes
@pytest.mark.parametrize("kind", ["beast", "avr"])
def test_kept_state_across_calls(twin, kind):
    T = twin(2)
    F, G = stream(kind, [sq(0xABCDEF, ts=0x1111)]), stream(kind, [sq(0x123456, ts=0x2222)])
    out = lambda addr, ts: frame(ord("3"), sq(addr)[0], ts if kind == "beast" else 0, 0x80 if kind == "beast" else 0)  # a '*' line
    _, a = T.wire(kind, [(0, F[:12])], 1, WIRE_BEAST, False, keep=True)
    assert a == [(0, b"", 0)]
    _, b = T.wire(kind, [(1, G)], 2, WIRE_BEAST, False, keep=True)  # receiver 1 in entry slot 0
    assert b[0][2] == 1 and b[0][1] == out(0x123456, 0x2222)
    _, c = T.wire(kind, [(0, F[12:])], 3, WIRE_BEAST, False, keep=True)
    assert c[0][2] == 1 and c[0][1] == out(0xABCDEF, 0x1111)
    T.same_state(random.Random(4), 4)


# 5. verbatim is the received bytes: DF17 with one flipped bit at 5, 40 and 111, level 1
@pytest.mark.parametrize("kind", ["beast", "avr"])
def test_verbatim_is_the_received_bytes(twin, kind):
    good = sq(0x4840D6)[0]
    for verbatim in (False, True):
        T = twin(1)
        for k, bit in enumerate((5, 40, 111)):
            bad = flipped(good, [bit])
            want, got = T.wire(kind, [(0, stream(kind, [(bad, 0, 0x80)]))], 10 + k, WIRE_BEAST, verbatim)
            assert len(want[0]) == 1 and int(want[0][0]["correctedbits"]) == 1, bit
            assert got[0][1] == frame(ord("3"), bad if verbatim else good, 0, 0x80 if kind == "beast" else 0), bit


# 6. timestamps: '@' lines with and without MSD_AVR_KEEP_TIMESTAMP in one call go out as '@' and '*' lines under
# MSD_WIRE_AVR_MLAT; Beast to Beast keeps the 48-bit timestamp and the signal byte
def test_timestamps(twin):
    T = twin(2)
    p = sq(0x4840D6)[0]
    line = b"@0123456789AB" + p.hex().upper().encode() + b";\n"
    _, got = T.wire("avr", [(0, line), (1, line)], 1, WIRE_AVR_MLAT, False, keep=[True, False])
    assert got[0][1] == line and got[1][1] == b"*" + p.hex().upper().encode() + b";\n"
    frames = b"".join(frame(ord("3"), p, ts, sig) for ts, sig in ((0xFEDCBA987654, 1), (1, 255), (0x1A0000001A1A, 0x1A), (0, 0)))
    _, got = T.wire("beast", [(0, frames)], 2, WIRE_BEAST, False)
    assert got[0][1] == frames and got[0][2] == 4


# 7. Mode A/C: type '1' frames and four-digit lines go out as such for a receiver with the switch on, nothing with it off
def test_mode_ac(twin):
    T = twin(2, modeac=[1, 0])
    replies = [(bytes([0x77, k]), 0x100 + k, 0x40) for k in range(5)]
    _, got = T.wire("beast", [(0, beast_stream(replies)), (1, beast_stream(replies))], 1, WIRE_BEAST, False)
    assert got[0][1] == beast_stream(replies) and got[0][2] == 5 and got[1] == (1, b"", 0)
    _, got = T.wire("avr", [(0, avr_stream(replies)), (1, avr_stream(replies))], 2, WIRE_AVR, False)
    assert got[0][1] == b"".join(b"*77%02X;\n" % k for k in range(5)) and got[1] == (1, b"", 0)
    _, got = T.wire("avr", [(0, avr_stream(replies))], 3, WIRE_BEAST, False, keep=True)
    assert got[0][1].count(b"\x1a1") == 5 and got[0][2] == 5


# 8. two pieces: nine entries of 1 MiB, exact across the seam
@pytest.mark.parametrize("kind", ["beast", "avr"])
def test_two_pieces(twin, torch_cuda, kind):
    rng = random.Random(8)
    T = twin(9)
    chunks = []
    for r in range(9):
        head = stream(kind, corpus(rng, 40), rng)
        tail = stream(kind, corpus(rng, 40), rng)
        fill = bytes([0x41 + r]) * ((1 << 20) - len(head) - len(tail) - 1) + b"\n"
        chunks.append((r, head + fill + tail))
    assert all(len(b) == 1 << 20 for _, b in chunks)
    want, _ = T.wire(kind, chunks, 20, WIRE_BEAST, True, keep=True, device=torch_cuda)
    assert all(len(m) > 10 for m in want)
    T.same_state(rng, 21, decoys=4)


# 9. arguments: after every refusal a valid call matches the twin that never saw the bad call; n == 0
@pytest.mark.parametrize("kind", ["beast", "avr"])
def test_arguments(pkg, twin, kind):
    capi = pkg.capi
    T = twin(2)
    call = T.new.accept_beast_wire if kind == "beast" else T.new.accept_avr_wire
    F = [stream(kind, [sq(0xABC000 + k, ts=k)]) for k in range(8)]
    T.wire(kind, [(0, F[0][:10]), (1, F[0] + F[1][:7])], 1, WIRE_BEAST, False)  # kept state in both receivers
    kept = [F[0][10:], F[1][7:]]  # what completes each receiver's kept frame or line
    refusals = [dict(format=3), dict(format=-1), dict(verbatim=2), dict(verbatim=0x80000001), "twice", "empty"]
    for k, bad in enumerate(refusals):
        if bad == "empty":
            assert call([], 2) == []  # n == 0: returns 0, no sink call
        else:
            with pytest.raises(capi.MsdError) as e:
                if bad == "twice":
                    call([(0, kept[0]), (0, F[7])], 2)  # the same receiver twice
                else:
                    call([(0, kept[0]), (1, kept[1])], 2, **bad)
            assert f"{-errno.EINVAL}" in str(e.value), bad
        # the valid call: the kept halves complete, and each receiver is left with a new half
        nxt = [F[k + 1][:9 + k], F[k + 1][:5 + k]]
        _, got = T.wire(kind, [(0, kept[0] + nxt[0]), (1, kept[1] + nxt[1])], 3 + k, WIRE_BEAST, bool(k % 2))
        assert [nm for _, _, nm in got] == [1, 1], bad
        kept = [F[k + 1][9 + k:], F[k + 1][5 + k:]]
        T.same_counters()
    T.same_state(random.Random(9), 20)


# 10. one group alternates plain, fields and wire accept calls of both inputs and an IQ wire call on the same
# receivers; addresses learnt through a wire accept call make the IQ path's address/parity replies acceptable
@pytest.mark.parametrize("stage", ["gpu", "host_resolve"])
def test_mixing(pkg, twin, torch_cuda, stage):
    rng = random.Random(10)
    flags = pkg.capi.CFG_DECODE_FIELDS | (pkg.capi.CFG_HOST_RESOLVE if stage == "host_resolve" else 0)
    T = twin(2, flags=flags)
    known = rng.sample(range(1, 1 << 24), 20)
    others = rng.sample(range(1, 1 << 24), 20)
    T.wire("beast", [(0, beast_stream([sq(a) for a in known[:10]])), (1, beast_stream([sq(a) for a in others]))], 0,
           WIRE_BEAST, False)
    T.wire("avr", [(0, avr_stream([sq(a) for a in known[10:]]))], 1, WIRE_AVR, True)
    scene = uc8_scene([(1000 + 3000 * k, (4, 5)[k % 2], known[k % 20]) for k in range(40)])
    iq = torch_cuda.from_numpy(np.concatenate([scene, scene])).to("cuda:0")
    a, b = T.plain.submit_device_wire(iq, [0, 1]), T.new.submit_device_wire(iq, [0, 1])
    assert a == b and a[0][2] >= 35 and a[1][2] == 0  # receiver 0 knows the aircraft, its neighbour does not
    data = [corpus(rng, 120) for _ in range(2)]
    T.fields("beast", [(r, beast_stream(data[r], rng)) for r in range(2)], 2)
    for r in range(2):  # a plain call on both
        x = T.records(T.plain, "avr", [(r, avr_stream(data[r]))], 3)
        y = T.records(T.new, "avr", [(r, avr_stream(data[r]))], 3)
        assert x[0].tobytes() == y[0].tobytes()
    T.wire("avr", [(1, avr_stream(data[0], rng)), (0, avr_stream(data[1], rng))], 4, WIRE_AVR_MLAT, True, keep=True)
    T.fields("avr", [(0, avr_stream(data[0]))], 5, keep=True)
    a, b = T.plain.submit_device_wire(iq, [1, 0]), T.new.submit_device_wire(iq, [1, 0])
    assert a == b
    for r in range(2):
        assert T.plain.stats(r) == T.new.stats(r)
    T.same_state(rng, 6)
