"""msd_accept_beast / msd_accept_frames on the GPU against the checker of tests/remote_decode.py: the records and every
remote counter equal, and the ICAO filter equal afterwards (a probe call: one DF4 per address the checker has seen
added, plus decoys, must be decided alike)."""
import errno
import random

import numpy as np
import pytest

from remote_decode import Checker, assert_same_records, assert_same_stats, frame, hulc
from test_remote_decode_model import DF17, df4, df11, df20, with_parity
from test_wire_readers import flipped

pytestmark = pytest.mark.gpu


def df17(aa, me=b"\x20\x2C\xC3\x71\xC3\x2C\xE0"):
    return with_parity(bytes([0x8D]) + aa.to_bytes(3, "big") + me)


def remote(dem):
    st = dem.remote_stats()
    st.pop("tile_rewalks")
    return st


def both(dem, chk, data, now_ms, chunks=None):
    """Feed `data` to both, in the same chunks; compare the records of every call and the counters at the end."""
    sizes = chunks or [len(data)]
    pos = 0
    for k in sizes:
        part = data[pos:pos + k]
        pos += k
        assert_same_records(dem.accept_beast(part, now_ms), chk.beast(part, now_ms))
    assert pos >= len(data)
    assert_same_stats(remote(dem), chk.stats)


def probe(dem, chk, now_ms, rng, decoys=64):
    """One DF4 per known address and a few random ones: the two filters must answer alike."""
    addrs = sorted(chk.known) + [rng.randrange(1 << 24) for _ in range(decoys)]
    data = b"".join(frame(ord("2"), df4(a)) for a in addrs)
    assert_same_records(dem.accept_beast(data, now_ms), chk.beast(data, now_ms))
    assert_same_stats(remote(dem), chk.stats)


def random_chunks(rng, n, small=False):
    out, left = [], n
    while left > 0:
        k = rng.choice([1, 1, 2, 3, 5, 17, 44, 45]) if small else rng.choice([1, 2, 7, 100, 4095, 4096, 4097, 20000])
        out.append(min(k, left))
        left -= k
    return out


@pytest.fixture
def make(pkg, oracle, torch_cuda):
    made = []

    def f(nfix=1, mode_ac=0):
        dem = pkg.Demodulator(fmt=pkg.FMT_UC8, nfix_crc=nfix, mode_ac=mode_ac, message_capacity=1 << 20,
                              max_batch_samples=4 * pkg.CHUNK)
        made.append(dem)
        return dem, Checker(pkg, oracle, nfix, mode_ac)

    yield f
    for d in made:
        d.close()


def replay_stream(pkg, O, seed, nbuf=3):
    cfg = pkg.siggen.make_cfg(seed=seed)
    iq = pkg.siggen.generate(cfg, nbuf * pkg.CHUNK + 777)
    msgs, _ = O.Oracle(O.FMT_UC8, 58, 1, 0).replay(iq)
    return iq, msgs, b"".join(O.beast_frame(m) for m in msgs)


# (a) oracle replays written as Beast frames, read back whole and in random chunks, from host and device memory
@pytest.mark.parametrize("chunking", ["whole", "random", "tiny"])
def test_replayed_capture_round_trip(pkg, oracle, make, chunking, torch_cuda):
    _, msgs, data = replay_stream(pkg, oracle, 1090)
    assert len(msgs) > 100
    rng = random.Random(7)
    dem, chk = make()
    if chunking == "whole":
        dev = torch_cuda.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
        assert_same_records(dem.accept_beast(dev, 5), chk.beast(data, 5))
        assert_same_stats(remote(dem), chk.stats)
    else:
        head = data if chunking == "random" else data[:3000]
        both(dem, chk, head, 5, random_chunks(rng, len(head), small=chunking == "tiny"))
    assert chk.stats["remote_accepted"][0] > 0
    probe(dem, chk, 6, rng)


def corrupted_corpus(rng, n):
    """Flipped bits, rewritten DFs, type / DF mismatches, 0x1A-dense payloads and timestamps, garbage runs, '4' / '5' /
    'H' frames (some with len > 24)."""
    addrs = [rng.randrange(1 << 24) for _ in range(40)] + [0x1A1A1A, 0x001A00]
    out = bytearray()
    for _ in range(n):
        a = rng.choice(addrs)
        kind = rng.randrange(12)
        ts = rng.choice([rng.randrange(1 << 48), 0x1A1A1A1A1A1A, 0x1A331A331A33])
        sig = rng.choice([0x1A, 0, 255, rng.randrange(256)])
        if kind <= 2:
            body = df17(a)
        elif kind == 3:
            body = df11(a, rng.choice([0, 0, 3]))
        elif kind == 4:
            body = df4(a)
        elif kind == 5:
            body = df20(a)
        elif kind == 6:
            body = bytes([rng.randrange(256) for _ in range(14)])
        elif kind == 7:
            body = bytes([0x1A] * 14)
        else:
            body = df17(a)
        body = bytearray(body)
        if rng.random() < 0.4:
            body = bytearray(flipped(bytes(body), rng.sample(range(len(body) * 8), rng.randrange(1, 4))))
        if rng.random() < 0.1:
            body[0] = (rng.randrange(32) << 3) | (body[0] & 7)
        if rng.random() < 0.1:
            body[:7] = bytes(7)
        t = ord("3") if len(body) == 14 else ord("2")
        if rng.random() < 0.1:  # type / DF mismatch
            t = ord("2") if t == ord("3") else ord("3")
            body = body[:7] if t == ord("2") else body + bytes([0x1A] * 7)
        out += frame(t, body, ts, sig)
        r = rng.random()
        if r < 0.1:
            out += bytes(rng.randrange(256) for _ in range(rng.randrange(201)))
        elif r < 0.15:
            out += frame(rng.choice(b"45"), bytes(14), ts, sig)
        elif r < 0.2:
            out += hulc(rng.randrange(40), ident=rng.choice([1, 0x1A]), fill=rng.choice([0x1A, 0x33]))
        elif r < 0.22:
            out += b"\x1a" + bytes([rng.choice(b"1x\x00")])
    return bytes(out)


# (b) corrupted corpora under --no-fix, --fix and --aggressive
@pytest.mark.parametrize("nfix", [0, 1, 2])
@pytest.mark.parametrize("seed", [1, 2])
def test_corrupted_corpora(make, nfix, seed):
    rng = random.Random(100 * nfix + seed)
    dem, chk = make(nfix, mode_ac=seed % 2)
    data = corrupted_corpus(rng, 3000)
    both(dem, chk, data, 1000, random_chunks(rng, len(data)))
    assert chk.stats["remote_rejected_bad"] > 0 and chk.stats["other_frames"] > 0
    probe(dem, chk, 1001, rng)


# (c) tiles whose own chain starts inside a frame (escaped 0x1A, '3' pairs), so that the true chain must be re-walked
def test_out_of_phase_tiles_are_walked_again(make):
    rng = random.Random(3)
    dem, chk = make()
    one = frame(ord("3"), df17(0x1A331A), ts=0x1A331A331A33, signal=0x1A)
    data = b"".join(one + bytes([0x41] * rng.randrange(3)) for _ in range(4000))
    both(dem, chk, data, 0)
    assert dem.remote_stats()["tile_rewalks"] > 0
    assert chk.stats["remote_accepted"][0] == 4000


# (d) more than 4096 distinct adding addresses in one call: the active table fills up mid-call
def test_active_table_fills_mid_call(make):
    rng = random.Random(4)
    dem, chk = make()
    addrs = rng.sample(range(1, 1 << 24), 6000)
    data = b"".join(frame(ord("3"), df17(a)) + frame(ord("2"), df4(rng.choice(addrs))) for a in addrs)
    both(dem, chk, data, 0)
    assert chk.stats["remote_rejected_unknown_icao"] > 0  # replies of aircraft the full table could not take
    probe(dem, chk, 1, rng)


# (e) an expiry flip between calls
def test_expiry_flip_between_calls(make):
    rng = random.Random(5)
    dem, chk = make()
    a, b = 0x111111, 0x222222
    for now, add in ((0, a), (30000, None), (70000, b), (140000, None), (200000, None)):
        data = (frame(ord("3"), df17(add)) if add else b"") + frame(ord("2"), df4(a)) + frame(ord("2"), df4(b))
        both(dem, chk, data, now)
    probe(dem, chk, 200001, rng)


# (f) the filter is shared with the demodulator: aircraft of a demodulated capture make Beast replies acceptable
def test_shared_filter_with_the_demodulator(pkg, oracle, make, torch_cuda):
    iq, msgs, _ = replay_stream(pkg, oracle, 2024)
    dem, _ = make()
    orc = oracle.Oracle(oracle.FMT_UC8, 58, 1, 0)
    want, _ = orc.replay(iq)
    got = dem.submit_device(torch_cuda.from_numpy(iq).to("cuda:0").data_ptr(), iq.size // 2, last=True)
    assert len(got) == len(want)
    chk = Checker(pkg, oracle, 1, 0, oracle=orc)
    squitters = {int(m["addr"]) for m in want if m["msgtype"] == 17 and m["correctedbits"] == 0}
    assert squitters
    data = b"".join(frame(ord("2"), df4(a)) + frame(ord("3"), df20(a)) for a in sorted(squitters))
    got = dem.accept_beast(data, 10 ** 6)
    assert_same_records(got, chk.beast(data, 10 ** 6))
    assert len(got) == 2 * len(squitters)  # every reply accepted: its aircraft is in the shared filter
    assert_same_stats(remote(dem), chk.stats)


# (g) AVR lines through msd_avr_parse_line and msd_accept_frames decide like the Beast path
def test_avr_records_match_the_beast_path(pkg, make):
    rng = random.Random(6)
    dem, chk = make(1, mode_ac=1)
    host = chk.host
    bodies = [df17(a) for a in (0x1, 0xABCDEF)] + [df4(0xABCDEF), flipped(df17(0x1), [50]), df20(0x1), bytes(7),
                                                    DF17[:7], df4(0x777777) + bytes(7)]
    recs = []
    for b in bodies * 20:
        rec = np.zeros(1, dtype=pkg.capi.MESSAGE_DTYPE)
        assert host.msd_avr_parse_line(b"*" + b.hex().upper().encode() + b";", 1, 0, rec.ctypes.data) == 1
        recs.append(rec[0])
    recs = np.array(recs, dtype=pkg.capi.MESSAGE_DTYPE)
    avr = dem.accept_frames(recs, 9)
    assert_same_records(avr, chk.frames(recs, 9))
    assert_same_stats(remote(dem), chk.stats)
    # the same bytes as Beast frames, on a fresh context: the same decisions
    dem2, chk2 = make(1, mode_ac=1)
    data = b"".join(frame(ord("3") if len(b) == 14 else ord("2"), b) for b in bodies * 20)
    beast = dem2.accept_beast(data, 9)
    assert_same_records(beast, chk2.beast(data, 9))
    assert len(beast) > 0
    for f in ("addr", "crc", "msgtype", "msgbits", "correctedbits", "msg"):
        assert np.array_equal(avr[f], beast[f]), f
    probe(dem, chk, 10, rng)


# (i) -EBUSY while a batch is outstanding
def test_busy_while_a_batch_is_outstanding(pkg, make, torch_cuda):
    dem, _ = make()
    iq = np.full(2 * pkg.CHUNK * 2, 127, dtype=np.uint8)
    d = torch_cuda.from_numpy(iq).to("cuda:0")
    dem.launch_device(d.data_ptr(), 2 * pkg.CHUNK, last=True)
    with pytest.raises(pkg.MsdError) as e:
        dem.accept_beast(frame(ord("3"), DF17), 0)
    assert f"{-errno.EBUSY}" in str(e.value)
    dem.collect()
    assert len(dem.accept_beast(frame(ord("3"), DF17), 0)) == 1


# (f), the other way round: Beast DF17 squitters make a later capture's DF4 / DF5 replies acceptable on the GPU resolve
# path, as they do in an oracle whose filter was given the same adds (through the checker's own orc_filter_add calls)
def test_beast_adds_reach_the_gpu_resolve_path(pkg, oracle, torch_cuda):
    import mag_scenes as ms
    C = pkg.CHUNK
    rng = random.Random(8)
    known = rng.sample(range(1, 1 << 24), 40)
    strangers = rng.sample(range(1, 1 << 24), 20)
    orc = oracle.Oracle(oracle.FMT_MAG16, 58, 1, 0)
    chk = Checker(pkg, oracle, 1, 0, oracle=orc)
    dem = pkg.Demodulator(fmt=pkg.FMT_MAG16, nfix_crc=1, max_batch_samples=4 * C, message_capacity=1 << 16)
    try:
        data = b"".join(frame(ord("3"), df17(a)) for a in known)
        assert_same_records(dem.accept_beast(data, 0), chk.beast(data, 0))
        assert all(orc.filter_test(a) for a in known)
        # a capture of replies only: no squitter in it adds anything, so every acceptance comes from the Beast adds
        sc = ms.Scene(8 * C - 5, seed=8)  # two batches of four buffers, both resolved on the GPU
        sample = 1000
        for k in range(400):
            a = known[k % len(known)] if k % 3 else strangers[k % len(strangers)]
            sc.frame(sample, df=4 if k % 2 else 5, addr=a, accept=a in known)
            sample += 2500
        want, wstats = orc.replay(sc.mag, cap=1 << 16)
        d = torch_cuda.from_numpy(sc.mag.view(np.uint8).copy()).to("cuda:0")
        got = pkg.replay_device(dem, d.data_ptr(), sc.n, 4 * C)
        assert dem.timing()["resolve_passes"] > 0  # the batches went through the GPU resolve kernel
        assert len(want) > 200 and {int(m["msgtype"]) for m in want} == {4, 5}
        assert set(int(m["addr"]) for m in want) == set(known)
        for f in ("timestampMsg", "sysTimestampMsg", "signalLevel", "addr", "msgtype", "correctedbits", "score", "crc",
                  "bestphase"):
            assert np.array_equal(got[f], want[f]), f
        assert np.array_equal(got["msg"], want["msg"])
        gstats = dem.stats()
        for k in ("demod_preambles", "demod_rejected_bad", "demod_rejected_unknown_icao", "demod_accepted"):
            assert gstats[k] == wstats[k], k
        assert wstats["demod_rejected_unknown_icao"] > 0  # the strangers' replies
    finally:
        dem.close()


# one call longer than a piece (MSD_FR_PIECE, 8 MiB): the kept frame, the pending gap and the filter carried inside the
# call, against the checker
def test_a_call_longer_than_one_piece(make):
    rng = random.Random(9)
    dem, chk = make(1)
    block = corrupted_corpus(rng, 4000)
    data = block * ((9 << 20) // len(block) + 1)
    assert len(data) > (9 << 20)
    both(dem, chk, data, 77)
    probe(dem, chk, 78, rng)
