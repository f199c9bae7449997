"""msd_wire_encode: constructed message records as Beast frames and AVR lines written on the GPU, byte for byte against
libmsd_host.so's msd_beast_frame_out / msd_avr_line_out called per record, and `ends` against the running sum of their
lengths.  Every record count in NS -- so that frames straddle every wavefront and workgroup run -- in all three
formats, with and without verbatim, from host and from device memory.  And, tiled from the same records, 65 536 to
131 329 of them: past 256 workgroups the scan over their sums runs in rounds and every offset rests on its carry."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
COMBOS = [(f, v) for f in (0, 1, 2) for v in (False, True)]  # WIRE_BEAST, WIRE_AVR, WIRE_AVR_MLAT
ESC_LEVEL = (26 / 255.0) ** 2  # signal byte 0x1A
DF17 = "8D4840D6202CC371C32CE0576098"


def record(pkg, payload, ts=0, level=0.0, msgtype=None, msgbits=None, crc=0, correctedbits=0, iid=0):
    rec = np.zeros(1, dtype=pkg.capi.MESSAGE_DTYPE)
    raw = bytes(payload)
    rec["msg"][0, : len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    rec["msgbits"] = 8 * len(raw) if msgbits is None else msgbits
    rec["timestampMsg"] = ts
    rec["signalLevel"] = level
    rec["msgtype"] = (32 if len(raw) == 2 else raw[0] >> 3) if msgtype is None else msgtype
    rec["crc"] = crc
    rec["correctedbits"] = correctedbits
    rec["iid"] = iid
    return rec[0]


def repaired_records(pkg, oracle):
    """Valid messages with one bit flipped (DF 17 and DF 11 with a non-zero interrogator id) and with two (DF 17), as the
    decoder delivers them after the repair: the repaired bytes, the syndrome of the received ones, the number of repaired
    bits.  Only patterns the oracle's modesChecksumDiagnose repairs, and to exactly the flipped bits.  Returns (records,
    the received bytes of each)."""
    rng = np.random.default_rng(1090)
    orc = oracle.Oracle(oracle.FMT_UC8, 58, 2, 0)
    one, two, df11, received = [], [], [], []

    def valid(df_byte, nbytes, iid=0):
        body = bytearray([df_byte]) + bytearray(rng.integers(0, 256, nbytes - 4, dtype=np.uint8).tobytes()) + bytearray(3)
        rem = oracle.checksum(bytes(body))
        body[-3:] = (rem ^ iid).to_bytes(3, "big")
        assert oracle.checksum(bytes(body)) == iid
        return body

    def flipped(msg, bits):
        out = bytearray(msg)
        for b in bits:
            out[b >> 3] ^= 0x80 >> (b & 7)
        return out

    while len(one) < 60:
        msg = valid(0x8D, 14)
        bit = int(rng.integers(5, 112))
        bad = flipped(msg, [bit])
        syn = oracle.checksum(bytes(bad))
        if orc.diagnose(syn, 112) == (1, [bit, -1]):
            one.append(record(pkg, msg, ts=int(rng.integers(1, 1 << 48)), level=float(rng.random()), crc=syn, correctedbits=1))
            received.append(bytes(bad))
    while len(two) < 60:
        msg = valid(0x8D, 14)
        b0, b1 = sorted(int(b) for b in rng.choice(np.arange(5, 112), 2, replace=False))
        bad = flipped(msg, [b0, b1])
        syn = oracle.checksum(bytes(bad))
        if orc.diagnose(syn, 112) == (2, [b0, b1]):
            two.append(record(pkg, msg, ts=int(rng.integers(1, 1 << 48)), level=float(rng.random()), crc=syn, correctedbits=2))
            received.append(bytes(bad))
    for bit in range(5, 56):
        iid = int(rng.integers(1, 128))
        msg = valid(0x5D, 7, iid)
        bad = flipped(msg, [bit])
        syn = oracle.checksum(bytes(bad))
        if orc.diagnose(syn & 0xFFFF80, 56) == (1, [bit, -1]):  # mode_s.c:476-480: the interrogator id masked out
            df11.append(record(pkg, msg, ts=int(rng.integers(1, 1 << 48)), level=float(rng.random()), crc=syn,
                               correctedbits=1, iid=syn & 0x7F))
            received.append(bytes(bad))
    assert len(one) >= 50 and len(two) >= 50 and len(df11) >= 1, (len(one), len(two), len(df11))
    assert any(r["iid"] != 0 for r in df11)
    return one + two + df11, received


def constructed(pkg, oracle):
    R = lambda *a, **k: record(pkg, *a, **k)
    df17, short = bytes.fromhex(DF17), bytes.fromhex("5D4840D6A1B2C3")
    recs = [R(df17, ts=0x0123456789AB, level=0.25),                       # the known answers of test_wire_formats.py
            R(bytes.fromhex("1A4840D61A2CC3"), ts=0x001A00001A00, level=ESC_LEVEL),
            R(bytes.fromhex("7700"), ts=5),
            R(short, ts=0), R(short, ts=1, level=1e-9), R(short, ts=1, level=1.5)]
    for k in range(6):                                                     # 0x1A at every timestamp byte
        recs.append(R(df17, ts=0x1A << (8 * k), level=0.5))
    recs.append(R(df17, ts=77, level=ESC_LEVEL))                           # in the signal byte
    for base in (short, df17):                                             # at every payload byte position
        for k in range(len(base)):
            p = bytearray(base)
            p[k] = 0x1A
            recs.append(R(p, ts=1000 + k, level=0.01, msgtype=base[0] >> 3))
    recs.append(R(b"\x1a" * 14, ts=0x1A1A1A1A1A1A, level=ESC_LEVEL))       # the 44-byte worst case
    recs.append(R(b"\x1a" * 7, ts=0x1A1A1A1A1A1A, level=ESC_LEVEL))
    for code in (0x7700, 0x1A1A, 0x0000, 0x0630, 0x7577):                  # Mode A/C
        recs.append(R(code.to_bytes(2, "big"), ts=0x1A0000 + code))
    recs.append(R(b"\x1a\x1a", ts=0x1A1A1A1A1A1A))
    recs.append(R(b"\x8d\x48\x40", ts=9, level=0.5, msgbits=24, msgtype=17))  # no Beast frame of three bytes
    recs.append(R(df17, ts=0, level=0.3))                                  # no timestamp: '*' in the mlat format too
    recs.append(R(df17, ts=(0xABCD << 48) | 0x0123456789AB, level=0.3))    # only the low 48 bits go out
    recs.append(R(df17, ts=1 << 48, level=0.3))
    levels = [0.0, 5e-324, 1e-9, 1.0, 1.5]                                 # the signal byte at its rounding boundaries
    for k in range(256):
        x = ((k + 0.5) / 255.0) ** 2
        lo1 = np.nextafter(x, 0.0)
        hi1 = np.nextafter(x, 2.0)
        levels += [float(np.nextafter(lo1, 0.0)), float(lo1), x, float(hi1), float(np.nextafter(hi1, 2.0))]
    for i, lv in enumerate(levels):
        recs.append(R(short, ts=5000 + i, level=lv))
    rep, received = repaired_records(pkg, oracle)
    return np.array(recs + rep, dtype=pkg.capi.MESSAGE_DTYPE), len(recs), received


@pytest.fixture(scope="module")
def host(pkg):
    L = C.CDLL(os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "libmsd_host.so"))
    L.msd_beast_frame_out.restype = C.c_size_t
    L.msd_beast_frame_out.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.msd_avr_line_out.restype = C.c_size_t
    L.msd_avr_line_out.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def pool(pkg, oracle, host):
    """The records, shuffled once, and per (format, verbatim) what the host writers make of each: computed once, shared
    by every test."""
    recs, first_repaired, received = constructed(pkg, oracle)
    want = {}
    buf = (C.c_uint8 * 64)()
    for fmt, verbatim in COMBOS:
        out = []
        for i in range(len(recs)):
            p = recs[i:i + 1].ctypes.data
            n = host.msd_beast_frame_out(p, int(verbatim), buf) if fmt == 0 else \
                host.msd_avr_line_out(p, int(fmt == 2), int(verbatim), buf)
            out.append(bytes(buf[:n]))
        want[(fmt, verbatim)] = out
    # the reference itself: a verbatim line carries the received bytes, a plain one the repaired ones
    for k, raw in enumerate(received):
        i = first_repaired + k
        assert want[(1, True)][i] == b"*" + raw.hex().upper().encode() + b";\n"
        plain = b"*" + bytes(recs[i]["msg"][: len(raw)]).hex().upper().encode() + b";\n"
        assert want[(1, False)][i] == (b"" if recs[i]["correctedbits"] == 2 else plain)
    assert max(len(b) for b in want[(0, False)]) == 44
    perm = np.random.default_rng(7).permutation(len(recs))
    return recs[perm], {k: [v[i] for i in perm] for k, v in want.items()}


def slices(pool_size):
    """(first, n) for every n of NS -- each slice starts where the one before ended, so that together they cover the pool
    -- and the whole pool once."""
    out, first = [], 0
    for n in NS:
        if first + n > pool_size:
            first = 0
        out.append((first, n))
        first += n
    return out + [(0, pool_size)]


@pytest.mark.parametrize("fmt,verbatim", COMBOS)
def test_bytes_and_ends(pkg, torch_cuda, pool, fmt, verbatim):
    recs, want = pool
    dem = pkg.capi.Demodulator(fmt=pkg.capi.FMT_UC8, nfix_crc=2)
    assert len(recs) > 1000 + 257
    for first, n in slices(len(recs)):
        part = np.ascontiguousarray(recs[first:first + n])
        exp = want[(fmt, verbatim)][first:first + n]
        exp_ends = np.cumsum([len(b) for b in exp], dtype=np.uint64)
        dev = torch_cuda.from_numpy(part.view(np.uint8).reshape(-1).copy()).cuda() if n else torch_cuda.zeros(0, dtype=torch_cuda.uint8, device="cuda")
        for on_device in (False, True):
            got, ends = dem.encode_wire(dev if on_device else part, fmt, verbatim=verbatim, on_device=on_device)
            what = (fmt, verbatim, first, n, on_device)
            assert len(ends) == n, what
            assert np.array_equal(ends.astype(np.uint64), exp_ends), (what, "ends")
            if got != b"".join(exp):  # name the first record that differs
                prev = 0
                for i, b in enumerate(exp):
                    assert got[prev:prev + len(b)] == b, (what, i, part[i], got[prev:prev + len(b)].hex(), b.hex())
                    prev += len(b)
            assert got == b"".join(exp), what


BIG_NS = (1 << 16, (1 << 16) + 1, 256 * 256 + 257, 2 * 256 * 256 + 257)  # 256, 257, 257 + a seam, 513 workgroups + a seam


def tiled(pool, key, start, n):
    """Records pool[(start + arange(n)) % len(pool)], the stream the host writers make of them and its ends -- put
    together from the pool's per-record answers by index, no call per record."""
    recs, want = pool
    lens = np.array([len(b) for b in want[key]], dtype=np.int64)
    blob = np.frombuffer(b"".join(want[key]), dtype=np.uint8)
    begins = np.cumsum(lens) - lens
    idx = (start + np.arange(n)) % len(recs)
    ends = np.cumsum(lens[idx])
    src = np.repeat(begins[idx] - (ends - lens[idx]), lens[idx]) + np.arange(ends[-1])
    return np.ascontiguousarray(recs[idx]), blob[src], ends.astype(np.uint64), idx


@pytest.mark.parametrize("fmt,verbatim", [(0, False), (2, True)])  # Beast plain, AVR-MLAT verbatim
def test_bytes_and_ends_past_one_round_of_the_scan(pkg, torch_cuda, pool, fmt, verbatim):
    """More than 256 workgroups of records: block_sums_scan (msd_block_scan_impl.h) then walks the workgroups' sums in
    rounds of 256 and every offset, every end and the stream's length rest on what it carries from round to round --
    one, two (by one record; by a workgroup and a record) and three rounds."""
    dem = pkg.capi.Demodulator(fmt=pkg.capi.FMT_UC8, nfix_crc=2)
    assert [(n + 255) // 256 for n in BIG_NS] == [256, 257, 258, 514]
    for k, n in enumerate(BIG_NS):
        part, exp, exp_ends, idx = tiled(pool, (fmt, verbatim), 101 * k + 3, n)
        assert len(exp) == int(exp_ends[-1]) > 15 * n  # (a short Beast frame is 16 bytes; a few records have none)
        dev = torch_cuda.from_numpy(part.view(np.uint8).reshape(-1)).cuda()
        for on_device in (False, True):
            got, ends = dem.encode_wire(dev if on_device else part, fmt, verbatim=verbatim, on_device=on_device)
            what = (fmt, verbatim, n, on_device)
            got = np.frombuffer(got, dtype=np.uint8)
            assert len(ends) == n, what
            wrong = np.flatnonzero(ends.astype(np.uint64) != exp_ends)
            assert wrong.size == 0, (what, "ends: first at record", int(wrong[0]), int(ends[wrong[0]]), int(exp_ends[wrong[0]]))
            m = min(len(got), len(exp))
            wrong = np.flatnonzero(got[:m] != exp[:m])
            if wrong.size:  # name the first record that differs
                i = int(np.searchsorted(exp_ends, wrong[0], side="right"))
                lo, hi = int(exp_ends[i - 1]) if i else 0, int(exp_ends[i])
                assert False, (what, "record", i, "pool", int(idx[i]), got[lo:hi].tobytes().hex(), exp[lo:hi].tobytes().hex())
            assert len(got) == len(exp), (what, len(got), len(exp))


def test_one_byte_short_past_one_round_of_the_scan(pkg, torch_cuda, pool):
    """-ENOSPC with the stream's length -- block_sums[nblocks], after two rounds -- and nothing written."""
    capi = pkg.capi
    n = BIG_NS[2]
    part, exp, exp_ends, _ = tiled(pool, (0, False), 57, n)
    dem = capi.Demodulator(fmt=capi.FMT_UC8, nfix_crc=2)
    L = capi.lib()
    used = C.c_size_t(12345)
    out = np.full(len(exp) + 8, 0xAA, dtype=np.uint8)
    ends = np.full(n, 0xAAAAAAAA, dtype=np.uint32)
    call = lambda cap: L.msd_wire_encode(dem._h, part.ctypes.data, n, 0, 0, 0, out.ctypes.data, cap, C.byref(used),
                                         ends.ctypes.data)
    assert call(len(exp) - 1) == -28
    assert used.value == len(exp) == int(exp_ends[-1])
    assert (out == 0xAA).all() and (ends == 0xAAAAAAAA).all()
    assert call(len(exp)) == 0 and used.value == len(exp)
    assert np.array_equal(out[: len(exp)], exp) and (out[len(exp):] == 0xAA).all()
    assert np.array_equal(ends.astype(np.uint64), exp_ends)


def test_errors(pkg, torch_cuda, pool):
    capi = pkg.capi
    recs, want = pool
    part = np.ascontiguousarray(recs[:300])
    exp = b"".join(want[(0, False)][:300])
    dem = capi.Demodulator(fmt=capi.FMT_UC8, max_batch_samples=capi.CHUNK)
    L = capi.lib()
    used = C.c_size_t(12345)
    out = np.full(len(exp) + 8, 0xAA, dtype=np.uint8)
    ends = np.full(300, 0xAAAAAAAA, dtype=np.uint32)
    call = lambda fmt, flags, cap: L.msd_wire_encode(dem._h, part.ctypes.data, 300, 0, fmt, flags, out.ctypes.data, cap,
                                                     C.byref(used), ends.ctypes.data)
    assert call(0, 0, len(exp) - 1) == -28  # -ENOSPC: the size needed, nothing else written
    assert used.value == len(exp)
    assert (out == 0xAA).all() and (ends == 0xAAAAAAAA).all()
    assert call(0, 0, used.value) == 0 and used.value == len(exp)
    assert out[: len(exp)].tobytes() == exp and (out[len(exp):] == 0xAA).all()
    assert ends[-1] == len(exp)
    for fmt, flags in ((3, 0), (-1, 0), (0, 2), (1, 0x80000000)):
        assert call(fmt, flags, out.size) == -22, (fmt, flags)
    assert L.msd_wire_encode(dem._h, part.ctypes.data, 300, 0, 0, 0, out.ctypes.data, out.size, None, None) == -22
    assert L.msd_wire_encode(None, part.ctypes.data, 300, 0, 0, 0, out.ctypes.data, out.size, C.byref(used), None) == -22
    used.value = 777
    assert L.msd_wire_encode(dem._h, None, 0, 0, 0, 0, None, 0, C.byref(used), None) == 0 and used.value == 0
    # a batch in flight: -EBUSY, and the batch is collected as if nobody had asked
    iq = torch_cuda.from_numpy(pkg.siggen.generate(pkg.siggen.make_cfg(seed=3), capi.CHUNK)).cuda()
    dem.launch_device(iq.data_ptr(), capi.CHUNK, last=True)
    assert call(0, 0, out.size) == -16
    with pytest.raises(capi.MsdError, match="-16"):
        dem.encode_wire(part, capi.WIRE_BEAST)
    msgs = dem.collect()
    got, _ = dem.encode_wire(msgs, capi.WIRE_AVR)
    assert got.count(b"\n") == len(msgs) > 0
    assert call(0, 0, out.size) == 0 and out[: len(exp)].tobytes() == exp
