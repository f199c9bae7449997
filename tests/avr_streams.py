"""AVR raw text streams (msd_avr_reader_feed, msd_accept_avr): the rules of include/modes_hip.h restated in a few lines
of Python (`Model`), libmsd_host.so's reader bound through ctypes (`Reader`), and the streams both test files feed."""
import ctypes as C
import os
import random

import numpy as np

LINE_MAX = 256
WS = b" \t\n\v\f\r"
HEXD = b"0123456789abcdefABCDEF"
SKIP = {ord("<"): 15, ord("@"): 13, ord("%"): 13, ord("*"): 1, ord(":"): 1}


def hv(c):
    return int(chr(c), 16) if c in HEXD else -1


def parse_line(text, mode_ac, keep):
    """(payload bytes, timestampMsg, signalLevel) of one line without its newline, or None: msd_avr_parse_line."""
    z = text.find(b"\0")
    if z >= 0:
        text = text[:z]
    text = text.strip(WS)
    if not text or text[-1] != ord(";") or text[0] not in SKIP:
        return None
    skip = SKIP[text[0]]
    if len(text) < skip + 1:
        return None
    ts, level = 0, 0.0
    if skip > 1:
        if all(c in HEXD for c in text[1:13]):
            ts = int(text[1:13], 16)
        if skip == 15:
            level = ((hv(text[13]) << 4) | hv(text[14])) / 255.0
            level *= level
    pay = text[skip:-1]
    if len(pay) not in (4, 14, 28) or (len(pay) == 4 and not mode_ac) or not all(c in HEXD for c in pay):
        return None
    return bytes.fromhex(pay.decode()), (ts if keep else 0), level


class Model:
    """The stream rule: cut at every newline, keep the incomplete line, drop lines of more than LINE_MAX bytes."""

    def __init__(self, mode_ac, keep):
        self.mode_ac, self.keep = mode_ac, keep
        self.kept, self.discard = b"", False
        self.stats = dict(lines=0, frames=0, dropped_lines=0, long_lines=0)

    def feed(self, data):
        out = []
        parts = (self.kept + bytes(data)).split(b"\n")
        for k, line in enumerate(parts[:-1]):
            self.stats["lines"] += 1
            if (k == 0 and self.discard) or len(line) > LINE_MAX:
                self.stats["long_lines"] += 1
            else:
                rec = parse_line(line, self.mode_ac, self.keep)
                if rec is None:
                    self.stats["dropped_lines"] += 1
                else:
                    self.stats["frames"] += 1
                    out.append(rec)
        if len(parts) > 1:
            self.discard = False
        if self.discard or len(parts[-1]) > LINE_MAX:
            self.kept, self.discard = b"", True
        else:
            self.kept = parts[-1]
        return out


class ReaderState(C.Structure):
    _fields_ = [("buf", C.c_uint8 * (LINE_MAX + 1)), ("len", C.c_size_t), ("discard", C.c_int), ("mode_ac", C.c_int),
                ("keep_timestamp", C.c_int), ("lines", C.c_uint64), ("frames", C.c_uint64),
                ("dropped_lines", C.c_uint64), ("long_lines", C.c_uint64)]


class Reader:
    """msd_avr_reader of libmsd_host.so; feed() returns the records of the call as a MESSAGE_DTYPE array (collected
    by the library's own msd_array_sink, no Python callback per record)."""

    def __init__(self, pkg, mode_ac, keep):
        self.pkg = pkg
        self.host = C.CDLL(os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "libmsd_host.so"))
        self.host.msd_avr_reader_init.restype = None
        self.host.msd_avr_reader_init.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self.host.msd_avr_reader_feed.restype = C.c_size_t
        self.host.msd_avr_reader_feed.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p]
        self.sink = C.cast(C.CDLL(pkg.capi.LIB_PATH).msd_array_sink, C.c_void_p)
        self.st = ReaderState()
        self.host.msd_avr_reader_init(C.byref(self.st), int(mode_ac), int(keep))

    def feed(self, data):
        data = bytes(data)
        dt = self.pkg.capi.MESSAGE_DTYPE
        out = np.zeros(len(data) // 7 + 2, dtype=dt)  # a line that yields a record takes at least 7 bytes
        state = self.pkg.capi._SinkState(out.ctypes.data, out.size, 0)
        n = self.host.msd_avr_reader_feed(C.byref(self.st), data, len(data), self.sink, C.byref(state))
        assert n == state.count <= out.size
        return out[:n].copy()

    @property
    def stats(self):
        return {k: int(getattr(self.st, k)) for k in ("lines", "frames", "dropped_lines", "long_lines")}


def chunked(data, size):
    return [data[i:i + size] for i in range(0, len(data), size)] or [b""]


def random_cuts(rng, data, sizes=(1, 2, 7, 31, 100, 255, 256, 257, 300, 4095, 4097, 20000)):
    out, pos = [], 0
    while pos < len(data):
        k = rng.choice(sizes)
        out.append(data[pos:pos + k])
        pos += k
    return out or [b""]


# ---- payloads ------------------------------------------------------------------------------------------------------
def crc24(b):
    rem = 0
    for x in b:
        rem ^= x << 16
        for _ in range(8):
            rem = ((rem << 1) ^ 0xFFF409) & 0xFFFFFF if rem & 0x800000 else (rem << 1) & 0xFFFFFF
    return rem


def df17(aa, me=b"\x20\x2C\xC3\x71\xC3\x2C\xE0"):
    body = bytes([0x8D]) + aa.to_bytes(3, "big") + me
    return body + crc24(body).to_bytes(3, "big")


def df4(addr):
    body = bytes([0x20, 0x00, 0x05, 0x30])
    return body + (crc24(body) ^ addr).to_bytes(3, "big")


def star(payload):
    return b"*" + payload.hex().upper().encode() + b";\n"


def padded(payload, total, rng=None):
    """A '*' line of exactly `total` bytes in front of its newline: white space around the message."""
    core = b"*" + payload.hex().encode() + b";"
    pad = total - len(core)
    assert pad >= 0
    left = pad // 2 if rng is None else rng.randrange(pad + 1)
    fill = b" \t\r\v\f"
    mk = (lambda n: b" " * n) if rng is None else (lambda n: bytes(rng.choice(fill) for _ in range(n)))
    return mk(left) + core + mk(pad - left) + b"\n"


def edge_streams():
    """name -> (stream, mode_ac): the cases the issue lists, each followed by a valid line so that a wrong state shows."""
    a, b, c = df17(0x4840D6), df17(0xABCDEF), df4(0x4840D6)
    ok = star(a)
    ts = b"0123456789AB"
    s = {}
    s["five prefixes"] = (star(a) + b":" + b.hex().encode() + b";\n" + b"@" + ts + a.hex().encode() + b";\n" +
                          b"%" + ts + c.hex().encode() + b";\n" + b"<" + ts + b"80" + b.hex().encode() + b";\n" +
                          b"<" + ts + b"zz" + a.hex().encode() + b";\n" + b"<" + ts + b"7g" + a.hex().encode() + b";\n" +
                          b"@0123456789xB" + a.hex().encode() + b";\n" + b"@" + ts + b";\n" + b"<" + ts + b";\n" + b"@;\n" +
                          b"<" + ts + b"8" + a.hex().encode() + b";\n", 0)
    s["white space"] = (b" " + star(a)[:-1] + b"\r\n" + b"\t\v\f\r " + star(b)[:-1] + b" \t\r\n" + b"*" + c.hex().encode() +
                        b" ;\n" + b"* " + c.hex().encode() + b";\n" + b"x" + star(a) + star(a)[:-1] + b"x\n" + ok, 0)
    s["empty lines"] = (b"\n\n" + ok + b"\n \n\r\n\t \r\n" + ok + b"\n", 0)
    s["nul"] = (b"*" + a.hex().encode()[:10] + b"\0" + a.hex().encode()[10:] + b";\n" + star(a)[:-1] + b"\0garbage\n" +
                b"\0" + star(a) + star(a)[:-1] + b" \0;\n" + b"  \0\n" + ok, 0)
    s["256 and 257"] = (padded(a, 256) + padded(b, 257) + ok + b" " * 256 + b"\n" + b" " * 257 + b"\n" +
                        b"x" * 256 + b"\n" + padded(c, 255) + ok, 0)
    s["long run"] = (b"y" * 10000 + b"\n" + ok + b"*" + a.hex().encode() * 400 + b";\n" + ok, 0)
    s["long run of lines inside"] = (b" " * 300 + star(a) + ok + b"\0" * 600 + b"\n" + ok, 0)
    s["mode a/c on"] = (b"*7700;\n" + b"@" + ts + b"1234;\n" + b"*77;\n" + b"*770000;\n" + ok, 1)
    s["mode a/c off"] = (b"*7700;\n" + b"@" + ts + b"1234;\n" + ok, 0)
    s["wrong lengths"] = (b"*" + a.hex().encode()[:-2] + b";\n" + b"*" + a.hex().encode() + b"00;\n" + b"*;\n" + b";\n" +
                          b"*" + a.hex().encode()[:-1] + b"g;\n" + b"#" + a.hex().encode() + b";\n" + star(a)[:-2] + b"\n" +
                          b"*" + a[:7].hex().encode() + b";\n" + ok, 0)
    s["newline first and last"] = (b"\n" + ok + star(b), 0)
    s["no newline at the end"] = (ok + star(b)[:-1], 0)
    return s


def corrupt(rng, data, rate=0.02):
    """Single-character substitutions in the text."""
    out = bytearray(data)
    alphabet = b"0123456789ABCDEFabcdef*:@%<;\n\r \t\0xg"
    for _ in range(max(1, int(len(out) * rate))):
        out[rng.randrange(len(out))] = rng.choice(alphabet)
    return bytes(out)


def mixed_prefix_stream(rng, n, addrs):
    out = bytearray()
    for _ in range(n):
        a = rng.choice(addrs)
        p = rng.choice([df17(a), df4(a), df17(a)[:7], bytes([0x77, rng.randrange(256)])])
        ts = b"%012X" % rng.randrange(1 << 48)
        kind = rng.randrange(5)
        h = p.hex().encode() if rng.random() < 0.5 else p.hex().upper().encode()
        out += [b"*" + h, b":" + h, b"@" + ts + h, b"%" + ts + h, b"<" + ts + b"%02x" % rng.randrange(256) + h][kind]
        out += rng.choice([b";\n", b";\r\n", b"; \n"])
    return bytes(out)
