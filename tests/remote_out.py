"""What the tests of msd_group_accept_*_fields and msd_group_accept_*_wire share: payload corpora that go out as a Beast
stream or as AVR text, the host writers of libmsd_host.so, and a pair of groups of one configuration fed the same
bytes -- one through the plain accept call, whose records say what the other's fields or wire call must deliver."""
import ctypes as C
import os

import numpy as np

from avr_streams import crc24
from remote_decode import frame
from test_wire_readers import flipped

WIRE_BEAST, WIRE_AVR, WIRE_AVR_MLAT = 0, 1, 2


def pi(body):
    """parity/interrogator formats (DF11/17/18): the CRC itself"""
    return body + crc24(body).to_bytes(3, "big")


def ap(body, addr):
    """address/parity formats (DF0/4/5/16/20/21)"""
    return body + (crc24(body) ^ addr).to_bytes(3, "big")


def es(rng, addr, metype, df=17):
    me = bytearray(rng.randrange(256) for _ in range(7))
    me[0] = (metype << 3) | (me[0] & 7)
    return pi(bytes([(df << 3) | rng.randrange(8)]) + addr.to_bytes(3, "big") + bytes(me))


def every_format(rng, addr):
    """One aircraft's squitter, then every format the field decoder knows: DF0/4/5/11/16, DF17 ME types 1-4, 5-8, 9-18,
    19, 28, 29, 31, DF18, DF20/21 with random Comm-B payloads.  The address/parity replies follow the squitter."""
    r8 = lambda n: bytes(rng.randrange(256) for _ in range(n))
    out = [es(rng, addr, rng.randrange(1, 5))]
    out += [ap(bytes([(df << 3) | rng.randrange(8)]) + r8(3), addr) for df in (0, 4, 5)]
    out.append(pi(bytes([(11 << 3) | rng.randrange(8)]) + addr.to_bytes(3, "big")))
    out.append(ap(bytes([(16 << 3) | rng.randrange(8)]) + r8(10), addr))
    out += [es(rng, addr, t) for t in (rng.randrange(5, 9), rng.randrange(9, 19), 19, 28, 29, 31)]
    out.append(es(rng, addr, rng.randrange(1, 32), df=18))
    out += [ap(bytes([(df << 3) | rng.randrange(8)]) + r8(10), addr) for df in (20, 21)]
    return out


def corpus(rng, n):
    """n items (payload, timestamp, signal byte): every_format of a few aircraft with one, two and three flipped bits,
    rewritten DFs, Mode A/C replies and noise in between"""
    items = []
    while len(items) < n:
        for p in every_format(rng, rng.choice([rng.randrange(1, 1 << 24), 0x1A1A1A, 0x001A00])):
            x = rng.random()
            if x < 0.25:
                p = flipped(p, [rng.randrange(5, 8 * len(p))])
            elif x < 0.4:
                p = flipped(p, rng.sample(range(5, 8 * len(p)), 2))
            elif x < 0.45:
                p = flipped(p, rng.sample(range(8 * len(p)), 3))
            elif x < 0.5:
                p = bytes(rng.randrange(256) for _ in range(len(p)))
            items.append((p, rng.choice([rng.randrange(1 << 48), 0, 0x1A1A1A1A1A1A, 0x1A331A331A33]),
                          rng.choice([0x1A, 0, 255, rng.randrange(256)])))
            if rng.random() < 0.1:
                items.append((bytes([rng.randrange(256), rng.randrange(256)]), rng.randrange(1 << 48), rng.randrange(256)))
    return items[:n]


def beast_stream(items, rng=None):
    out = bytearray()
    for p, ts, sig in items:
        out += frame({2: ord("1"), 7: ord("2"), 14: ord("3")}[len(p)], p, ts, sig)
        if rng and rng.random() < 0.1:
            out += rng.choice([bytes(rng.randrange(256) for _ in range(rng.randrange(40))), frame(ord("4"), bytes(14), ts, sig)])
    return bytes(out)


def avr_stream(items, rng=None):
    out = bytearray()
    for k, (p, ts, sig) in enumerate(items):
        h = p.hex().upper().encode()
        kind = rng.randrange(3) if rng else k % 3
        out += [b"*" + h, b"@%012X" % ts + h, b"<%012X%02X" % (ts, sig) + h][kind] + b";\n"
        if rng and rng.random() < 0.1:
            out += rng.choice([b"\n", b"*8D;\n", b"garbage\r\n", b"x" * 300 + b"\n"])
    return bytes(out)


def host_writers(pkg):
    L = C.CDLL(os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "libmsd_host.so"))
    L.msd_beast_frame_out.restype = C.c_size_t
    L.msd_beast_frame_out.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.msd_avr_line_out.restype = C.c_size_t
    L.msd_avr_line_out.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return L


def host_bytes(host, msgs, fmt, verbatim):
    """the host writers over one entry's records, in order"""
    msgs = np.ascontiguousarray(msgs)
    buf = (C.c_uint8 * 64)()
    out = []
    for i in range(len(msgs)):
        p = msgs[i:i + 1].ctypes.data
        k = host.msd_beast_frame_out(p, int(verbatim), buf) if fmt == WIRE_BEAST else \
            host.msd_avr_line_out(p, int(fmt == WIRE_AVR_MLAT), int(verbatim), buf)
        out.append(bytes(buf[:k]))
    return b"".join(out)


def cut_at(data, cuts):
    edges = [0] + list(cuts) + [len(data)]
    return [data[a:b] for a, b in zip(edges[:-1], edges[1:])]


class Twin:
    """Two groups of one configuration.  `plain` gets the plain accept call, `new` the fields or wire call on the same
    bytes; what `new` delivers must be the host writers' bytes, or msd_decode_fields(mm, NULL), over plain's records."""

    def __init__(self, pkg, K, levels=None, modeac=None, flags=0, nfix=1):
        self.pkg, self.K = pkg, K
        self.host = host_writers(pkg)
        self.plain, self.new = (pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, nfix_crc=nfix, flags=flags) for _ in range(2))
        for g in (self.plain, self.new):
            for r in range(K):
                if levels and levels[r] != nfix:
                    g.set_receiver_options(r, nfix_crc=levels[r])
                if modeac and modeac[r]:
                    g.set_receiver_mode_ac(r, 1)
        self.seen = set()

    def close(self):
        self.plain.close()
        self.new.close()

    def _entries(self, kind, chunks, now_ms, keep):
        G = self.pkg.capi.ReceiverGroup
        nows = [now_ms] * len(chunks) if isinstance(now_ms, int) else list(now_ms)
        if kind == "beast":
            return G.beast_entries(chunks, nows)
        ent, n, data = G.avr_entries(chunks, nows, False)
        keeps = [keep] * n if isinstance(keep, bool) else list(keep)
        for i in range(n):
            ent[i].flags = self.pkg.capi.AVR_KEEP_TIMESTAMP if keeps[i] else 0
        return ent, n, data

    def records(self, g, kind, chunks, now_ms, keep=False):
        """the plain call on g: one record array per entry, in entry order"""
        ent, n, data = self._entries(kind, chunks, now_ms, keep)
        got = (g.accept_beast if kind == "beast" else g.accept_avr)(data, None, entries=(ent, n))
        rank = {r: i for i, (r, _) in enumerate(chunks)}
        rx = [int(r) for r in got["receiver"]]
        assert all(rank[a] <= rank[b] for a, b in zip(rx[:-1], rx[1:])), "delivery is by entry, in entry order"
        per = [np.ascontiguousarray(got["m"][got["receiver"] == r]) for r, _ in chunks]
        for m in per:
            self.seen.update(int(a) for a in m["addr"][np.isin(m["msgtype"], (11, 17, 18))])
        return per

    def wire(self, kind, chunks, now_ms, fmt, verbatim, keep=False, device=None):
        """Returns (plain's records per entry, new's (receiver, bytes, nmessages) per entry) after comparing them."""
        want = self.records(self.plain, kind, chunks, now_ms, keep)
        ent, n, data = self._entries(kind, chunks, now_ms, keep)
        if device is not None:
            data = device.from_numpy(np.frombuffer(data + b"\0", dtype=np.uint8).copy()).to("cuda:0")
        call = self.new.accept_beast_wire if kind == "beast" else self.new.accept_avr_wire
        got = call(data, None, format=fmt, verbatim=verbatim, entries=(ent, n))
        assert [r for r, _, _ in got] == [r for r, _ in chunks], "the sink is called once per entry, in entry order"
        for i, ((r, b, nm), recs) in enumerate(zip(got, want)):
            expect = host_bytes(self.host, recs, fmt, verbatim)
            assert nm == len(recs), (i, r, nm, len(recs))
            assert b == expect, (i, r, len(b), len(expect), first_difference(b, expect))
        return want, got

    def fields(self, kind, chunks, now_ms, keep=False):
        want = self.records(self.plain, kind, chunks, now_ms, keep)
        ent, n, data = self._entries(kind, chunks, now_ms, keep)
        call = self.new.accept_beast_fields if kind == "beast" else self.new.accept_avr_fields
        got = call(data, None, entries=(ent, n))
        assert sorted(got) == sorted(r for r, _ in chunks)
        for (r, _), recs in zip(chunks, want):
            assert len(got[r]) == len(recs), (r, len(got[r]), len(recs))
            for k, (m, f) in enumerate(got[r]):
                assert m.tobytes() == recs[k].tobytes(), (r, k)
                assert f.tobytes() == self.pkg.capi.decode_fields(recs[k]).tobytes(), (r, k, int(recs[k]["msgtype"]))
        return want, got

    def same_counters(self):
        for r in range(self.K):
            a, b = self.plain.remote_stats(r), self.new.remote_stats(r)
            a.pop("tile_rewalks"), b.pop("tile_rewalks")
            assert a == b, (r, a, b)
            assert self.plain.avr_stats(r) == self.new.avr_stats(r), r

    def same_state(self, rng, now_ms, decoys=16):
        """Equal counters, and equal answers to a probe: one DF4 per address a squitter carried and a few random ones,
        as Beast frames and as AVR lines to every receiver (behind whatever frame or line it has kept)."""
        self.same_counters()
        addrs = sorted(self.seen) + [rng.randrange(1 << 24) for _ in range(decoys)]
        bodies = [ap(bytes([0x20, 0x00, 0x05, 0x30]), a) for a in addrs]
        for kind, data in (("beast", b"".join(frame(ord("2"), p) for p in bodies)),
                           ("avr", b"".join(b"*" + p.hex().encode() + b";\n" for p in bodies))):
            chunks = [(r, data) for r in range(self.K)]
            a, b = self.records(self.plain, kind, chunks, now_ms), self.records(self.new, kind, chunks, now_ms)
            for r in range(self.K):
                assert a[r].tobytes() == b[r].tobytes(), (kind, r, len(a[r]), len(b[r]))
        self.same_counters()


def first_difference(a, b):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return k, a[max(k - 8, 0):k + 24].hex(), b[max(k - 8, 0):k + 24].hex()
