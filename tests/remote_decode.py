"""The checker of the Beast / AVR input (msd_accept_beast, msd_accept_frames): decodeBinMessage + decodeModesMessage
(net_io.c:1486-1627, mode_s.c:424-555,717-726) restated in Python over the oracle's own primitives -- orc_checksum,
orc_diagnose, orc_filter_add / orc_filter_test -- with icaoFilterExpire after every call (one empty buffer through
orc_demod_buffer: it sets the oracle's clock to the call's now_ms and expires, and demodulates nothing).

Framing: the frames are the ones libmsd_host.so's msd_beast_reader_feed delivers; the READ_MODE_BEAST scanner
(net_io.c:2504-2569) is restated here only for what the host reader does not report -- where each run of bytes in
front of a 0x1A ends, which the reference charges floor(gap / 15) to remote_rejected_bad, and that bytes behind the
last frame stay in the buffer until the next 0x1A arrives.  Every call checks that both framings agree."""
import ctypes as C
import os

import numpy as np

MODEAC_ADDR_FLAG = 1 << 24
SHORT_DFS_AP = {0, 4, 5}
LONG_DFS_AP = {16, 24, 25, 26, 27, 28, 29, 30, 31}


class BeastReader(C.Structure):
    _fields_ = [("buf", C.c_uint8 * 256), ("len", C.c_size_t), ("mode_ac", C.c_int), ("frames", C.c_uint64),
                ("modeac_ignored", C.c_uint64), ("other_frames", C.c_uint64), ("garbage_bytes", C.c_uint64)]


_SINK = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)


def host_lib(pkg):
    host = C.CDLL(os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "libmsd_host.so"))
    host.msd_beast_reader_init.argtypes = [C.c_void_p, C.c_int]
    host.msd_beast_reader_feed.restype = C.c_size_t
    host.msd_beast_reader_feed.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, _SINK, C.c_void_p]
    host.msd_avr_parse_line.restype = C.c_int
    host.msd_avr_parse_line.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    return host


def escape(body):
    """Every 0x1A after the type byte doubled (modesSendBeastOutput, net_io.c:795-830)."""
    return body.replace(b"\x1a", b"\x1a\x1a")


def frame(type_byte, payload, ts=0, signal=0x80):
    """A Beast frame: 0x1A, type, 6-byte timestamp, signal byte, payload, escaped."""
    body = ts.to_bytes(6, "big") + bytes([signal]) + bytes(payload)
    return b"\x1a" + bytes([type_byte]) + escape(body)


def hulc(length, ident=0x01, fill=0x33):
    """A GNS HULC frame: 0x1A 'H' id len payload (len + 2 bytes behind the type byte)."""
    return b"\x1a" + b"H" + escape(bytes([ident, length]) + bytes([fill]) * length)


def remote_counters():
    return {"remote_received_modes": 0, "remote_received_modeac": 0, "remote_rejected_bad": 0,
            "remote_rejected_unknown_icao": 0, "remote_accepted": [0, 0, 0], "frames": 0, "other_frames": 0,
            "garbage_bytes": 0}


class Checker:
    """One receiver's remote input.  `oracle` may be an Oracle that has already demodulated captures (its filter and
    clock are then the shared ones); it must have been made with mode_ac=0 (the empty buffer of the expiry must not
    run the Mode A/C demodulator).  mode_ac here is the receiver's --modeac for type '1' frames."""

    def __init__(self, pkg, O, nfix, mode_ac=0, oracle=None):
        self.pkg, self.O = pkg, O
        self.nfix, self.mode_ac = nfix, mode_ac
        self.orc = oracle if oracle is not None else O.Oracle(O.FMT_UC8, 58, nfix, 0)
        self.host = host_lib(pkg)
        self.reader = BeastReader()
        self.host.msd_beast_reader_init(C.byref(self.reader), int(mode_ac))
        self.kept = b""
        self.stats = remote_counters()
        self.known = set()  # every address that reached icaoFilterAdd (for probes)

    # --- the filter and its clock ---------------------------------------------------------------------------------
    def expire(self, now_ms):
        self.orc.demod_buffer(np.zeros(self.O.OVERLAP, dtype=np.uint16), 0, now_ms)

    # --- decodeModesMessage ---------------------------------------------------------------------------------------
    def decide(self, payload, nbytes):
        """(verdict, record fields) of one Mode S frame: verdict 0 accepted, -1 unknown address, -2 bad."""
        msg = bytearray(payload[:nbytes]) + bytearray(14 - nbytes)
        if not any(msg[:7]):
            return -2, None
        df = msg[0] >> 3
        bits = 112 if df & 0x10 else 56
        if bits > 8 * nbytes:  # the documented divergence: no CRC over bytes that never arrived
            return -2, None
        crc = self.O.checksum(bytes(msg[: bits // 8]))
        corrected, add = 0, False

        def aa():
            return (msg[1] << 16) | (msg[2] << 8) | msg[3]

        def fix(bitlist):
            for b in bitlist:
                if b >= 0:
                    msg[b >> 3] ^= 0x80 >> (b & 7)

        if df in SHORT_DFS_AP or df in LONG_DFS_AP or df in (20, 21):
            if not self.orc.filter_test(crc):
                return -1, None
            addr = crc
        elif df == 11:
            if crc & 0xFFFF80:
                n, b = self.orc.diagnose(crc & 0xFFFF80, bits)
                if n < 0 or n > 1:
                    return -2, None
                fix(b[:n])
                corrected = n
                if not self.orc.filter_test(aa()):
                    return -1, None
            addr = aa()
            add = corrected == 0 and (crc & 0x7F) == 0
        elif df in (17, 18):
            if crc != 0:
                n, b = self.orc.diagnose(crc, bits)
                if n < 0:
                    return -2, None
                a1 = aa()
                fix(b[:n])
                corrected = n
                if a1 != aa() and not self.orc.filter_test(aa()):
                    return -1, None
            addr = aa()
            add = corrected == 0 and df == 17
        else:
            return -2, None
        if add:  # mode_s.c:717-726
            self.orc.filter_add(addr)
            self.known.add(addr)
        return 0, dict(addr=addr, crc=crc, msgtype=df, msgbits=bits, correctedbits=corrected, msg=bytes(msg),
                       iid=(crc & 0x7F) if df == 11 else 0)

    def _record(self, out, ts, level, now_ms, f):
        r = np.zeros(1, dtype=self.pkg.capi.MESSAGE_DTYPE)[0]
        r["timestampMsg"], r["sysTimestampMsg"], r["signalLevel"] = ts, now_ms, level
        for k in ("addr", "crc", "msgtype", "msgbits", "correctedbits", "iid"):
            r[k] = f[k]
        r["msg"] = np.frombuffer(f["msg"], dtype=np.uint8)
        out.append(r)

    def _modeac(self, out, ts, level, now_ms, two):
        modeac = (two[0] << 8) | two[1]
        self._record(out, ts, level, now_ms, dict(addr=(modeac & 0xFF7F) | MODEAC_ADDR_FLAG, crc=0, msgtype=32,
                                                  msgbits=16, correctedbits=0, msg=bytes(two) + bytes(12), iid=0))

    def _message(self, out, ts, level, payload, nbytes, now_ms):
        """decodeBinMessage's part for one '1' / '2' / '3' frame (or one framed record)."""
        if nbytes == 2:
            self.stats["remote_received_modeac"] += 1
            if self.mode_ac:
                self.stats["frames"] += 1
                self._modeac(out, ts, level, now_ms, payload[:2])
            return
        self.stats["frames"] += 1
        self.stats["remote_received_modes"] += 1
        v, f = self.decide(payload, nbytes)
        if v == -2:
            self.stats["remote_rejected_bad"] += 1
        elif v == -1:
            self.stats["remote_rejected_unknown_icao"] += 1
        else:
            self.stats["remote_accepted"][f["correctedbits"]] += 1
            self._record(out, ts, level, now_ms, f)

    # --- the READ_MODE_BEAST scanner ------------------------------------------------------------------------------
    def _scan(self, data):
        """(events, garbage bytes): events are ("gap", length) and ("frame", type, unescaped bytes behind the type)."""
        buf = self.kept + bytes(data)
        som, ev, garbage = 0, [], 0
        n = len(buf)
        while som < n:
            p = buf.find(b"\x1a", som)
            if p < 0:
                break
            ev.append(("gap", p - som))
            som = p
            if p + 1 >= n:
                break
            t = buf[p + 1]
            if t in b"12345":
                eom = p + 1 + {ord("1"): 10, ord("2"): 15}.get(t, 22)
            elif t == ord("H"):
                if p + 3 >= n:
                    break
                if buf[p + 3] > 24:
                    som += 1
                    ev.append(("skip",))
                    continue
                eom = p + buf[p + 3] + 4
            else:
                som += 1
                ev.append(("skip",))
                continue
            q = som + 1
            while q < n and q < eom:
                if buf[q] == 0x1A:
                    q += 1
                    eom += 1
                q += 1
            if eom > n:
                break
            plain, q = bytearray(), p + 2
            while q < eom:
                plain.append(buf[q])
                q += 2 if buf[q] == 0x1A else 1
            ev.append(("frame", t, bytes(plain)))
            som = eom
        self.kept = buf[som:]
        return ev

    def beast(self, data, now_ms):
        """One msd_accept_beast call: the accepted records, as a MESSAGE_DTYPE array."""
        data = bytes(data)
        got = []

        def sink(p, user):
            got.append(np.frombuffer(C.string_at(p, self.pkg.capi.MESSAGE_DTYPE.itemsize),
                                     dtype=self.pkg.capi.MESSAGE_DTYPE)[0].copy())

        cb = _SINK(sink)
        g0, o0 = self.reader.garbage_bytes, self.reader.other_frames
        self.host.msd_beast_reader_feed(C.byref(self.reader), data, len(data), cb, None)
        self.stats["garbage_bytes"] += self.reader.garbage_bytes - g0
        self.stats["other_frames"] += self.reader.other_frames - o0
        events = self._scan(data)
        mine = [e for e in events if e[0] == "frame" and (e[1] in b"23" or (e[1] == ord("1") and self.mode_ac))]
        assert len(mine) == len(got), ("the two framings disagree", len(mine), len(got))
        out, k = [], 0
        for e in events:
            if e[0] == "gap":
                self.stats["remote_rejected_bad"] += e[1] // 15  # net_io.c:2510, per gap
            elif e[0] == "frame":
                t, plain = e[1], e[2]
                if t == ord("1") and not self.mode_ac:
                    self.stats["remote_received_modeac"] += 1
                    continue
                if t not in b"123":
                    continue
                rec = got[k]
                k += 1
                nbytes = len(plain) - 7
                ts = int.from_bytes(plain[:6], "big")
                lvl = plain[6] / 255.0
                assert rec["timestampMsg"] == ts and bytes(rec["msg"][:nbytes]) == plain[7:], "framings disagree"
                self._message(out, ts, lvl * lvl, plain[7:], nbytes, now_ms)
        self.expire(now_ms)
        return self._array(out)

    def frames(self, records, now_ms):
        """One msd_accept_frames call over records (msgbits 16 / 56 / 112)."""
        out = []
        for r in records:
            nbytes = int(r["msgbits"]) // 8
            self._message(out, int(r["timestampMsg"]), float(r["signalLevel"]), bytes(r["msg"]), nbytes, now_ms)
        self.expire(now_ms)
        return self._array(out)

    def _array(self, out):
        dt = self.pkg.capi.MESSAGE_DTYPE
        return np.array(out, dtype=dt) if out else np.zeros(0, dtype=dt)


def assert_same_records(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in ("timestampMsg", "sysTimestampMsg", "signalLevel", "addr", "crc", "score", "msgtype", "msgbits",
              "correctedbits", "bestphase", "iid"):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(got["msg"], want["msg"])


def assert_same_stats(got, want):
    for k, v in want.items():
        assert got[k] == v, (k, got[k], v)
