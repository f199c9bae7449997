"""A second reading of the reference's Mode A/C matching in plain Python, written from track.c, track.h and mode_ac.c and
not from msd_modeac_impl.h: the count of trackUpdateFromMessage (track.c:999-1003), the two resets of modeC_hit / modeA_hit
inside it (:1096-1102, :1154-1156), trackMatchAC (:1411-1485), modeAToIndex / indexToModeA (track.h:246-256), and
modeACInit / modeCToModeA with the Gillham decode behind them (mode_ac.c:63-163).

It sits on top of indep_aircraft.Tracker, whose feed_table it wraps: nothing in front of the altitude block touches the
altitude's validity or value, and nothing in front of the squawk store touches the squawk's, so both resets can be
decided on the state the record finds.  The reference keeps one set of modeAC_* arrays; the library keeps one per
receiver and matches an aircraft against its own receiver's, and so does this.  C's division truncates towards zero
(indep_aircraft.c_div).  Imports nothing from the package."""
import indep_aircraft as ia
from indep_aircraft import c_div
from indep_positions import INVALID, U64

INVALID_ALTITUDE = -9999
MIN_MESSAGES = 4  # TRACK_MODEAC_MIN_MESSAGES, track.h:66
U32 = 0xFFFFFFFF


def mode_a_to_index(mode_a):  # track.h:247-250
    return (mode_a & 0x0007) | ((mode_a & 0x0070) >> 1) | ((mode_a & 0x0700) >> 2) | ((mode_a & 0x7000) >> 3)


def index_to_mode_a(index):  # track.h:253-256
    return (index & 0o0007) | ((index & 0o0070) << 1) | ((index & 0o0700) << 2) | ((index & 0o7000) << 3)


def internal_mode_a_to_mode_c(mode_a):  # mode_ac.c:100-163
    if (mode_a & 0xFFFF8889) != 0 or (mode_a & 0x00F0) == 0:
        return INVALID_ALTITUDE
    one_hundreds = 0
    if mode_a & 0x0010:
        one_hundreds ^= 0x007
    if mode_a & 0x0020:
        one_hundreds ^= 0x003
    if mode_a & 0x0040:
        one_hundreds ^= 0x001
    if (one_hundreds & 5) == 5:
        one_hundreds ^= 2
    if one_hundreds > 5:
        return INVALID_ALTITUDE
    five_hundreds = 0
    for bit, mask in ((0x0002, 0x0FF), (0x0004, 0x07F), (0x1000, 0x03F), (0x2000, 0x01F), (0x4000, 0x00F), (0x0100, 0x007),
                      (0x0200, 0x003), (0x0400, 0x001)):
        if mode_a & bit:
            five_hundreds ^= mask
    if five_hundreds & 1:
        one_hundreds = 6 - one_hundreds
    return five_hundreds * 5 + one_hundreds - 13


def build_tables():  # modeACInit, mode_ac.c:63-75
    a_to_c, c_to_a = [0] * 4096, [0] * 4096
    for i in range(4096):
        mode_a = index_to_mode_a(i)
        mode_c = internal_mode_a_to_mode_c(mode_a)
        a_to_c[i] = mode_c
        mode_c += 13
        if 0 <= mode_c < 4096:
            assert c_to_a[mode_c] == 0  # the reference's assert
            c_to_a[mode_c] = mode_a
    return a_to_c, c_to_a


A_TO_C, C_TO_A = build_tables()


def mode_c_to_mode_a(mode_c):  # mode_ac.c:92-98
    mode_c += 13
    if mode_c < 0 or mode_c >= 4096:
        return 0
    return C_TO_A[mode_c]


class Codes:
    """modeAC_count / _lastcount / _match / _age[4096], track.c:59-62"""

    def __init__(self):
        self.count, self.lastcount, self.match, self.age = ([0] * 4096 for _ in range(4))


class Tracker(ia.Tracker):
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.codes = [Codes() for _ in self.rx]

    def reset(self):
        self.aircraft = {}
        self.codes = [Codes() for _ in self.rx]

    def update(self, msgs, fields, receiver=None):
        out = super().update(msgs, fields, receiver)  # raises, with nothing changed, when the call does not fit
        for i in range(len(msgs)):
            if msgs["msgtype"][i] == 32:  # :999-1003: just count it (we ignore SPI)
                c = self.codes[int(receiver[i]) if receiver is not None else 0]
                k = mode_a_to_index(int(fields["squawk"][i]))
                c.count[k] = (c.count[k] + 1) & U32
        return out

    def would_accept(self, d, source):  # accept_data's two refusals, track.c:172-180
        return not (self.now < d.updated) and not (source < d.source and self.now < d.stale)

    def feed_table(self, a, m, f, location_result):
        if not hasattr(a, "mode_a_hit"):
            a.mode_a_hit = a.mode_c_hit = 0  # calloc, track.c:73
        source, ab = int(f["source"]), a.v["altitude_baro"]
        if f["altitude_baro_valid"] and (source >= ab.source or self.age(ab) > 15 * 1000):  # :1091-1102
            alt = ia.altitude_to_feet(int(f["altitude_baro"]), int(f["altitude_baro_unit"]))
            if a.mode_c_hit:
                if c_div(a.alt_baro + 49, 100) != c_div(alt + 49, 100):
                    a.mode_c_hit = 0
        if f["squawk_valid"] and self.would_accept(a.v["squawk"], source):  # :1153-1157
            if int(f["squawk"]) != a.squawk:
                a.mode_a_hit = 0
        return super().feed_table(a, m, f, location_result)

    def match_ac(self, now, message_now):  # trackMatchAC(now), with messageNow() = message_now
        self.now = message_now  # what trackDataValid reads
        for c in self.codes:
            c.match = [0] * 4096
        for (r, addr), a in self.aircraft.items():
            if not hasattr(a, "mode_a_hit"):
                a.mode_a_hit = a.mode_c_hit = 0
            c = self.codes[r]
            if ((now - a.seen) & U64) > 5000:
                continue

            def live(i):
                return ((c.count[i] - c.lastcount[i]) & U32) >= MIN_MESSAGES

            if self.valid(a.v["squawk"]):
                i = mode_a_to_index(a.squawk)
                if live(i):
                    a.mode_a_hit = 1
                    c.match[i] = U32 if c.match[i] else addr
            if self.valid(a.v["altitude_baro"]):
                mode_c = c_div(a.alt_baro + 49, 100)
                for cc in (mode_c, mode_c + 1, mode_c - 1):
                    mode_a = mode_c_to_mode_a(cc)
                    i = mode_a_to_index(mode_a)
                    if mode_a and live(i):
                        a.mode_c_hit = 1
                        c.match[i] = U32 if c.match[i] else addr
        for c in self.codes:  # :1462-1484
            for i in range(4096):
                if not c.count[i]:
                    continue
                if ((c.count[i] - c.lastcount[i]) & U32) < MIN_MESSAGES:
                    c.age[i] = (c.age[i] + 1) & U32
                    if c.age[i] > 15:
                        c.lastcount[i] = c.count[i] = c.age[i] = 0
                else:
                    c.age[i] = 10 if c.match[i] else 0
                c.lastcount[i] = c.count[i]

    def codes_of(self, receiver):
        """-> [(count, lastcount, match, age)] * 4096 in index order"""
        c = self.codes[receiver]
        return list(zip(c.count, c.lastcount, c.match, c.age))

    def hits(self):
        """-> [(receiver, addr, mode_a_hit, mode_c_hit)] in (receiver, addr) order"""
        return [(r, addr, getattr(self.aircraft[(r, addr)], "mode_a_hit", 0), getattr(self.aircraft[(r, addr)], "mode_c_hit", 0))
                for (r, addr) in sorted(self.aircraft)]
