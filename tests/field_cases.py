"""Constructed message families for the field decoder (msd_fields_impl.h): every decision of the header taken both ways.
Each family returns (records, note): records a MESSAGE_DTYPE array as msd_decode_fields takes it, note a dict with "what"
(a line for reports) and "known" -- hand-typed answers [(record index, {member: value})] where a decision is small enough
to state by hand.  FAMILIES lists them by letter; build(dtype, letter) makes one.

The records are accepted messages: msgtype, msgbits, the bytes, and addr as the CRC switch leaves it (the AA field for
DF11/17/18, a fixed address otherwise).  Nothing here looks at the decoder under test or at the second reading, except
family g, which asks the second reading for nothing either: its enumeration is plain float64 arithmetic over the raw
values (turn_rate_subspace)."""
import math

import numpy as np

AP_ADDR = 0x3C6DD0  # what the address/parity formats' syndrome is taken to be
AA = 0xABCDEF


def pack(nbits, fields):
    """[(first, last, value)] with bits numbered from 1 at the most significant -> int"""
    v = 0
    for first, last, value in fields:
        assert 0 <= value < (1 << (last - first + 1)), (first, last, value)
        v |= value << (nbits - last)
    return v


def short(df, payload27=0):
    return ((df << 27) | payload27).to_bytes(4, "big") + bytes(3)


def long_(df, payload27=0, body56=0):
    return ((df << 27) | payload27).to_bytes(4, "big") + body56.to_bytes(7, "big") + bytes(3)


def es(me56, df=17, sub=5, aa=AA):
    return bytes([(df << 3) | sub]) + aa.to_bytes(3, "big") + me56.to_bytes(7, "big") + bytes(3)


def me(metype, *fields):
    return pack(56, [(1, 5, metype)] + list(fields))


def commb(mb56, df=20, fs=0, dr=0, um=0, code13=0):
    return long_(df, pack(32, [(6, 8, fs), (9, 13, dr), (14, 19, um), (20, 32, code13)]), mb56)


class Build:
    def __init__(self):
        self.raws, self.known = [], []

    def add(self, raw, **known):
        if known:
            self.known.append((len(self.raws), known))
        self.raws.append(raw)

    def done(self, dtype, what):
        return to_records(dtype, self.raws), {"what": what, "known": self.known}


def to_records(dtype, raws):
    rec = np.zeros(len(raws), dtype=dtype)
    for i, raw in enumerate(raws):
        rec["msg"][i, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        if len(raw) == 2:
            rec["msgtype"][i], rec["msgbits"][i] = 32, 16
        else:
            df = raw[0] >> 3
            rec["msgtype"][i], rec["msgbits"][i] = df, 8 * len(raw)
            rec["addr"][i] = int.from_bytes(raw[1:4], "big") if df in (11, 17, 18) else AP_ADDR
    return rec


# ------------------------------------------------------------------------------------------------------------ a. headers
def family_a(dtype):
    b = Build()
    for df in range(32):  # every DF, with every other header bit set, with alternating bits, and with none
        for payload, body in ((0x7FFFFFF, (1 << 56) - 1), (0x2AAAAAA, 0xAAAAAAAAAAAAAA), (0x5555555, 0x55555555555555), (0, 0)):
            b.add(long_(df, payload, body) if df & 16 else short(df, payload))
    b.add(short(4, 0), AC=0, altitude_baro_valid=0, altitude_baro=0, airground=3, FS=0, alert_valid=1, spi_valid=1, source=3)
    b.add(short(0, 0), AC=0, altitude_baro_valid=0, VS=0, airground=3)
    b.add(long_(16, 0), AC=0, altitude_baro_valid=0)
    b.add(commb(0, df=20), AC=0, altitude_baro_valid=0, commb_format=2)
    b.add(short(5, 0), ID=0, squawk_valid=0, squawk=0)
    b.add(commb(0, df=21), ID=0, squawk_valid=0, commb_format=2)
    b.add(short(4, 0x1838), AC=0x1838, altitude_baro=38000, altitude_baro_valid=1, altitude_baro_unit=0)  # Q bit, 25 ft steps
    b.add(short(4, 0x0040), AC=0x0040, altitude_baro=-9999, altitude_baro_valid=0, altitude_baro_unit=1)  # M bit alone
    b.add(short(5, 0x0AAA), ID=0x0AAA, squawk=0x7700, squawk_valid=1)
    b.add(short(5, 0x1555), ID=0x1555, squawk=0x0077, squawk_valid=1)  # C and D pulses (and the X bit, dropped)
    for code in range(8192):  # all AC13 / ID13 codes
        b.add(short(4, code))
        b.add(short(5, code))
    for ac12 in range(4096):  # all AC12 codes, barometric (type 11) and geometric (type 20)
        b.add(es(me(11, (9, 20, ac12), (23, 39, 1), (40, 56, 1))))
        b.add(es(me(20, (9, 20, ac12), (23, 39, 1), (40, 56, 1))))
    # FS 0..7 (mode_s.c:613-650): airground, alert, spi, valid
    fs_table = {0: (3, 0, 0, 1), 1: (1, 0, 0, 1), 2: (3, 1, 0, 1), 3: (1, 1, 0, 1), 4: (3, 1, 1, 1), 5: (3, 0, 1, 1),
                6: (0, 0, 0, 0), 7: (0, 0, 0, 0)}
    for df in (4, 5, 20, 21):
        for fs, (ag, alert, spi, valid) in fs_table.items():
            raw = short(df, fs << 24) if df < 16 else commb(0, df=df, fs=fs)
            b.add(raw, FS=fs, airground=ag, alert=alert, spi=spi, alert_valid=valid, spi_valid=valid)
    for df in (11, 17):  # CA 0..7 (mode_s.c:577-597)
        for ca, ag in {0: 3, 1: 0, 2: 0, 3: 0, 4: 1, 5: 2, 6: 3, 7: 3}.items():
            raw = short(11, ca << 24) if df == 11 else es(me(24), sub=ca)
            b.add(raw, CA=ca, airground=ag, source=4 if df == 11 else 7)
    for df in (0, 16):
        for vs in (0, 1):
            raw = short(0, vs << 26) if df == 0 else long_(16, vs << 26)
            b.add(raw, VS=vs, airground=1 if vs else 3)
    return b.done(dtype, "headers: every DF, AC / ID zero, all AC13, ID13 and AC12 codes, FS, CA, VS")


# --------------------------------------------------------------------------------------------------------------- b. DF18
def imf_bit(metype):
    """the ME bit setIMF looks at for this type, None where the type has none"""
    if metype == 0 or 9 <= metype <= 18 or 20 <= metype <= 22:
        return 8
    if metype == 19:
        return 9
    if 5 <= metype <= 8:
        return 21
    if metype == 29:
        return 51
    if metype in (28, 31):
        return 56
    return None


def me_base(metype):
    """a payload of this type that reaches the type's IMF test, with something in every field around it"""
    if 1 <= metype <= 4:
        return me(metype, (6, 8, 3), *[(9 + 6 * i, 14 + 6 * i, c) for i, c in enumerate((11, 12, 13, 49, 48, 50, 51, 32))])
    if metype == 19:
        return me(19, (6, 8, 1), (11, 13, 2), (14, 14, 1), (15, 24, 9), (26, 35, 160), (37, 37, 1), (38, 46, 14), (50, 56, 23))
    if 5 <= metype <= 8:
        return me(metype, (6, 12, 17), (13, 13, 1), (14, 20, 33), (22, 22, 1), (23, 39, 39195), (40, 56, 110320))
    if metype == 0 or 9 <= metype <= 18 or 20 <= metype <= 22:
        return me(metype, (9, 20, 0xC38), (22, 22, 1), (23, 39, 74158), (40, 56, 50194))
    if metype == 23:
        return me(23, (6, 8, 7), (9, 21, 0x0AAA))
    if metype == 28:
        return me(28, (6, 8, 1), (9, 11, 2), (12, 24, 0x0AAA))
    if metype == 29:
        return me(29, (6, 7, 1), (10, 20, 532), (21, 29, 267), (30, 30, 1), (31, 39, 95), (40, 43, 9), (47, 47, 1), (48, 48, 1))
    if metype == 31:
        return me(31, (6, 8, 0), (41, 43, 2), (11, 11, 1), (45, 48, 10), (51, 52, 3))
    return me(metype, (6, 8, 5), (30, 40, 0x555))


def family_b(dtype):
    b = Build()
    for df in (18, 17):
        for sub in range(8):  # CF, or CA where the bit means NIC-B or nothing
            for metype in range(32):
                bit = imf_bit(metype) or 8
                base = me_base(metype) & ~(1 << (56 - bit))
                for imf in (0, 1):
                    known = {}
                    if df == 18 and metype == 11:
                        known = {0: dict(addrtype=1, imf=0, source=7, addr=AA, nic_b_valid=1, nic_b=imf),
                                 1: dict(addrtype=4, imf=0, source=7, addr=AA | 1 << 24),
                                 2: dict(addrtype=6 if imf else 3, imf=imf, source=5, addr=AA | imf << 24, nic_b_valid=0),
                                 3: dict(addrtype=3, imf=0, source=5, addr=AA, cpr_valid=0, metype=11),
                                 4: dict(addrtype=9, imf=0, source=7, addr=AA | 1 << 24, cpr_valid=0),
                                 5: dict(addrtype=7, imf=0, source=5, addr=AA | 1 << 24),
                                 6: dict(addrtype=5 if imf else 2, imf=imf, source=6, addr=AA | imf << 24),
                                 7: dict(addrtype=9, imf=0, source=7, addr=AA | 1 << 24)}[sub]
                    elif df == 18 and sub == 6 and imf_bit(metype):
                        known = dict(addrtype=5 if imf else 2, imf=imf, source=6)
                    elif df == 18 and sub == 2 and imf_bit(metype):
                        known = dict(addrtype=6 if imf else 3, imf=imf, source=5)
                    elif df == 18 and sub == 3:  # coarse TIS-B: ME bit 1 alone
                        known = dict(addrtype=6 if metype >= 16 else 3, imf=int(metype >= 16), source=5, cpr_valid=0, mesub=0)
                    elif df == 17:
                        known = dict(addrtype=0, imf=0, source=7, addr=AA, CA=sub)
                    b.add(es(base | imf << (56 - bit), df=df, sub=sub), CF=sub if df == 18 else 0, **known)
    return b.done(dtype, "DF18 CF 0..7 x ME type 0..31 x the type's IMF bit, and the same in DF17")


# ------------------------------------------------------------------------------------------- c. ES zero and edge values
def family_c(dtype):
    b = Build()
    # velocity: raw values 0 / 1 / top, every subtype (0 and 5..7 decode nothing)
    for sub in range(8):
        for ew in (0, 1, 1023):
            for ns in (0, 1, 1023):
                for signs in range(4):
                    b.add(es(me(19, (6, 8, sub), (11, 13, 5), (14, 14, signs & 1), (15, 24, ew), (25, 25, signs >> 1), (26, 35, ns),
                                (36, 36, signs & 1), (37, 37, signs >> 1), (38, 46, (0, 1, 511)[(ew + ns) % 3]),
                                (49, 49, signs & 1), (50, 56, (0, 1, 127)[(ew + ns + signs) % 3]))))
    b.add(es(me(19, (6, 8, 1), (15, 24, 0), (26, 35, 5))), velocity_valid=0, nac_v_valid=1, ew_vel=0, ns_vel=0)
    b.add(es(me(19, (6, 8, 1), (15, 24, 5), (26, 35, 0))), velocity_valid=0)
    b.add(es(me(19, (6, 8, 1), (15, 24, 1), (26, 35, 1))), velocity_valid=1, ew_vel=0, ns_vel=0)
    b.add(es(me(19, (6, 8, 2), (14, 14, 1), (15, 24, 3), (26, 35, 1023))), velocity_valid=1, ew_vel=-8, ns_vel=4088)
    b.add(es(me(19, (6, 8, 0), (11, 13, 5), (15, 24, 5), (26, 35, 5), (38, 46, 5), (50, 56, 5))),
          mesub=0, nac_v_valid=0, velocity_valid=0, geom_rate_valid=0, geom_delta_valid=0)
    b.add(es(me(19, (6, 8, 5), (11, 13, 5), (15, 24, 5), (26, 35, 5), (38, 46, 5), (50, 56, 5))),
          mesub=5, nac_v_valid=0, velocity_valid=0, geom_rate_valid=0, geom_delta_valid=0)
    b.add(es(me(19, (6, 8, 3), (14, 14, 1), (15, 24, 512), (26, 35, 0))), heading_valid=1, heading_raw=512, heading_type=4,
          ias_valid=0, tas_valid=0)
    b.add(es(me(19, (6, 8, 3), (14, 14, 0), (15, 24, 512), (25, 25, 1), (26, 35, 1))), heading_valid=0, heading_raw=0,
          tas_valid=1, tas=0, ias_valid=0)
    b.add(es(me(19, (6, 8, 4), (26, 35, 101))), ias_valid=1, ias=400, tas_valid=0)
    b.add(es(me(19, (6, 8, 1), (36, 36, 1), (37, 37, 1), (38, 46, 0))), baro_rate_valid=0, geom_rate_valid=0)
    b.add(es(me(19, (6, 8, 1), (36, 36, 1), (37, 37, 1), (38, 46, 1))), baro_rate_valid=1, baro_rate=0, geom_rate_valid=0)
    b.add(es(me(19, (6, 8, 1), (36, 36, 0), (37, 37, 1), (38, 46, 511))), geom_rate_valid=1, geom_rate=-32640, baro_rate_valid=0)
    b.add(es(me(19, (6, 8, 1), (49, 49, 1), (50, 56, 0))), geom_delta_valid=0, geom_delta=0)
    b.add(es(me(19, (6, 8, 1), (49, 49, 1), (50, 56, 127))), geom_delta_valid=1, geom_delta=-3150)
    # surface movement
    for metype in (5, 6, 7, 8):
        for movement in (0, 1, 2, 3, 8, 9, 12, 13, 38, 39, 93, 94, 108, 109, 123, 124, 125, 126, 127):
            for status in (0, 1):
                known = dict(movement=movement if 0 < movement < 125 else 0, airground=1, cpr_valid=1, cpr_type=0,
                             heading_valid=status, heading_raw=77 if status else 0, heading_type=5 if status else 0)
                b.add(es(me(metype, (6, 12, movement), (13, 13, status), (14, 20, 77), (22, 22, movement & 1), (23, 39, 1 << 16),
                            (40, 56, 3))), **known)
    # test message and aircraft status
    b.add(es(me(23, (6, 8, 7), (9, 21, 0))), squawk_valid=0, squawk=0, mesub=7)
    b.add(es(me(23, (6, 8, 7), (9, 21, 0x0AAA))), squawk_valid=1, squawk=0x7700)
    b.add(es(me(23, (6, 8, 7), (9, 21, 0x0040))), squawk_valid=1, squawk=0)  # the X bit alone: non-zero, and dropped
    b.add(es(me(23, (6, 8, 6), (9, 21, 0x0AAA))), squawk_valid=0, mesub=6)
    b.add(es(me(23, (6, 8, 0), (9, 21, 0x0AAA))), squawk_valid=0, mesub=0)
    b.add(es(me(28, (6, 8, 1), (9, 11, 5), (12, 24, 0))), squawk_valid=0, emergency_valid=1, emergency=5)
    b.add(es(me(28, (6, 8, 1), (9, 11, 0), (12, 24, 0x0AAA), (56, 56, 1))), squawk_valid=1, squawk=0x7700, emergency_valid=1,
          emergency=0, imf=0)
    b.add(es(me(28, (6, 8, 0), (9, 11, 5), (12, 24, 0x0AAA))), squawk_valid=0, emergency_valid=0, mesub=0)
    b.add(es(me(28, (6, 8, 2), (9, 11, 5), (12, 24, 0x0AAA))), squawk_valid=0, emergency_valid=0, mesub=2)
    # the type 15 transmitter fault (mode_s.c:991), and each of its four conditions off by one
    def pos(metype, ac12, lat, lon, sub=5):
        return es(me(metype, (9, 20, ac12), (22, 22, 1), (23, 39, lat), (40, 56, lon)), sub=sub)
    b.add(pos(15, 0, 0x1F000, 0), cpr_valid=0, cpr_odd=0, cpr_type=0, cpr_lat=0x1F000, cpr_lon=0, altitude_baro_valid=0)
    b.add(pos(15, 0, 0x1000, 0), cpr_valid=0, cpr_lat=0x1000)
    b.add(pos(15, 0, 0, 0), cpr_valid=0)
    b.add(pos(15, 1, 0x1F000, 0), cpr_valid=1, cpr_odd=1, cpr_type=1)
    b.add(pos(15, 0, 0x1F000, 1), cpr_valid=1, cpr_lon=1)
    b.add(pos(15, 0, 0x1F001, 0), cpr_valid=1, cpr_lat=0x1F001)
    b.add(pos(15, 0, 0x1F800, 0), cpr_valid=1)
    b.add(pos(14, 0, 0x1F000, 0), cpr_valid=1, metype=14)
    b.add(pos(16, 0, 0x1F000, 0), cpr_valid=1, metype=16)
    # airborne position: on the ground (CA 4) no altitude is decoded; the type ranges; type 0; surveillance status
    b.add(pos(11, 0xC38, 5, 9, sub=4), airground=1, altitude_baro_valid=0, altitude_baro=0, cpr_valid=1)
    b.add(pos(11, 0xC38, 5, 9, sub=5), airground=2, altitude_baro_valid=1, altitude_baro=38000)
    b.add(pos(11, 0xC38, 5, 9, sub=0), airground=3, altitude_baro_valid=1, altitude_baro=38000)
    b.add(pos(21, 0xC38, 5, 9, sub=4), airground=1, altitude_geom_valid=0, altitude_baro_valid=0)
    b.add(pos(0, 0xC38, 5, 9), metype=0, cpr_valid=0, cpr_lat=0, cpr_lon=0, cpr_odd=0, altitude_baro_valid=1, altitude_baro=38000,
          nic_b_valid=1)
    b.add(pos(0, 0, 5, 9), metype=0, cpr_valid=0, altitude_baro_valid=0)
    b.add(pos(0, 0, 0, 0), metype=0, cpr_valid=0, altitude_baro_valid=0, alert_valid=1, spi_valid=1)
    for metype in range(32):  # every type with an altitude code, a position and no subtype: who takes which
        geom = 20 <= metype <= 22
        is_pos = metype == 0 or 9 <= metype <= 18 or geom
        known = dict(altitude_baro_valid=int(is_pos and not geom), altitude_geom_valid=int(geom)) if metype not in (19, 29, 31) else {}
        b.add(pos(metype, 0xC38, 5, 9), metype=metype, **known)
        b.add(pos(metype, 0x001, 5, 9), metype=metype)  # Gillham: C pulses all zero, no altitude
    for ss, (alert, alert_valid, spi, spi_valid) in {0: (0, 1, 0, 1), 1: (1, 1, 0, 0), 2: (1, 1, 0, 0), 3: (0, 1, 1, 1)}.items():
        for nicb in (0, 1):
            b.add(es(me(12, (6, 7, ss), (8, 8, nicb), (9, 20, 0xC38))), alert=alert, alert_valid=alert_valid, spi=spi,
                  spi_valid=spi_valid, nic_b_valid=1, nic_b=nicb)
    # callsign characters at the charset's edges: A-Z, 0-9 and space make a valid callsign, nothing else does
    charset = b"@ABCDEFGHIJKLMNOPQRSTUVWXYZ[\\]^_ !\"#$%&'()*+,-./0123456789:;<=>?"
    for c in (0, 1, 26, 27, 31, 32, 33, 47, 48, 57, 58, 63):
        for where in range(8):
            chars = [2] * 8
            chars[where] = c
            want = bytes(charset[x] for x in chars)
            b.add(es(me(1 + where % 4, (6, 8, where), *[(9 + 6 * i, 14 + 6 * i, x) for i, x in enumerate(chars)])),
                  callsign=want, callsign_valid=int(c in (1, 26, 32, 48, 57)), category=((0x0E - (1 + where % 4)) << 4) | where,
                  category_valid=1)
    return b.done(dtype, "ES zero and edge values: velocity, movement, types 23 / 28, the type 15 fault, CA 4, type 0, callsigns")


# ---------------------------------------------------------------------------- d. target state and operational status
def family_d(dtype):
    b = Build()
    for bit11 in (0, 1):  # ME type 29, the DO-260A layout (subtype 0, bit 11 clear)
        for vsrc in range(4):
            for vmode in range(4):
                for hsrc in range(4):
                    for hmode in range(4):
                        tcas = (vsrc + hmode) % 4 if bit11 == 0 else 2
                        alt = (0, 1023, 390, 1)[(vmode + hsrc) % 4]
                        b.add(es(me(29, (6, 7, 0), (8, 9, vsrc), (11, 11, bit11), (14, 15, vmode), (16, 25, alt), (26, 27, hsrc),
                                    (28, 36, 300 + hsrc), (37, 37, hmode & 1), (38, 39, hmode), (40, 43, 9), (44, 44, 1), (45, 46, 2),
                                    (52, 53, tcas), (54, 56, 5))))
    for tcas, (valid, modes) in {0: (0, 32), 1: (1, 0), 2: (1, 32), 3: (1, 32)}.items():
        b.add(es(me(29, (6, 7, 0), (52, 53, tcas))), nav_valid=valid, nav_modes=modes, emergency_valid=1, sil_type=1, acc_valid=3)
    b.add(es(me(29, (6, 7, 0), (8, 9, 1), (16, 25, 0))), nav_altitude_source=3, nav_valid=4, nav_mcp_altitude=-1000)
    b.add(es(me(29, (6, 7, 0), (8, 9, 3), (14, 15, 2), (16, 25, 390))), nav_altitude_source=4, nav_valid=8 | 1, nav_fms_altitude=38000,
          nav_modes=2 | 32)
    b.add(es(me(29, (6, 7, 0), (8, 9, 2), (14, 15, 2), (16, 25, 390))), nav_altitude_source=2, nav_valid=1, nav_modes=4 | 32,
          nav_mcp_altitude=0, nav_fms_altitude=0)
    b.add(es(me(29, (6, 7, 0), (26, 27, 0), (28, 36, 300), (37, 37, 1))), nav_valid=0, nav_heading_raw=0, nav_heading_type=0)
    b.add(es(me(29, (6, 7, 0), (26, 27, 1), (28, 36, 0), (37, 37, 1))), nav_valid=2, nav_heading_raw=0, nav_heading_type=1)
    b.add(es(me(29, (6, 7, 0), (11, 11, 1), (8, 9, 1), (16, 25, 390), (40, 43, 9))), nav_valid=0, acc_valid=0, emergency_valid=0)
    for sub in (1, 2, 3):  # DO-260B (subtype 1); 2 and 3 decode nothing
        for fms in (0, 1):
            for alt in (0, 1, 2047):
                for baro in (0, 1, 511):
                    for hv in (0, 1):
                        for hdg in (0, 511):
                            for mv, modes in ((0, 0), (0, 0x7F), (1, 0), (1, 0x7F), (1, 0x40), (1, 0x20), (1, 0x10), (1, 0x04),
                                              (1, 0x02), (1, 0x01), (1, 0x08)):
                                b.add(es(me(29, (6, 7, sub), (9, 9, fms), (10, 20, alt), (21, 29, baro), (30, 30, hv), (31, 39, hdg),
                                            (40, 43, 11), (44, 44, hv), (45, 46, 3), (47, 47, mv), (48, 54, modes))))
    b.add(es(me(29, (6, 7, 1), (10, 20, 0), (21, 29, 0), (30, 30, 0), (31, 39, 511), (47, 47, 0), (48, 54, 0x7F))),
          nav_valid=0, nav_modes=0, nav_heading_raw=0, nav_qnh_raw=0, acc_valid=3, sil_type=1)
    b.add(es(me(29, (6, 7, 1), (9, 9, 0), (10, 20, 1), (21, 29, 1), (30, 30, 1), (31, 39, 0), (47, 47, 1), (48, 54, 0))),
          nav_valid=1 | 2 | 4 | 16 | 32, nav_mcp_altitude=0, nav_qnh_raw=1, nav_heading_raw=0, nav_heading_type=4, nav_modes=0)
    b.add(es(me(29, (6, 7, 1), (9, 9, 1), (10, 20, 2047))), nav_valid=8, nav_fms_altitude=65472)
    b.add(es(me(29, (6, 7, 1), (47, 47, 1), (48, 54, 0x7F))), nav_valid=1, nav_modes=63)  # bit 51 is no mode bit
    b.add(es(me(29, (6, 7, 1), (47, 47, 1), (51, 51, 1))), nav_valid=1, nav_modes=0, imf=0)
    # ME type 31: every version and subtype against patterns that set and clear every bit the decoder reads
    patterns = [0, (1 << 48) - 1, 0xAAAAAAAAAAAA, 0x555555555555]
    patterns += [1 << (56 - bit) for bit in list(range(9, 41)) + list(range(44, 57))]
    patterns += [((1 << 48) - 1) & ~(1 << (56 - bit)) for bit in (9, 10, 13, 14, 25, 26)]
    patterns += [((1 << 48) - 1) & ~pack(56, [(9, 10, 3), (13, 14, 3), (25, 26, 3)])]
    for version in range(8):
        for sub in range(8):
            for p in patterns:
                keep = p & ~pack(56, [(1, 8, 255), (41, 43, 7)])
                b.add(es(me(31, (6, 8, sub), (41, 43, version)) | keep))
    b.add(es(me(31, (6, 8, 2), (41, 43, 2), (45, 48, 10))), opstatus=0, acc_valid=0, mesub=2)
    b.add(es(me(31, (6, 8, 0), (41, 43, 0), (12, 12, 0), (13, 13, 1))), opstatus=1 | 1 << 8 | 1 << 9, acc_valid=0, sil_type=0)
    b.add(es(me(31, (6, 8, 0), (41, 43, 0), (9, 10, 1), (13, 13, 1))), opstatus=1)
    b.add(es(me(31, (6, 8, 1), (41, 43, 0), (13, 13, 1))), opstatus=1)
    b.add(es(me(31, (6, 8, 0), (41, 43, 3), (45, 48, 10))), opstatus=1 | 3 << 1, acc_valid=0)
    b.add(es(me(31, (6, 8, 0), (41, 43, 1), (11, 11, 1), (54, 54, 1), (53, 53, 1))), opstatus=1 | 1 << 1 | 3 << 23,
          acc_valid=1 | 2 | 4, nic_baro=1, sil_type=1)
    b.add(es(me(31, (6, 8, 0), (41, 43, 2), (11, 11, 1), (55, 55, 1), (49, 50, 2))), opstatus=1 | 2 << 1 | 1 << 8 | 2 << 23,
          acc_valid=1 | 2 | 4 | 16 | 32, gva=2, sil_type=2)
    b.add(es(me(31, (6, 8, 1), (41, 43, 2), (21, 24, 9), (33, 40, 0xA5), (53, 53, 0))),
          opstatus=1 | 2 << 1 | 1 << 18 | 9 << 19 | 2 << 23 | 1 << 26, cc_antenna_offset=0xA5, nac_v_valid=1, sil_type=3,
          acc_valid=1 | 4 | 8 | 32)
    b.add(es(me(31, (6, 8, 1), (41, 43, 1), (53, 53, 1), (54, 54, 1))), opstatus=1 | 1 << 1 | 1 << 18 | 3 << 23 | 3 << 26)
    return b.done(dtype, "ME type 29 (both layouts) and 31 (every version and subtype): validity bits against values")


# ------------------------------------------------------------------------------------------------------------ e. Comm-B
def bds40(mcp_v=1, mcp=2000, fms_v=1, fms=2000, baro_v=1, baro=2132, res1=0, mode_v=1, mode=5, res2=0, src_v=1, src=2):
    return pack(56, [(1, 1, mcp_v), (2, 13, mcp), (14, 14, fms_v), (15, 26, fms), (27, 27, baro_v), (28, 39, baro), (40, 47, res1),
                     (48, 48, mode_v), (49, 51, mode), (52, 53, res2), (54, 54, src_v), (55, 56, src)])


def bds50(roll_v=1, roll=57, trk_v=1, trk=650, gs_v=1, gs=200, tr_v=1, trq=4, tas_v=1, tas=200, roll_bits=None, tr_bits=None):
    """roll and trq signed (10-bit two's complement with the sign bit in front); *_bits give sign and value as they are"""
    return pack(56, [(1, 1, roll_v), (2, 11, (roll & 0x3FF) if roll_bits is None else roll_bits), (12, 12, trk_v), (13, 23, trk),
                     (24, 24, gs_v), (25, 34, gs), (35, 35, tr_v), (36, 45, (trq & 0x3FF) if tr_bits is None else tr_bits),
                     (46, 46, tas_v), (47, 56, tas)])


def bds60(hdg_v=1, hdg=300, ias_v=1, ias=250, mach_v=1, mach=100, br_v=1, br=-10, ir_v=1, ir=-10, br_bits=None, ir_bits=None):
    return pack(56, [(1, 1, hdg_v), (2, 12, hdg), (13, 13, ias_v), (14, 23, ias), (24, 24, mach_v), (25, 34, mach), (35, 35, br_v),
                     (36, 45, (br & 0x3FF) if br_bits is None else br_bits), (46, 46, ir_v),
                     (47, 56, (ir & 0x3FF) if ir_bits is None else ir_bits)])


def family_e(dtype):
    b = Build()
    k = [0]

    def add(mb, **known):
        k[0] += 1
        b.add(commb(mb, df=20 + k[0] % 2, fs=k[0] % 6, um=k[0] % 64, code13=0x1838 if k[0] % 2 == 0 else 0x0AAA), **known)

    # BDS 4,0
    add(bds40(), commb_format=7, nav_mcp_altitude=32000, nav_fms_altitude=32000, nav_qnh_raw=2132, nav_modes=2 | 8,
        nav_altitude_source=3, nav_valid=1 | 4 | 8 | 16 | 64)
    for which in ("mcp", "fms"):
        for raw, ok in ((0, 0), (62, 0), (63, 1), (3125, 1), (3126, 0), (4095, 0)):  # 992 / 1008 / 50000 / 50016 ft
            for v in (0, 1):
                fmt = 7 if (v and ok) or (not v and raw == 0) else 0
                add(bds40(**{which + "_v": v, which: raw}), commb_format=fmt)
    for raw, ok in ((0, 0), (999, 0), (1000, 1), (3000, 1), (3001, 0), (4095, 0)):
        for v in (0, 1):
            add(bds40(baro_v=v, baro=raw), commb_format=7 if (v and ok) or (not v and raw == 0) else 0)
    for bit in range(8):
        add(bds40(res1=1 << bit), commb_format=0)
    for res2 in (1, 2):
        add(bds40(res2=res2), commb_format=0)
    add(bds40(mode_v=0, mode=0), commb_format=7, nav_modes=0, nav_valid=4 | 8 | 16 | 64)
    add(bds40(mode_v=0, mode=1), commb_format=0)
    add(bds40(src_v=0, src=0), commb_format=7, nav_altitude_source=0)
    add(bds40(src_v=0, src=1), commb_format=0)
    for src, want in enumerate((1, 2, 3, 4)):
        add(bds40(src=src), commb_format=7, nav_altitude_source=want)
    add(bds40(mcp=2000, fms=2001), commb_format=7, nav_mcp_altitude=32000, nav_fms_altitude=32016)  # the mcp != fms penalty
    add(bds40(mcp_v=0, mcp=0, fms_v=0, fms=0, baro_v=0, baro=0, mode_v=0, mode=0, src_v=0, src=0), commb_format=2)
    add(bds40(mcp_v=0, mcp=0, fms_v=0, fms=0, baro_v=0, baro=0, mode_v=0, mode=0, src_v=1, src=0), commb_format=7, nav_valid=0,
        nav_altitude_source=1)
    # altitude % 500 is a multiple of 4 (the altitude is one of 16): 12 | 16 and 484 | 488 are the values around the two bounds
    for raw in (157, 126, 124, 93):
        add(bds40(mcp=raw, fms_v=0, fms=0), commb_format=7, nav_mcp_altitude=raw * 16)
        add(bds40(fms=raw, mcp_v=0, mcp=0), commb_format=7, nav_fms_altitude=raw * 16)
    # BDS 5,0
    add(bds50(), commb_format=8, roll_q=57, heading_raw=650, heading_type=1, gs=400, track_rate_q=4, tas=400, tas_valid=1,
        commb_valid=7)
    add(bds50(roll=227), commb_format=8, roll_q=227)
    add(bds50(roll=228), commb_format=0)
    add(bds50(roll_bits=512 | 284), commb_format=0)  # - 90 + 284 * 45 / 256 = -40.08
    add(bds50(roll_bits=512 | 285), commb_format=8, roll_q=-227)
    add(bds50(roll_bits=512), commb_format=0)  # the sign alone: -90 degrees
    add(bds50(roll_bits=511), commb_format=0)
    add(bds50(roll_bits=1023), commb_format=8, roll_q=-1)
    for which in ("gs", "tas"):
        for raw, ok in ((0, 0), (24, 0), (25, 1), (350, 1), (351, 0), (1023, 0)):
            add(bds50(**{which: raw}), commb_format=8 if ok else 0)
            add(bds50(**{which: raw, which + "_v": 0}), commb_format=0)
    for trq, ok in ((320, 1), (321, 0), (-320, 1), (-321, 0), (511, 0), (-512, 0), (0, 1)):
        add(bds50(trq=trq, roll=0), commb_format=8 if ok else 0)
    add(bds50(tr_v=0, tr_bits=0), commb_format=8, commb_valid=3, track_rate_q=0)
    add(bds50(tr_v=0, tr_bits=4), commb_format=0)     # an invalid turn rate with a value
    add(bds50(tr_v=0, tr_bits=512), commb_format=0)   # ... with the sign alone
    for off in ("roll_v", "trk_v", "gs_v", "tas_v"):
        add(bds50(**{off: 0}), commb_format=0)
    add(bds50(trk=0), commb_format=8, heading_raw=0, heading_valid=1)
    add(bds50(trk=2047), commb_format=8, heading_raw=2047)
    add(bds50(roll=227, trq=0), commb_format=8)  # 39.9 degrees of bank without a turn: penalised, and still alone
    # BDS 6,0
    add(bds60(), commb_format=9, heading_raw=300, heading_type=3, ias=250, ias_valid=1, mach_raw=100, baro_rate=-320,
        baro_rate_valid=1, geom_rate=-320, geom_rate_valid=1, commb_valid=8)
    for raw, ok in ((0, 0), (49, 0), (50, 1), (700, 1), (701, 0), (1023, 0)):
        add(bds60(ias=raw), commb_format=9 if ok else 0)
    for raw, ok in ((0, 0), (24, 0), (25, 1), (225, 1), (226, 0), (1023, 0)):
        add(bds60(mach=raw), commb_format=9 if ok else 0)
    for which in ("br", "ir"):
        for bits, ok in ((187, 1), (188, 0), (512 | 325, 1), (512 | 324, 0), (511, 0), (512, 0), (0, 1)):  # +-5984 / +-6016 ft/min
            add(bds60(**{which + "_bits": bits, ("ir" if which == "br" else "br") + "_bits": 125 if bits < 512 else 512 | 387}),
                commb_format=9 if ok else 0)
        add(bds60(**{which + "_v": 0, which + "_bits": 0}), commb_format=9)
        add(bds60(**{which + "_v": 0, which + "_bits": 512}), commb_format=9)  # invalid with the sign alone: comm_b.c:676,694
        add(bds60(**{which + "_v": 0, which + "_bits": 1}), commb_format=0)   # invalid with a value
    add(bds60(br_v=0, br_bits=512, ir=5), commb_format=9, baro_rate_valid=0, baro_rate=0, geom_rate_valid=1, geom_rate=160)
    add(bds60(br_v=0, br_bits=0, ir_v=0, ir_bits=0), commb_format=0)
    add(bds60(br_bits=62, ir_bits=0), commb_format=9, baro_rate=1984, geom_rate=0)  # rate difference 1984: no penalty
    add(bds60(br_bits=63, ir_bits=0), commb_format=9, baro_rate=2016, geom_rate=0)  # 2016: penalised, still alone
    # ... and where the penalty decides: BDS 5,0 reads the same bits (turn-rate raw = barometric rate / 32, TAS raw = inertial
    # rate / 32).  A difference of 62 x 32 = 1984 leaves BDS 6,0 at 56, one of 63 x 32 = 2016 takes it to 44, below BDS 5,0.
    def both(roll, trq, tas):
        return bds50(roll=roll, trk=1024 | 300, gs=100, trq=trq, tas=tas)
    # 4.9 degrees of bank at 50 kt turn 1.9 degrees per second: BDS 5,0 unpenalised, 56
    add(both(28, 87, 25), commb_format=1, heading_valid=0, tas_valid=0, baro_rate_valid=0)
    add(both(28, 88, 25), commb_format=8, roll_q=28, track_rate_q=88, tas=50, gs=200, heading_raw=1324, baro_rate_valid=0)
    # wings level: BDS 5,0 penalised, 50
    add(both(0, 162, 100), commb_format=9, baro_rate=5184, geom_rate=3200, ias=300, mach_raw=100)
    add(both(0, 163, 100), commb_format=8, track_rate_q=163, tas=200, baro_rate_valid=0, geom_rate_valid=0)
    add(both(0, 38, 100), commb_format=1, baro_rate_valid=0, tas_valid=0)  # (1.2 degrees per second: unpenalised)
    add(both(0, 37, 100), commb_format=8, track_rate_q=37, tas=200)
    add(both(0, -1, 61), commb_format=1, baro_rate_valid=0, tas_valid=0)  # (hardly turning: BDS 5,0 unpenalised again)
    add(both(0, -2, 61), commb_format=8, track_rate_q=-2, tas=122)
    for off in ("hdg_v", "ias_v", "mach_v"):
        add(bds60(**{off: 0}), commb_format=0)
    add(bds60(hdg=2047), commb_format=9, heading_raw=2047)
    # BDS 1,7: every scored bit from two bases, and every reserved bit
    for base in (0, 0xFE8101, 0xFA8180):
        add(base << 32)
        for bit in range(1, 25):
            add((base ^ (1 << (24 - bit))) << 32)
    for bit in range(25, 57):
        add((0xFE8101 << 32) | (1 << (56 - bit)), commb_format=0)
    add(0xFE8101 << 32, commb_format=4)
    add(0x020000 << 32, commb_format=4)  # bit 7 alone: 1 + 1 + 1
    # ... and every scored bit where it decides commb_format.  Bit 7 (+1), not ES-capable (+1), bits 16 and 24 (+2): 4.  Each
    # "unlikely" bit takes 2 off: one leaves 2, two leave 0 and the register is no BDS 1,7 any more; bit 9 gives 1 back.
    def caps(*bits):
        return sum(1 << (56 - bit) for bit in bits)
    unlikely = (10, 11, 12, 13, 14, 20, 21, 22)
    add(caps(7, 16, 24), commb_format=4)
    for i, u in enumerate(unlikely):
        v = unlikely[(i + 1) % 8]
        add(caps(7, 16, 24, u), commb_format=4)
        add(caps(7, 16, 24, u, v), commb_format=0)
        add(caps(7, 16, 24, 9, u, v), commb_format=4)
        if u != 14:  # (bit 14 alone in front is a BDS 4,0 FMS altitude status)
            add(caps(16, 24, u), commb_format=0)  # without bit 7: -2 + 1 + 2 - 2
    add(caps(16, 24), commb_format=4)              # -2 + 1 + 2
    add(caps(7, 9), commb_format=0)                # 1 + 1 - 6: vertical intent without track and heading
    add(caps(7, 16), commb_format=0)               # 1 + 1 - 6
    add(caps(7, 24), commb_format=0)
    add(caps(1, 2, 3, 4, 5, 7, 16), commb_format=0)      # 1 + 5 - 6
    add(caps(1, 2, 3, 4, 5, 6, 7, 16), commb_format=4)   # ES EDI: + 1
    add(caps(1, 2, 3, 4, 5, 16, 24, 10, 11), commb_format=4)      # -2 + 5 + 2 - 4
    add(caps(1, 2, 3, 4, 5, 16, 24, 10, 11, 12), commb_format=0)  # ... - 6
    add(caps(1, 2, 3, 4, 7, 16, 24, 9), commb_format=0)  # partial ES: 1 - 12 + 3
    add(caps(6, 7, 16, 24, 9), commb_format=0)           # bit 6 without ES: 1 - 12 + 3
    add(0x000000 << 32, commb_format=2)
    # BDS 2,0: every position at the charset's edges
    def ident(chars, first=0x20):
        return pack(56, [(1, 8, first)] + [(9 + 6 * i, 14 + 6 * i, c) for i, c in enumerate(chars)])
    add(ident([11, 12, 13, 49, 48, 50, 51, 32]), commb_format=5, callsign=b"KLM1023 ", callsign_valid=1)
    add(ident([0] * 8), commb_format=5, callsign_valid=0)
    add(ident([11, 12, 13, 49, 48, 50, 51, 32], first=0x21), commb_format=0)
    for c in (0, 1, 26, 27, 31, 32, 33, 47, 48, 57, 58, 63):
        for where in range(8):
            chars = [2] * 8
            chars[where] = c
            add(ident(chars), commb_format=5 if c in (0, 1, 26, 32, 48, 57) else 0, callsign_valid=int(c in (1, 26, 32, 48, 57)))
    # BDS 1,0 and 3,0
    add(0x10 << 48, commb_format=3)
    add((0x10 << 48) | (1 << 47) | 0x123456789A, commb_format=3)
    for bit in range(10, 15):
        add((0x10 << 48) | (1 << (56 - bit)), commb_format=0)
    add(0x11 << 48, commb_format=0)
    add(0x30 << 48, commb_format=6)
    add((0x30 << 48) | 0xFFFFFFFFFFFF, commb_format=6)
    add(0x31 << 48, commb_format=0)
    # the empty register, ties, DR
    add(0, commb_format=2)
    add(1, commb_format=0)
    add(1 << 55, commb_format=0)
    tie = pack(56, [(1, 1, 1), (3, 11, 0), (12, 12, 1), (13, 13, 1), (14, 23, 300), (24, 24, 1), (25, 34, 100), (35, 35, 1),
                    (36, 45, 64), (46, 46, 1), (47, 56, 100)])  # wings level, 2.0 degrees per second: delta == 2.0, 56 against 56
    add(tie, commb_format=1, heading_valid=0, tas_valid=0, commb_valid=0)
    add(tie + (1 << 11), commb_format=9)  # trq 65: 2.03 degrees per second, penalised
    b.add(commb(bds40(), dr=1), commb_format=0, DR=1, nav_valid=0)
    b.add(commb(bds40(), dr=16, um=0), commb_format=0)
    b.add(commb(bds40(), dr=0, um=63), commb_format=7, UM=63)
    b.add(commb(0, dr=31), commb_format=0)
    return b.done(dtype, "Comm-B: every bound of every layout on both sides, the empty register, ties, DR")


# ---------------------------------------------------------------------------------------------------------- f. Mode A/C
def family_f(dtype):
    b = Build()
    b.add(bytes([0x06, 0x20]), squawk=0x0620, squawk_valid=1, spi=0, spi_valid=1, altitude_baro=0, altitude_baro_valid=1, source=1,
          addrtype=8, addr=0x0620 | 1 << 24)
    b.add(bytes([0x06, 0xA0]), squawk=0x0620, spi=1, altitude_baro_valid=0, altitude_baro=0, addr=0x0620 | 1 << 24)
    b.add(bytes([0x00, 0x40]), altitude_baro=-1200, altitude_baro_valid=1)
    b.add(bytes([0x00, 0x00]), altitude_baro_valid=0, squawk=0, squawk_valid=1)           # C pulses all zero
    b.add(bytes([0x00, 0x41]), altitude_baro_valid=0, squawk=0x0041)                      # D1
    b.add(bytes([0x77, 0x77]), altitude_baro_valid=0, squawk=0x7777)
    for i in range(4096):  # the twelve code pulses, one bit a Mode A reply never has, SPI
        code = (i & 0o7) | ((i & 0o70) << 1) | ((i & 0o700) << 2) | ((i & 0o7000) << 3)
        for stray in (0, 0x0800):
            for spi in (0, 0x0080):
                v = code | stray | spi
                b.add(bytes([v >> 8, v & 0xFF]))
    # the other two bits a reply never has: like 0x0800 they stay in the address (mode_ac.c:179) and nowhere else
    b.add(bytes([0x86, 0x20]), squawk=0x0620, altitude_baro=0, altitude_baro_valid=1, addr=0x8620 | 1 << 24)
    b.add(bytes([0x06, 0x28]), squawk=0x0620, altitude_baro=0, altitude_baro_valid=1, addr=0x0628 | 1 << 24)
    b.add(bytes([0x8E, 0xA8]), squawk=0x0620, spi=1, altitude_baro_valid=0, addr=0x8E28 | 1 << 24)
    for i in range(0, 4096, 37):
        code = (i & 0o7) | ((i & 0o70) << 1) | ((i & 0o700) << 2) | ((i & 0o7000) << 3)
        for stray in (0x8000, 0x0008, 0x8808):
            for spi in (0, 0x0080):
                v = code | stray | spi
                b.add(bytes([v >> 8, v & 0xFF]))
    return b.done(dtype, "Mode A/C through msgtype 32: every code with SPI and each bit a reply never has, no carry")


# ------------------------------------------------------------------------------------------- g. the turn-rate check
def turn_rate_subspace():
    """The triples (roll, TAS raw, turn-rate raw) where BDS 6,0 can read the same MB field and score 56, with the float64
    distance of the BDS 5,0 turn-rate check from its threshold: |68625 tan(roll) / (tas 20 pi) - rate| - 2.
    -> (roll_bits [455] (unsigned 0..227, then 512 + 285..511), tas_raw [n], trq [n] (the pairs, TAS raw 25..187 outermost),
    margin [455, n])."""
    roll_bits = np.concatenate([np.arange(0, 228), 512 + np.arange(285, 512)])
    roll = (roll_bits & 511) * 45.0 / 256.0
    roll = np.where(roll_bits & 512, roll.astype(np.float32).astype(np.float64) - 90.0, roll).astype(np.float32).astype(np.float64)
    pairs = [(tas, trq) for tas in range(25, 188) for trq in range(max(-187, tas - 62), min(187, tas + 62) + 1)]
    tas = np.array([p[0] for p in pairs], dtype=np.int64)
    trq = np.array([p[1] for p in pairs], dtype=np.int64)
    turn = 68625 * np.tan(roll * math.pi / 180.0)[:, None] / (tas * 2 * 20 * math.pi)[None, :]
    margin = np.abs(turn - (trq / 32.0)[None, :]) - 2.0
    return roll_bits, tas, trq, margin


G_NEAR = 1e-2
G_STRIDE = 97


def family_g(dtype):
    roll_all, tas_all, trq_all, margin = turn_rate_subspace()
    margin = margin.reshape(-1)
    total = len(margin)
    ties = margin == 0.0
    near = ~ties & (np.abs(margin) < G_NEAR)
    rest = np.flatnonzero(~ties & ~near)[::G_STRIDE]
    pick = np.concatenate([np.flatnonzero(ties), np.flatnonzero(near), rest])
    roll_bits, tas, trq = roll_all[pick // len(tas_all)], tas_all[pick % len(tas_all)], trq_all[pick % len(tas_all)]
    k = np.arange(len(pick), dtype=np.uint64)
    u = lambda a: a.astype(np.uint64)  # noqa: E731
    # BDS 5,0 layout; the bits left free make BDS 6,0 score 56: bit 12 (track status) and bit 13 (IAS status) set, bits
    # 14-23 (IAS) 50..700, bit 24 set, bits 25-34 (ground speed / Mach raw) 25..225
    mb = (u(np.ones_like(pick)) << u(np.full_like(pick, 55))) | (u(roll_bits) << np.uint64(45)) | (np.uint64(3) << np.uint64(43))
    mb |= (np.uint64(50) + k % np.uint64(651)) << np.uint64(33)
    mb |= np.uint64(1) << np.uint64(32)
    mb |= (np.uint64(25) + k % np.uint64(201)) << np.uint64(22)
    mb |= np.uint64(1) << np.uint64(21)
    mb |= u(trq & 0x3FF) << np.uint64(11)
    mb |= np.uint64(1) << np.uint64(10)
    mb |= u(tas)
    rec = np.zeros(len(pick), dtype=dtype)
    rec["msgtype"], rec["msgbits"], rec["addr"] = 20, 112, AP_ADDR
    rec["msg"][:, 0] = 20 << 3
    for j in range(7):
        rec["msg"][:, 4 + j] = ((mb >> np.uint64(8 * (6 - j))) & np.uint64(0xFF)).astype(np.uint8)
    note = {"what": "the BDS 5,0 turn-rate check where BDS 6,0 reads the same bits: ties, all within 1e-2, every 97th of the rest",
            "known": [], "total": total, "ties": int(ties.sum()), "near": int(near.sum()), "rest": len(rest),
            "penalised_total": int((margin > 0).sum()), "nearest": float(np.abs(margin[~ties]).min()),
            "within_1e-3": int((~ties & (np.abs(margin) < 1e-3)).sum()), "margin": margin[pick], "tie": ties[pick]}
    return rec, note


FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e, "f": family_f, "g": family_g}
_made = {}


def build(dtype, letter):
    """(records, note) of one family, made once per process and left unchanged"""
    if letter not in _made:
        _made[letter] = FAMILIES[letter](dtype)
        _made[letter][0].setflags(write=False)
    return _made[letter]


def random_payloads(dtype, n=20000, seed=7071):
    """random bytes behind every DF the decoder is handed, ES and Comm-B twice as often"""
    rng = np.random.default_rng(seed)
    raws = []
    dfs = [0, 4, 5, 11, 16, 17, 17, 18, 18, 20, 20, 21, 21, 24, 28, 31]
    for k in range(n):
        raw = bytearray(rng.integers(0, 256, 14, dtype=np.uint8).tobytes())
        raw[0] = (dfs[k % len(dfs)] << 3) | (raw[0] & 7)
        if raw[0] >> 3 in (20, 21) and k % 3:
            raw[1] &= 0x07  # DR = 0 for most
        raws.append(bytes(raw[:14 if raw[0] & 0x80 else 7]))
    return to_records(dtype, raws)


# ------------------------------------------------------------------- what the CPU and the GPU tests do with the families
def host_decode(pkg, records):
    """msd_decode_fields (the host build of msd_fields_impl.h) on every record, no carry"""
    import ctypes as C
    lib = pkg.capi.lib()
    records = np.ascontiguousarray(records)
    out = np.zeros(len(records), dtype=pkg.capi.FIELDS_DTYPE)
    fn = lib.msd_decode_fields
    src, dst, ss, ds = records.ctypes.data, out.ctypes.data, records.dtype.itemsize, out.dtype.itemsize
    for i in range(len(records)):
        fn(C.c_void_p(src + i * ss), None, C.c_void_p(dst + i * ds))
    return out


def host_floats(pkg, fields):
    """msd_fields_to_float on every decoded record"""
    import ctypes as C
    lib = pkg.capi.lib()
    fields = np.ascontiguousarray(fields)
    out = np.zeros(len(fields), dtype=pkg.capi.FIELDS_FLOAT_DTYPE)
    fn = lib.msd_fields_to_float
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_void_p]
    src, dst, ss, ds = fields.ctypes.data, out.ctypes.data, fields.dtype.itemsize, out.dtype.itemsize
    for i in range(len(fields)):
        fn(src + i * ss, dst + i * ds)
    return out


def oracle_decode(oracle, records):
    """orc_fields_of on every record"""
    import ctypes as C
    lib = oracle.lib()
    records = np.ascontiguousarray(records).astype(oracle.MESSAGE_DTYPE)
    out = np.zeros(len(records), dtype=oracle.FIELDS_DTYPE)
    fn = lib.orc_fields_of
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_void_p]
    src, dst, ss, ds = records.ctypes.data, out.ctypes.data, records.dtype.itemsize, out.dtype.itemsize
    for i in range(len(records)):
        fn(src + i * ss, dst + i * ds)
    return out


_read = {}


def second_reading(records, key=None):
    """indep_fields on a record array: (members, source_known, floats, detail), kept per key"""
    import indep_fields
    if key is None or key not in _read:
        detail = {}
        cols = indep_fields.read(records, detail)
        members, source_known = indep_fields.members_of(cols)
        got = (members, source_known, indep_fields.floats_of(cols), detail)
        if key is None:
            return got
        _read[key] = got
    return _read[key]


def where(records, i):
    return "record %d, msgtype %d, %s" % (i, int(records["msgtype"][i]), records["msg"][i].tobytes().hex())


def assert_members(fields, members, source_known, records, who):
    """a decoded msd_fields array against the second reading, member by member"""
    for name, want in members.items():
        got = fields[name] if name == "callsign" else fields[name].astype(np.int64)
        bad = got != want
        if name == "source":
            bad &= source_known
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError("%s: %s is %r, the second reading has %r (%d records differ; %s)"
                                 % (who, name, got[i], want[i], int(bad.sum()), where(records, i)))


def assert_same_members(a, b, names, records, who):
    for name in names:
        bad = a[name] != b[name]
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError("%s: %s %r against %r (%s)" % (who, name, a[name][i], b[name][i], where(records, i)))


def assert_floats(got, floats, records, who):
    """msd_fields_to_float's members against the second reading's, bit for bit (the rule of test_fields.assert_floats_equal)"""
    for name, want in floats.items():
        want = want.astype(got.dtype[name])
        bad = got[name].view("u%d" % got.dtype[name].itemsize) != want.view("u%d" % want.dtype.itemsize)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError("%s: %s is %r, the second reading has %r (%s)" % (who, name, got[name][i], want[i], where(records, i)))


def assert_known(fields, note, records, who):
    """the hand-typed answers"""
    for i, known in note["known"]:
        for name, want in known.items():
            got = fields[name][i]
            got = bytes(got) if name == "callsign" else int(got)
            assert got == want, "%s: %s is %r, by hand %r (%s)" % (who, name, got, want, where(records, i))


def assert_family_g(note, detail):
    """What family g must hold, on the second reading alone: the chosen set has the ties and the near ones, every non-tie
    is clear of the threshold by more than 1e-9 in float64, and both outcomes are there in numbers."""
    delta, scores = detail["delta"], detail["scores"]
    assert detail["checked"].all() and (scores[:, 7] == 56).all() and (scores[:, :6] < 50).all()
    tie = delta == 2.0
    assert note["total"] == 8382010 and int(tie.sum()) == note["ties"] >= 100
    margin = np.abs(delta - 2.0)
    assert (margin[~tie] > 1e-9).all(), float(margin[~tie].min())
    assert int((margin < G_NEAR).sum()) >= 20000
    assert np.array_equal(tie, note["tie"]) and np.array_equal(delta - 2.0 > 0, note["margin"] > 0)
    assert np.array_equal(scores[:, 6], np.where(delta > 2.0, 50, 56))
    ambiguous, unique = int((scores[:, 6] == 56).sum()), int((scores[:, 6] == 50).sum())
    assert ambiguous >= 10000 and unique >= 10000, (ambiguous, unique)
    return ambiguous, unique
