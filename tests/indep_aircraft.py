"""A second reading of the rest of the reference's tracker in plain Python, written from track.c and track.h and not from
msd_trk_impl.h: compute_nic / compute_rc / compute_v0_nacp / compute_v0_sil / compute_nic_rc_from_message (track.c:690-976),
trackUpdateFromMessage's stores (:1020-1378) with every data_validity record kept whole (source, updated, stale, expires and
the two intervals of :108-143), combine_validity and compare_validity (:200-228), the NIC / Rc of doGlobalCPR (:378-379),
doLocalCPR (:458-473) and updatePosition (:662-674), and trackRemoveStaleAircraft's EXPIRE list (:1520-1563).

The position path is indep_positions.Tracker's: its feed() runs first and says what updatePosition returned for the
record (anything but NOT_TRIED: the record's CPR half was accepted, :1313-1329).  Nothing of the table feeds back into it.

Values are kept the way the library delivers them (modes_hip.h, msd_aircraft): a heading is (kind, raw, ew, ns) with the
kind naming the expression of mode_s.c / comm_b.c that gives the degrees, roll / track rate / Mach / QNH / the selected
heading stay the integers the message carries.  snapshot() returns one dict per aircraft under the names of
capi.AIRCRAFT_DTYPE, in (receiver, addr) order."""
import indep_positions as ip
from indep_positions import INVALID, MLAT, TISB, ADSR, ADSB, NOT_TRIED

RELIABLE_MAX = 20  # ALTITUDE_BARO_RELIABLE_MAX, track.h:71
HEADING_INVALID, GROUND_TRACK, TRUE, MAGNETIC, MAGNETIC_OR_TRUE, TRACK_OR_HEADING = range(6)  # readsb.h:158-165
HDG_NONE, HDG_COMMB, HDG_ES19, HDG_SURFACE, HDG_VELOCITY = range(5)
AG_INVALID, AG_GROUND, AG_AIRBORNE, AG_UNCERTAIN = range(4)
SIL_INVALID, SIL_UNKNOWN = 0, 1

# F(member, stale, expire), track.c:109-142; alert, spi and emergency have no line: accept_data's ?: gives 60 / 70
INTERVALS = dict(callsign=60, altitude_baro=15, altitude_geom=60, geom_delta=60, gs=60, ias=60, tas=60, mach=60, track=60,
                 track_rate=60, roll=60, mag_heading=60, true_heading=60, baro_rate=60, geom_rate=60, squawk=15, airground=15,
                 nav_qnh=60, nav_altitude_mcp=60, nav_altitude_fms=60, nav_altitude_src=60, nav_heading=60, nav_modes=60,
                 cpr_odd=60, cpr_even=60, position=60, nic_a=60, nic_c=60, nic_baro=60, nac_p=60, nac_v=60, sil=60, gva=60,
                 sda=60, emergency=0, alert=0, spi=0)
# EXPIRE(member), track.c:1521-1553: no nac_v, emergency, alert, spi
EXPIRE = ("callsign", "altitude_baro", "altitude_geom", "geom_delta", "gs", "ias", "tas", "mach", "track", "track_rate", "roll",
          "mag_heading", "true_heading", "baro_rate", "geom_rate", "squawk", "airground", "nav_qnh", "nav_altitude_mcp",
          "nav_altitude_fms", "nav_altitude_src", "nav_heading", "nav_modes", "cpr_odd", "cpr_even", "position", "nic_a",
          "nic_c", "nic_baro", "nac_p", "sil", "gva", "sda")
POSITION_MEMBERS = ("gs", "ias", "tas", "cpr_odd", "cpr_even", "position")


def c_int(x):
    """(int) of a 64-bit unsigned value, as gcc and clang convert: the low 32 bits, two's complement."""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def c_div(a, b):
    """C's integer division: towards zero."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def compute_nic(metype, version, nic_a, nic_b, nic_c):  # track.c:690-776
    if metype in (5, 9, 20):
        return 11
    if metype in (6, 10, 21):
        return 10
    if metype == 7:
        if version == 2:
            return 9 if nic_a and not nic_c else 8
        if version == 1:
            return 9 if nic_a else 8
        return 8
    if metype == 8:
        if version == 2:
            if nic_a and nic_c:
                return 7
            if nic_a and not nic_c:
                return 6
            if not nic_a and nic_c:
                return 6
        return 0
    if metype == 11:
        if version == 2:
            return 9 if nic_a and nic_b else 8
        if version == 1:
            return 9 if nic_a else 8
        return 8
    if metype == 16:
        return 3 if nic_a and nic_b else 2
    return {12: 7, 13: 6, 14: 5, 15: 4, 17: 1}.get(metype, 0)


def compute_rc(metype, version, nic_a, nic_b, nic_c):  # track.c:778-892
    if metype in (5, 9, 20):
        return 8
    if metype in (6, 10, 21):
        return 25
    if metype == 7:
        if version == 2:
            return 75 if nic_a and not nic_c else 186
        if version == 1:
            return 75 if nic_a else 186
        return 186
    if metype == 8:
        if version == 2:
            if nic_a and nic_c:
                return 371
            if nic_a and not nic_c:
                return 556
            if not nic_a and nic_c:
                return 926
        return 0
    if metype == 11:
        if version == 2:
            return 75 if nic_a and nic_b else 186
        if version == 1:
            return 75 if nic_a else 186
        return 186
    if metype == 12:
        return 371
    if metype == 13:
        if version == 2:
            if not nic_a and nic_b:
                return 556
            if not nic_a and not nic_b:
                return 926
            if nic_a and nic_b:
                return 1112
            return 0
        if version == 1:
            return 1112 if nic_a else 926
        return 926
    if metype == 14:
        return 1852
    if metype == 15:
        return 3704
    if metype == 16:
        if version == 2:
            return 7408 if nic_a and nic_b else 14816
        if version == 1:
            return 7408 if nic_a else 14816
        return 18520
    if metype == 17:
        return 37040
    return 0


V0_NACP = {0: 0, 5: 11, 6: 10, 7: 8, 8: 0, 9: 11, 10: 10, 11: 8, 12: 7, 13: 6, 14: 5, 15: 4, 16: 1, 17: 1, 18: 0, 20: 11, 21: 10,
           22: 0}  # ED-102A table N-7, track.c:903-923
V0_SIL = {0: 0, 18: 0, 22: 0, 20: 2, 21: 2, **{k: 2 for k in range(5, 18)}}  # table N-8, track.c:935-966


def altitude_to_feet(raw, unit):  # track.c:978-987
    if unit == 1:
        return int(raw / 0.3048)
    if unit == 0:
        return raw
    return 0


class Validity(ip.Validity):
    def __init__(self, stale_s=0, expire_s=0):
        super().__init__()
        self.stale_interval, self.expire_interval = stale_s * 1000, expire_s * 1000

    def copy_from(self, o):  # `*to = *from`
        self.__dict__.update(o.__dict__)


class Aircraft(ip.Aircraft):
    def __init__(self):
        super().__init__()
        for k in POSITION_MEMBERS:  # the position members' records get their intervals too (all 60 / 70, as ip assumes)
            self.v[k].stale_interval, self.v[k].expire_interval = 60000, 70000
        for k, s in INTERVALS.items():
            if k not in self.v:
                self.v[k] = Validity(s, 70 if s else 0)
        self.addr_type = None  # the first message's (track.c:82)
        self.signal = [1e-5] * 8
        self.signal_next = 0
        self.category = 0
        self.hrd, self.tah = MAGNETIC, GROUND_TRACK
        self.heading_type = HEADING_INVALID
        self.alt_baro = self.alt_geom = self.geom_delta = self.baro_rate = self.geom_rate = 0
        self.altitude_baro_reliable = 0
        self.squawk = self.emergency = self.air_ground = self.alert = self.spi = 0
        self.track = self.mag_heading = self.true_heading = (HDG_NONE, 0, 0, 0)
        self.track_rate_q = self.roll_q = self.mach_raw = 0
        self.callsign = b""
        self.nav_altitude_mcp = self.nav_altitude_fms = self.nav_altitude_src = self.nav_modes = 0
        self.nav_heading = (0, 0)  # raw, version-2 layout
        self.nav_qnh = (0, 0)      # raw, Comm-B layout
        self.sda = self.nic_a = self.nic_c = self.nic_baro = self.nac_p = self.nac_v = self.sil = self.sil_type = self.gva = 0
        self.nic = self.rc = 0
        self.cpr_nic = {0: 0, 1: 0}  # odd flag -> cpr_even_nic / cpr_odd_nic
        self.cpr_rc = {0: 0, 1: 0}


class Tracker(ip.Tracker):
    def fresh(self, d):  # track.h:223-225
        return d.source != INVALID and self.now < d.stale

    def accept(self, d, source):  # track.c:170-196
        if self.now < d.updated:
            return False
        if source < d.source and self.now < d.stale:
            return False
        d.source, d.updated = source, self.now
        d.stale = self.now + (getattr(d, "stale_interval", 0) or 60000)
        d.expires = self.now + (getattr(d, "expire_interval", 0) or 70000)
        return True

    def compare(self, lhs, rhs):  # track.c:217-228
        if self.now < lhs.stale and lhs.source > rhs.source:
            return 1
        if self.now < rhs.stale and lhs.source < rhs.source:
            return -1
        if lhs.updated > rhs.updated:
            return 1
        if lhs.updated < rhs.updated:
            return -1
        return 0

    @staticmethod
    def combine(to, from1, from2):  # track.c:200-215
        if from1.source == INVALID:
            to.copy_from(from2)
            return
        if from2.source == INVALID:
            to.copy_from(from1)
            return
        to.source = min(from1.source, from2.source)
        to.updated = max(from1.updated, from2.updated)
        to.stale = min(from1.stale, from2.stale)
        to.expires = min(from1.expires, from2.expires)

    def update(self, msgs, fields, receiver=None):
        """-> (rows as indep_positions.Tracker.update gives them, [(nic, rc, set)] per record)"""
        keys = set(self.aircraft)
        for i in range(len(msgs)):
            if msgs["msgtype"][i] != 32 and fields["addr"][i] != 0:
                keys.add((int(receiver[i]) if receiver is not None else 0, int(fields["addr"][i]) & 0x1FFFFFF))
        if self.capacity is not None and len(keys) > self.capacity:
            raise OverflowError("ENOSPC")
        rows, nicrc = [], []
        for i in range(len(msgs)):
            m, f = msgs[i], fields[i]
            r = int(receiver[i]) if receiver is not None else 0
            if m["msgtype"] == 32 or f["addr"] == 0:  # track.c:999-1008
                rows.append((0, 0, 0, NOT_TRIED, 0.0, 0.0))
                nicrc.append((0, 0, 0))
                continue
            a = self.aircraft.setdefault((r, int(f["addr"]) & 0x1FFFFFF), Aircraft())
            row = self.feed(a, self.rx[r], m, f)
            rows.append(row)
            nicrc.append(self.feed_table(a, m, f, row[3]))
        return rows, nicrc

    def record_heading(self, f):
        """heading_valid, heading_type and the value of a record: decodeModesMessage's assignments (mode_s.c:826-853,
        :917-923; comm_b.c:485-490,623-628) in the order the field decoder's float step applies them."""
        valid, htype, value = bool(f["heading_valid"]), int(f["heading_type"]), (HDG_NONE, 0, 0, 0)
        if f["velocity_valid"]:  # gs = sqrt(ns^2 + ew^2 + 0.5) > 0 always: the ground track is always derived
            valid, htype, value = True, GROUND_TRACK, (HDG_VELOCITY, 0, int(f["ew_vel"]), int(f["ns_vel"]))
        if f["heading_valid"]:
            if int(f["commb_format"]) in (8, 9):
                value = (HDG_COMMB, int(f["heading_raw"]), 0, 0)
            elif int(f["metype"]) == 19:
                value = (HDG_ES19, int(f["heading_raw"]), 0, 0)
            else:
                value = (HDG_SURFACE, int(f["heading_raw"]), 0, 0)
        return valid, htype, value

    def feed_table(self, a, m, f, location_result):
        now, source, v = self.now, int(f["source"]), a.v
        if float(m["signalLevel"]) > 0:  # :1020-1023
            a.signal[a.signal_next] = float(m["signalLevel"])
            a.signal_next = (a.signal_next + 1) & 7
        if a.addr_type is None or int(f["addrtype"]) < a.addr_type:  # :82, :1028
            a.addr_type = int(f["addrtype"])
        # ip.Tracker.feed has stored the version of this source already (:1032-1064)
        message_version = a.version[source] if source in a.version else (
            (int(f["opstatus"]) >> 1) & 7 if int(f["opstatus"]) & 1 else 0)
        if f["category_valid"]:
            a.category = int(f["category"])
        ops = int(f["opstatus"])
        if ops & 1:
            if (ops >> 23) & 7 != HEADING_INVALID:
                a.hrd = (ops >> 23) & 7
            if (ops >> 26) & 7 != HEADING_INVALID:
                a.tah = (ops >> 26) & 7
        acc = int(f["acc_valid"])
        nac_p_valid, nac_p = bool(acc & 1), int(f["nac_p"])
        sil_type, sil = int(f["sil_type"]), int(f["sil"])
        es = int(m["msgtype"]) in (17, 18)
        if message_version == 0 and not nac_p_valid and es and int(f["metype"]) in V0_NACP:  # :1075-1081
            nac_p_valid, nac_p = True, V0_NACP[int(f["metype"])]
        if message_version == 0 and sil_type == SIL_INVALID and es and int(f["metype"]) in V0_SIL:  # :1083-1089
            sil_type, sil = SIL_UNKNOWN, V0_SIL[int(f["metype"])]

        ab = v["altitude_baro"]
        if f["altitude_baro_valid"] and (source >= ab.source or self.age(ab) > 15 * 1000):  # :1091-1151
            alt = altitude_to_feet(int(f["altitude_baro"]), int(f["altitude_baro_unit"]))
            delta = alt - a.alt_baro
            fpm, max_fpm, min_fpm = 0, 12500, -12500
            if abs(delta) >= 300:
                fpm = c_div(delta * 60 * 10, abs(c_div(c_int(self.age(ab)), 100)) + 10)
                gr, br = v["geom_rate"], v["baro_rate"]
                if self.valid(gr) and self.age(gr) < self.age(br):
                    w = min(11000, c_div(c_int(self.age(gr)), 2))
                    min_fpm, max_fpm = a.geom_rate - 1500 - w, a.geom_rate + 1500 + w
                elif self.valid(br):
                    w = min(11000, c_div(c_int(self.age(br)), 2))
                    min_fpm, max_fpm = a.baro_rate - 1500 - w, a.baro_rate + 1500 + w
                if self.valid(ab) and self.age(ab) < 30000:
                    a.altitude_baro_reliable = min(RELIABLE_MAX - (RELIABLE_MAX * self.age(ab) // 30000), a.altitude_baro_reliable)
                else:
                    a.altitude_baro_reliable = 0
            good_crc = (RELIABLE_MAX // 2 - 1) if (int(m["crc"]) == 0 and source != MLAT) else 0
            if (a.altitude_baro_reliable <= 0 or abs(delta) < 300 or (min_fpm < fpm < max_fpm)
                    or (good_crc and a.altitude_baro_reliable <= RELIABLE_MAX // 2 + 2)):
                if self.accept(ab, source):
                    a.altitude_baro_reliable = min(RELIABLE_MAX, a.altitude_baro_reliable + good_crc + 1)
                    a.alt_baro = alt
            else:
                a.altitude_baro_reliable -= good_crc + 1
                if a.altitude_baro_reliable <= 0:
                    a.altitude_baro_reliable = 0
                    ab.source = INVALID

        if f["squawk_valid"] and self.accept(v["squawk"], source):
            a.squawk = int(f["squawk"])
        if f["emergency_valid"] and self.accept(v["emergency"], source):
            a.emergency = int(f["emergency"])
        if f["altitude_geom_valid"] and self.accept(v["altitude_geom"], source):
            a.alt_geom = altitude_to_feet(int(f["altitude_geom"]), int(f["altitude_geom_unit"]))
        if f["geom_delta_valid"] and self.accept(v["geom_delta"], source):
            a.geom_delta = int(f["geom_delta"])

        hv, htype, hvalue = self.record_heading(f)
        if hv:  # :1197-1212
            a.heading_type = htype
            if a.heading_type == MAGNETIC_OR_TRUE:
                a.heading_type = a.hrd
            elif a.heading_type == TRACK_OR_HEADING:
                a.heading_type = a.tah
            if a.heading_type == GROUND_TRACK and self.accept(v["track"], source):
                a.track = hvalue
            elif a.heading_type == MAGNETIC and self.accept(v["mag_heading"], source):
                a.mag_heading = hvalue
            elif a.heading_type == TRUE and self.accept(v["true_heading"], source):
                a.true_heading = hvalue

        commb = int(f["commb_valid"])
        if commb & 4 and self.accept(v["track_rate"], source):
            a.track_rate_q = int(f["track_rate_q"])
        if commb & 1 and self.accept(v["roll"], source):
            a.roll_q = int(f["roll_q"])
        if commb & 8 and self.accept(v["mach"], source):
            a.mach_raw = int(f["mach_raw"])
        if f["baro_rate_valid"] and self.accept(v["baro_rate"], source):
            a.baro_rate = int(f["baro_rate"])
        if f["geom_rate_valid"] and self.accept(v["geom_rate"], source):
            a.geom_rate = int(f["geom_rate"])

        ag = int(f["airground"])
        if ag != AG_INVALID:  # :1249-1258
            if ag != AG_UNCERTAIN or not self.fresh(v["airground"]):
                if self.accept(v["airground"], source):
                    a.air_ground = ag
        if f["callsign_valid"] and self.accept(v["callsign"], source):
            a.callsign = bytes(f["callsign"])
        nav = int(f["nav_valid"])
        if nav & 4 and self.accept(v["nav_altitude_mcp"], source):
            a.nav_altitude_mcp = int(f["nav_mcp_altitude"])
        if nav & 8 and self.accept(v["nav_altitude_fms"], source):
            a.nav_altitude_fms = int(f["nav_fms_altitude"])
        if int(f["nav_altitude_source"]) != 0 and self.accept(v["nav_altitude_src"], source):
            a.nav_altitude_src = int(f["nav_altitude_source"])
        if nav & 2 and self.accept(v["nav_heading"], source):
            a.nav_heading = (int(f["nav_heading_raw"]), int(bool(nav & 32)))
        if nav & 1 and self.accept(v["nav_modes"], source):
            a.nav_modes |= int(f["nav_modes"])  # :1281-1298 set flags, none is cleared
        if nav & 16 and self.accept(v["nav_qnh"], source):
            a.nav_qnh = (int(f["nav_qnh_raw"]), int(bool(nav & 64)))
        if f["alert_valid"] and self.accept(v["alert"], source):
            a.alert = int(f["alert"])
        if f["spi_valid"] and self.accept(v["spi"], source):
            a.spi = int(f["spi"])

        cpr_new = bool(f["cpr_valid"]) and location_result != NOT_TRIED  # :1313-1329
        odd = int(f["cpr_odd"])
        if cpr_new:  # compute_nic_rc_from_message, :969-976
            nic_a = self.valid(v["nic_a"]) and a.nic_a
            nic_b = bool(f["nic_b_valid"]) and int(f["nic_b"])
            nic_c = self.valid(v["nic_c"]) and a.nic_c
            a.cpr_nic[odd] = compute_nic(int(f["metype"]), a.version[ADSB], nic_a, nic_b, nic_c)
            a.cpr_rc[odd] = compute_rc(int(f["metype"]), a.version[ADSB], nic_a, nic_b, nic_c)

        if acc & 32 and self.accept(v["sda"], source):
            a.sda = int(f["sda"])
        if acc & 4 and self.accept(v["nic_a"], source):
            a.nic_a = int(f["nic_a"]) & 1
        if acc & 8 and self.accept(v["nic_c"], source):
            a.nic_c = int(f["nic_c"]) & 1
        if acc & 2 and self.accept(v["nic_baro"], source):
            a.nic_baro = int(f["nic_baro"])
        if nac_p_valid and self.accept(v["nac_p"], source):
            a.nac_p = nac_p
        if f["nac_v_valid"] and self.accept(v["nac_v"], source):
            a.nac_v = int(f["nac_v"])
        if sil_type != SIL_INVALID and self.accept(v["sil"], source):  # :1355-1360
            a.sil = sil
            if a.sil_type == SIL_INVALID or sil_type != SIL_UNKNOWN:
                a.sil_type = sil_type
        if acc & 16 and self.accept(v["gva"], source):
            a.gva = int(f["gva"])
        if acc & 32 and self.accept(v["sda"], source):  # :1366, again
            a.sda = int(f["sda"])

        if (a.altitude_baro_reliable >= 3 and self.compare(ab, v["altitude_geom"]) > 0
                and self.compare(v["geom_delta"], v["altitude_geom"]) > 0):  # :1373-1378
            a.alt_geom = a.alt_baro + a.geom_delta
            self.combine(v["altitude_geom"], ab, v["geom_delta"])

        if not cpr_new or location_result < 0:
            return (0, 0, 0)
        if location_result == 0:  # doGlobalCPR :378-379
            nic, rc = min(a.cpr_nic[0], a.cpr_nic[1]), max(a.cpr_rc[0], a.cpr_rc[1])
        else:  # doLocalCPR :458-473
            nic, rc = a.cpr_nic[odd], a.cpr_rc[odd]
            if location_result == 1:
                nic, rc = min(nic, a.nic), min(rc, a.rc)
        a.nic, a.rc = nic, rc  # :667-674
        return (nic, rc, 1)

    def expire(self, now):  # track.c:1494-1570
        for key in list(self.aircraft):
            a = self.aircraft[key]
            gone = (now - a.seen) & ip.U64
            if gone > 600000 or (a.messages == 1 and gone > 60000):
                del self.aircraft[key]
                continue
            for k in EXPIRE:
                d = a.v[k]
                if d.source != INVALID and now >= d.expires:
                    d.source = INVALID
            if a.v["position"].source == INVALID:
                a.reliable_odd = a.reliable_even = 0
            if a.v["altitude_baro"].source == INVALID:
                a.altitude_baro_reliable = 0

    def snapshot(self, members):
        """members: capi.AC_MEMBERS.  -> [dict] in (receiver, addr) order."""
        out = []
        for (r, addr) in sorted(self.aircraft):
            a = self.aircraft[(r, addr)]
            g = a.v["altitude_geom"]
            d = dict(receiver=r, addr=addr, seen=a.seen, messages=a.messages, lat=a.lat, lon=a.lon, gs=a.gs, ias=a.ias,
                     tas=a.tas, pos_reliable_odd=a.reliable_odd, pos_reliable_even=a.reliable_even,
                     altitude_baro_reliable=a.altitude_baro_reliable, signal_level=list(a.signal),
                     updated=[a.v[k].updated for k in members], source=[a.v[k].source for k in members],
                     altitude_geom_stale=g.stale, altitude_geom_expires=g.expires,
                     altitude_geom_stale_15s=int(g.stale_interval == 15000), alt_baro=a.alt_baro, alt_geom=a.alt_geom,
                     geom_delta=a.geom_delta, baro_rate=a.baro_rate, geom_rate=a.geom_rate,
                     nav_altitude_mcp=a.nav_altitude_mcp, nav_altitude_fms=a.nav_altitude_fms, track=a.track,
                     mag_heading=a.mag_heading, true_heading=a.true_heading, squawk=a.squawk, mach_raw=a.mach_raw,
                     nav_qnh_raw=a.nav_qnh[0], nav_qnh_commb=a.nav_qnh[1], nav_heading_raw=a.nav_heading[0],
                     nav_heading_v2=a.nav_heading[1], rc=a.rc, cpr_odd_rc=a.cpr_rc[1], cpr_even_rc=a.cpr_rc[0],
                     roll_q=a.roll_q, track_rate_q=a.track_rate_q, callsign=a.callsign, signal_next=a.signal_next,
                     addr_type=a.addr_type, category=a.category, adsb_hrd=a.hrd, adsb_tah=a.tah, heading_type=a.heading_type,
                     air_ground=a.air_ground, emergency=a.emergency, alert=a.alert, spi=a.spi,
                     nav_altitude_src=a.nav_altitude_src, nav_modes=a.nav_modes, nic=a.nic, cpr_odd_nic=a.cpr_nic[1],
                     cpr_even_nic=a.cpr_nic[0], nic_a=a.nic_a, nic_c=a.nic_c, nic_baro=a.nic_baro, nac_p=a.nac_p,
                     nac_v=a.nac_v, sil=a.sil, sil_type=a.sil_type, gva=a.gva, sda=a.sda, adsb_version=a.version[ADSB],
                     tisb_version=a.version[TISB], adsr_version=a.version[ADSR])
            out.append(d)
        return out
