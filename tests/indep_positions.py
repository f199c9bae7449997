"""A second reading of the reference's position path in plain Python, written from cpr.c, track.c and track.h and not
from msd_pos_impl.h: struct aircraft's position members with their data_validity records kept whole (source, updated,
stale, expires), trackUpdateFromMessage's stores, updatePosition, doGlobalCPR, doLocalCPR, speed_check, greatcircle and
trackRemoveStaleAircraft.  Python floats are IEEE doubles and math.floor / math.fmod are exact, so the coordinates are
the reference's bit for bit; math.sin / cos / acos / atan2 are the C library's.  Also a CPR encoder (1090-WP-9-14 /
DO-260B A.1.7) for the tests that need positions to encode.

Records are rows of capi.MESSAGE_DTYPE / FIELDS_DTYPE; the tracker is keyed by (receiver, addr) as the library's is."""
import math

import numpy as np

INVALID, MODE_AC, MLAT, MODE_S, MODE_S_CHECKED, TISB, ADSR, ADSB = range(8)  # datasource_t, readsb.h:133-142
NOT_TRIED = -3

# cpr.c:82-143
NL_TABLE = [10.47047130, 14.82817437, 18.18626357, 21.02939493, 23.54504487, 25.82924707, 27.93898710, 29.91135686,
            31.77209708, 33.53993436, 35.22899598, 36.85025108, 38.41241892, 39.92256684, 41.38651832, 42.80914012,
            44.19454951, 45.54626723, 46.86733252, 48.16039128, 49.42776439, 50.67150166, 51.89342469, 53.09516153,
            54.27817472, 55.44378444, 56.59318756, 57.72747354, 58.84763776, 59.95459277, 61.04917774, 62.13216659,
            63.20427479, 64.26616523, 65.31845310, 66.36171008, 67.39646774, 68.42322022, 69.44242631, 70.45451075,
            71.45986473, 72.45884545, 73.45177442, 74.43893416, 75.42056257, 76.39684391, 77.36789461, 78.33374083,
            79.29428225, 80.24923213, 81.19801349, 82.13956981, 83.07199445, 83.99173563, 84.89166191, 85.75541621,
            86.53536998, 87.00000000]


def nl(lat):
    lat = abs(lat)
    for i, t in enumerate(NL_TABLE):
        if lat < t:
            return 59 - i
    return 1


def n_func(lat, fflag):
    return max(nl(lat) - (1 if fflag else 0), 1)


def dlon_func(lat, fflag, surface):
    return (90.0 if surface else 360.0) / n_func(lat, fflag)


def mod_int(a, b):
    return a % b  # Python's % is already non-negative for b > 0


def mod_double(a, b):
    r = math.fmod(a, b)
    return r + b if r < 0 else r


def _global_lon(rlat0, rlat1, lon0, lon1, fflag, surface):
    rl = rlat1 if fflag else rlat0
    ni = n_func(rl, fflag)
    m = math.floor((((lon0 * (nl(rl) - 1)) - (lon1 * nl(rl))) / 131072.0) + 0.5)
    return rl, dlon_func(rl, fflag, surface) * (mod_int(m, ni) + (lon1 if fflag else lon0) / 131072)


def decode_airborne(elat, elon, olat, olon, fflag):
    lat0, lat1, lon0, lon1 = float(elat), float(olat), float(elon), float(olon)
    j = math.floor(((59 * lat0 - 60 * lat1) / 131072) + 0.5)
    rlat0 = (360.0 / 60.0) * (mod_int(j, 60) + lat0 / 131072)
    rlat1 = (360.0 / 59.0) * (mod_int(j, 59) + lat1 / 131072)
    if rlat0 >= 270:
        rlat0 -= 360
    if rlat1 >= 270:
        rlat1 -= 360
    if rlat0 < -90 or rlat0 > 90 or rlat1 < -90 or rlat1 > 90:
        return -2, 0.0, 0.0
    if nl(rlat0) != nl(rlat1):
        return -1, 0.0, 0.0
    rlat, rlon = _global_lon(rlat0, rlat1, lon0, lon1, fflag, False)
    rlon -= math.floor((rlon + 180) / 360) * 360
    return 0, rlat, rlon


def decode_surface(reflat, reflon, elat, elon, olat, olon, fflag):
    lat0, lat1, lon0, lon1 = float(elat), float(olat), float(elon), float(olon)
    j = math.floor(((59 * lat0 - 60 * lat1) / 131072) + 0.5)
    rl = [(90.0 / 60.0) * (mod_int(j, 60) + lat0 / 131072), (90.0 / 59.0) * (mod_int(j, 59) + lat1 / 131072)]
    for k in range(2):
        if rl[k] == 0:
            if reflat < -45:
                rl[k] = -90.0
            elif reflat > 45:
                rl[k] = 90.0
        elif (rl[k] - reflat) > 45:
            rl[k] -= 90
    if rl[0] < -90 or rl[0] > 90 or rl[1] < -90 or rl[1] > 90:
        return -2, 0.0, 0.0
    if nl(rl[0]) != nl(rl[1]):
        return -1, 0.0, 0.0
    rlat, rlon = _global_lon(rl[0], rl[1], lon0, lon1, fflag, True)
    rlon += math.floor((reflon - rlon + 45) / 90) * 90
    rlon -= math.floor((rlon + 180) / 360) * 360
    return 0, rlat, rlon


def decode_relative(reflat, reflon, cprlat, cprlon, fflag, surface):
    flat, flon = cprlat / 131072.0, cprlon / 131072.0
    dlat = (90.0 if surface else 360.0) / (59.0 if fflag else 60.0)
    j = int(math.floor(reflat / dlat) + math.floor(0.5 + mod_double(reflat, dlat) / dlat - flat))
    rlat = dlat * (j + flat)
    if rlat >= 270:
        rlat -= 360
    if rlat < -90 or rlat > 90:
        return -1, 0.0, 0.0
    if abs(rlat - reflat) > (dlat / 2):
        return -1, 0.0, 0.0
    dlon = dlon_func(rlat, fflag, surface)
    m = int(math.floor(reflon / dlon) + math.floor(0.5 + mod_double(reflon, dlon) / dlon - flon))
    rlon = dlon * (m + flon)
    if rlon > 180:
        rlon -= 360
    if abs(rlon - reflon) > (dlon / 2):
        return -1, 0.0, 0.0
    return 0, rlat, rlon


def cpr_encode(lat, lon, odd, surface=False):
    """(lat, lon) in degrees -> the 17-bit YZ, XZ of an airborne (17-bit) or surface (19-bit, low 17 sent) position."""
    nb = 19 if surface else 17
    dlat = 360.0 / (59 if odd else 60)
    yz = math.floor((1 << nb) * mod_double(lat, dlat) / dlat + 0.5)
    rlat = dlat * (yz / (1 << nb) + math.floor(lat / dlat))
    dlon = 360.0 / max(nl(rlat) - (1 if odd else 0), 1)
    xz = math.floor((1 << nb) * mod_double(lon, dlon) / dlon + 0.5)
    return int(yz) & 0x1FFFF, int(xz) & 0x1FFFF


# ---------------------------------------------------------------------------------------------------------------------
def movement_v0(m):  # decodeMovementFieldV0, mode_s.c:216-236
    if m >= 125: return np.float32(0)
    if m == 124: return np.float32(180)
    if m >= 109: return np.float32(100 + (m - 109 + 0.5) * 5)
    if m >= 94: return np.float32(70 + (m - 94 + 0.5) * 2)
    if m >= 39: return np.float32(15 + (m - 39 + 0.5) * 1)
    if m >= 13: return np.float32(2 + (m - 13 + 0.5) * 0.50)
    if m >= 9: return np.float32(1 + (m - 9 + 0.5) * 0.25)
    if m >= 2: return np.float32(0.125 + (m - 2 + 0.5) * 0.125)
    return np.float32(0)


def movement_v2(m):  # decodeMovementFieldV2, mode_s.c:238-259
    if m >= 9: return movement_v0(m)
    if m >= 3: return np.float32(0.125 + (m - 3 + 0.5) * 0.875 / 6)
    if m >= 2: return np.float32(0.125 / 2)
    return np.float32(0)


class Validity:
    def __init__(self):
        self.source = INVALID
        self.updated = self.stale = self.expires = 0


class Aircraft:
    def __init__(self):
        self.seen = self.messages = 0
        self.version = {ADSB: -1, TISB: -1, ADSR: -1}
        self.v = {k: Validity() for k in ("gs", "ias", "tas", "cpr_odd", "cpr_even", "position")}
        self.gs = self.ias = self.tas = 0
        self.gs_last_pos = np.float32(0)
        self.cpr = {0: (0, 0, 0), 1: (0, 0, 0)}  # odd flag -> (type, lat, lon)
        self.reliable_odd = self.reliable_even = 0
        self.lat = self.lon = 0.0


COUNTERS = ("cpr_surface", "cpr_airborne", "cpr_global_ok", "cpr_global_bad", "cpr_global_skipped",
            "cpr_global_range_checks", "cpr_global_speed_checks", "cpr_local_ok", "cpr_local_aircraft_relative",
            "cpr_local_receiver_relative", "cpr_local_skipped", "cpr_local_range_checks", "cpr_local_speed_checks")
U64 = (1 << 64) - 1


def greatcircle(lat0, lon0, lat1, lon1):
    lat0, lon0, lat1, lon1 = (x * math.pi / 180.0 for x in (lat0, lon0, lat1, lon1))
    dlat, dlon = abs(lat1 - lat0), abs(lon1 - lon0)
    if dlat < 0.001 and dlon < 0.001:
        a = math.sin(dlat / 2) * math.sin(dlat / 2) + math.cos(lat0) * math.cos(lat1) * math.sin(dlon / 2) * math.sin(dlon / 2)
        return 6371e3 * 2 * math.atan2(math.sqrt(a), math.sqrt(1.0 - a))
    return 6371e3 * math.acos(math.sin(lat0) * math.sin(lat1) + math.cos(lat0) * math.cos(lat1) * math.cos(dlon))


class Tracker:
    """receivers: list of dicts lat, lon, latlon_valid, max_range_m (missing keys 0)."""

    def __init__(self, receivers=None, filter_persistence=8, capacity=None):
        self.rx = [{**dict(lat=0.0, lon=0.0, latlon_valid=0, max_range_m=0.0), **(r or {})} for r in (receivers or [None])]
        self.fp = filter_persistence
        self.capacity = capacity
        self.aircraft = {}
        self.stats = {k: 0 for k in COUNTERS}
        self.margin = math.inf
        self.now = 0

    # track.h:217-235
    def valid(self, d):
        return d.source != INVALID and self.now < d.expires

    def age(self, d):
        if d.source == INVALID:
            return U64
        if d.updated >= self.now:
            return 0
        return self.now - d.updated

    def accept(self, d, source):  # track.c:170-196
        if self.now < d.updated:
            return False
        if source < d.source and self.now < d.stale:
            return False
        d.source, d.updated, d.stale, d.expires = source, self.now, self.now + 60000, self.now + 70000
        return True

    def gate(self, distance, limit):
        self.margin = min(self.margin, abs(distance - limit))

    def speed_check(self, a, lat, lon, surface):  # track.c:313-369
        if not self.valid(a.v["position"]):
            return True
        elapsed = self.age(a.v["position"])
        if self.valid(a.v["gs"]):
            speed = int(max(a.gs_last_pos, np.float32(a.gs)))
            speed = int(speed + (2 * self.age(a.v["gs"]) / 1000.0))
        elif self.valid(a.v["tas"]):
            speed = a.tas * 4 // 3
        elif self.valid(a.v["ias"]):
            speed = a.ias * 2
        else:
            speed = 100 if surface else 700
        speed = speed * 4 // 3
        if surface:
            speed = min(max(speed, 20), 150)
        else:
            speed = max(speed, 200)
        rng = (0.1e3 if surface else 0.5e3) + ((elapsed + 1000.0) / 1000.0) * (speed * 1852.0 / 3600.0)
        distance = greatcircle(a.lat, a.lon, lat, lon)
        self.gate(distance, rng)
        return distance <= rng

    def global_cpr(self, a, rx, source, fflag, surface):  # track.c:371-446
        (_, elat, elon), (_, olat, olon) = a.cpr[0], a.cpr[1]
        if surface:
            if self.valid(a.v["position"]):
                ref = (a.lat, a.lon)
            elif rx["latlon_valid"]:
                ref = (rx["lat"], rx["lon"])
            else:
                return -1, 0.0, 0.0
            r, lat, lon = decode_surface(ref[0], ref[1], elat, elon, olat, olon, fflag)
        else:
            r, lat, lon = decode_airborne(elat, elon, olat, olon, fflag)
        if r < 0:
            return r, 0.0, 0.0
        if rx["max_range_m"] > 0 and rx["latlon_valid"]:
            rng = greatcircle(rx["lat"], rx["lon"], lat, lon)
            self.gate(rng, rx["max_range_m"])
            if rng > rx["max_range_m"]:
                self.stats["cpr_global_range_checks"] += 1
                return -2, lat, lon
        if self.valid(a.v["position"]) and source <= a.v["position"].source and not self.speed_check(a, lat, lon, surface):
            self.stats["cpr_global_speed_checks"] += 1
            return -2, lat, lon
        return r, lat, lon

    def local_cpr(self, a, rx, source, fflag, surface, cprlat, cprlon):  # track.c:448-542
        if ((self.now - a.v["position"].updated) & U64) < 10 * 60 * 1000:
            ref, limit, rel = (a.lat, a.lon), 1852.0 * 100, 1
        elif not surface and rx["latlon_valid"]:
            ref, rel, mr = (rx["lat"], rx["lon"]), 2, rx["max_range_m"]
            if mr == 0:
                return -1, 0.0, 0.0
            elif mr <= 1852 * 180:
                limit = mr
            elif mr < 1852 * 360:
                limit = (1852 * 360) - mr
            else:
                return -1, 0.0, 0.0
        else:
            return -1, 0.0, 0.0
        r, lat, lon = decode_relative(ref[0], ref[1], cprlat, cprlon, fflag, surface)
        if r < 0:
            return -1, 0.0, 0.0
        if limit > 0:
            rng = greatcircle(ref[0], ref[1], lat, lon)
            self.gate(rng, limit)
            if rng > limit:
                self.stats["cpr_local_range_checks"] += 1
                return -1, lat, lon
        if self.valid(a.v["position"]) and source <= a.v["position"].source and not self.speed_check(a, lat, lon, surface):
            self.stats["cpr_local_speed_checks"] += 1
            return -1, lat, lon
        return rel, lat, lon

    def update_position(self, a, rx, f, gs_valid, gs_selected):  # track.c:551-688
        surface, fflag, source = int(f["cpr_type"]) == 0, int(f["cpr_odd"]), int(f["source"])
        S = self.stats
        if surface:
            S["cpr_surface"] += 1
            max_elapsed = 50000 if (gs_valid and gs_selected <= 25) else 25000
        else:
            S["cpr_airborne"] += 1
            max_elapsed = 10000
        result, lat, lon = -1, 0.0, 0.0
        o, e = a.v["cpr_odd"], a.v["cpr_even"]
        if (self.valid(o) and self.valid(e) and o.source == e.source and a.cpr[1][0] == a.cpr[0][0]
                and abs(o.updated - e.updated) <= max_elapsed):
            result, lat, lon = self.global_cpr(a, rx, source, fflag, surface)
            if result == -2:
                S["cpr_global_bad"] += 1
                o.source = e.source = INVALID
                a.reliable_odd -= 1
                a.reliable_even -= 1
                if a.reliable_odd <= 0 or a.reliable_even <= 0:
                    a.v["position"].source = INVALID
                    a.reliable_odd = a.reliable_even = 0
                return -2, 0.0, 0.0
            elif result == -1:
                S["cpr_global_skipped"] += 1
            elif self.accept(a.v["position"], source):
                S["cpr_global_ok"] += 1
                if a.reliable_odd <= 0 or a.reliable_even <= 0:
                    a.reliable_odd = a.reliable_even = 1
                elif fflag:
                    a.reliable_odd = min(a.reliable_odd + 1, self.fp)
                else:
                    a.reliable_even = min(a.reliable_even + 1, self.fp)
                if self.valid(a.v["gs"]):
                    a.gs_last_pos = np.float32(a.gs)
            else:
                S["cpr_global_skipped"] += 1
                result = -2
        if result == -1:
            result, lat, lon = self.local_cpr(a, rx, source, fflag, surface, int(f["cpr_lat"]), int(f["cpr_lon"]))
            if result >= 0 and self.accept(a.v["position"], source):
                S["cpr_local_ok"] += 1
                if self.valid(a.v["gs"]):
                    a.gs_last_pos = np.float32(a.gs)
                if result == 1:
                    S["cpr_local_aircraft_relative"] += 1
                if result == 2:
                    S["cpr_local_receiver_relative"] += 1
            else:
                S["cpr_local_skipped"] += 1
                result = -1
        if result >= 0:
            a.lat, a.lon = lat, lon
            return result, lat, lon
        return result, 0.0, 0.0

    def update(self, msgs, fields, receiver=None):
        """-> list of (decoded, relative, surface, result, lat, lon), one per record."""
        keys = set(self.aircraft)
        for i in range(len(msgs)):
            if msgs["msgtype"][i] != 32 and fields["addr"][i] != 0:
                keys.add((int(receiver[i]) if receiver is not None else 0, int(fields["addr"][i]) & 0x1FFFFFF))
        if self.capacity is not None and len(keys) > self.capacity:
            raise OverflowError("ENOSPC")
        out = []
        for i in range(len(msgs)):
            m, f = msgs[i], fields[i]
            r = int(receiver[i]) if receiver is not None else 0
            if m["msgtype"] == 32 or f["addr"] == 0:  # track.c:999-1008
                out.append((0, 0, 0, NOT_TRIED, 0.0, 0.0))
                continue
            out.append(self.feed(self.aircraft.setdefault((r, int(f["addr"]) & 0x1FFFFFF), Aircraft()), self.rx[r], m, f))
        return out

    def feed(self, a, rx, m, f):
        self.now = int(m["sysTimestampMsg"])
        source = int(f["source"])
        a.seen = self.now
        a.messages += 1
        version = a.version.get(source, -1)  # track.c:1032-1054
        if version < 0:
            version = 0
        if int(f["opstatus"]) & 1:
            version = (int(f["opstatus"]) >> 1) & 7
        if source in a.version:
            a.version[source] = version
        gs_valid, v0, v2 = False, np.float32(0), np.float32(0)
        if f["velocity_valid"]:
            ew, ns = int(f["ew_vel"]), int(f["ns_vel"])
            gs_valid, v0 = True, np.sqrt(np.float32((ns * ns) + (ew * ew) + 0.5))
            v2 = v0
        elif f["movement"]:
            gs_valid, v0, v2 = True, movement_v0(int(f["movement"])), movement_v2(int(f["movement"]))
        elif int(f["commb_valid"]) & 2:
            gs_valid, v0 = True, np.float32(int(f["gs"]))
            v2 = v0
        gs_selected = np.float32(0)
        if gs_valid:  # track.c:1222-1227
            gs_selected = v2 if version == 2 else v0
            if self.accept(a.v["gs"], source):
                a.gs = int(gs_selected)
        if f["ias_valid"] and self.accept(a.v["ias"], source):
            a.ias = int(f["ias"])
        if f["tas_valid"] and self.accept(a.v["tas"], source):
            a.tas = int(f["tas"])
        cpr_new = False
        if f["cpr_valid"]:
            odd = int(f["cpr_odd"])
            if self.accept(a.v["cpr_odd" if odd else "cpr_even"], source):  # track.c:1313-1329
                a.cpr[odd] = (int(f["cpr_type"]), int(f["cpr_lat"]), int(f["cpr_lon"]))
                cpr_new = True
        surface = int(bool(f["cpr_valid"]) and int(f["cpr_type"]) == 0)
        if not cpr_new:
            return (0, 0, surface, NOT_TRIED, 0.0, 0.0)
        result, lat, lon = self.update_position(a, rx, f, gs_valid, gs_selected)
        if result >= 0:
            return (1, result, surface, result, lat, lon)
        return (0, 0, surface, result, 0.0, 0.0)

    def expire(self, now):  # track.c:1494-1570
        for key in list(self.aircraft):
            a = self.aircraft[key]
            gone = (now - a.seen) & U64
            if gone > 600000 or (a.messages == 1 and gone > 60000):
                del self.aircraft[key]
                continue
            for d in a.v.values():
                if d.source != INVALID and now >= d.expires:
                    d.source = INVALID
            if a.v["position"].source == INVALID:
                a.reliable_odd = a.reliable_even = 0

    def get_stats(self):
        return dict(self.stats, aircraft=len(self.aircraft), min_gate_margin_m=self.margin)
