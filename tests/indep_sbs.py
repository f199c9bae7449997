"""A second reading of readsb's SBS (BaseStation) output in plain Python, on top of indep_aircraft.Tracker and written
from net_io.c:1038-1241 (modesSendSBSOutput), :1263-1270 (modesQueueOutput), mode_s.c:2164-2172 (useModesMessage) and the
decoders' heading / speed assignments (mode_s.c:826-853, :910-922, comm_b.c:485-490,575-578), not from the C of this
project.

Numbers are formatted by CPython's '%' operator, whose %f is correctly rounded like glibc's; floats are numpy.float32
where the reference's are float.  Times: the reference calls localtime_r; the caller states the zone as an offset, and a
time is ms + offset read as POSIX time, by datetime -- beyond its range (year 9999) by the Gregorian calendar's period of
146097 days = 400 years.  A negative sum prints as 0, the year modulo 10000 (the project's convention for device data).

A record's row is what the tracker hands the writer: (flags, gs_selected, geom_delta, lat, lon)."""
import datetime
import math

import numpy as np

import indep_aircraft as ia
from indep_positions import NOT_TRIED, movement_v0, movement_v2

TRACKED, SEEN_TWICE, GS_VALID, GEOM_DELTA_VALID, CPR_DECODED = 1, 2, 4, 8, 16
NON_ICAO = 1 << 24
GROUND_TRACK = 1  # heading_type_t, readsb.h:158-165
EPOCH = datetime.datetime(1970, 1, 1)
SBS_TYPES = {4: 5, 20: 5, 5: 6, 21: 6, 0: 7, 16: 7, 11: 8}


def c_int32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & (1 << 31) else x


def record_gs(f, version):
    """(gs_valid, gs.selected) of a message once track.c:1223 has chosen between gs.v0 and gs.v2"""
    if f["velocity_valid"]:  # mode_s.c:831
        ew, ns = int(f["ew_vel"]), int(f["ns_vel"])
        return True, np.sqrt(np.float32((ns * ns) + (ew * ew) + 0.5))
    if f["movement"]:        # mode_s.c:910-915
        m = int(f["movement"])
        return True, np.float32(movement_v2(m) if version == 2 else movement_v0(m))
    if int(f["commb_valid"]) & 2:  # comm_b.c:575-578
        return True, np.float32(int(f["gs"]))
    return False, np.float32(0)


class Tracker(ia.Tracker):
    """indep_aircraft.Tracker that also says what modesSendSBSOutput reads of the aircraft after each record"""

    def update_sbs(self, msgs, fields, receiver=None):
        """-> (rows, [(nic, rc, set)], [(flags, gs_selected, geom_delta, lat, lon)]) per record"""
        rows, nicrc, sbs = [], [], []
        for i in range(len(msgs)):
            m, f = msgs[i], fields[i]
            r = int(receiver[i]) if receiver is not None else 0
            if m["msgtype"] == 32 or f["addr"] == 0:  # track.c:999-1008: a is NULL, modesQueueOutput sends no SBS
                rows.append((0, 0, 0, NOT_TRIED, 0.0, 0.0))
                nicrc.append((0, 0, 0))
                sbs.append((0, np.float32(0), 0, 0.0, 0.0))
                continue
            a = self.aircraft.setdefault((r, int(f["addr"]) & 0x1FFFFFF), ia.Aircraft())
            # the version the message's source has once this message's operational status is in (track.c:1032-1072)
            source = int(f["source"])
            version = max(a.version.get(source, -1), 0)
            if int(f["opstatus"]) & 1:
                version = (int(f["opstatus"]) >> 1) & 7
            gs_valid, gs = record_gs(f, version)
            row = self.feed(a, self.rx[r], m, f)
            rows.append(row)
            nicrc.append(self.feed_table(a, m, f, row[3]))
            flags = TRACKED | (SEEN_TWICE if a.messages > 1 else 0) | (GS_VALID if gs_valid else 0)
            flags |= GEOM_DELTA_VALID if self.valid(a.v["geom_delta"]) else 0  # trackDataValid at messageNow()
            flags |= CPR_DECODED if row[0] else 0
            sbs.append((flags, gs, int(a.geom_delta), row[4], row[5]))
        return rows, nicrc, sbs


def sbs_type(msgtype, metype):  # net_io.c:1058-1096
    if msgtype in SBS_TYPES:
        return SBS_TYPES[msgtype]
    if msgtype in (17, 18):
        if 1 <= metype <= 4:
            return 1
        if 5 <= metype <= 8:
            return 2
        if 9 <= metype <= 18:
            return 3
        if metype == 19:
            return 4
    return None


def stamp(ms, utc_offset_ms):
    """fields 7-8 / 9-10 -> ('YYYY/MM/DD', 'HH:MM:SS.mmm')"""
    s = ms + utc_offset_ms
    if s >= 1 << 63:  # the sum wraps as an int64_t
        s -= 1 << 64
    s = max(s, 0)
    days, rest = divmod(s, 86400000)
    periods, days = divmod(days, 146097)
    d = EPOCH + datetime.timedelta(days=days, milliseconds=rest)
    year = (d.year + 400 * periods) % 10000
    return "%04d/%02d/%02d" % (year, d.month, d.day), "%02d:%02d:%02d.%03d" % (d.hour, d.minute, d.second, rest % 1000)


def heading(f, gs_selected):
    """(heading_valid, heading_type, heading) of the message as the decoders leave them"""
    valid, kind, value = bool(f["heading_valid"]), int(f["heading_type"]), np.float32(0)
    if f["velocity_valid"] and gs_selected > 0:  # mode_s.c:834-842
        track = np.float32(math.atan2(int(f["ew_vel"]), int(f["ns_vel"])) * 180.0 / math.pi)
        if track < 0:
            track = np.float32(track + np.float32(360))
        valid, kind, value = True, GROUND_TRACK, track
    if f["heading_valid"]:
        raw = int(f["heading_raw"])
        if int(f["commb_format"]) in (8, 9):  # comm_b.c:485-490, :623-628
            value = np.float32((raw & 1023) * 90.0 / 512.0)
            if raw & 1024:
                value = np.float32(float(value) + 180.0)
        elif int(f["metype"]) == 19:  # mode_s.c:853
            value = np.float32(raw * 360.0 / 1024.0)
        else:  # mode_s.c:922
            value = np.float32(raw * 360.0 / 128.0)
    return valid, kind, value


def line(m, f, row, verbatim=False, net_only=False, gnss=False, now_ms=0, utc_offset_ms=0, now_is_received=False):
    """The bytes one message adds to the SBS stream: b'' where useModesMessage or modesQueueOutput hold it back or
    modesSendSBSOutput returns early."""
    flags, gs_selected, geom_delta, lat, lon = row
    if not flags & TRACKED:  # a == NULL
        return b""
    if not (verbatim or net_only or flags & SEEN_TWICE):  # mode_s.c:2164-2172
        return b""
    if int(m["correctedbits"]) >= 2:  # net_io.c:1266
        return b""
    if int(f["addr"]) & NON_ICAO:  # :1043
        return b""
    kind = sbs_type(int(m["msgtype"]), int(f["metype"]))
    if kind is None:
        return b""
    out = ["MSG", "%d" % kind, "1", "1", "%06X" % (int(f["addr"]) & 0xFFFFFF), "1"]
    received = int(m["sysTimestampMsg"])
    out += stamp(received, utc_offset_ms)
    out += stamp(received if now_is_received else now_ms, utc_offset_ms)
    callsign = bytes(f["callsign"]).split(b"\0")[0].decode("latin-1") if f["callsign_valid"] else ""  # %s
    out.append(callsign)
    delta_valid = bool(flags & GEOM_DELTA_VALID)
    baro, geom = int(f["altitude_baro"]), int(f["altitude_geom"])
    if gnss:  # :1136-1146
        if f["altitude_geom_valid"]:
            out.append("%dH" % geom)
        elif f["altitude_baro_valid"] and delta_valid:
            out.append("%dH" % c_int32(baro + geom_delta))
        elif f["altitude_baro_valid"]:
            out.append("%d" % baro)
        else:
            out.append("")
    else:  # :1147-1155
        if f["altitude_baro_valid"]:
            out.append("%d" % baro)
        elif f["altitude_geom_valid"] and delta_valid:
            out.append("%d" % c_int32(geom - geom_delta))
        else:
            out.append("")
    out.append("%.0f" % float(gs_selected) if flags & GS_VALID else "")
    hv, ht, hd = heading(f, gs_selected)
    out.append("%.0f" % float(hd) if hv and ht == GROUND_TRACK else "")
    out += ["%1.5f" % lat, "%1.5f" % lon] if flags & CPR_DECODED else ["", ""]
    if gnss:  # :1179-1186
        out.append("%dH" % int(f["geom_rate"]) if f["geom_rate_valid"] else "%d" % int(f["baro_rate"]) if f["baro_rate_valid"] else "")
    else:
        out.append("%d" % int(f["baro_rate"]) if f["baro_rate_valid"] else "%d" % int(f["geom_rate"]) if f["geom_rate_valid"] else "")
    squawk = int(f["squawk"])
    out.append("%04x" % squawk if f["squawk_valid"] else "")
    out.append(("-1" if f["alert"] else "0") if f["alert_valid"] else "")
    out.append(("-1" if squawk in (0x7500, 0x7600, 0x7700) else "0") if f["squawk_valid"] else "")
    out.append(("-1" if f["spi"] else "0") if f["spi_valid"] else "")
    out.append({1: "-1", 2: "0"}.get(int(f["airground"]), ""))
    return (",".join(out) + "\r\n").encode("latin-1")


def stream(msgs, fields, rows, **kw):
    """-> (bytes, ends) over the records in order"""
    out, ends = bytearray(), np.zeros(len(msgs), dtype=np.uint32)
    for i in range(len(msgs)):
        out += line(msgs[i], fields[i], rows[i], **kw)
        ends[i] = len(out)
    return bytes(out), ends


def rows_of(trk):
    """a capi.SBS_TRACK_DTYPE array -> the rows of this module"""
    return [(int(t["flags"]), np.float32(t["gs_selected"]), int(t["geom_delta"]), float(t["lat"]), float(t["lon"])) for t in trk]
