"""A second reading of generateVRS (net_io.c:3230-3377) and jsonEscapeString (:1786-1805) in Python, over msd_aircraft
snapshot rows: what the VRS tests hold the host object against.  Nothing here calls the library.  Numbers are printed with
Python's '%f' % and '%.2f' %, which round the exact binary value correctly, as glibc's printf does; '%.0f' likewise.
The one deliberate difference from the reference is the order -- ascending address within a receiver (modes_hip.h)."""
import math

import numpy as np

import indep_aircraft_pb as ipb

NON_ICAO = 1 << 24
BUCKETS = 2048  # AIRCRAFTS_BUCKETS
SOURCE_MLAT, SOURCE_MODE_S_CHECKED, SOURCE_TISB = 2, 4, 5
AG_GROUND = 1
HEAD, TAIL = b'{"acList":[', b']}\n'


def f32(x):
    return float(np.float32(x))


def valid(e, AC, member, now):
    """trackDataValid at _messageNow = now; altitude_geom keeps its own expiry (combine_validity)"""
    k = AC[member]
    if int(e["source"][k]) == 0:
        return False
    if member == "altitude_geom":
        return now < int(e["altitude_geom_expires"])
    return now < int(e["updated"][k]) + 70000


def part_of(addr, n_parts):
    """the part whose buckets hold addr: buckets part * (2048 / n_parts) up to the next part's start"""
    return (addr % BUCKETS) // (BUCKETS // n_parts)


def selected(e, now, part, n_parts):
    addr = int(e["addr"])
    if part_of(addr, n_parts) != part or int(e["messages"]) < 2:
        return False
    if float((now - int(e["seen"])) & 0xFFFFFFFFFFFFFFFF) > 5E3:  # uint64 arithmetic, compared as a double
        return False
    return not addr & NON_ICAO


def escape(callsign):
    out = ""
    for ch in callsign.tobytes().split(b"\0")[0][:8]:
        if ch in (0x22, 0x5C):
            out += "\\" + chr(ch)
        elif ch < 32 or ch > 127:
            out += "\\u%04x" % ch
        else:
            out += chr(ch)
    return out


def sig(e):
    s = [float(x) for x in e["signal_level"]]
    v = 255 * ((s[0] + s[1] + s[2] + s[3] + s[4] + s[5] + s[6] + s[7] + 1e-5) / 8)
    if math.copysign(1.0, v) < 0 or not v < 4294967296.0:  # modes_hip.h: what no decoder delivers is written as 0
        v = 0.0
    return "%.0f" % v


def c_int(v):
    """%d of a uint32_t"""
    return v - (1 << 32) if v >= 1 << 31 else v


def nav_qnh(e):
    raw = int(e["nav_qnh_raw"])
    return f32(800 + raw * 0.1) if int(e["nav_qnh_commb"]) else f32(800.0 + (raw - 1) * 0.8)


def nav_heading(e):
    raw = int(e["nav_heading_raw"])
    return int(f32(raw * 180.0 / 256.0)) if int(e["nav_heading_v2"]) else raw


def aircraft_object(e, AC, now):
    def ok(member):
        return valid(e, AC, member, now)

    p = '{"Sig":' + sig(e)
    p += ',"Icao":"%06X"' % (int(e["addr"]) & 0xFFFFFF)
    if ok("altitude_baro") and int(e["altitude_baro_reliable"]) >= 3:
        p += ',"Alt":%d' % int(e["alt_baro"])
    if ok("altitude_geom"):
        p += ',"GAlt":%d' % int(e["alt_geom"])
    if ok("nav_qnh"):
        p += ',"InHg":%.2f' % (nav_qnh(e) * 0.02952998307)
    if ok("nav_altitude_mcp"):
        p += ',"TAlt":%d' % int(e["nav_altitude_mcp"])
    elif ok("nav_altitude_fms"):
        p += ',"TAlt":%d' % int(e["nav_altitude_fms"])
    if ok("callsign"):
        p += ',"Call":"%s"' % escape(e["callsign"])
    lat, lon = float(e["lat"]), float(e["lon"])
    if ok("position") and abs(lat) <= 360.0 and abs(lon) <= 360.0:  # modes_hip.h: else the three keys are left out
        p += ',"Lat":%f,"Long":%f' % (lat, lon)
        p += ',"PosTime":%d' % int(e["updated"][AC["position"]])
    src = int(e["source"][AC["position"]])
    p += ',"Mlat":true' if src == SOURCE_MLAT else ',"Mlat":false'
    p += ',"Tisb":true' if src == SOURCE_TISB else ',"Tisb":false'
    if ok("gs"):
        p += ',"Spd":%d,"SpdTyp":0' % c_int(int(e["gs"]))
    elif ok("ias"):
        p += ',"Spd":%d,"SpdTyp":2' % int(e["ias"])
    elif ok("tas"):
        p += ',"Spd":%d,"SpdTyp":3' % int(e["tas"])
    if ok("track"):
        p += ',"Trak":%d,"TrkH":false' % int(ipb.heading_degrees(e["track"]))
    elif ok("mag_heading"):
        p += ',"Trak":%d,"TrkH":true' % int(ipb.heading_degrees(e["mag_heading"]))
    elif ok("true_heading"):
        p += ',"Trak":%d,"TrkH":true' % int(ipb.heading_degrees(e["true_heading"]))
    if ok("nav_heading"):
        p += ',"TTrk":%d' % nav_heading(e)
    if ok("squawk"):
        p += ',"Sqk":"%04x"' % int(e["squawk"])
    if ok("geom_rate"):
        p += ',"Vsi":%d,"VsiT":1' % int(e["geom_rate"])
    elif ok("baro_rate"):
        p += ',"Vsi":%d,"VsiT":0' % int(e["baro_rate"])
    if ok("airground") and int(e["source"][AC["airground"]]) >= SOURCE_MODE_S_CHECKED and int(e["air_ground"]) == AG_GROUND:
        p += ',"Gnd":true'
    else:
        p += ',"Gnd":false'
    v = int(e["adsb_version"])
    p += ',"Trt":%d' % (v + 3 if v >= 0 else 1)
    p += ',"Cmsgs":%d' % int(e["messages"])
    return p + "}"


def documents(snapshot, AC, receivers, now, part=0, n_parts=1):
    """-> ([bytes per receiver], [aircraft written per receiver])"""
    docs, counts = [], []
    order = sorted(range(len(snapshot)), key=lambda j: (int(snapshot[j]["receiver"]), int(snapshot[j]["addr"])))
    for r in range(receivers):
        objs = [aircraft_object(snapshot[j], AC, now) for j in order
                if int(snapshot[j]["receiver"]) == r and selected(snapshot[j], now, part, n_parts)]
        docs.append(HEAD + ",".join(objs).encode("latin-1") + TAIL)
        counts.append(len(objs))
    return docs, counts
