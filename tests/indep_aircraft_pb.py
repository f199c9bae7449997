"""A second reading of aircraft.pb (modes_hip.h "aircraft.pb"), independent of the C: a protobuf wire reader and writer
in plain Python over a table of (field number, wire kind, member) read off readsb.proto, the values of an aircraft table
entry by the expressions of mode_s.c / comm_b.c / net_io.c:1977-2080, and the selection and written-state rules.

Entries are capi.AIRCRAFT_DTYPE scalars (a snapshot); AC is capi.AC, the index of a validity by its name."""
import math
import struct

import numpy as np

# wire kinds: u = uint32 / uint64 / bool varint, i = int32 / enum varint (sign-extended), f = float, d = double,
# s = string, m = sub-message
META = [(1, "u", "addr"), (2, "s", "flight"), (3, "u", "squawk"), (4, "u", "category"), (5, "i", "alt_baro"),
        (6, "i", "mag_heading"), (7, "u", "ias"), (8, "d", "lat"), (9, "d", "lon"), (10, "u", "messages"), (11, "u", "seen"),
        (12, "f", "rssi"), (13, "u", "distance"), (15, "i", "air_ground"), (20, "i", "alt_geom"), (21, "i", "baro_rate"),
        (22, "i", "geom_rate"), (23, "u", "gs"), (24, "u", "tas"), (25, "f", "mach"), (26, "i", "true_heading"),
        (27, "i", "track"), (28, "f", "track_rate"), (29, "f", "roll"), (30, "f", "nav_qnh"), (31, "i", "nav_altitude_mcp"),
        (32, "i", "nav_altitude_fms"), (33, "i", "nav_heading"), (34, "u", "nic"), (35, "u", "rc"), (36, "i", "version"),
        (37, "u", "nic_baro"), (38, "u", "nac_p"), (39, "u", "nac_v"), (40, "u", "sil"), (41, "u", "seen_pos"),
        (42, "u", "alert"), (43, "u", "spi"), (44, "u", "gva"), (45, "u", "sda"), (46, "d", "declination"),
        (47, "u", "wind_speed"), (48, "u", "wind_direction"), (100, "i", "addr_type"), (101, "i", "emergency"),
        (102, "i", "sil_type"), (150, "m", "nav_modes"), (151, "m", "valid_source")]
NAV_MODES = [(k + 1, "u", name) for k, name in enumerate(("autopilot", "vnav", "althold", "approach", "lnav", "tcas"))]
VALID_SOURCE = [(100 + k, "u", name) for k, name in enumerate(
    ("callsign", "altitude", "alt_geom", "gs", "ias", "tas", "mach", "track", "track_rate", "roll", "mag_heading",
     "true_heading", "baro_rate", "geom_rate", "squawk", "emergency", "nav_qnh", "nav_altitude_mcp", "nav_altitude_fms",
     "nav_heading", "nav_modes", "lat", "lon", "nic", "rc", "nic_baro", "nac_p", "nac_v", "sil", "sil_type", "gva", "sda",
     "wind"))]
UPDATE = [(1, "u", "now"), (2, "u", "messages"), (14, "r", "history"), (15, "r", "aircraft")]
# which validity a valid_source member repeats
SOURCE_OF = dict(callsign="callsign", altitude="altitude_baro", alt_geom="altitude_geom", gs="gs", ias="ias", tas="tas",
                 mach="mach", track="track", track_rate="track_rate", roll="roll", mag_heading="mag_heading",
                 true_heading="true_heading", baro_rate="baro_rate", geom_rate="geom_rate", squawk="squawk",
                 emergency="emergency", nav_qnh="nav_qnh", nav_altitude_mcp="nav_altitude_mcp",
                 nav_altitude_fms="nav_altitude_fms", nav_heading="nav_heading", nav_modes="nav_modes", lat="position",
                 lon="position", nic="position", rc="position", nic_baro="nic_baro", nac_p="nac_p", nac_v="nac_v", sil="sil",
                 sil_type="sil", gva="gva", sda="sda")
WIRE_TYPE = dict(u=0, i=0, d=1, s=2, m=2, r=2, f=5)
SOURCE_TISB = 5
HDG_COMMB, HDG_ES19, HDG_SURFACE, HDG_VELOCITY = 1, 2, 3, 4


# ---- the wire -------------------------------------------------------------------------------------------------------
def varint(v):
    assert 0 <= v < 1 << 64
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def write(table, values):
    """values: {member: value}; a member that is absent, None, zero or empty is not written.  A sub-message is a dict
    (written even when empty), a repeated member a list of dicts, each written with the table given as (table, dict)."""
    out = b""
    for number, kind, name in table:
        v = values.get(name)
        if v is None:
            continue
        key = varint(number << 3 | WIRE_TYPE[kind])
        if kind == "u":
            out += key + varint(int(v)) if int(v) else b""
        elif kind == "i":
            out += key + varint(int(v) & 0xFFFFFFFFFFFFFFFF) if int(v) else b""
        elif kind == "f":
            out += key + struct.pack("<f", v) if not (v == 0) else b""
        elif kind == "d":
            out += key + struct.pack("<d", v) if not (v == 0) else b""
        elif kind == "s":
            out += key + varint(len(v)) + v if len(v) else b""
        elif kind == "m":
            body = write(*v)
            out += key + varint(len(body)) + body
        else:
            for sub in v:
                body = write(*sub)
                out += key + varint(len(body)) + body
    return out


def read_varint(b, i):
    v, shift = 0, 0
    while True:
        assert i < len(b) and shift < 70, "a varint runs off its message"
        v |= (b[i] & 0x7F) << shift
        shift += 7
        i += 1
        if not b[i - 1] & 0x80:
            return v, i


def read(table, b, subtables=None):
    """-> {member: value}; checks that every field is in the table with its wire type, in ascending order, at most once
    unless repeated, and that no scalar written is zero (proto3 never writes one).  subtables: {member: table}."""
    by_number = {n: (k, name) for n, k, name in table}
    out, i, last = {}, 0, 0
    while i < len(b):
        key, i = read_varint(b, i)
        number, wt = key >> 3, key & 7
        assert number in by_number, f"field {number} is not in the message"
        kind, name = by_number[number]
        assert wt == WIRE_TYPE[kind], (name, wt)
        assert number > last or (kind == "r" and number == last), f"field {number} after {last}"
        last = number
        if wt == 0:
            v, i = read_varint(b, i)
            if kind == "i":
                assert v < 1 << 31 or v >= (1 << 64) - (1 << 31), (name, v)
                v = v - (1 << 64) if v >> 63 else v
            assert v != 0, name
        elif wt == 1:
            v, i = struct.unpack_from("<d", b, i)[0], i + 8
            assert not v == 0, name
        elif wt == 5:
            v, i = struct.unpack_from("<f", b, i)[0], i + 4
            assert not v == 0, name
        else:
            n, i = read_varint(b, i)
            assert i + n <= len(b), name
            v, i = b[i:i + n], i + n
            if kind == "s":
                assert n > 0, name
            elif subtables and name in subtables:
                v = read(subtables[name][0], v, subtables[name][1])
        if kind == "r":
            out.setdefault(name, []).append(v)
        else:
            out[name] = v
    return out


def read_file(b):
    """an aircraft.pb -> {now, messages, aircraft: [ {member: value, nav_modes: {...}, valid_source: {...}} ]}"""
    meta = (META, dict(nav_modes=(NAV_MODES, None), valid_source=(VALID_SOURCE, None)))
    d = read(UPDATE, b, dict(aircraft=meta))
    assert "history" not in d
    d.setdefault("aircraft", [])
    for a in d["aircraft"]:
        assert "valid_source" in a and not {"distance", "declination", "wind_speed", "wind_direction"} & set(a)
        assert "wind" not in a["valid_source"]
    return d


# ---- the values -----------------------------------------------------------------------------------------------------
def f32(x):
    return float(np.float32(x))


def heading_degrees(h):
    kind, raw = int(h["kind"]), int(h["raw"])
    if kind == HDG_COMMB:  # comm_b.c: BDS 5,0 / 6,0
        v = f32((raw & 1023) * 90.0 / 512.0)
        return f32(v + 180.0) if raw & 1024 else v
    if kind == HDG_ES19:
        return f32(raw * 360.0 / 1024.0)
    if kind == HDG_SURFACE:
        return f32(raw * 360.0 / 128.0)
    if kind == HDG_VELOCITY:  # mode_s.c:835-839; a pair no subtype 1 / 2 message carries writes 0
        ew, ns = int(h["ew"]), int(h["ns"])
        small = abs(ew) <= 1022 and abs(ns) <= 1022
        if not small and (ew % 4 or ns % 4 or abs(ew) > 4088 or abs(ns) > 4088):
            return 0.0
        t = f32(math.atan2(ew, ns) * 180.0 / math.pi)
        return f32(t + 360) if t < 0 else t
    return 0.0


def rssi_double(e):
    s = [float(x) for x in e["signal_level"]]
    return 10 * math.log10((s[0] + s[1] + s[2] + s[3] + s[4] + s[5] + s[6] + s[7] + 1e-5) / 8)


def rssi_margin_ulps(d):
    """the distance of the double d to the nearest midpoint of two adjacent floats, in ulps of d"""
    f = np.float32(d)
    mids = [(float(f) + float(np.nextafter(f, np.float32(s)))) / 2 for s in (-np.inf, np.inf)]
    return min(abs(d - m) for m in mids) / math.ulp(d)


def valid(e, AC, member, now):
    k = AC[member]
    return int(e["source"][k]) != 0 and now < int(e["updated"][k]) + 70000


def selected(e, now):
    return int(e["messages"]) >= 2 and not now > int(e["seen"]) + 90000


def next_state(state, e, AC, now):
    """state: (flight attached, nav_modes attached, seen_pos) -> the state after a write at now"""
    flight, nav, seen_pos = state
    flight = flight or valid(e, AC, "callsign", now)
    nav = nav or valid(e, AC, "nav_modes", now)
    if valid(e, AC, "position", now):
        seen_pos = min(((now - int(e["updated"][AC["position"]])) & 0xFFFFFFFFFFFFFFFF) // 1000, 0xFFFFFFFF)
    return (flight, nav, seen_pos)


def meta_values(e, AC, state):
    def was_set(member):
        return int(e["updated"][AC[member]]) != 0 or int(e["source"][AC[member]]) != 0

    flight, nav, seen_pos = state
    v = {k: int(e[k]) for k in ("addr", "squawk", "category", "alt_baro", "ias", "messages", "seen", "air_ground", "alt_geom",
                                "baro_rate", "geom_rate", "gs", "tas", "nav_altitude_mcp", "nav_altitude_fms", "nic", "rc",
                                "nic_baro", "nac_p", "nac_v", "sil", "gva", "sda", "addr_type", "emergency", "sil_type")}
    v["lat"], v["lon"] = float(e["lat"]), float(e["lon"])
    v["alert"], v["spi"] = int(e["alert"]) != 0, int(e["spi"]) != 0
    v["version"] = max(int(e["adsb_version"]), 0)
    v["rssi"] = f32(rssi_double(e))
    for k in ("mag_heading", "true_heading", "track"):
        v[k] = int(heading_degrees(e[k]))
    if was_set("mach"):
        v["mach"] = f32(int(e["mach_raw"]) * 2.048 / 512)
    if was_set("track_rate"):
        q = int(e["track_rate_q"])
        r = f32((q & 511) * 8.0 / 256.0)
        v["track_rate"] = f32(r - 16) if q < 0 else r
    if was_set("roll"):
        q = int(e["roll_q"])
        r = f32((q & 511) * 45.0 / 256.0)
        v["roll"] = f32(r - 90.0) if q < 0 else r
    if was_set("nav_qnh"):
        raw = int(e["nav_qnh_raw"])
        v["nav_qnh"] = f32(800 + raw * 0.1) if int(e["nav_qnh_commb"]) else f32(800.0 + (raw - 1) * 0.8)
    if was_set("nav_heading"):
        raw = int(e["nav_heading_raw"])
        v["nav_heading"] = int(f32(raw * 180.0 / 256.0)) if int(e["nav_heading_v2"]) else raw
    if flight:
        v["flight"] = e["callsign"].tobytes().split(b"\0")[0][:8]
    if nav:
        v["nav_modes"] = (NAV_MODES, {name: (int(e["nav_modes"]) >> (n - 1)) & 1 for n, _, name in NAV_MODES})
    v["seen_pos"] = seen_pos
    v["valid_source"] = (VALID_SOURCE, {name: int(e["source"][AC[SOURCE_OF[name]]]) for _, _, name in VALID_SOURCE
                                        if name in SOURCE_OF})
    return v


class Writer:
    """generateAircraftProtoBuf once per call over a snapshot, per receiver; keeps the written state per aircraft."""

    def __init__(self, AC, receivers):
        self.AC, self.nrx, self.state = AC, receivers, {}

    def files(self, snapshot, now, messages_total=None, commit=True):
        """-> ([bytes per receiver], [(aircraft, with_positions, tisb_positions) per receiver], smallest rssi margin)"""
        AC = self.AC
        files, rows, margin = [], [], math.inf
        live = {(int(e["receiver"]), int(e["addr"])) for e in snapshot}
        new = {k: s for k, s in self.state.items() if k in live}  # the state goes with the aircraft
        order = sorted(range(len(snapshot)), key=lambda j: (int(snapshot[j]["receiver"]), int(snapshot[j]["addr"])))
        for r in range(self.nrx):
            entries, n_pos, n_tisb = [], 0, 0
            for j in order:
                e = snapshot[j]
                if int(e["receiver"]) != r or not selected(e, now):
                    continue
                key = (r, int(e["addr"]))
                st = next_state(new.get(key, (False, False, 0)), e, AC, now)
                new[key] = st
                if valid(e, AC, "position", now):
                    n_pos += 1
                    n_tisb += int(e["source"][AC["position"]]) == SOURCE_TISB
                margin = min(margin, rssi_margin_ulps(rssi_double(e)))
                entries.append((META, meta_values(e, AC, st)))
            files.append(write(UPDATE, dict(now=now // 1000, messages=0 if messages_total is None else int(messages_total[r]),
                                            aircraft=entries)))
            rows.append((len(entries), n_pos, n_tisb))
        if commit:
            self.state = new
        return files, rows, margin
