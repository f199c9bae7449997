"""A second reading of history_N.pb (modes_hip.h "history_N.pb"), independent of the C: generateHistoryProtoBuf
(net_io.c:2086-2150) and the AircraftHistory / AircraftsUpdate messages of readsb.proto, on top of the wire reader and
writer, `valid` and `selected` of tests/indep_aircraft_pb.py.

Entries are capi.AIRCRAFT_DTYPE scalars (a snapshot); AC is capi.AC, the index of a validity by its name."""
import indep_aircraft_pb as ipb

HISTORY = [(1, "u", "addr"), (5, "i", "alt_baro"), (8, "d", "lat"), (9, "d", "lon")]  # readsb.proto, AircraftHistory
INVALID_ALTITUDE = -9999          # readsb.h
SOURCE_MODE_S_CHECKED = 4         # datasource_t, readsb.h:133-142
AG_GROUND = 1                     # AircraftMeta.AirGround, readsb.proto
REFUSALS = ("messages", "seen", "position")
ALTITUDES = ("ground", "baro", "geom", "none")


def geom_valid(e, AC, now):
    """trackDataValid(&a->altitude_geom_valid): the one validity that keeps an expiry time of its own"""
    return int(e["source"][AC["altitude_geom"]]) != 0 and now < int(e["altitude_geom_expires"])


def refusal(e, AC, now):
    """None for an aircraft that is written, else the first condition of net_io.c:2115-2124 that sends it away"""
    if int(e["messages"]) < 2:
        return "messages"
    if not ipb.selected(e, now):
        return "seen"
    if not ipb.valid(e, AC, "position", now):
        return "position"
    return None


def altitude(e, AC, now):
    """-> (which arm of net_io.c:2138-2146, the value of alt_baro)"""
    if (ipb.valid(e, AC, "airground", now) and int(e["source"][AC["airground"]]) >= SOURCE_MODE_S_CHECKED
            and int(e["air_ground"]) == AG_GROUND):
        return "ground", INVALID_ALTITUDE
    if ipb.valid(e, AC, "altitude_baro", now) and int(e["altitude_baro_reliable"]) >= 3:
        return "baro", int(e["alt_baro"])
    if geom_valid(e, AC, now):
        return "geom", int(e["alt_geom"])
    return "none", 0


def entry_values(e, AC, now):
    return dict(addr=int(e["addr"]) & 0x1FFFFFF, alt_baro=altitude(e, AC, now)[1], lat=float(e["lat"]), lon=float(e["lon"]))


def entry(e, AC, now):
    """one `history` element of AircraftsUpdate: tag, length, body"""
    return ipb.write(ipb.UPDATE, dict(history=[(HISTORY, entry_values(e, AC, now))]))


def files(snapshot, AC, receivers, now, counts=None):
    """-> ([bytes per receiver], [aircraft written per receiver]).  counts: a dict that collects how often each refusal
    and each altitude arm occurred"""
    out, rows = [], []
    order = sorted(range(len(snapshot)), key=lambda j: (int(snapshot[j]["receiver"]), int(snapshot[j]["addr"])))
    for r in range(receivers):
        entries = []
        for j in order:
            e = snapshot[j]
            if int(e["receiver"]) != r:
                continue
            why = refusal(e, AC, now)
            if counts is not None:
                key = why or "alt_" + altitude(e, AC, now)[0]
                counts[key] = counts.get(key, 0) + 1
            if why is None:
                entries.append((HISTORY, entry_values(e, AC, now)))
        out.append(ipb.write(ipb.UPDATE, dict(now=now // 1000, history=entries)))
        rows.append(len(entries))
    return out, rows


def read_file(b):
    """a history_N.pb -> {now, history: [ {addr, alt_baro, lat, lon} ]}: no messages, no aircraft"""
    d = ipb.read(ipb.UPDATE, b, dict(history=(HISTORY, None)))
    assert "messages" not in d and "aircraft" not in d
    d.setdefault("history", [])
    return d
