"""A second reading of the receiver range in plain Python math, written from track.c:238-308 (getBearing, greatcircle,
update_polar_range) and :683-686 (the last lines of updatePosition) alone and not from msd_pos_impl.h, on top of the second
reading of the position path (tests/indep_positions.py): per receiver the 72 buckets of the polar range, the longest
distance and the number of ranges evaluated; per aircraft a->meta.distance; the two margins of the contract in modes_hip.h
("Receiver range"), also per aircraft so that a stream builder can tell which aircraft came too close; and the
Statistics.polar_range entries as protobuf-c packs them.  math.sin / cos / acos / atan2 are the C library's.

The tracker answers the calls of capi.PositionTracker that the range tests use, so one runner drives all three."""
import math

import indep_positions as ip

BUCKETS = 72       # POLAR_RANGE_BUCKETS, stats.h:124
RESOLUTION = 5     # POLAR_RANGE_RESOLUTION, stats.h:125


def get_bearing(lat0, lon0, lat1, lon1):  # track.c:238-250
    lat0, lon0, lat1, lon1 = (v * math.pi / 180.0 for v in (lat0, lon0, lat1, lon1))
    dlon = lon1 - lon0
    x = math.cos(lat0) * math.sin(dlon)
    y = math.cos(lat1) * math.sin(lat0) - math.sin(lat1) * math.cos(lat0) * math.cos(dlon)
    return 180 / math.pi * math.atan2(x, y) + 180


def c_round(x):
    """C's round(): halves away from zero (Python's round() goes to even)."""
    return math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)


def edge_distance(bearing):
    """Degrees from `bearing` to the nearest bucket edge 2.5 + 5k."""
    k = (bearing - 2.5) / RESOLUTION
    return abs(k - c_round(k)) * RESOLUTION


class Receiver:
    def __init__(self):
        self.polar = [0] * BUCKETS
        self.longest = 0.0
        self.evaluated = 0


class RangeTracker(ip.Tracker):
    """ip.Tracker with the receiver range.  polar: --stats-range."""

    def __init__(self, receivers=None, filter_persistence=8, capacity=None, polar=True):
        super().__init__(receivers, filter_persistence or 8, capacity)
        self.polar = polar
        self.clear_range()

    def clear_range(self):
        self.range = [Receiver() for _ in self.rx]
        self.min_range_margin = self.min_bearing_margin = math.inf
        self.by_aircraft = {}  # key -> [range margin, bearing margin, gate margin], the smallest seen
        self.by_record = {}    # the same per record, counted over every update since the creation / reset
        self.key, self.record = None, -1

    # ---- the calls of capi.PositionTracker ----
    def reset(self):
        self.aircraft = {}
        self.stats = {k: 0 for k in ip.COUNTERS}
        self.margin = math.inf
        self.clear_range()

    def set_receiver(self, receiver, lat=0.0, lon=0.0, max_range_m=0.0, latlon_valid=1):
        self.rx[receiver] = dict(lat=lat, lon=lon, max_range_m=max_range_m, latlon_valid=latlon_valid)

    def range_read(self, first=0, count=None, take_longest=False):
        """-> [(72 buckets, longest_m, longest_nm, evaluated)] of receivers first .. first + count - 1."""
        count = len(self.rx) - first if count is None else count
        rows = []
        for r in self.range[first:first + count]:
            rows.append((tuple(r.polar), int(r.longest), int(r.longest / 1852.0), r.evaluated))  # net_io.c:2249-2250
            if take_longest:
                r.longest = 0.0
        return rows

    def range_distances(self):
        """One distance per live aircraft in (receiver, addr) order."""
        return [getattr(self.aircraft[k], "distance", 0) for k in sorted(self.aircraft)]

    def range_margins(self):
        return dict(min_range_margin_m=self.min_range_margin, min_bearing_margin_deg=self.min_bearing_margin)

    def snapshot_keys(self):
        return sorted(self.aircraft)

    # ---- the rule ----
    def note(self, which, value):
        if self.key is not None:
            for m in (self.by_aircraft.setdefault(self.key, [math.inf] * 3), self.by_record.setdefault(self.record, [math.inf] * 3)):
                m[which] = min(m[which], value)

    def gate(self, distance, limit):
        super().gate(distance, limit)
        self.note(2, abs(distance - limit))

    def update(self, msgs, fields, receiver=None):
        """ip.Tracker.update, keeping hold of the key and the receiver of the record in hand."""
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
            self.record += 1
            if m["msgtype"] == 32 or f["addr"] == 0:  # track.c:999-1008
                out.append((0, 0, 0, ip.NOT_TRIED, 0.0, 0.0))
                continue
            self.key = (r, int(f["addr"]) & 0x1FFFFFF)
            out.append(self.feed(self.aircraft.setdefault(self.key, ip.Aircraft()), self.rx[r], m, f))
        return out

    def update_position(self, a, rx, f, gs_valid, gs_selected):
        result, lat, lon = super().update_position(a, rx, f, gs_valid, gs_selected)
        if result >= 0:
            a.distance = 0  # :683
            if a.reliable_odd >= 1 and a.reliable_even >= 1 and int(f["source"]) == ip.ADSB:  # :684
                a.distance = self.update_polar_range(self.range[self.key[0]], rx, lat, lon)
        return result, lat, lon

    def update_polar_range(self, R, rx, lat, lon):  # track.c:281-308
        if not rx["latlon_valid"]:
            return 0
        rng = ip.greatcircle(rx["lat"], rx["lon"], lat, lon)
        R.evaluated += 1
        margin = abs(rng - c_round(rng))
        if rx["max_range_m"] != 0:
            margin = min(margin, abs(rng - rx["max_range_m"]))
        self.min_range_margin = min(self.min_range_margin, margin)
        self.note(0, margin)
        if (rng <= rx["max_range_m"] or rx["max_range_m"] == 0) and rng > R.longest:
            R.longest = rng
        if self.polar:
            bearing = get_bearing(rx["lat"], rx["lon"], lat, lon)
            margin = edge_distance(bearing) if rng >= 1 else 0.0
            self.min_bearing_margin = min(self.min_bearing_margin, margin)
            self.note(1, margin)
            bucket = int(c_round(bearing / RESOLUTION))
            if bucket >= BUCKETS:
                bucket = 0
            if R.polar[bucket] < rng:
                R.polar[bucket] = int(rng)
        return int(rng)


# ---- Statistics.polar_range (readsb.proto:271, field 6: map<uint32, uint32>) as protobuf-c's statistics__pack writes it ----
def varint(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def polar_range_pb(polar):
    """72 map entries in bucket order: tag 0x32, length, key (field 1) and value (field 2) each left out when 0."""
    out = bytearray()
    for bucket, value in enumerate(polar):
        body = (b"\x08" + varint(bucket) if bucket else b"") + (b"\x10" + varint(value) if value else b"")
        out += b"\x32" + varint(len(body)) + body
    return bytes(out)
