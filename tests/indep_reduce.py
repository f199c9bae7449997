"""A second reading of readsb's reduced Beast output in plain Python, on top of indep_aircraft.Tracker and written from
track.c, mode_s.c and net_io.c, not from msd_trk_impl.h:

  accept_data's reduce_forward half (track.c:182-193): every data_validity record keeps its next_reduce_forward -- inside
  the Validity, so that combine_validity's `*to = *from` (:201-208, Validity.copy_from) carries it and its two-source
  branch (:211-214) does not;
  reduce_often, the fourth argument of each accept_data call (:617 .. :1366), by member;
  the aircraft's next_reduce_forward_DF11 (:1396-1400);
  the delivery conditions of useModesMessage (mode_s.c:2164-2172) and modesQueueOutput (net_io.c:1278-1285).

Timers start at 0 (trackCreateAircraft's calloc); trackRemoveStaleAircraft's EXPIRE leaves them alone; mm->sbs_in is never
set.  A record's verdict byte is bit 0 = mm->reduce_forward, bit 1 = a->meta.messages > 1 after the record."""
import indep_aircraft as ia
from indep_positions import NOT_TRIED

# accept_data(..., 1): track.c:617,643 position; :1133 altitude_baro; :1189 altitude_geom; :1193 geom_delta; :1205-1209 the
# three headings; :1214 track_rate; :1218 roll; :1224 gs; :1241 baro_rate; :1245 geom_rate; :1314 cpr_even; :1323 cpr_odd
REDUCE_OFTEN = frozenset(("position", "altitude_baro", "altitude_geom", "geom_delta", "track", "mag_heading", "true_heading",
                          "track_rate", "roll", "gs", "baro_rate", "geom_rate", "cpr_even", "cpr_odd"))
FORWARD, SEEN_TWICE = 1, 2


class Tracker(ia.Tracker):
    def __init__(self, receivers=None, filter_persistence=8, interval_ms=125, capacity=None):
        super().__init__(receivers, filter_persistence, capacity)
        self.interval = interval_ms
        self.cur = None       # (aircraft, message, fields) of the record being fed
        self.forward = 0      # mm->reduce_forward

    def accept(self, d, source):  # track.c:170-196, the whole of it
        if not super().accept(d, source):
            return False
        a, m, f = self.cur
        name = next(k for k, v in a.v.items() if v is d)
        if self.now > getattr(d, "next_reduce_forward", 0):  # :182; mm->sbs_in is 0
            if int(m["msgtype"]) == 17 or name in REDUCE_OFTEN:
                d.next_reduce_forward = self.now + self.interval
            else:
                d.next_reduce_forward = self.now + self.interval * 4
            if self.interval > 7000 and f["cpr_valid"]:
                d.next_reduce_forward = self.now + 7000
            self.forward = 1
        return True

    def update(self, msgs, fields, receiver=None):
        """-> (rows, [(nic, rc, set)], [verdict byte]) per record"""
        keys = set(self.aircraft)
        for i in range(len(msgs)):
            if msgs["msgtype"][i] != 32 and fields["addr"][i] != 0:
                keys.add((int(receiver[i]) if receiver is not None else 0, int(fields["addr"][i]) & 0x1FFFFFF))
        if self.capacity is not None and len(keys) > self.capacity:
            raise OverflowError("ENOSPC")
        rows, nicrc, verdict = [], [], []
        for i in range(len(msgs)):
            m, f = msgs[i], fields[i]
            r = int(receiver[i]) if receiver is not None else 0
            if m["msgtype"] == 32 or f["addr"] == 0:  # track.c:999-1008: reduce_forward stays 0, a is NULL
                rows.append((0, 0, 0, NOT_TRIED, 0.0, 0.0))
                nicrc.append((0, 0, 0))
                verdict.append(0)
                continue
            a = self.aircraft.setdefault((r, int(f["addr"]) & 0x1FFFFFF), ia.Aircraft())
            self.cur, self.forward = (a, m, f), 0
            row = self.feed(a, self.rx[r], m, f)
            rows.append(row)
            nicrc.append(self.feed_table(a, m, f, row[3]))
            if (int(m["msgtype"]) == 11 and int(m["iid"]) == 0 and int(m["correctedbits"]) == 0
                    and self.now > getattr(a, "next_reduce_forward_DF11", 0)):  # :1396-1400
                a.next_reduce_forward_DF11 = self.now + self.interval * 4
                self.forward = 1
            verdict.append((FORWARD if self.forward else 0) | (SEEN_TWICE if a.messages > 1 else 0))
        return rows, nicrc, verdict

    def timers(self, receiver, addr, members):
        """members: capi.AC_MEMBERS -> the aircraft's next_reduce_forward per member, then next_reduce_forward_DF11; None
        when there is no such aircraft"""
        a = self.aircraft.get((receiver, addr))
        if a is None:
            return None
        return [getattr(a.v[k], "next_reduce_forward", 0) for k in members] + [getattr(a, "next_reduce_forward_DF11", 0)]


def delivered(verdict, correctedbits, verbatim=False, net_only=False):
    """does the record reach beast_reduce_out?  mode_s.c:2164-2172 (a is never NULL for a record with reduce_forward),
    net_io.c:1278-1285 (no MLAT here)"""
    if not verdict & FORWARD:
        return False
    if not (verbatim or net_only or verdict & SEEN_TWICE):
        return False
    return verbatim or correctedbits < 2
