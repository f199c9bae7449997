"""tests/indep_aircraft_pb.py extended by the one member a tracker with the receiver range adds to aircraft.pb: distance
(13), a->meta.distance as the second reading of tests/indep_range.py keeps it, written when non-zero between rssi (12) and
air_ground (15) -- the table META of indep_aircraft_pb.py has had the field all along, its reader only refused to meet it."""
import math

import indep_aircraft_pb as pb


class Writer(pb.Writer):
    def files(self, snapshot, now, distances, messages_total=None, commit=True):
        """pb.Writer.files with distances: {(receiver, addr): metres}."""
        AC = self.AC
        files, rows, margin = [], [], math.inf
        live = {(int(e["receiver"]), int(e["addr"])) for e in snapshot}
        new = {k: s for k, s in self.state.items() if k in live}
        order = sorted(range(len(snapshot)), key=lambda j: (int(snapshot[j]["receiver"]), int(snapshot[j]["addr"])))
        for r in range(self.nrx):
            entries, n_pos, n_tisb = [], 0, 0
            for j in order:
                e = snapshot[j]
                if int(e["receiver"]) != r or not pb.selected(e, now):
                    continue
                key = (r, int(e["addr"]))
                st = pb.next_state(new.get(key, (False, False, 0)), e, AC, now)
                new[key] = st
                if pb.valid(e, AC, "position", now):
                    n_pos += 1
                    n_tisb += int(e["source"][AC["position"]]) == pb.SOURCE_TISB
                margin = min(margin, pb.rssi_margin_ulps(pb.rssi_double(e)))
                entries.append((pb.META, dict(pb.meta_values(e, AC, st), distance=distances.get(key, 0))))
            files.append(pb.write(pb.UPDATE, dict(now=now // 1000, messages=0 if messages_total is None else int(messages_total[r]),
                                                  aircraft=entries)))
            rows.append((len(entries), n_pos, n_tisb))
        if commit:
            self.state = new
        return files, rows, margin


def distance_places(file_bytes):
    """The aircraft entries of one aircraft.pb -> [(addr, distance or None, the field number in front of it, behind it)]:
    where `68 <varint>` stands in each entry."""
    out, i = [], 0
    while i < len(file_bytes):
        key, i = pb.read_varint(file_bytes, i)
        if key & 7 == 0:
            _, i = pb.read_varint(file_bytes, i)
            continue
        n, i = pb.read_varint(file_bytes, i)
        body, i = file_bytes[i:i + n], i + n
        if key >> 3 != 15:
            continue
        fields, j = [], 0
        while j < len(body):
            k, j = pb.read_varint(body, j)
            start = j
            if k & 7 == 0:
                v, j = pb.read_varint(body, j)
            elif k & 7 == 1:
                v, j = None, j + 8
            elif k & 7 == 5:
                v, j = None, j + 4
            else:
                ln, j = pb.read_varint(body, j)
                v, j = None, j + ln
            fields.append((k >> 3, v, body[start - 1]))
        numbers = [f[0] for f in fields]
        addr = fields[0][1]
        if 13 in numbers:
            at = numbers.index(13)
            assert fields[at][2] == 0x68
            out.append((addr, fields[at][1], numbers[at - 1], numbers[at + 1]))
        else:
            out.append((addr, None, None, None))
    return out
