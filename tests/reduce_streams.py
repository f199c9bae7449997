"""Constructed record streams for the tests of the reduced Beast output (test_reduce_model.py on the CPU,
test_gpu_reduce.py on the GPU): one small hand-derived scenario per rule of accept_data's reduce_forward half
(track.c:182-193, :1396-1400) and of the delivery conditions (mode_s.c:2164-2172, net_io.c:1278-1285), the aircraft
table's mixed stream cut into steps with an expiry every second, and runners for the three implementations (the GPU
object, the host twin, the second reading of tests/indep_reduce.py).

A scenario is a dict:
  receivers, interval (ms), capacity, steps -- ("update", msgs, fields, receiver) or ("expire", now_ms);
  verdicts -- the expected verdict byte of every record of the update steps in order, derived by hand:
              F = mm->reduce_forward, S = the aircraft's messages > 1 after the record;
  timers   -- {(receiver, addr): {member or "df11": next_reduce_forward}} after the last step, derived by hand: the timers
              that moved.  Every timer not named is 0; an aircraft mapped to None has left the table;
  wire     -- (optional) {(verbatim, net_only): [indices of the records that get bytes]}.
In the comments T is T0, I the interval, and `x -> t` says that member x's timer becomes t."""
import numpy as np

import aircraft_streams as acs
import indep_aircraft as ia
import indep_positions as ip
import indep_reduce as ir
import pos_streams as ps

T0 = ps.T0
S4 = ip.MODE_S_CHECKED
F, S = ir.FORWARD, ir.SEEN_TWICE
# ME types that compute_v0_nacp / compute_v0_sil (track.c:897-967) leave alone: a DF17 / DF18 record with another one has
# nac_p and sil accepted besides what it carries
ME_VELOCITY, ME_STATUS = 19, 28


class Builder(acs.Builder):
    def rec(self, t, addr, msg=None, **kw):
        """msg: members of the msd_message (iid, correctedbits, ...) besides those acs.Builder sets"""
        super().rec(t, addr, **kw)
        m = self.m[-1]
        m["msg"] = [(addr >> 16) & 0xFF, (addr >> 8) & 0xFF, addr & 0xFF] + [(7 * len(self.m) + 13 * k) & 0xFF for k in range(11)]
        m["timestampMsg"], m["signalLevel"] = 12000 * (t % 1000000) + len(self.m), 0.01 + 0.001 * (len(self.m) % 50)
        for k, v in (msg or {}).items():
            m[k] = v
        return self

    def squawk5(self, t, addr, **kw):
        """a DF5 identity reply: squawk, reduce_often 0"""
        return self.rec(t, addr, source=S4, msgtype=5, crc=0x123456, squawk_valid=1, squawk=0x1200, **kw)

    def df11(self, t, addr, iid=0, correctedbits=0, **kw):
        return self.rec(t, addr, source=ip.MODE_S, msgtype=11, crc=iid, msg=dict(iid=iid, correctedbits=correctedbits, msgbits=56), **kw)


NAMES = ["first_at_clock_zero", "df17_interval", "df5_squawk", "df4_altitude", "df18_members", "interval_8000",
         "refused_member", "one_due_one_not", "df11_own_timer", "df11_airground", "combine_validity", "expiry_rebuild_chain",
         "removed_and_seen_again", "two_receivers", "modeac_and_addr0", "seen_twice_bit", "corrected_two_bits"]


def scenarios(pkg):
    out = {}
    B = lambda: Builder(pkg)  # noqa: E731
    T = T0

    def add(name, steps, verdicts, timers, interval=125, receivers=None, capacity=1024, wire=None):
        out[name] = dict(receivers=receivers or [None], interval=interval, capacity=capacity, steps=steps, verdicts=verdicts,
                         timers=timers, wire=wire)

    # messageNow() > next_reduce_forward is strict and the timers start at 0: a first message at clock 0 is not
    # forwarded (0 > 0), at clock 1 it is (squawk -> 1 + 4 I)
    b = B().squawk5(0, 0x100001).squawk5(1, 0x100002)
    add("first_at_clock_zero", [b.step()], [0, F], {(0, 0x100001): {}, (0, 0x100002): {"squawk": 501}})

    # DF17: every member at I.  A velocity squitter is gs and track: T yes (-> T + 125), T + 125 no, T + 126 yes
    b = B().vel(T, 0x110001, 100, 100).vel(T + 125, 0x110001, 100, 100).vel(T + 126, 0x110001, 100, 100)
    add("df17_interval", [b.step()], [F, S, F | S], {(0, 0x110001): {"gs": T + 251, "track": T + 251}})

    # a DF5 squawk: reduce_often 0 and not DF17, 4 I
    b = B().squawk5(T, 0x120001).squawk5(T + 500, 0x120001).squawk5(T + 501, 0x120001)
    add("df5_squawk", [b.step()], [F, S, F | S], {(0, 0x120001): {"squawk": T + 1001}})

    # a DF4 altitude: reduce_often 1, I
    b = B().alt(T, 0x130001, 10000).alt(T + 125, 0x130001, 10000).alt(T + 126, 0x130001, 10000)
    add("df4_altitude", [b.step()], [F, S, F | S], {(0, 0x130001): {"altitude_baro": T + 251}})

    # DF18 is not DF17: baro_rate (reduce_often 1) at I, nac_v (0) at 4 I.  T both (rate -> T + 125, nac_v -> T + 500);
    # T + 126 the rate alone: due (-> T + 251); T + 127 nac_v alone: not due; T + 501 nac_v alone: due
    kw = dict(msgtype=18, metype=ME_VELOCITY)
    b = B().rec(T, 0x140001, baro_rate_valid=1, baro_rate=640, nac_v_valid=1, nac_v=2, **kw)
    b.rec(T + 126, 0x140001, baro_rate_valid=1, baro_rate=640, **kw).rec(T + 127, 0x140001, nac_v_valid=1, nac_v=2, **kw)
    b.rec(T + 501, 0x140001, nac_v_valid=1, nac_v=2, **kw)
    add("df18_members", [b.step()], [F, F | S, S, F | S], {(0, 0x140001): {"baro_rate": T + 251, "nac_v": T + 1001}})

    # I = 8000.  A position squitter (an even half each time, so nothing decodes; ME type 11 and version 0: nac_p and sil
    # are accepted too) has every timer at now + 7000: due again at + 7001, not at + 7000.  A velocity squitter without
    # CPR: 8000.  A DF4 with the flight status' alert bit alone (reduce_often 0): 32000
    b = B()
    b.pos(T, 0x150001, 50.0, 8.0, 0).vel(T, 0x150002, 100, 100).rec(T, 0x150003, source=S4, msgtype=4, crc=0x123456, alert_valid=1)
    b.pos(T + 7000, 0x150001, 50.0, 8.0, 0).pos(T + 7001, 0x150001, 50.0, 8.0, 0)
    b.vel(T + 8000, 0x150002, 100, 100).vel(T + 8001, 0x150002, 100, 100)
    for dt in (32000, 32001):
        b.rec(T + dt, 0x150003, source=S4, msgtype=4, crc=0x123456, alert_valid=1)
    add("interval_8000", [b.step()], [F, F, F, S, F | S, S, F | S, S, F | S],
        {(0, 0x150001): {"cpr_even": T + 14001, "nac_p": T + 14001, "sil": T + 14001},
         (0, 0x150002): {"gs": T + 16001, "track": T + 16001}, (0, 0x150003): {"alert": T + 64001}}, interval=8000)

    # a refused member makes no verdict and moves no timer.  A: an ADS-B squawk at T (-> T + 125), a Mode S squawk 1 s
    # later -- the timer is due, but ADS-B is fresh for 15 s and the lesser source is refused.  B: a squawk at T + 1000,
    # one with the older timestamp T + 500 is refused by `updated`
    st = dict(metype=ME_STATUS, squawk_valid=1, squawk=0x1200)
    b = B().rec(T, 0x160001, **st).squawk5(T + 1000, 0x160001).rec(T + 1000, 0x160002, **st).rec(T + 500, 0x160002, **st)
    add("refused_member", [b.step()], [F, S, F, S], {(0, 0x160001): {"squawk": T + 125}, (0, 0x160002): {"squawk": T + 1125}})

    # one member due, one not: forwarded, and only the due one's timer moves.  T: rate -> T + 125, nac_v -> T + 500.
    # T + 200 both: the rate is due (-> T + 325), nac_v is not and stays: nac_v alone at T + 501 is due -- had its timer
    # moved at T + 200 it would be T + 700
    kw = dict(msgtype=18, metype=ME_VELOCITY)
    b = B()
    for dt in (0, 200):
        b.rec(T + dt, 0x170001, baro_rate_valid=1, baro_rate=640, nac_v_valid=1, nac_v=2, **kw)
    b.rec(T + 501, 0x170001, nac_v_valid=1, nac_v=2, **kw)
    add("one_due_one_not", [b.step()], [F, F | S, F | S], {(0, 0x170001): {"baro_rate": T + 325, "nac_v": T + 1001}})

    # a DF11 brings no member; with IID 0 and no repaired bit the aircraft's own timer forwards it, at 4 I.  Not with
    # IID 5, not with one repaired bit
    b = B()
    for dt in (0, 500, 501):
        b.df11(T + dt, 0x180001)
    b.df11(T, 0x180002, iid=5).df11(T + 501, 0x180002, iid=5).df11(T, 0x180003, correctedbits=1).df11(T + 501, 0x180003, correctedbits=1)
    add("df11_own_timer", [b.step()], [F, S, F | S, 0, S, 0, S],
        {(0, 0x180001): {"df11": T + 1001}, (0, 0x180002): {}, (0, 0x180003): {}})

    # a DF11 that cannot use its own timer (IID 3) is forwarded through the air / ground state its CA field brought
    b = B()
    for dt in (0, 500, 501):
        b.df11(T + dt, 0x190001, iid=3, airground=ia.AG_GROUND)
    add("df11_airground", [b.step()], [F, S, F | S], {(0, 0x190001): {"airground": T + 1001}})

    # combine_validity (:200-215) and altitude_geom's timer.  The derived altitude needs altitude_baro_reliable >= 3:
    # three DF4 altitudes, each due (126 ms apart).  The branch for an invalid altitude_baro cannot be reached: whatever
    # clears its source clears altitude_baro_reliable.
    # B, both sources valid: delta at T (-> T + 125); altitudes at T + 1, + 127, + 253 (baro -> T + 378); the third derives
    # the geometric altitude from both and leaves its timer at 0: a geometric altitude at T + 260 is due (-> T + 385) --
    # with baro's timer copied it would not be.
    # A, geom_delta expired: delta at T and T + 10, expiry at T + 70010; altitudes at T + 80000, + 80126, + 80252
    # (baro -> T + 80377); the third copies baro's validity whole, timer included: a geometric altitude at T + 80300 is
    # accepted (ADS-B over Mode S) and not due -- with its own timer of 0 it would be
    sq = dict(metype=ME_VELOCITY)
    b = B().rec(T, 0x1A0001, geom_delta_valid=1, geom_delta=250, **sq).rec(T + 10, 0x1A0001, geom_delta_valid=1, geom_delta=250, **sq)
    b.rec(T, 0x1A0002, geom_delta_valid=1, geom_delta=250, **sq)
    for dt in (1, 127, 253):
        b.alt(T + dt, 0x1A0002, 10000)
    b.rec(T + 260, 0x1A0002, altitude_geom_valid=1, altitude_geom=9000, **sq)
    first = b.step()
    for dt in (80000, 80126, 80252):
        b.alt(T + dt, 0x1A0001, 10000)
    b.rec(T + 80300, 0x1A0001, altitude_geom_valid=1, altitude_geom=9000, **sq)
    add("combine_validity", [first, ("expire", T + 70010), b.step()], [F, S, F, F | S, F | S, F | S, F | S, F | S, F | S, F | S, S],
        {(0, 0x1A0001): {"geom_delta": T + 125, "altitude_baro": T + 80377, "altitude_geom": T + 80377},
         (0, 0x1A0002): {"geom_delta": T + 125, "altitude_baro": T + 378, "altitude_geom": T + 385}})

    # the timers move with the slot when the expiry rebuilds the table: pos_streams.chain_addresses' five aircraft in one
    # probe chain of a 64-slot table, I = 15000 (a DF5 squawk: 60000).  All at T (-> T + 60000); 0, 2, 4 again at
    # T + 61000 (due, -> T + 121000); the expiry at T + 61001 removes 1 and 3 from the middle of the chain and moves the
    # others; at T + 61002 they are not due -- a survivor with timers of 0, or its neighbour's, would be
    addrs = ps.chain_addresses(pkg, 64)
    b = B()
    for j in range(5):
        b.squawk5(T, addrs[j])
    for j in (0, 2, 4):
        b.squawk5(T + 61000, addrs[j])
    first = b.step()
    for j in (0, 2, 4):
        b.squawk5(T + 61002, addrs[j])
    add("expiry_rebuild_chain", [first, ("expire", T + 61001), b.step()], [F] * 5 + [F | S] * 3 + [S] * 3,
        {(0, addrs[j]): ({"squawk": T + 121000} if j in (0, 2, 4) else None) for j in range(5)}, interval=15000, capacity=64)

    # an aircraft that was removed and is seen again starts at 0, in whichever of the two tables its slot is.  I = 15000:
    # a squawk at T (-> T + 60000); heard once, the expiry at T + 60001 removes it.  A record with the older timestamp
    # T + 100 makes a new aircraft: due (-> T + 60100), first message.  Removed at T + 70000, the table is rebuilt into
    # the first one, where the slot's timer of the first life still stands; the aircraft of T + 200 must not find it
    b = B().squawk5(T, 0x1C0001)
    one = b.step()
    two = b.squawk5(T + 100, 0x1C0001).step()
    three = b.squawk5(T + 200, 0x1C0001).step()
    add("removed_and_seen_again", [one, ("expire", T + 60001), two, ("expire", T + 70000), three], [F, F, F],
        {(0, 0x1C0001): {"squawk": T + 60200}}, interval=15000)

    # the same address on two receivers is two aircraft with timers of their own
    b = B().squawk5(T, 0x1D0001, rx=0).squawk5(T + 1, 0x1D0001, rx=1).squawk5(T + 2, 0x1D0001, rx=0).squawk5(T + 502, 0x1D0001, rx=1)
    add("two_receivers", [b.step()], [F, F, S, F | S], {(0, 0x1D0001): {"squawk": T + 500}, (1, 0x1D0001): {"squawk": T + 1002}},
        receivers=[None, None])

    # Mode A/C replies and address 0 never reach the tracker
    b = B().rec(T, 0x1E0001, source=ip.MODE_AC, msgtype=32, squawk_valid=1, squawk=0x1200).rec(T, 0, squawk_valid=1, squawk=0x1200, metype=ME_STATUS)
    add("modeac_and_addr0", [b.step()], [0, 0], {(0, 0x1E0001): None, (0, 0): None})

    # bit 1: clear on an aircraft's first record, set on its second
    b = B().squawk5(T, 0x1F0001).squawk5(T + 1000, 0x1F0001)
    add("seen_twice_bit", [b.step()], [F, F | S], {(0, 0x1F0001): {"squawk": T + 1500}})

    # delivery.  Record 0 is its aircraft's first message: bytes only with --net-only or --net-verbatim.  Record 1 has two
    # repaired bits: the verdict is set and the timer moves (-> T + 1125) as for any other, bytes only with --net-verbatim
    st = dict(metype=ME_STATUS, squawk_valid=1, squawk=0x1200)
    b = B().rec(T, 0x200001, **st).rec(T + 1000, 0x200001, msg=dict(correctedbits=2), **st)
    add("corrected_two_bits", [b.step()], [F, F | S], {(0, 0x200001): {"squawk": T + 1125}},
        wire={(False, False): [], (False, True): [0], (True, False): [0, 1], (True, True): [0, 1]})
    assert sorted(out) == sorted(NAMES)
    return out


def mixed_steps(pkg, every_ms=1000):
    """aircraft_streams.mixed_stream in steps: an expiry whenever the stream's clock has passed another every_ms
    -> (receivers, steps)"""
    receivers, m, f, r = acs.mixed_stream(pkg)
    t = m["sysTimestampMsg"].astype(np.int64)
    steps, lo, due = [], 0, int(t[0]) + every_ms
    for i in range(len(m)):
        if int(t[i]) >= due:
            steps += [("update", m[lo:i], f[lo:i], r[lo:i]), ("expire", due)]
            lo = i
            while int(t[i]) >= due:
                due += every_ms
    steps.append(("update", m[lo:], f[lo:], r[lo:]))
    return receivers, steps


def records(steps):
    """the records of the update steps in order -> (msgs, fields, receiver)"""
    u = [s for s in steps if s[0] == "update"]
    return tuple(np.concatenate([s[k] for s in u]) for k in (1, 2, 3))


# ---- runners -------------------------------------------------------------------------------------------------------
def run_library(tracker, steps, pieces=None, update=None):
    """steps through a reducing capi.PositionTracker -> (POSITION_DTYPE rows, NICRC_DTYPE rows, verdict bytes).
    pieces: cut every update into calls of that many records; update: called instead of tracker.update_reduce"""
    update = update or tracker.update_reduce
    rows, nic, fwd = [], [], []
    for s in steps:
        if s[0] == "expire":
            tracker.expire(s[1])
            continue
        _, m, f, r = s
        k = pieces or max(len(m), 1)
        for i in range(0, len(m), k):
            o, q, w = update(m[i:i + k], f[i:i + k], r[i:i + k])
            rows.append(o), nic.append(q), fwd.append(w)
    return np.concatenate(rows), np.concatenate(nic), np.concatenate(fwd)


def run_model(pkg, receivers, interval, steps, capacity=None):
    """-> (rows, nicrc, verdicts, tracker) from the second reading"""
    t = ir.Tracker(receivers, 8, interval, capacity)
    rows, nic, fwd = [], [], []
    for s in steps:
        if s[0] == "expire":
            t.expire(s[1])
        else:
            o, q, w = t.update(s[1], s[2], s[3])
            rows += o
            nic += q
            fwd += w
    return rows, nic, fwd, t


def expected_timers(pkg, spec):
    """a scenario's timers entry for one aircraft -> the list capi.PositionTracker.reduce_timers delivers"""
    if spec is None:
        return None
    assert set(spec) <= set(pkg.capi.AC_MEMBERS) | {"df11"}
    return [spec.get(k, 0) for k in pkg.capi.AC_MEMBERS] + [spec.get("df11", 0)]


def stream_of(pkg, msgs, verdicts, correctedbits=None, verbatim=False, net_only=False):
    """libmsd_host.so's msd_beast_frame_out on the records that the second reading's delivery conditions let through, one
    after the other -> (bytes, ends)"""
    import ctypes as C
    host = C.CDLL(pkg.capi.HOST_LIB_PATH)
    host.msd_beast_frame_out.restype = C.c_size_t
    host.msd_beast_frame_out.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    msgs = np.ascontiguousarray(msgs)
    buf = (C.c_uint8 * 64)()
    out, ends = bytearray(), np.zeros(len(msgs), dtype=np.uint32)
    for i in range(len(msgs)):
        if ir.delivered(int(verdicts[i]), int(msgs["correctedbits"][i]), verbatim, net_only):
            out += bytes(buf[:host.msd_beast_frame_out(msgs[i:i + 1].ctypes.data, int(verbatim), buf)])
        ends[i] = len(out)
    return bytes(out), ends
