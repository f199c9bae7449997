"""Constructed record streams for the Mode A/C matching's tests (test_modeac_model.py on the CPU, test_gpu_modeac.py on
the GPU): aircraft_streams.Builder with Mode A/C replies, one small named scenario per rule of trackMatchAC and of the
two hit resets, a 2000-record mixed stream with replies in between and a match every second, and runners for the three
implementations (the GPU object, the host twin, the second reading of tests/indep_modeac.py).

A scenario is (receivers, steps, check); a step is ("update", msgs, fields, receiver), ("expire", now_ms) or
("match", now_ms, message_now_ms); check(obs) asserts the value the scenario is named for against an expectation derived
by hand from track.c -- obs[i] is what the tracker holds after step i: obs[i]["codes"][receiver] a MODEAC_CODE_DTYPE
array of 4096, obs[i]["hits"] {(receiver, addr): (mode_a_hit, mode_c_hit)}, obs[i]["snap"] {(receiver, addr): entry}."""
import numpy as np

import aircraft_streams as acs
import indep_modeac as im
import indep_positions as ip
import pos_streams as ps

T0 = ps.T0
S4 = ip.MODE_S_CHECKED
ALL = 0xFFFFFFFF


def idx(code):
    return im.mode_a_to_index(code)


def code_of_feet(feet):
    """the Mode A code a Mode C reply at this altitude carries (a multiple of 100 ft)"""
    assert feet % 100 == 0
    code = im.mode_c_to_mode_a(feet // 100)
    assert code
    return code


class Builder(acs.Builder):
    def reply(self, t, code, rx=0, spi=0, n=1):
        """n Mode A/C replies as msd_fields_mode_ac leaves them; spi: the squawk field keeps the SPI bit, which
        modeAToIndex does not look at"""
        for _ in range(n):
            self.rec(t, ((code | (0x80 if spi else 0)) & 0xFF7F) | (1 << 24), rx=rx, source=ip.MODE_AC, msgtype=32,
                     squawk_valid=1, squawk=(code & 0x7777) | (0x80 if spi else 0), spi_valid=1, spi=spi)
            self.m[-1]["msgbits"] = 16
        return self

    def squawk(self, t, addr, code, rx=0):
        return self.rec(t, addr, rx=rx, source=S4, msgtype=5, crc=addr & 0xFFFFFF, squawk_valid=1, squawk=code)

    def df11(self, t, addr, rx=0):
        return self.rec(t, addr, rx=rx, source=ip.MODE_S, msgtype=11)


NAMES = ["threshold", "seen_5000", "squawk_expired", "two_on_one_squawk", "own_mode_c", "negative_altitudes", "c_plus_one",
         "ageing", "mode_a_hit_reset", "mode_c_hit_reset", "expiry_rebuild", "two_receivers", "spi", "mode_c_outside_the_table"]


def scenarios(pkg):
    S = {}
    B = lambda: Builder(pkg)  # noqa: E731

    # three replies against four: count - lastcount >= 4 at equality
    b = B()
    b.squawk(T0, 0x100001, 0x1200).squawk(T0, 0x100002, 0x1300).reply(T0 + 10, 0x1200, n=3).reply(T0 + 10, 0x1300, n=4)

    def check(obs):
        o = obs[-1]
        assert o["hits"] == {(0, 0x100001): (0, 0), (0, 0x100002): (1, 0)}
        c = o["codes"][0]
        assert tuple(c[idx(0x1200)]) == (3, 3, 0, 1) and tuple(c[idx(0x1300)]) == (4, 4, 0x100002, 10)
    S["threshold"] = ([None], [b.step(), ("match", T0 + 1000, T0 + 1000)], check)

    # (now - seen) > 5000: 5000 ms is matched, 5001 is not, and `seen` after `now` wraps to a huge age
    b = B()
    b.squawk(T0, 0x110001, 0x1200).squawk(T0 - 1, 0x110002, 0x1300).squawk(T0 + 5001, 0x110003, 0x1400)
    for code in (0x1200, 0x1300, 0x1400):
        b.reply(T0 + 10, code, n=4)

    def check(obs):
        assert obs[-1]["hits"] == {(0, 0x110001): (1, 0), (0, 0x110002): (0, 0), (0, 0x110003): (0, 0)}
        c = obs[-1]["codes"][0]
        assert [int(c[idx(k)]["match"]) for k in (0x1200, 0x1300, 0x1400)] == [0x110001, 0, 0]
        assert [int(c[idx(k)]["age"]) for k in (0x1200, 0x1300, 0x1400)] == [10, 0, 0]
    S["seen_5000"] = ([None], [b.step(), ("match", T0 + 5000, T0 + 5001)], check)

    # a squawk 70 s old is not valid any more (trackDataValid: messageNow() < expires) although DF11s keep `seen` fresh
    b = B()
    b.squawk(T0, 0x120001, 0x1200).squawk(T0 + 1, 0x120002, 0x1300)
    for a in (0x120001, 0x120002):
        b.df11(T0 + 69000, a)
    b.reply(T0 + 69500, 0x1200, n=4).reply(T0 + 69500, 0x1300, n=4)

    def check(obs):
        assert obs[-1]["hits"] == {(0, 0x120001): (0, 0), (0, 0x120002): (1, 0)}
        e = obs[-1]["snap"][(0, 0x120001)]
        assert int(e["squawk"]) == 0x1200 and int(e["seen"]) == T0 + 69000
    S["squawk_expired"] = ([None], [b.step(), ("match", T0 + 70000, T0 + 70000)], check)

    # two aircraft on one squawk: the code is ambiguous
    b = B()
    b.squawk(T0, 0x130001, 0x2345).squawk(T0, 0x130002, 0x2345).reply(T0 + 10, 0x2345, n=5)

    def check(obs):
        assert obs[-1]["hits"] == {(0, 0x130001): (1, 0), (0, 0x130002): (1, 0)}
        assert tuple(obs[-1]["codes"][0][idx(0x2345)]) == (5, 5, ALL, 10)
    S["two_on_one_squawk"] = ([None], [b.step(), ("match", T0 + 1000, T0 + 1000)], check)

    # one aircraft whose squawk is the code of its own altitude reaches the code twice
    own = code_of_feet(10000)
    b = B()
    b.squawk(T0, 0x140001, own).alt(T0 + 1, 0x140001, 10000).reply(T0 + 10, own, n=4)

    def check(obs):
        assert obs[-1]["hits"] == {(0, 0x140001): (1, 1)}
        assert tuple(obs[-1]["codes"][0][idx(own)]) == (4, 4, ALL, 10)
    S["own_mode_c"] = ([None], [b.step(), ("match", T0 + 1000, T0 + 1000)], check)

    # -150 ft: (-150 + 49) / 100 = -1 in C (floor would say -2), so C + 1 = 0 is tried: a reply at 0 ft matches.
    # -1300 ft: C = -12, C - 1 = -13 has no code (modeCToModeA gives 0): replies under squawk 0000 match nobody
    zero, low = code_of_feet(0), code_of_feet(-1200)
    b = B()
    b.alt(T0, 0x150001, -150).alt(T0, 0x150002, -1300).alt(T0, 0x150003, -1300, rx=1)
    b.reply(T0 + 10, zero, n=4).reply(T0 + 10, 0x0000, n=4).reply(T0 + 10, low, rx=1, n=4)

    def check(obs):
        assert im.mode_c_to_mode_a(-13) == 0 and im.mode_c_to_mode_a(-12) == low
        assert obs[-1]["hits"] == {(0, 0x150001): (0, 1), (0, 0x150002): (0, 0), (1, 0x150003): (0, 1)}
        c = obs[-1]["codes"]
        assert tuple(c[0][idx(zero)]) == (4, 4, 0x150001, 10) and tuple(c[0][0]) == (4, 4, 0, 0)
        assert tuple(c[1][idx(low)]) == (4, 4, 0x150003, 10)
    S["negative_altitudes"] = ([None, None], [b.step(), ("match", T0 + 1000, T0 + 1000)], check)

    # replies 100 ft above the aircraft only
    up = code_of_feet(10100)
    b = B()
    b.alt(T0, 0x160001, 10000).reply(T0 + 10, up, n=4)

    def check(obs):
        assert obs[-1]["hits"] == {(0, 0x160001): (0, 1)}
        assert tuple(obs[-1]["codes"][0][idx(up)]) == (4, 4, 0x160001, 10)
        assert int(obs[-1]["codes"][0][idx(code_of_feet(10000))]["count"]) == 0
    S["c_plus_one"] = ([None], [b.step(), ("match", T0 + 1000, T0 + 1000)], check)

    # a code heard once ages 1, 2, .. 15 and is cleared by the 16th match; a live matched code has age 10, a live
    # unmatched one age 0
    b = B()
    b.squawk(T0, 0x170001, 0x1200).reply(T0 + 10, 0x1200, n=4).reply(T0 + 10, 0x3300, n=4).reply(T0 + 10, 0x4400)
    steps = [b.step()] + [("match", T0 + 1000 * k, T0 + 1000 * k) for k in range(1, 17)]

    def check(obs):
        once = [tuple(o["codes"][0][idx(0x4400)]) for o in obs[1:]]
        assert once[:15] == [(1, 1, 0, k) for k in range(1, 16)] and once[15] == (0, 0, 0, 0)
        assert tuple(obs[1]["codes"][0][idx(0x1200)]) == (4, 4, 0x170001, 10)
        assert tuple(obs[1]["codes"][0][idx(0x3300)]) == (4, 4, 0, 0)
        # not heard again: the matched code ages from 10 and goes with the 7th match, the other from 0
        assert tuple(obs[6]["codes"][0][idx(0x1200)]) == (4, 4, 0, 15) and tuple(obs[7]["codes"][0][idx(0x1200)]) == (0, 0, 0, 0)
        assert tuple(obs[16]["codes"][0][idx(0x3300)]) == (4, 4, 0, 15)
        assert obs[16]["hits"] == {(0, 0x170001): (1, 0)}  # nothing but a message clears a hit
    S["ageing"] = ([None], steps, check)

    # modeA_hit: kept by an accepted squawk that is the same, cleared by one that differs; a refused one (older than the
    # stored squawk) clears nothing
    b = B()
    for a in (0x180001, 0x180002):
        b.squawk(T0, a, 0x1200)
    b.reply(T0 + 10, 0x1200, n=4)
    first = b.step()
    same = b.squawk(T0 + 1500, 0x180001, 0x1200).squawk(T0 + 1500, 0x180002, 0x1200).step()
    b.squawk(T0 + 2000, 0x180001, 0x7700)
    b.rec(T0 - 500, 0x180002, source=S4, msgtype=5, squawk_valid=1, squawk=0x7700)

    def check(obs):
        assert obs[1]["hits"] == {(0, 0x180001): (1, 0), (0, 0x180002): (1, 0)} and obs[2]["hits"] == obs[1]["hits"]
        assert obs[3]["hits"] == {(0, 0x180001): (0, 0), (0, 0x180002): (1, 0)}
        assert int(obs[3]["snap"][(0, 0x180001)]["squawk"]) == 0x7700 and int(obs[3]["snap"][(0, 0x180002)]["squawk"]) == 0x1200
    S["mode_a_hit_reset"] = ([None], [first, ("match", T0 + 1000, T0 + 1000), same, b.step()], check)

    # modeC_hit: (alt + 49) / 100 is 100 for 10 040 and 10 050 ft, 101 for 10 051 ft.  The third aircraft's jump to
    # 30 000 ft is refused by the plausibility gate (as gate_fpm_default's), and clears the hit all the same
    at = code_of_feet(10000)
    b = B()
    b.alt(T0, 0x190001, 10040).alt(T0, 0x190002, 10040)
    for k in range(3):
        b.alt(T0 + 100 * k, 0x190003, 10000)
    b.reply(T0 + 300, at, n=4)
    first = b.step()
    b.alt(T0 + 1500, 0x190001, 10050).alt(T0 + 1500, 0x190002, 10051).alt(T0 + 1500, 0x190003, 30000)

    def check(obs):
        assert obs[1]["hits"] == {(0, 0x190001): (0, 1), (0, 0x190002): (0, 1), (0, 0x190003): (0, 1)}
        assert tuple(obs[1]["codes"][0][idx(at)]) == (4, 4, ALL, 10)
        assert obs[2]["hits"] == {(0, 0x190001): (0, 1), (0, 0x190002): (0, 0), (0, 0x190003): (0, 0)}
        s = obs[2]["snap"]
        assert [int(s[(0, a)]["alt_baro"]) for a in (0x190001, 0x190002, 0x190003)] == [10050, 10051, 10000]
        assert int(s[(0, 0x190003)]["altitude_baro_reliable"]) == 2
    S["mode_c_hit_reset"] = ([None], [first, ("match", T0 + 1000, T0 + 1000), b.step()], check)

    # the expiry rebuild moves the hits with their aircraft; an aircraft that arrives afterwards has none.  The four
    # aircraft share a home slot in a table of 64 (a probe chain), the one that goes sits in front of the one with the hit
    chain = ps.chain_addresses(pkg, 64)
    gone, keeps, later = chain[0], chain[1], chain[2]
    b = B()
    b.df11(T0, gone).squawk(T0 + 1, keeps, 0x1200).df11(T0 + 2, keeps).reply(T0 + 10, 0x1200, n=4)
    first = b.step()
    b.squawk(T0 + 62000, later, 0x1200)

    def check(obs):
        assert obs[1]["hits"] == {(0, gone): (0, 0), (0, keeps): (1, 0)}
        assert obs[2]["hits"] == {(0, keeps): (1, 0)}
        assert obs[3]["hits"] == {(0, keeps): (1, 0), (0, later): (0, 0)}
    S["expiry_rebuild"] = ([None], [first, ("match", T0 + 1000, T0 + 1000), ("expire", T0 + 61000), b.step()], check)

    # two receivers hear the same address with the same squawk; the replies arrive on one of them only
    b = B()
    b.squawk(T0, 0x1B0001, 0x1200, rx=0).squawk(T0, 0x1B0001, 0x1200, rx=1).reply(T0 + 10, 0x1200, rx=1, n=4)

    def check(obs):
        assert obs[-1]["hits"] == {(0, 0x1B0001): (0, 0), (1, 0x1B0001): (1, 0)}
        assert not obs[-1]["codes"][0].view(np.uint32).any()
        assert tuple(obs[-1]["codes"][1][idx(0x1200)]) == (4, 4, 0x1B0001, 10)
    S["two_receivers"] = ([None, None], [b.step(), ("match", T0 + 1000, T0 + 1000)], check)

    # SPI is ignored: two replies with it and two without are four of the same code
    b = B()
    b.squawk(T0, 0x1C0001, 0x1200).reply(T0 + 10, 0x1200, n=2).reply(T0 + 11, 0x1200, spi=1, n=2)

    def check(obs):
        assert obs[-1]["hits"] == {(0, 0x1C0001): (1, 0)}
        c = obs[-1]["codes"][0]
        assert tuple(c[idx(0x1200)]) == (4, 4, 0x1C0001, 10) and int(c["count"].sum()) == 4
    S["spi"] = ([None], [b.step(), ("match", T0 + 1000, T0 + 1000)], check)

    # altitudes whose C, C + 1 or C - 1 lies outside modeCToATable (modeCToModeA's range test, mode_ac.c:93-98).
    # -1400 ft: C = (-1400 + 49) / 100 = -13 has no code, C - 1 = -14 is below the table, C + 1 = -12 is -1200 ft: a reply
    # there matches.  408 300 ft: C = 4083 is the first index past the table, C + 1 is further out, C - 1 = 4082 is the
    # table's last entry and has no code: replies under squawk 0000 -- what a careless lookup would return -- match nobody
    low = code_of_feet(-1200)
    b = B()
    b.alt(T0, 0x1D0001, -1400).alt(T0, 0x1D0002, 408300, rx=1)
    b.reply(T0 + 10, low, n=4).reply(T0 + 10, 0x0000, n=4).reply(T0 + 10, low, rx=1, n=4).reply(T0 + 10, 0x0000, rx=1, n=4)

    def check(obs):
        assert obs[-1]["hits"] == {(0, 0x1D0001): (0, 1), (1, 0x1D0002): (0, 0)}
        c = obs[-1]["codes"]
        assert tuple(c[0][idx(low)]) == (4, 4, 0x1D0001, 10) and tuple(c[0][0]) == (4, 4, 0, 0)
        assert tuple(c[1][idx(low)]) == (4, 4, 0, 0) and tuple(c[1][0]) == (4, 4, 0, 0)
        assert int(obs[-1]["snap"][(1, 0x1D0002)]["alt_baro"]) == 408300
    S["mode_c_outside_the_table"] = ([None, None], [b.step(), ("match", T0 + 1000, T0 + 1000)], check)
    return S


def mixed_steps(pkg, n=2000, seed=23):
    """aircraft_streams.mixed_stream's 2000 records with Mode A/C replies in between -- bursts of 1 to 6 on the squawks
    the stream's aircraft use, on the codes of their altitudes and 100 ft beside them, and on codes nobody has --, cut
    as trackPeriodicUpdate would: whenever a record's time reaches next_update, expiry and a match run first and
    next_update moves a second on.  -> (receivers, steps, (msgs, fields, receiver) of the whole stream)"""
    rng = np.random.default_rng(seed)
    receivers, m, f, r = acs.mixed_stream(pkg, n - n // 5)
    alts = sorted({int(a) // 100 for a, v in zip(f["altitude_baro"], f["altitude_baro_valid"]) if v and int(a) % 100 == 0})
    codes = [0x1200, 0x7000, 0x2345, 0x0000, 0x7777, 0x4321]
    codes += [c for c in (im.mode_c_to_mode_a(a + d) for a in alts[::3] for d in (-1, 0, 1)) if c]
    b = Builder(pkg)
    at = np.sort(rng.integers(0, len(m), size=n // 5 // 3))
    for k in at:
        b.reply(int(m["sysTimestampMsg"][k]), int(rng.choice(codes)), rx=int(rng.integers(0, 2)), spi=int(rng.uniform() < 0.1),
                n=int(rng.integers(1, 7)))
    _, rm, rf, rr = b.step()
    rm, rf, rr = rm[:n - len(m)], rf[:n - len(m)], rr[:n - len(m)]
    am, af, ar = np.concatenate([m, rm]), np.concatenate([f, rf]), np.concatenate([r, rr])
    order = np.argsort(am["sysTimestampMsg"], kind="stable")
    am, af, ar = am[order], af[order], ar[order]
    steps, start, next_update, last = [], 0, 0, 0
    for i in range(len(am)):
        t = int(am["sysTimestampMsg"][i])
        if t >= next_update:
            if i > start:
                steps.append(("update", am[start:i], af[start:i], ar[start:i]))
                start = i
            if next_update:
                steps += [("expire", t), ("match", t, last)]
            next_update = t + 1000
        if am["msgtype"][i] != 32 and af["addr"][i] != 0:
            last = t
    steps.append(("update", am[start:], af[start:], ar[start:]))
    steps += [("match", int(am["sysTimestampMsg"][-1]), last)]
    return receivers, steps, (am, af, ar)


# ---- runners -------------------------------------------------------------------------------------------------------
def observe(tracker, nrx):
    snap, hits = tracker.snapshot(), tracker.modeac_hits()
    assert len(snap) == len(hits) and np.array_equal(snap["addr"], hits["addr"]) and np.array_equal(snap["receiver"], hits["receiver"])
    assert not hits["pad"].any()
    return dict(codes=[tracker.modeac_codes(k) for k in range(nrx)], hits_raw=hits, snap_raw=snap,
                hits={(int(h["receiver"]), int(h["addr"])): (int(h["mode_a_hit"]), int(h["mode_c_hit"])) for h in hits},
                snap={(int(e["receiver"]), int(e["addr"])): e for e in snap})


def run_library(tracker, nrx, steps, pieces=None, every_step=True):
    """steps through an enabled capi.PositionTracker -> (POSITION_DTYPE rows, NICRC_DTYPE rows, [observe() per step])"""
    rows, nic, obs = [], [], []
    for s in steps:
        if s[0] == "expire":
            tracker.expire(s[1])
        elif s[0] == "match":
            tracker.modeac_match(s[1], s[2])
        else:
            _, m, f, r = s
            k = pieces or max(len(m), 1)
            for i in range(0, len(m), k):
                o, q = tracker.update_nicrc(m[i:i + k], f[i:i + k], r[i:i + k])
                rows.append(o), nic.append(q)
        if every_step:
            obs.append(observe(tracker, nrx))
    if not every_step:
        obs.append(observe(tracker, nrx))
    if not rows:  # no update step
        return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), obs
    return np.concatenate(rows), np.concatenate(nic), obs


def run_model(pkg, receivers, steps):
    """-> (rows, nicrc, [dict(codes=[..], hits=[..], snap=[..]) per step]) from the second reading"""
    t = im.Tracker(receivers, 8)
    rows, nic, obs = [], [], []
    for s in steps:
        if s[0] == "expire":
            t.expire(s[1])
        elif s[0] == "match":
            t.match_ac(s[1], s[2])
        else:
            o, q = t.update(s[1], s[2], s[3])
            rows += o
            nic += q
        obs.append(dict(codes=[t.codes_of(k) for k in range(len(receivers))], hits=t.hits(), snap=t.snapshot(pkg.capi.AC_MEMBERS)))
    return rows, nic, obs


def same_bytes(got, want):
    """two run_library results, byte for byte"""
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert len(got[2]) == len(want[2])
    for k, (g, w) in enumerate(zip(got[2], want[2])):
        assert g["hits_raw"].tobytes() == w["hits_raw"].tobytes(), (k, g["hits"], w["hits"])
        for rx, (cg, cw) in enumerate(zip(g["codes"], w["codes"])):
            if cg.tobytes() != cw.tobytes():
                bad = [(i, tuple(cg[i]), tuple(cw[i])) for i in range(4096) if cg[i] != cw[i]]
                raise AssertionError((k, rx, bad[:6]))
        assert g["snap_raw"].tobytes() == w["snap_raw"].tobytes(), k
