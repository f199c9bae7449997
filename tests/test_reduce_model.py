"""The reduced Beast output on the CPU: the host twin (libmsd_host.so: msd_trk_impl.h's rule compiled for the host,
msd_beast_frame_out for the bytes) against the second reading of track.c in tests/indep_reduce.py and against the
expectations reduce_streams.py derives by hand -- the verdict byte of every record and every timer of every aircraft --, on
one scenario per rule and on the aircraft table's mixed stream at intervals 0, 125 and 15000 with an expiry every second;
the stream's bytes against msd_beast_frame_out on the records the delivery conditions let through; and what the feature
promises around it: a tracker that reduces delivers what one that does not delivers, results do not depend on which
update call fed a record or on how a stream is cut, and the refusals."""
import errno

import numpy as np
import pytest

import aircraft_streams as acs
import indep_reduce as ir
import reduce_streams as rs


@pytest.fixture(scope="module")
def scen(pkg):
    return rs.scenarios(pkg)


def make_twin(pkg, receivers, interval, capacity=1024, **kw):
    return pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, host=True, table=True, reduce_interval_ms=interval,
                                    **kw)


def timers_of(t, receiver, addr):
    g = t.reduce_timers(receiver, addr)
    return None if g is None else [int(x) for x in g]


def all_timers_match(pkg, twin, model):
    """every aircraft of the second reading, every timer"""
    n = 0
    for (r, a) in model.aircraft:
        assert timers_of(twin, r, a) == model.timers(r, a, pkg.capi.AC_MEMBERS), (r, hex(a))
        n += 1
    assert twin.live() == n
    return n


def test_scenario_list_is_complete(scen):
    assert sorted(scen) == sorted(rs.NAMES)


@pytest.mark.parametrize("name", rs.NAMES)
def test_scenario_by_hand_second_reading_and_twin(pkg, scen, name):
    s = scen[name]
    t = make_twin(pkg, s["receivers"], s["interval"], s["capacity"])
    rows, nic, fwd = rs.run_library(t, s["steps"])
    mrows, mnic, mfwd, model = rs.run_model(pkg, s["receivers"], s["interval"], s["steps"])
    assert mfwd == s["verdicts"], "the second reading against the hand-derived verdicts"
    assert [int(x) for x in fwd] == s["verdicts"]
    for (r, a), spec in s["timers"].items():
        want = rs.expected_timers(pkg, spec)
        assert model.timers(r, a, pkg.capi.AC_MEMBERS) == want, (hex(a), "second reading")
        assert timers_of(t, r, a) == want, hex(a)
    all_timers_match(pkg, t, model)
    assert t.stats()["min_gate_margin_m"] >= 1.0
    t.close()


@pytest.mark.parametrize("name", rs.NAMES)
@pytest.mark.parametrize("pieces", [1, 3])
def test_scenario_cut_into_calls(pkg, scen, name, pieces):
    s = scen[name]
    t = make_twin(pkg, s["receivers"], s["interval"], s["capacity"])
    assert [int(x) for x in rs.run_library(t, s["steps"], pieces=pieces)[2]] == s["verdicts"]
    for (r, a), spec in s["timers"].items():
        assert timers_of(t, r, a) == rs.expected_timers(pkg, spec)
    t.close()


@pytest.fixture(scope="module")
def mixed(pkg):
    receivers, steps = rs.mixed_steps(pkg)
    assert sum(1 for s in steps if s[0] == "expire") >= 10
    return receivers, steps


@pytest.mark.parametrize("interval", [0, 125, 15000])
def test_mixed_stream_equals_second_reading(pkg, mixed, interval):
    receivers, steps = mixed
    t = make_twin(pkg, receivers, interval)
    rows, nic, fwd = rs.run_library(t, steps)
    mrows, mnic, mfwd, model = rs.run_model(pkg, receivers, interval, steps)
    assert [int(x) for x in fwd] == mfwd
    assert all_timers_match(pkg, t, model) >= 30
    assert t.stats()["min_gate_margin_m"] >= 1.0
    print("interval", interval, "forwarded", np.count_nonzero(fwd & ir.FORWARD), "of", len(fwd))
    assert (fwd & ir.FORWARD).any() and not (fwd & ir.FORWARD).all()
    # cutting does not matter
    c = make_twin(pkg, receivers, interval)
    assert rs.run_library(c, steps, pieces=7)[2].tobytes() == fwd.tobytes()
    all_timers_match(pkg, c, model)
    c.close()
    t.close()


def test_wire_bytes_are_the_host_writers_on_the_selected_records(pkg, mixed):
    receivers, steps = mixed
    m, f, r = rs.records(steps)
    m = m.copy()
    rng = np.random.default_rng(5)
    m["msg"] = rng.integers(0, 256, (len(m), 14))
    m["msg"][::17, 3:9] = 0x1A  # escapes
    m["msgbits"] = rng.choice([16, 56, 112], len(m))
    m["timestampMsg"] = rng.integers(0, 1 << 48, len(m))
    m["correctedbits"] = rng.choice([0, 0, 1, 2], len(m))
    t = make_twin(pkg, receivers, 125)
    fwd = t.update_reduce(m, f, r)[2]
    for verbatim in (False, True):
        for net_only in (False, True):
            want, wends = rs.stream_of(pkg, m, fwd, verbatim=verbatim, net_only=net_only)
            got, ends = t.reduce_wire(m, fwd, verbatim=verbatim, net_only=net_only)
            assert got == want and (ends == wends).all() and len(want) > 1000
    # the size comes back with -ENOSPC and nothing is written; then the exact size succeeds
    want, _ = rs.stream_of(pkg, m, fwd)
    with pytest.raises(pkg.MsdError) as e:
        t.reduce_wire(m, fwd, cap=len(want) - 1)
    assert e.value.code == -errno.ENOSPC and t.reduce_needed == len(want) and not t.reduce_out.any()
    assert t.reduce_wire(m, fwd, cap=len(want))[0] == want
    empty = t.reduce_wire(m[:0], fwd[:0])
    assert empty[0] == b"" and len(empty[1]) == 0 and t.reduce_needed == 0
    t.close()


def test_delivery_conditions(pkg, scen):
    s = scen["corrected_two_bits"]
    m, f, r = rs.records(s["steps"])
    t = make_twin(pkg, s["receivers"], s["interval"])
    fwd = t.update_reduce(m, f, r)[2]
    for (verbatim, net_only), which in s["wire"].items():
        got, ends = t.reduce_wire(m, fwd, verbatim=verbatim, net_only=net_only)
        want, wends = rs.stream_of(pkg, m, fwd, verbatim=verbatim, net_only=net_only)
        assert got == want and list(ends) == list(wends)
        sizes = np.diff(np.concatenate([[0], ends]))
        assert [i for i in range(len(m)) if sizes[i]] == which, (verbatim, net_only)
    t.close()


def test_reducing_changes_nothing_else(pkg, mixed):
    """an enabled tracker's msd_position, msd_pos_nicrc, snapshot and Mode A/C results, byte for byte"""
    receivers, steps = mixed
    res = []
    for interval in (None, 125):
        t = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, host=True, table=True, modeac=True,
                                     reduce_interval_ms=interval)
        rows, nic, snaps = acs.run_library(t, steps, every_step=False)
        t.modeac_match(acs.T0 + 5000, acs.T0 + 5000)
        res.append((rows.tobytes(), nic.tobytes(), snaps[-1].tobytes(), t.modeac_hits().tobytes(),
                    t.modeac_codes(0).tobytes(), t.stats()))
        t.close()
    assert res[0] == res[1]


def test_which_update_call_feeds_a_record_does_not_matter(pkg, mixed):
    receivers, steps = mixed
    whole = make_twin(pkg, receivers, 125)
    fwd = rs.run_library(whole, steps)[2]
    t = make_twin(pkg, receivers, 125)
    got, calls = [], 0
    for s in steps:
        if s[0] == "expire":
            t.expire(s[1])
            continue
        _, m, f, r = s
        for i in range(0, len(m), 50):
            part = (m[i:i + 50], f[i:i + 50], r[i:i + 50])
            if calls % 3 == 0:
                t.update(*part)
            elif calls % 3 == 1:
                t.update_nicrc(*part)
            got.append(t.update_reduce(*part, nicrc=False)[2] if calls % 3 == 2 else np.full(len(part[0]), 255, dtype=np.uint8))
            calls += 1
    got = np.concatenate(got)
    seen = got != 255
    assert 0.2 < seen.mean() < 0.5 and (got[seen] == fwd[seen]).all()
    m, f, r = rs.records(steps)
    keys = {(int(x), int(a) & 0x1FFFFFF) for x, a, mt in zip(r, f["addr"], m["msgtype"]) if mt != 32 and a != 0}
    assert len(keys) == 40 and all(timers_of(t, *k) == timers_of(whole, *k) for k in keys)
    t.close()
    whole.close()


def test_refusals_and_rollback(pkg, scen):
    s = scen["df5_squawk"]
    m, f, r = rs.records(s["steps"])
    E = pkg.MsdError

    def code(call):
        with pytest.raises(E) as e:
            call()
        return e.value.code
    # no table; an interval above readsb's cap; the two calls on a tracker that does not reduce
    t = pkg.capi.PositionTracker(capacity=64, host=True)
    assert code(lambda: t.reduce_enable(125)) == -errno.EINVAL
    t.close()
    t = pkg.capi.PositionTracker(capacity=64, host=True, table=True)
    assert code(lambda: t.reduce_enable(15001)) == -errno.EINVAL
    assert code(lambda: t.update_reduce(m, f, r)) == -errno.EINVAL
    assert code(lambda: t.reduce_wire(m, np.zeros(len(m), dtype=np.uint8))) == -errno.EINVAL
    t.update(m[:1], f[:1], r[:1])  # an aircraft from before the call starts at 0 and its message counts
    t.reduce_enable(15000)
    t.reduce_enable(15000)  # the same interval again: nothing changes
    assert code(lambda: t.reduce_enable(125)) == -errno.EINVAL
    assert timers_of(t, 0, 0x120001) == [0] * pkg.capi.REDUCE_TIMERS
    assert list(t.update_reduce(m[1:2], f[1:2], r[1:2])[2]) == [ir.FORWARD | ir.SEEN_TWICE]
    # an unknown flag, NULL
    fwd = np.ones(len(m), dtype=np.uint8)
    assert code(lambda: t.reduce_wire(m, fwd, flags=4)) == -errno.EINVAL
    n = pkg.capi.C.c_size_t(0)
    assert t.f["reduce_wire"](t.h, None, fwd.ctypes.data, len(m), 0, None, 0, pkg.capi.C.byref(n), None) == -errno.EINVAL
    assert t.f["reduce_wire"](t.h, m.ctypes.data, fwd.ctypes.data, len(m), 0, None, 0, None, None) == -errno.EINVAL
    assert t.f["update_reduce"](t.h, m.ctypes.data, f.ctypes.data, None, len(m), m.ctypes.data, None, None) == -errno.EINVAL
    t.close()
    # a rolled-back call moves no timer and writes no verdict: 64 slots, 70 new aircraft
    t = make_twin(pkg, [None], 125, capacity=64)
    t.update_reduce(m[:1], f[:1], r[:1])
    before = timers_of(t, 0, 0x120001)
    b = rs.Builder(pkg)
    b.squawk5(rs.T0 + 600, 0x120001)
    for k in range(70):
        b.squawk5(rs.T0 + 600, 0x300000 + k)
    _, bm, bf, br = b.step()
    out = np.zeros(len(bm), dtype=pkg.capi.POSITION_DTYPE)
    fwd = np.full(len(bm), 0xEE, dtype=np.uint8)
    rc = t.f["update_reduce"](t.h, bm.ctypes.data, bf.ctypes.data, br.ctypes.data, len(bm), out.ctypes.data, None, fwd.ctypes.data)
    assert rc == -errno.ENOSPC and (fwd == 0xEE).all() and timers_of(t, 0, 0x120001) == before and t.live() == 1
    br[5] = 9  # a receiver index out of range
    rc = t.f["update_reduce"](t.h, bm.ctypes.data, bf.ctypes.data, br.ctypes.data, 6, out.ctypes.data, None, fwd.ctypes.data)
    assert rc == -errno.EINVAL and (fwd == 0xEE).all() and timers_of(t, 0, 0x120001) == before
    # the repeated call, now fitting, gives what a tracker gives that never saw the failed ones
    fresh = make_twin(pkg, [None], 125, capacity=64)
    fresh.update_reduce(m[:1], f[:1], r[:1])
    assert t.update_reduce(bm[:40], bf[:40], br[:40] * 0)[2].tobytes() == fresh.update_reduce(bm[:40], bf[:40], br[:40] * 0)[2].tobytes()
    t.reset()  # forgets the timers with the aircraft and stays enabled
    assert timers_of(t, 0, 0x120001) is None
    assert list(t.update_reduce(m, f, r)[2]) == s["verdicts"]
    t.close()
    fresh.close()
