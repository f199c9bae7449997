"""The reduced Beast output on the GPU (msd_pos_reduce_enable, msd_pos_update_reduce, msd_pos_reduce_wire) against the host
twin, which test_reduce_model.py holds equal to a second reading of track.c and to expectations derived by hand.
Everything is compared by bytes -- the verdict byte of every record, the stream, its ends --: the contract is the table's,
equality wherever the msd_position rows are equal, and has no tolerance.  Beside the rule (every scenario, the mixed
stream with its expiries, cut into calls of 1, 63 and 257 records) this covers what exists on the device only: the reduce
instantiations of the two walks over the grouped order and the byte they hand over, the timers that move with a slot
through the expiry rebuild, verdicts into device memory, and the compacting writer's tiles, runs and seams.
Every stream keeps every plausibility gate at least 1 m from its limit on the twin, and the tests assert it."""
import ctypes as C
import errno
import time

import numpy as np
import pytest

import aircraft_streams as acs
import indep_reduce as ir
import reduce_streams as rs

pytestmark = pytest.mark.gpu
F, S = ir.FORWARD, ir.SEEN_TWICE


def tracker(pkg, host, receivers, interval, capacity=1024, **kw):
    return pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, host=host, table=True, reduce_interval_ms=interval, **kw)


def run(pkg, host, receivers, interval, steps, capacity=1024, pieces=None):
    t = tracker(pkg, host, receivers, interval, capacity)
    out = rs.run_library(t, steps, pieces)
    st = t.stats()
    t.close()
    if host:
        assert st["min_gate_margin_m"] >= 1.0, st["min_gate_margin_m"]
    return out


def same(got, want):
    assert got[0].tobytes() == want[0].tobytes(), "msd_position rows"
    assert got[1].tobytes() == want[1].tobytes(), "NIC / Rc"
    assert got[2].tobytes() == want[2].tobytes(), [(i, int(got[2][i]), int(want[2][i])) for i in range(len(want[2])) if got[2][i] != want[2][i]][:8]


@pytest.fixture(scope="module")
def scen(pkg):
    return rs.scenarios(pkg)


@pytest.fixture(scope="module")
def mixed(pkg):
    receivers, steps = rs.mixed_steps(pkg)
    return receivers, steps, {i: run(pkg, True, receivers, i, steps) for i in (0, 125, 15000)}


# ---- the rule ----
@pytest.mark.parametrize("name", rs.NAMES)
def test_scenario(pkg, torch_cuda, scen, name):
    s = scen[name]
    want = run(pkg, True, s["receivers"], s["interval"], s["steps"], s["capacity"])
    assert [int(x) for x in want[2]] == s["verdicts"]
    same(run(pkg, False, s["receivers"], s["interval"], s["steps"], s["capacity"]), want)
    for pieces in (1, 63, 257):
        same(run(pkg, False, s["receivers"], s["interval"], s["steps"], s["capacity"], pieces), want)


@pytest.mark.parametrize("interval", [0, 125, 15000])
def test_mixed_stream(pkg, torch_cuda, mixed, interval):
    receivers, steps, want = mixed
    same(run(pkg, False, receivers, interval, steps), want[interval])


@pytest.mark.parametrize("pieces", [1, 63, 257])
def test_mixed_stream_cut_into_calls(pkg, torch_cuda, mixed, pieces):
    receivers, steps, want = mixed
    same(run(pkg, False, receivers, 125, steps, pieces=pieces), want[125])


def test_scenario_wire(pkg, torch_cuda, scen):
    s = scen["corrected_two_bits"]
    m, f, r = rs.records(s["steps"])
    t = tracker(pkg, False, s["receivers"], s["interval"])
    fwd = t.update_reduce(m, f, r)[2]
    assert [int(x) for x in fwd] == s["verdicts"]
    for (verbatim, net_only), which in s["wire"].items():
        got, ends = t.reduce_wire(m, fwd, verbatim=verbatim, net_only=net_only)
        want, wends = rs.stream_of(pkg, m, fwd, verbatim=verbatim, net_only=net_only)
        assert got == want and list(ends) == list(wends)
        assert [i for i in range(len(m)) if np.diff(np.concatenate([[0], ends]))[i]] == which
    t.close()


# ---- where the verdicts go, and which call feeds a record ----
def on_device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def test_verdicts_into_device_memory_and_the_writer_from_it(pkg, torch_cuda, mixed):
    receivers, steps, want = mixed
    m, f, r = rs.records(steps)
    n = len(m)
    t = tracker(pkg, False, receivers, 125)
    d_fwd = torch_cuda.full((n + 64,), 0xEE, dtype=torch_cuda.uint8, device="cuda")
    at = 0
    for s in steps:
        if s[0] == "expire":
            t.expire(s[1])
            continue
        k = len(s[1])
        dm, df, dr = on_device(torch_cuda, s[1]), on_device(torch_cuda, s[2]), on_device(torch_cuda, s[3])
        torch_cuda.cuda.synchronize()
        t.update_reduce_device(dm.data_ptr(), df.data_ptr(), k, d_fwd.data_ptr() + at, dr.data_ptr())
        at += k
    back = d_fwd.cpu().numpy()
    assert back[:n].tobytes() == want[125][2].tobytes() and (back[n:] == 0xEE).all()
    dm = on_device(torch_cuda, m)
    torch_cuda.cuda.synchronize()
    got, ends = t.reduce_wire(dm.data_ptr(), d_fwd.data_ptr(), n=n, on_device=True)
    wbytes, wends = rs.stream_of(pkg, m, want[125][2])
    assert got == wbytes and (ends == wends).all() and len(wbytes) > 10000
    t.close()


def test_update_calls_without_verdicts_advance_the_timers(pkg, torch_cuda, mixed):
    receivers, steps, want = mixed
    t = tracker(pkg, False, receivers, 125)
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
    t.close()
    got = np.concatenate(got)
    seen = got != 255
    assert seen.sum() > 400 and (got[seen] == want[125][2][seen]).all()


# ---- shapes of the walk ----
def test_one_aircraft_is_a_serial_walk(pkg, torch_cuda):
    receivers, m, f, r = acs.wide_stream(pkg, aircraft=1, records=300, replies=True)
    steps = [("update", m, f, r)]
    want = run(pkg, True, receivers, 15000, steps, 64)  # a record every 500 ms: both outcomes occur
    assert 0 < np.count_nonzero(want[2] & F) < 300 and np.count_nonzero(want[2] & S) == 299
    same(run(pkg, False, receivers, 15000, steps, 65536), want)


def test_more_walkers_than_a_wavefront(pkg, torch_cuda):
    receivers, m, f, r = acs.wide_stream(pkg, aircraft=65, records=65 * 12, replies=True)
    steps = [("update", m, f, r)]
    want = run(pkg, True, receivers, 1000, steps)
    assert 65 <= np.count_nonzero(want[2] & F) < 65 * 12  # every aircraft's first record, not every record
    same(run(pkg, False, receivers, 1000, steps), want)


def test_pieces(pkg, torch_cuda):
    """2^20 + 300 records of 4099 aircraft in one call, squitters and replies mixed: the walks are cut after 2^20 records,
    and the 300 aircraft of the second piece continue from the timers the first piece's table walk left."""
    t0 = time.perf_counter()
    n = (1 << 20) + 300
    receivers, m, f, r = acs.wide_stream(pkg, aircraft=4099, records=n, replies=True)
    steps = [("update", m, f, r)]
    want = run(pkg, True, receivers, 1000, steps, 8192)
    got = run(pkg, False, receivers, 1000, steps, 8192)
    same(got, want)
    tail = want[2][1 << 20:]
    # an aircraft is heard every 500 ms with a different kind of message each time: of the second piece's records some
    # find their members due and some do not
    assert (tail & S).all() and 0 < np.count_nonzero(tail & F) < 300
    print("pieces: forwarded %d of %d, the test %.1f s" % (np.count_nonzero(want[2] & F), n, time.perf_counter() - t0))


# ---- the writer ----
def writer_records(pkg, n, seed=3):
    """n records for the stateless writer: 2-, 7- and 14-byte messages mixed, every fifth with payload, timestamp and
    signal bytes of 0x1A (a frame of up to 44 bytes), 0, 1 and 2 repaired bits"""
    rng = np.random.default_rng(seed + n)
    m = np.zeros(n, dtype=pkg.capi.MESSAGE_DTYPE)
    m["msgbits"] = rng.choice([16, 56, 112], n)
    m["msg"] = rng.integers(0, 256, (n, 14))
    m["timestampMsg"] = rng.integers(0, 1 << 48, n)
    m["signalLevel"] = rng.uniform(0, 1, n)
    esc = np.arange(n) % 5 == 0
    m["msg"][esc] = 0x1A
    m["timestampMsg"][esc] = 0x1A1A1A1A1A1A
    m["signalLevel"][esc] = (26 / 255.0) ** 2
    m["correctedbits"] = rng.choice([0, 0, 0, 1, 2], n)
    m["msgtype"] = np.where(m["msgbits"] == 16, 32, 17)
    m["crc"] = np.where(m["correctedbits"] > 0, rng.integers(1, 1 << 24, n), 0)
    return m


PATTERNS = ("all", "none", "last_of_each_tile", "first_of_second_tile", "random")


def verdicts_for(pattern, n):
    i = np.arange(n)
    if pattern == "all":
        on = np.ones(n, dtype=bool)
    elif pattern == "none":
        on = np.zeros(n, dtype=bool)
    elif pattern == "last_of_each_tile":
        on = (i % 256 == 255) | (i == n - 1)
    elif pattern == "first_of_second_tile":
        on = i == 256
    else:
        on = np.random.default_rng(n).uniform(size=n) < 0.4
    return np.where(on, F | S, np.where(i % 3 == 0, S, 0)).astype(np.uint8)


@pytest.fixture(scope="module")
def writers(pkg, torch_cuda):
    t = {h: tracker(pkg, h, [None], 125, 64) for h in (False, True)}
    yield t
    for x in t.values():
        x.close()


@pytest.mark.parametrize("n", [255, 256, 257, 1025])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_writer_shapes(pkg, writers, n, pattern):
    m, fwd = writer_records(pkg, n), verdicts_for(pattern, n)
    for verbatim in (False, True):
        want, wends = rs.stream_of(pkg, m, fwd, verbatim=verbatim)
        twin, tends = writers[True].reduce_wire(m, fwd, verbatim=verbatim)
        got, ends = writers[False].reduce_wire(m, fwd, verbatim=verbatim)
        assert twin == want and (tends == wends).all()
        assert got == want and (ends == wends).all()
        if pattern == "none":
            assert writers[False].reduce_needed == 0 and not ends.any()
        if pattern == "all" and verbatim:
            # with --net-verbatim every record goes out, in 11 bytes at least, the escaped long ones in 44
            assert len(want) >= 11 * n and max(np.diff(wends)) == 44


def test_writer_first_message_flags(pkg, writers):
    """without MSD_REDUCE_SEEN_TWICE a record needs --net-only or --net-verbatim; correctedbits 2 needs --net-verbatim"""
    n = 600
    m = writer_records(pkg, n)
    fwd = np.where(np.arange(n) % 2 == 0, F, F | S).astype(np.uint8)
    seen = []
    for verbatim in (False, True):
        for net_only in (False, True):
            want, wends = rs.stream_of(pkg, m, fwd, verbatim=verbatim, net_only=net_only)
            got, ends = writers[False].reduce_wire(m, fwd, verbatim=verbatim, net_only=net_only)
            assert got == want and (ends == wends).all()
            seen.append(len(got))
    assert seen[0] < seen[1] < seen[2] == seen[3]


def test_writer_capacity_and_empty_call(pkg, writers):
    t = writers[False]
    n = 1025
    m, fwd = writer_records(pkg, n), verdicts_for("random", n)
    want, _ = rs.stream_of(pkg, m, fwd)
    out = np.full(len(want), 0xAA, dtype=np.uint8)
    ends = np.full(n, 0xAAAAAAAA, dtype=np.uint32)
    need = C.c_size_t(0)
    args = (t.h, m.ctypes.data, fwd.ctypes.data, n, 0, 0, out.ctypes.data)
    assert t.f["reduce_wire"](*args, len(want) - 1, C.byref(need), ends.ctypes.data) == -errno.ENOSPC
    assert need.value == len(want) and (out == 0xAA).all() and (ends == 0xAAAAAAAA).all()
    assert t.f["reduce_wire"](*args, len(want), C.byref(need), ends.ctypes.data) == 0
    assert need.value == len(want) and out.tobytes() == want
    need.value = 77
    assert t.f["reduce_wire"](t.h, None, None, 0, 0, 0, None, 0, C.byref(need), None) == 0 and need.value == 0
    assert t.f["reduce_wire"](*args[:5], 4, out.ctypes.data, len(want), C.byref(need), None) == -errno.EINVAL
    assert t.f["reduce_wire"](t.h, None, fwd.ctypes.data, n, 0, 0, out.ctypes.data, len(want), C.byref(need), None) == -errno.EINVAL
    assert t.f["reduce_wire"](t.h, m.ctypes.data, fwd.ctypes.data, (1 << 24) + 1, 0, 0, out.ctypes.data, len(want), C.byref(need),
                              None) == -errno.EINVAL


# ---- machinery ----
def test_rolled_back_update_moves_no_timer(pkg, torch_cuda, scen):
    s = scen["df5_squawk"]
    m, f, r = rs.records(s["steps"])
    b = rs.Builder(pkg)
    b.squawk5(rs.T0 + 600, 0x120001)
    for k in range(70):
        b.squawk5(rs.T0 + 600, 0x300000 + k)
    _, bm, bf, br = b.step()
    res = []
    for fail_first in (True, False):
        t = tracker(pkg, False, [None], 125, 64)
        t.update_reduce(m[:1], f[:1], r[:1])
        if fail_first:  # 71 aircraft do not fit 64 slots: nothing changes, no verdict is written
            out = np.zeros(len(bm), dtype=pkg.capi.POSITION_DTYPE)
            fwd = np.full(len(bm), 0xEE, dtype=np.uint8)
            rc = t.f["update_reduce"](t.h, bm.ctypes.data, bf.ctypes.data, br.ctypes.data, len(bm), 0, out.ctypes.data, None,
                                      fwd.ctypes.data)
            assert rc == -errno.ENOSPC and (fwd == 0xEE).all() and t.live() == 1
        res.append(t.update_reduce(bm[:40], bf[:40], br[:40])[2].tobytes() + t.update_reduce(m[1:], f[1:], r[1:])[2].tobytes())
        t.close()
    assert res[0] == res[1]
    # the first of the forty was the known aircraft's, 600 ms after its squawk of T0: due (T0 + 500)
    assert res[0][0] == F | S and res[0][1] == F


def test_reset_and_refusals(pkg, torch_cuda, scen):
    s = scen["df5_squawk"]
    m, f, r = rs.records(s["steps"])

    def code(call):
        with pytest.raises(pkg.MsdError) as e:
            call()
        return e.value.code
    t = pkg.capi.PositionTracker(capacity=64)
    assert code(lambda: t.reduce_enable(125)) == -errno.EINVAL
    t.close()
    t = pkg.capi.PositionTracker(capacity=64, table=True)
    assert code(lambda: t.reduce_enable(15001)) == -errno.EINVAL
    t.update_nicrc(m[:1], f[:1], r[:1])  # before enabling: the aircraft starts with timers of 0
    t.reduce_enable(125)
    t.reduce_enable(125)
    assert code(lambda: t.reduce_enable(126)) == -errno.EINVAL
    assert list(t.update_reduce(m[1:], f[1:], r[1:])[2]) == [F | S, S]  # T0 + 500: due against 0 (-> T0 + 1000); T0 + 501: not
    t.reset()
    assert list(t.update_reduce(m, f, r)[2]) == s["verdicts"]
    t.close()


def test_a_tracker_that_does_not_reduce(pkg, torch_cuda):
    """delivers what it delivered, whether or not another one reduces, and refuses the two new calls"""
    receivers, m, f, r = acs.mixed_stream(pkg)
    steps = [("update", m, f, r)]
    res = {}
    for key, host, interval in (("twin", True, None), ("plain", False, None), ("reducing", False, 125)):
        t = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, host=host, table=True, modeac=True,
                                     reduce_interval_ms=interval)
        rows, nic, snaps = acs.run_library(t, steps, every_step=False)
        t.modeac_match(acs.T0 + 5000, acs.T0 + 5000)
        res[key] = (rows.tobytes(), nic.tobytes(), snaps[-1].tobytes(), t.modeac_hits().tobytes(), t.modeac_codes(0).tobytes())
        if key == "plain":
            for call in (lambda: t.update_reduce(m[:5], f[:5], r[:5]), lambda: t.reduce_wire(m[:5], np.ones(5, dtype=np.uint8))):
                with pytest.raises(pkg.MsdError) as e:
                    call()
                assert e.value.code == -errno.EINVAL
        t.close()
    assert res["plain"] == res["twin"] and res["reducing"] == res["twin"]
