"""The machinery around the position tracker's per-record logic, which exists on the device only (msd_pos_kernels.hip,
msd_pos.cpp): the compare-and-swap table with linear probing, the rollback after -ENOSPC / -EINVAL, the expiry rebuild
into the second table, one to four stable 8-bit counting passes (tile counts, the one-workgroup scan with its carry, the
ballot-rank scatter), the head-of-run walk, the cut of a call into pieces of 2^20 records, the atomic reductions.  The
host twin does all of it with a serial loop and is the reference: the POSITION_DTYPE rows byte for byte, the thirteen
counters and the live-aircraft count.  Nothing delivered depends on the capacity except -ENOSPC (asserted on the twin in
test_positions_model.py), so the twin runs at whatever capacity holds the stream.  Every stream keeps every gate at
least 1 m from its limit on the twin (asserted in every test)."""
import errno
import time

import numpy as np
import pytest

import pos_streams as ps

pytestmark = pytest.mark.gpu
COUNTERS = ("cpr_surface", "cpr_airborne", "cpr_global_ok", "cpr_global_bad", "cpr_global_skipped", "cpr_global_range_checks",
            "cpr_global_speed_checks", "cpr_local_ok", "cpr_local_aircraft_relative", "cpr_local_receiver_relative",
            "cpr_local_skipped", "cpr_local_range_checks", "cpr_local_speed_checks", "aircraft")


def run(pkg, host, capacity, receivers, fp, steps, pieces=None):
    t = pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, filter_persistence=fp, host=host)
    out = ps.run_library(t, steps, pieces)
    st = t.stats()
    t.close()
    if host:
        assert st["min_gate_margin_m"] >= 1.0, st["min_gate_margin_m"]
    return out, st


def same(got, want):
    (g, gst), (h, hst) = got, want
    assert len(g) == len(h)
    assert g.tobytes() == h.tobytes(), [(i, g[i], h[i]) for i in range(len(g)) if g[i].tobytes() != h[i].tobytes()][:5]
    assert {k: gst[k] for k in COUNTERS} == {k: hst[k] for k in COUNTERS}
    assert gst["min_gate_margin_m"] >= 1.0 and hst["min_gate_margin_m"] >= 1.0


def on_device(torch, m, f, r):
    """-> device tensors of the records and the receiver indices (keep them alive over the call)"""
    return (torch.from_numpy(m.view(np.uint8).copy()).cuda(), torch.from_numpy(f.view(np.uint8).copy()).cuda(),
            torch.from_numpy(r.view(np.int32).copy()).cuda())


def drive(pkg, torch, t, ops):
    """ops through one tracker, the GPU's or the twin: ("update", m, f, r), ("device", m, f, r) -- the records and the
    receiver array in device memory where the tracker is the GPU's --, ("expire", now), ("alive", n),
    ("fails", code, kind, m, f, r) -- the call fails with that code and changes nothing --, ("receiver", index, kw or
    None for the C entry's null pointer).  -> the rows of the calls that passed, the statistics."""
    outs = []

    def call(kind, m, f, r):
        if kind == "device" and not t.host:
            dm, df, dr = on_device(torch, m, f, r)
            return t.update_device(dm.data_ptr(), df.data_ptr(), len(m), dr.data_ptr())
        return t.update(m, f, r)

    for op in ops:
        if op[0] in ("update", "device"):
            outs.append(call(*op))
        elif op[0] == "expire":
            t.expire(op[1])
        elif op[0] == "alive":
            assert t.stats()["aircraft"] == op[1], (t.host, op[1], t.stats()["aircraft"])
        elif op[0] == "fails":
            before = t.stats()
            with pytest.raises(pkg.MsdError) as e:
                call(*op[2:])
            assert e.value.code == op[1], (t.host, e.value.code)
            assert t.stats() == before
        elif op[0] == "receiver":
            if op[2] is None:
                assert t.f["set_receiver"](t.h, op[1], None) == 0
            else:
                t.set_receiver(op[1], **op[2])
        else:
            raise ValueError(op[0])
    return np.concatenate(outs), t.stats()


def drive_both(pkg, torch, capacity, receivers, ops):
    res = []
    for host in (False, True):
        t = pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, host=host)
        res.append(drive(pkg, torch, t, ops))
        t.close()
    same(*res)
    return res[0]


def place(k):
    return 10.0 + 0.1 * k, 20.0 + 0.05 * k


# ---- a. one to four counting passes ----
@pytest.fixture(scope="module")
def mixed(pkg):
    receivers, m, f, r = ps.mixed_stream(pkg)
    steps = [("update", m, f, r)]
    return receivers, steps, run(pkg, True, 1024, receivers, 0, steps)


@pytest.mark.parametrize("capacity", [64, 128, 256, 32768, 65536, 1 << 18, 1 << 24])
def test_pass_count(pkg, torch_cuda, mixed, capacity):
    """1, 1, 2, 2, 3, 3 and 4 passes.  At 128 the skipped records' slot value is the largest value of the one digit, at
    256 the second pass has nothing to separate but them; at 2^24 the device table is 4.8 GB and the twin's is not made."""
    receivers, steps, want = mixed
    same(run(pkg, False, capacity, receivers, 0, steps), want)


@pytest.mark.parametrize("capacity", [128, 256, 65536])
def test_skipped_records_beside_slot_zero(pkg, torch_cuda, capacity):
    """Aircraft in slot 0, slot 1 and the last slot, their records between Mode A/C records and address 0.  The skipped
    records' slot value `cap` has the digits of slot 0 below its top bit: a pass too few (256 and 65536 need their last
    pass for nothing else) would leave them inside slot 0's run and start a second walker in it."""
    addrs = ps.chain_addresses(pkg, capacity)
    b = ps.Builder(pkg)
    for k in range(100):
        t = ps.T0 + 500 * k
        b.pos(t, addrs[3], 40.0 + 2e-4 * k, 5.0, k & 1)
        b.rec(t + 1, 0x7123, msgtype=32, source=ps.ip.MODE_AC)
        b.pos(t + 2, addrs[4], -30.0, 100.0 + 2e-4 * k, k & 1)
        b.rec(t + 3, 0, msgtype=11, source=ps.ip.MODE_S)
        b.pos(t + 4, addrs[0], 60.0 - 2e-4 * k, -70.0, k & 1)
    steps = [b.step()]
    want = run(pkg, True, 1024, [None], 0, steps)
    assert want[1]["aircraft"] == 3 and want[1]["cpr_global_ok"] == 3 * 99
    same(run(pkg, False, capacity, [None], 0, steps), want)


def test_one_aircraft_three_passes(pkg, torch_cuda):
    """Every tile is one digit only in every pass: rank 0..63 per wave and the sum over the waves before."""
    b = ps.Builder(pkg)
    for k in range(300):
        if k % 10 == 9:
            b.vel(ps.T0 + 500 * k, 0x4B1234, 300, 300)
        else:
            b.pos(ps.T0 + 500 * k, 0x4B1234, 47.0 + 5e-4 * k, 8.0 + 5e-4 * k, k & 1)
    steps = [b.step()]
    want = run(pkg, True, 64, [None], 0, steps)
    assert want[1]["aircraft"] == 1 and want[1]["cpr_global_ok"] > 250
    same(run(pkg, False, 65536, [None], 0, steps), want)


# ---- b. tile and scan-chunk edges ----
@pytest.fixture(scope="module")
def edges(pkg):
    receivers, m, f, r = ps.wide_stream(pkg, aircraft=300, records=2048, skipped_every=17)
    steps = [("update", m, f, r)]
    return receivers, steps, run(pkg, True, 1024, receivers, 0, steps)


@pytest.mark.parametrize("pieces", [None, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_call_lengths_on_wave_tile_and_scan_edges(pkg, torch_cuda, edges, pieces):
    """Calls of a wave, a tile and a scan chunk (1024 records are 1024 count words, 1025 are 1280 and the first carry),
    one less and one more; every cut also leaves a last call of another length."""
    receivers, steps, want = edges
    same(run(pkg, False, 1024, receivers, 0, steps, pieces), want)


# ---- c. many tiles; g. the margin ----
@pytest.fixture(scope="module")
def many(pkg):
    receivers, m, f, r = ps.wide_stream(pkg, aircraft=5000, records=20000, receivers=3, skipped_every=17)
    return receivers, (m, f, r), run(pkg, True, 8192, receivers, 0, [("update", m, f, r)])


@pytest.mark.parametrize("capacity", [8192, 65536])
def test_many_tiles(pkg, torch_cuda, many, capacity):
    """79 tiles, 20 scan chunks with 19 carries, every aircraft's run across tile boundaries, two and three passes, the
    smaller table 61 % full."""
    receivers, (m, f, r), want = many
    same(run(pkg, False, capacity, receivers, 0, [("update", m, f, r)]), want)


def test_many_tiles_from_device_memory(pkg, torch_cuda, many):
    receivers, (m, f, r), want = many
    t = pkg.capi.PositionTracker(capacity=8192, receivers=receivers)
    dm, df, dr = on_device(torch_cuda, m, f, r)
    got = t.update_device(dm.data_ptr(), df.data_ptr(), len(m), dr.data_ptr())
    st = t.stats()
    t.close()
    same((got, st), want)


def test_gate_margin_is_the_minimum_over_all_walkers(pkg, torch_cuda, many):
    """5000 walkers reduce their margins with an integer minimum over the double's bits.  The contract (modes_hip.h)
    promises equal records while the twin's margin is above 1e-3 m, which holds only if no device distance is further
    than that from the host's; the minimum of two sets that differ pairwise by at most d differs by at most d.
    Measured on an MI355X: the two margins are 1103.394605962673 m both, difference 0."""
    receivers, (m, f, r), (_, hst) = many
    _, gst = run(pkg, False, 8192, receivers, 0, [("update", m, f, r)])
    diff = abs(gst["min_gate_margin_m"] - hst["min_gate_margin_m"])
    print("min_gate_margin_m: gpu %.17g twin %.17g difference %.3g m" % (gst["min_gate_margin_m"], hst["min_gate_margin_m"], diff))
    assert diff <= 1e-3


# ---- d. a call of more than one piece ----
def test_pieces(pkg, torch_cuda):
    """2^20 + 4099 + 257 records of 4099 aircraft in one call: 255 or 256 records of every aircraft in the first piece,
    its last one or two in the second, which is 17 tiles and a bit; the walk of the second piece starts from the state
    the first one stored.  Measured on an MI355X: the GPU call takes 0.03 s, the whole test with the stream and the twin 0.4 s."""
    t0 = time.perf_counter()
    n = (1 << 20) + 4099 + 257
    receivers, m, f, r = ps.wide_stream(pkg, aircraft=4099, records=n)
    steps = [("update", m, f, r)]
    want = run(pkg, True, 8192, receivers, 0, steps)
    t = pkg.capi.PositionTracker(capacity=8192, receivers=receivers)
    t1 = time.perf_counter()
    whole = t.update(m, f, r)
    t2 = time.perf_counter()
    wst = t.stats()
    t.reset()
    cut = (1 << 20) - 100
    two = np.concatenate([t.update(m[:cut], f[:cut], r[:cut]), t.update(m[cut:], f[cut:], r[cut:])])
    tst = t.stats()
    t.close()
    same((whole, wst), want)
    same((two, tst), want)
    assert np.float64(tst["min_gate_margin_m"]).tobytes() == np.float64(wst["min_gate_margin_m"]).tobytes()
    tail = whole[1 << 20:]
    assert int(((tail["decoded"] == 1) & (tail["relative"] == 0)).sum()) > 4000
    print("pieces: the GPU call of %d records %.3f s, the test %.1f s" % (n, t2 - t1, time.perf_counter() - t0))


# ---- e. a rolled-back call leaves no key behind ----
def test_rollback_leaves_nothing(pkg, torch_cuda):
    b = ps.Builder(pkg)
    for k in range(200):
        b.pos(ps.T0 + k, 0xA00000 + k, *place(k), 0)
    for k in range(200):
        b.pos(ps.T0 + 400 + k, 0xA00000 + k, *place(k), 1)
    fill = b.step()
    for rep in range(3):  # 100 new aircraft x 3 records between records of 50 known ones, which must not move either
        for k in range(100):
            b.pos(ps.T0 + 600 + 100 * rep, 0xB00000 + k, *place(k), rep & 1)
            if rep == 1 and k % 2 == 0:
                b.pos(ps.T0 + 700, 0xA00000 + k, place(k)[0] + 0.05, place(k)[1], 1)
    over = b.step()
    for k in range(56):
        b.pos(ps.T0 + 800, 0xC00000 + k, *place(k), 0)
    _, bm, bf, br = b.step()
    br = br.copy()
    br[30] = 1  # one receiver there is
    for k in range(56):
        b.pos(ps.T0 + 900, 0xD00000 + k, *place(k), 0)
    fit = b.step()
    one_more = b.pos(ps.T0 + 950, 0xE00000, 1.0, 1.0, 0).step()
    for k in range(200):
        b.pos(ps.T0 + 1000 + k, 0xA00000 + k, *place(k), 0)
    for k in range(56):
        b.pos(ps.T0 + 1300, 0xD00000 + k, *place(k), 1)
    last = b.step()
    assert len(over[1]) == 350
    ops = [fill, ("alive", 200), ("fails", -errno.ENOSPC, *over), ("fails", -errno.EINVAL, "device", bm, bf, br),
           fit, ("alive", 256), ("fails", -errno.ENOSPC, *one_more), last, ("alive", 256)]
    g, st = drive_both(pkg, torch_cuda, 256, [None], ops)
    assert [int(x) for x in g["result"][-256:]] == [0] * 256  # every live aircraft's pair, the 50 as if never disturbed
    assert st["cpr_global_ok"] == 200 + 256 and st["cpr_global_speed_checks"] == 0


# ---- f. a probe chain across the table's end, and aircraft leaving from its middle ----
@pytest.mark.parametrize("variant", ps.CHAIN_VARIANTS)
def test_chain_across_the_end(pkg, torch_cuda, variant):
    receivers, fp, steps = ps.chain_scenario(pkg, 64, variant)
    ops = []
    for s, alive in zip(steps, ps.CHAIN_ALIVE[variant]):
        ops += [s, ("alive", alive)]
    g, st = drive_both(pkg, torch_cuda, 64, receivers, ops)
    assert [int(x) for x in g["result"][-3:]] == [0, 0, 0] and st["cpr_global_ok"] == 6


def test_crowded_table_through_expiry(pkg, torch_cuda):
    """60 aircraft in 64 slots, every second one heard once: after the expiry 30 remain in the other table, 34 new ones
    fit exactly, and the survivors' late odd halves pair with the even halves that were stored before the rebuild."""
    b = ps.Builder(pkg)
    for k in range(60):
        b.pos(ps.T0, 0x4A0000 + 7 * k, *place(k), 0)
    for k in range(0, 60, 2):
        b.pos(ps.T0 + 400, 0x4A0000 + 7 * k, *place(k), 1)
    fill = b.step()
    for k in range(0, 60, 2):
        b.pos(ps.T0 + 61000, 0x4A0000 + 7 * k, *place(k), 0)
    even = b.step()
    for k in range(34):
        b.pos(ps.T0 + 61200, 0x4B0000 + k, *place(k), 0)
    new = b.step()
    one_more = b.pos(ps.T0 + 61300, 0x4C0000, 1.0, 1.0, 0).step()
    for k in range(0, 60, 2):
        b.pos(ps.T0 + 61400, 0x4A0000 + 7 * k, *place(k), 1)
    late = b.step()
    ops = [fill, ("alive", 60), even, ("expire", ps.T0 + 61001), ("alive", 30), new, ("alive", 64),
           ("fails", -errno.ENOSPC, *one_more), late, ("alive", 64)]
    g, st = drive_both(pkg, torch_cuda, 64, [None], ops)
    assert [int(x) for x in g["result"][-30:]] == [0] * 30
    assert np.allclose(g["lat"][-30:], [place(k)[0] for k in range(0, 60, 2)], atol=1e-4)


# ---- h. msd_pos_set_receiver ----
def test_set_receiver(pkg, torch_cuda):
    b = ps.Builder(pkg)
    nowhere = b.pos(ps.T0, 0x4C0001, 52.5, 5.0, 0, rx=0).pos(ps.T0, 0x4C0002, 52.5, 5.0, 0, rx=1).step()
    placed = b.pos(ps.T0 + 1000, 0x4C0003, 52.5, 5.0, 0, rx=0).pos(ps.T0 + 1000, 0x4C0004, 52.5, 5.0, 1, rx=1).step()
    gone = b.pos(ps.T0 + 2000, 0x4C0005, 52.5, 5.0, 0, rx=1).step()
    ops = [nowhere, ("receiver", 1, dict(lat=52.0, lon=4.0, max_range_m=150 * ps.NM)), placed, ("receiver", 1, None), gone]
    g, st = drive_both(pkg, torch_cuda, 64, [None, None], ops)
    assert [int(x) for x in g["result"]] == [-1, -1, -1, 2, -1]
    assert int(g["relative"][3]) == 2 and abs(g["lat"][3] - 52.5) < 1e-4 and abs(g["lon"][3] - 5.0) < 1e-4
    assert st["cpr_local_receiver_relative"] == 1 and st["aircraft"] == 5
