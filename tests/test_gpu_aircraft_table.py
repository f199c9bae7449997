"""The aircraft table on the GPU (msd_pos_create_table, msd_pos_update_nicrc, msd_pos_snapshot) against the host twin,
which test_aircraft_model.py holds equal to a second reading of track.c.  Everything is compared by the bytes of the
snapshot and of the NIC / Rc array: the contract has no tolerance.  Beside the per-record rules (every scenario, the
mixed stream) this covers what exists on the device only: the second walk over the grouped order, the table entry that
moves with its key through the expiry rebuild, the rollback, and the snapshot's compaction and key-ordered counting passes.
Every stream keeps every plausibility gate at least 1 m from its limit on the twin."""
import ctypes as C
import errno
import time

import numpy as np
import pytest

import aircraft_streams as acs
import indep_positions as ip
import pos_streams as ps
import range_streams as rs
import whole_stack as ws

pytestmark = pytest.mark.gpu
T0 = ps.T0


def run(pkg, host, capacity, receivers, fp, steps, pieces=None, every_step=True):
    t = pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, filter_persistence=fp, host=host, table=True)
    out = acs.run_library(t, steps, pieces, every_step)
    st = t.stats()
    t.close()
    if host:
        assert st["min_gate_margin_m"] >= 1.0, st["min_gate_margin_m"]
    return out


def same(got, want):
    assert got[0].tobytes() == want[0].tobytes()
    assert got[1].tobytes() == want[1].tobytes(), [(i, got[1][i], want[1][i]) for i in range(len(want[1])) if got[1][i] != want[1][i]][:5]
    assert len(got[2]) == len(want[2])
    for k, (g, w) in enumerate(zip(got[2], want[2])):
        assert len(g) == len(w), (k, len(g), len(w))
        if g.tobytes() != w.tobytes():
            bad = [(hex(int(w[i]["addr"])), n) for i in range(len(w)) for n in w.dtype.names if g[i][n].tobytes() != w[i][n].tobytes()]
            raise AssertionError((k, bad[:8]))


@pytest.fixture(scope="module")
def scen(pkg):
    return acs.scenarios(pkg)


@pytest.fixture(scope="module")
def mixed(pkg):
    receivers, m, f, r = acs.mixed_stream(pkg)
    steps = [("update", m, f, r)]
    return receivers, steps, run(pkg, True, 1024, receivers, 0, steps)


# ---- the rules ----
@pytest.mark.parametrize("name", acs.NAMES)
def test_scenario(pkg, torch_cuda, scen, name):
    receivers, fp, steps, check = scen[name]
    got = run(pkg, False, 1024, receivers, fp, steps)
    same(got, run(pkg, True, 1024, receivers, fp, steps))
    # the device's own result against the answer derived by hand: a rule wrong in the shared header fails here too
    check([{int(e["addr"]): e for e in s} for s in got[2]], [(int(q["nic"]), int(q["rc"]), int(q["set"])) for q in got[1]])


def test_mixed_stream(pkg, torch_cuda, mixed):
    receivers, steps, want = mixed
    same(run(pkg, False, 1024, receivers, 0, steps), want)


@pytest.mark.parametrize("pieces", [1, 64])
def test_cutting(pkg, torch_cuda, mixed, pieces):
    """The mixed stream as calls of 1 and of 64 records: the rows, the NIC / Rc and the snapshot of the one call."""
    receivers, steps, want = mixed
    got = run(pkg, False, 1024, receivers, 0, steps, pieces, every_step=False)
    same(got, want)


# ---- the drawn stream through everything at once (whole_stack.py): table, Mode A/C, verdicts, SBS, aircraft.pb, VRS, range ----
@pytest.fixture(scope="module")
def drawn(pkg):
    receivers, m, f, r = acs.random_stream(pkg)
    steps, now = ws.steps_of(m, f, r)
    t = ws.tracker(pkg, receivers, True)
    host = ws.run_library(t, steps, now)
    t.close()
    assert host["stats"]["min_gate_margin_m"] >= rs.GATE_MARGIN and host["pb_margin"] >= pkg.capi.PB_RSSI_MARGIN_ULPS
    assert host["margins"]["min_range_margin_m"] >= rs.RANGE_MARGIN and host["margins"]["min_bearing_margin_deg"] >= rs.BEARING_MARGIN
    return receivers, steps, now, host


def test_drawn_stream(pkg, torch_cuda, drawn):
    """Every byte the device delivers is the host object's, and after the last step equal to the second readings'."""
    receivers, steps, now, host = drawn
    t = ws.tracker(pkg, receivers, False)
    got = ws.run_library(t, steps, now)
    t.close()
    ws.same_bytes(got, host)
    ws.run_models(pkg, receivers, steps, now, got, margins=False)


@pytest.mark.parametrize("pieces", [1, 64, 97])
def test_drawn_stream_cut_into_calls(pkg, torch_cuda, drawn, pieces):
    receivers, steps, now, host = drawn
    t = ws.tracker(pkg, receivers, False)
    got = ws.run_library(t, steps, now, pieces)
    t.close()
    ws.same_bytes(got, host)


# ---- shapes of the walk ----
def test_more_walkers_than_a_wavefront(pkg, torch_cuda):
    receivers, m, f, r = acs.wide_stream(pkg, aircraft=65, records=65 * 12)
    steps = [("update", m, f, r)]
    want = run(pkg, True, 1024, receivers, 0, steps)
    assert len(want[2][-1]) == 65 and int(want[1]["set"].sum()) > 65 * 9
    same(run(pkg, False, 1024, receivers, 0, steps), want)


def test_one_aircraft_is_a_serial_walk(pkg, torch_cuda):
    receivers, m, f, r = acs.wide_stream(pkg, aircraft=1, records=300)
    steps = [("update", m, f, r)]
    want = run(pkg, True, 64, receivers, 0, steps)
    e = want[2][-1][0]
    assert len(want[2][-1]) == 1 and int(e["messages"]) == 300 and int(e["alt_baro"]) > 5000
    same(run(pkg, False, 65536, receivers, 0, steps), want)


@pytest.fixture(scope="module")
def edges(pkg):
    receivers, m, f, r = acs.wide_stream(pkg, aircraft=300, records=2048, skipped_every=17)
    steps = [("update", m, f, r)]
    return receivers, steps, run(pkg, True, 1024, receivers, 0, steps, every_step=False)


@pytest.mark.parametrize("pieces", [63, 64, 65, 255, 256, 257])
def test_call_lengths_on_wave_and_tile_edges(pkg, torch_cuda, edges, pieces):
    receivers, steps, want = edges
    same(run(pkg, False, 1024, receivers, 0, steps, pieces, every_step=False), want)


def test_pieces(pkg, torch_cuda):
    """2^20 + 300 records of 4099 aircraft in one call: the walk is cut after 2^20 records, and the 300 aircraft of the
    second piece continue from the table entries the first piece's walk left."""
    t0 = time.perf_counter()
    n = (1 << 20) + 300
    receivers, m, f, r = acs.wide_stream(pkg, aircraft=4099, records=n)
    steps = [("update", m, f, r)]
    want = run(pkg, True, 8192, receivers, 0, steps)
    t1 = time.perf_counter()
    got = run(pkg, False, 8192, receivers, 0, steps)
    t2 = time.perf_counter()
    same(got, want)
    tail = want[1][1 << 20:]
    assert len(want[2][-1]) == 4099 and int(tail["set"].sum()) > 290
    print("pieces: the GPU tracker with its snapshot %.3f s, the test %.1f s" % (t2 - t1, time.perf_counter() - t0))


# ---- shapes of the snapshot ----
def population(pkg, count, receivers=1, t=T0):
    b = acs.Builder(pkg)
    for k in range(count):
        b.alt(t + k, 0x400000 + 7919 * k % 0xFFFFF, 1000 + 25 * k, rx=k % receivers, squawk_valid=1, squawk=k & 0xFFF)
    return [b.step()] if count else []


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_snapshot_sizes(pkg, torch_cuda, count):
    steps = population(pkg, count)
    res = []
    for host in (False, True):
        t = pkg.capi.PositionTracker(capacity=2048, host=host, table=True)
        acs.run_library(t, steps, every_step=False) if steps else None
        res.append(t.snapshot())
        assert t.live() == count
        t.close()
    assert len(res[0]) == count and res[0].tobytes() == res[1].tobytes()
    assert list(res[0]["addr"]) == sorted(res[0]["addr"])


def test_snapshot_of_a_full_table(pkg, torch_cuda):
    steps = population(pkg, 64)
    got, want = run(pkg, False, 64, [None], 0, steps), run(pkg, True, 64, [None], 0, steps)
    assert len(want[2][-1]) == 64
    same(got, want)


def test_snapshot_order_is_receiver_then_address(pkg, torch_cuda):
    b = acs.Builder(pkg)
    for k, (rx, addr) in enumerate(((1, 0x10), (0, 0xFFFFFF), (1, 0x0F), (0, 0x10), (2, 0x01), (0, 0x1000010))):
        b.alt(T0 + k, addr, 1000 * (k + 1), rx=rx)
    steps = [b.step()]
    got, want = run(pkg, False, 64, [None] * 3, 0, steps), run(pkg, True, 64, [None] * 3, 0, steps)
    same(got, want)
    s = got[2][-1]
    assert [(int(e["receiver"]), int(e["addr"])) for e in s] == [(0, 0x10), (0, 0xFFFFFF), (0, 0x1000010), (1, 0x0F), (1, 0x10), (2, 0x01)]
    assert [int(e["alt_baro"]) for e in s] == [4000, 2000, 6000, 3000, 1000, 5000]


def test_snapshot_with_the_highest_key_byte_in_use(pkg, torch_cuda):
    """65536 receivers: the key has 41 bits and the snapshot six passes, the last over bits 40 and up."""
    b = acs.Builder(pkg)
    rxs = [65535, 0, 32768, 255, 256, 65534, 1]
    for k, rx in enumerate(rxs):
        b.alt(T0 + k, 0x4840D6, 1000 * (k + 1), rx=rx).alt(T0 + k, 0x000001 + k, 500, rx=rx)
    steps = [b.step()]
    got, want = run(pkg, False, 64, [None] * 65536, 0, steps), run(pkg, True, 64, [None] * 65536, 0, steps)
    same(got, want)
    assert [int(e["receiver"]) for e in got[2][-1]][::2] == sorted(rxs)


def test_snapshot_capacity_one_too_small_and_device_output(pkg, torch_cuda):
    steps = population(pkg, 100, receivers=2)
    t = pkg.capi.PositionTracker(capacity=256, receivers=[None, None], table=True)
    acs.run_library(t, steps, every_step=False)
    want = t.snapshot()
    buf = np.full(99 * pkg.capi.AIRCRAFT_DTYPE.itemsize, 0xAA, dtype=np.uint8)
    n = C.c_size_t(0)
    assert t.f["snapshot"](t.h, buf.ctypes.data, 99, 0, C.byref(n)) == -errno.ENOSPC
    assert n.value == 100 and (buf == 0xAA).all()
    d = torch_cuda.full((101 * pkg.capi.AIRCRAFT_DTYPE.itemsize,), 0x55, dtype=torch_cuda.uint8, device="cuda")
    assert t.snapshot_device(d.data_ptr(), 101) == 100
    back = d.cpu().numpy()
    assert back[:100 * 592].tobytes() == want.tobytes() and (back[100 * 592:] == 0x55).all()
    t.close()


# ---- machinery ----
@pytest.mark.parametrize("variant", ps.CHAIN_VARIANTS)
def test_table_entries_move_with_their_keys(pkg, torch_cuda, variant):
    """chain_scenario's five aircraft in one probe chain across the table's end; two expire from the middle and the
    survivors are inserted into the other table: their entries, NIC / Rc of the late odd halves included, are the twin's."""
    receivers, fp, steps = ps.chain_scenario(pkg, 64, variant)
    got, want = run(pkg, False, 64, receivers, fp, steps), run(pkg, True, 64, receivers, fp, steps)
    same(got, want)
    assert [len(s) for s in want[2]] == ps.CHAIN_ALIVE[variant]
    assert [tuple(int(x) for x in q) for q in want[1][-3:]] == [(186, 8, 1)] * 3
    assert all(int(e["nac_p"]) == 8 and int(e["messages"]) == 4 for e in want[2][-1])


def test_rolled_back_call_leaves_every_entry(pkg, torch_cuda):
    fill = population(pkg, 60)[0]
    b = acs.Builder(pkg)
    for k in range(10):  # ten new aircraft between records of five known ones: 70 do not fit 64 slots
        b.alt(T0 + 5000, 0x700000 + k, 9000).alt(T0 + 5000, 0x400000 + 7919 * k % 0xFFFFF, 30000, squawk_valid=1, squawk=0x7700)
    _, m, f, r = b.step()
    t = pkg.capi.PositionTracker(capacity=64, table=True)
    acs.run_library(t, [fill], every_step=False)
    before = t.snapshot()
    with pytest.raises(pkg.MsdError) as e:
        t.update_nicrc(m, f, r)
    assert e.value.code == -errno.ENOSPC
    after = t.snapshot()
    assert len(before) == 60 and after.tobytes() == before.tobytes()
    t.reset()
    assert len(t.snapshot()) == 0 and t.live() == 0
    acs.run_library(t, [fill], every_step=False)
    assert t.snapshot().tobytes() == before.tobytes()
    t.close()


@pytest.mark.parametrize("capacity", [64, 1 << 16])
def test_nothing_depends_on_capacity(pkg, torch_cuda, mixed, capacity):
    receivers, steps, want = mixed
    same(run(pkg, False, capacity, receivers, 0, steps), want)


# ---- table-less trackers ----
def test_table_less_tracker_refuses_and_agrees(pkg, torch_cuda):
    receivers, m, f, r = ps.mixed_stream(pkg)
    plain = pkg.capi.PositionTracker(capacity=1024, receivers=receivers)
    for call in (lambda: plain.update_nicrc(m[:10], f[:10], r[:10]), lambda: plain.snapshot(4)):
        with pytest.raises(pkg.MsdError) as e:
            call()
        assert e.value.code == -errno.EINVAL
    table = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, table=True)
    a, b = plain.update(m, f, r), table.update(m, f, r)
    sa, sb = plain.stats(), table.stats()
    plain.close(), table.close()
    assert a.tobytes() == b.tobytes()
    counters = [k for k in sa if k.startswith("cpr_")]
    assert len(counters) == 13 and {k: sa[k] for k in counters} == {k: sb[k] for k in counters} and sa["aircraft"] == sb["aircraft"]
