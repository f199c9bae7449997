"""Mode A/C matching on the GPU (msd_pos_modeac_enable / _match / _codes / _hits and the counting inside msd_pos_update)
against the host twin, which test_modeac_model.py holds equal to a second reading of track.c.  Everything is integer
work, so everything is compared by bytes: every receiver's 4096 entries, the hit rows, the msd_position and NIC / Rc rows
and the snapshots.  Beside the rules (every scenario, the mixed stream, each also cut into calls of 1, 63 and 257 records)
this covers what exists on the device only: the counting kernel's in-wave combining at wave and tile edges, the
compare-and-swap on the match word under contention, the per-slot and per-code sweeps at their tile edges, the hit bytes
that move through the expiry rebuild, the gather in snapshot order, and the rollback."""
import ctypes as C
import errno

import numpy as np
import pytest

import aircraft_streams as acs
import indep_modeac as im
import modeac_streams as mas
import pos_streams as ps

pytestmark = pytest.mark.gpu
T0 = ps.T0


def run(pkg, host, capacity, receivers, steps, pieces=None, every_step=True):
    t = pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, host=host, table=True, modeac=True)
    out = mas.run_library(t, len(receivers), steps, pieces, every_step)
    t.close()
    return out


def both(pkg, capacity, receivers, steps, pieces=None, every_step=True):
    got = run(pkg, False, capacity, receivers, steps, pieces, every_step)
    want = run(pkg, True, capacity, receivers, steps, pieces, every_step)
    mas.same_bytes(got, want)
    return want


@pytest.fixture(scope="module")
def scen(pkg):
    return mas.scenarios(pkg)


@pytest.fixture(scope="module")
def mixed(pkg):
    receivers, steps, whole = mas.mixed_steps(pkg)
    return receivers, steps, whole, run(pkg, True, 1024, receivers, steps)


# ---- the rules ----
@pytest.mark.parametrize("name", mas.NAMES)
def test_scenario(pkg, torch_cuda, scen, name):
    receivers, steps, check = scen[name]
    want = run(pkg, True, 64, receivers, steps)
    got = run(pkg, False, 64, receivers, steps)
    mas.same_bytes(got, want)
    check(got[2])
    for pieces in (1, 63, 257):
        mas.same_bytes(run(pkg, False, 64, receivers, steps, pieces), want)


@pytest.mark.parametrize("pieces", [None, 1, 63, 257])
def test_mixed_stream(pkg, torch_cuda, mixed, pieces):
    receivers, steps, _, want = mixed
    mas.same_bytes(run(pkg, False, 1024, receivers, steps, pieces), want)


# ---- shapes of the counting kernel ----
def counted(pkg, receivers, step, capacity=64):
    """one update step and a match on both -> the twin's last observation"""
    return both(pkg, capacity, receivers, [step, ("match", T0 + 1000, T0 + 1000)])[2][-1]


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_replies_of_one_code_at_wave_and_tile_edges(pkg, torch_cuda, n):
    o = counted(pkg, [None], mas.Builder(pkg).squawk(T0, 0x200001, 0x1200).reply(T0 + 1, 0x1200, n=n).step())
    assert tuple(o["codes"][0][mas.idx(0x1200)]) == (n, n, 0x200001, 10) and o["hits"] == {(0, 0x200001): (1, 0)}


def test_a_wave_of_two_codes_alternating(pkg, torch_cuda):
    b = mas.Builder(pkg)
    for k in range(150):
        b.reply(T0 + k, 0x1200 if k % 2 else 0x3400)
    c = counted(pkg, [None], b.step())["codes"][0]
    assert int(c[mas.idx(0x1200)]["count"]) == 75 and int(c[mas.idx(0x3400)]["count"]) == 75 and int(c["count"].sum()) == 150


def test_all_4096_codes_once_and_more_codes_than_combining_rounds(pkg, torch_cuda):
    b = mas.Builder(pkg)
    for i in range(4096):
        b.reply(T0 + i, im.index_to_mode_a(i))
    for k in range(640):  # waves of ten codes, unevenly often
        b.reply(T0 + 5000 + k, im.index_to_mode_a((k * k) % 10))
    c = counted(pkg, [None], b.step())["codes"][0]
    assert (c["count"][10:] == 1).all() and int(c["count"].sum()) == 4096 + 640


def test_one_code_on_two_receivers(pkg, torch_cuda):
    b = mas.Builder(pkg)
    for k in range(200):
        b.reply(T0 + k, 0x1200, rx=k % 2 if k < 100 else 1)
    c = counted(pkg, [None, None], b.step())["codes"]
    assert int(c[0][mas.idx(0x1200)]["count"]) == 50 and int(c[1][mas.idx(0x1200)]["count"]) == 150


def test_replies_interleaved_with_mode_s_records(pkg, torch_cuda):
    b = mas.Builder(pkg)
    for k in range(300):
        b.reply(T0 + k, 0x1200).alt(T0 + k, 0x210000 + k % 7, 10000 + 25 * (k // 7), squawk_valid=1, squawk=0x1200)
    o = counted(pkg, [None], b.step())
    assert tuple(o["codes"][0][mas.idx(0x1200)]) == (300, 300, 0xFFFFFFFF, 10) and len(o["hits"]) == 7
    assert all(h == (1, 0) for h in o["hits"].values())


def test_pieces_with_every_eighth_record_a_reply(pkg, torch_cuda):
    """2^20 + 300 records in one call: the walk is cut after 2^20 records, the counting kernel runs once over all of them"""
    n = (1 << 20) + 300
    receivers, m, f, r = acs.wide_stream(pkg, aircraft=4099, records=n)
    i = np.arange(0, n, 8)
    index = (i // 8) % 37 + np.where(i % 24 == 0, 1000, 0)
    m["msgtype"][::8] = 32
    f["squawk"][::8] = (index & 0o7) | ((index & 0o70) << 1) | ((index & 0o700) << 2) | ((index & 0o7000) << 3)
    steps = [("update", m, f, r), ("match", int(m["sysTimestampMsg"][-1]), int(m["sysTimestampMsg"][-1]))]
    want = both(pkg, 8192, receivers, steps, every_step=False)
    c = want[2][-1]["codes"][0]
    assert int(c["count"].sum()) == len(i) and int((c["count"] != 0).sum()) == 74
    assert (want[0]["result"][::8] == pkg.capi.POS_NOT_TRIED).all() and len(want[2][-1]["snap_raw"]) == 4099


def test_rolled_back_call_counts_nothing_then_a_call_counts(pkg, torch_cuda):
    b = mas.Builder(pkg)
    for k in range(60):
        b.squawk(T0 + k, 0x400000 + k, 0x1200)
    fill = b.step()
    for k in range(10):
        b.squawk(T0 + 100, 0x700000 + k, 0x1200).reply(T0 + 100, 0x1200, n=2)
    _, m, f, r = b.step()
    res = []
    for host in (False, True):
        t = pkg.capi.PositionTracker(capacity=64, host=host, table=True, modeac=True)
        mas.run_library(t, 1, [fill, b.reply(T0 + 90, 0x3300, n=3).step()])
        before = mas.observe(t, 1)
        with pytest.raises(pkg.MsdError) as e:
            t.update_nicrc(m, f, r)
        assert e.value.code == -errno.ENOSPC
        after = mas.observe(t, 1)
        assert after["codes"][0].tobytes() == before["codes"][0].tobytes() and int(after["codes"][0]["count"].sum()) == 3
        assert after["hits_raw"].tobytes() == before["hits_raw"].tobytes() and after["snap_raw"].tobytes() == before["snap_raw"].tobytes()
        t.update_nicrc(m[1::3], f[1::3], r[1::3])
        t.modeac_match(T0 + 1000, T0 + 1000)
        res.append(mas.observe(t, 1))
        assert int(res[-1]["codes"][0][mas.idx(0x1200)]["count"]) == 10 and int(res[-1]["hits_raw"]["mode_a_hit"].sum()) == 60
        t.reset()
        assert len(t.modeac_hits()) == 0 and not t.modeac_codes(0).view(np.uint32).any()
        mas.run_library(t, 1, [fill])
        assert len(t.modeac_hits()) == 60 and not t.modeac_hits()["mode_a_hit"].any()
        t.close()
    assert res[0]["codes"][0].tobytes() == res[1]["codes"][0].tobytes() and res[0]["hits_raw"].tobytes() == res[1]["hits_raw"].tobytes()


# ---- shapes of the match ----
def population(pkg, count, receivers=1, squawk=None):
    """count aircraft with a squawk (their own, or one for all) and an altitude 300 ft from the next one's, and four
    replies for every third one's squawk and for every fifth one's altitude"""
    b = mas.Builder(pkg)
    for k in range(count):
        code = squawk if squawk is not None else im.index_to_mode_a(1 + k % 4000)
        b.alt(T0 + k % 1000, 0x400000 + 7919 * k % 0xFFFFF, 1000 + 300 * (k % 100), rx=k % receivers, squawk_valid=1, squawk=code)
        if k % 3 == 0:
            b.reply(T0 + 1000, code, rx=k % receivers, n=4)
        if k % 5 == 0:
            b.reply(T0 + 1000, mas.code_of_feet(1000 + 300 * (k % 100)), rx=k % receivers, n=4)
    return b.step()


@pytest.mark.parametrize("capacity,count", [(64, 0), (64, 1), (64, 64), (256, 256), (512, 257)])
def test_match_sweep_over_tables_of_these_sizes(pkg, torch_cuda, capacity, count):
    """the per-slot sweep at its tile edges (a table of 256 slots holds at most 256 aircraft: full, one whole tile)"""
    steps = ([population(pkg, count)] if count else []) + [("match", T0 + 2000, T0 + 2000)]
    if not count:
        steps = [mas.Builder(pkg).reply(T0, 0x1200, n=4).step()] + steps
    o = both(pkg, capacity, [None], steps)[2][-1]
    assert len(o["hits"]) == count
    if count:
        assert sum(a for a, _ in o["hits"].values()) >= (count + 2) // 3 and sum(c for _, c in o["hits"].values()) >= (count + 4) // 5


def test_64_aircraft_on_one_squawk(pkg, torch_cuda):
    """one wave's worth of compare-and-swaps on one word, and a second word reached by exactly one aircraft"""
    steps = [population(pkg, 64, squawk=0x4321), ("match", T0 + 2000, T0 + 2000)]
    o = both(pkg, 64, [None], steps)[2][-1]
    assert tuple(o["codes"][0][mas.idx(0x4321)])[2:] == (0xFFFFFFFF, 10) and all(a == 1 for a, _ in o["hits"].values())
    alone = o["codes"][0][mas.idx(mas.code_of_feet(1000 + 300 * 5))]
    assert int(alone["match"]) == 0x400000 + 7919 * 5 % 0xFFFFF


@pytest.mark.parametrize("nrx", [1, 65])
def test_per_code_sweep_over_this_many_receivers(pkg, torch_cuda, nrx):
    steps = [population(pkg, 130, receivers=nrx), ("match", T0 + 2000, T0 + 2000)]
    for k in range(2, 6):
        steps.append(("match", T0 + 1000 * k + 1000, T0 + 2000))
    o = both(pkg, 256, [None] * nrx, steps)[2]
    assert any(c["age"].any() for c in o[-1]["codes"]) and o[1]["codes"][nrx - 1]["count"].any()


def test_probe_chain_across_the_end_of_the_table(pkg, torch_cuda):
    """five aircraft in one probe chain over slots 63, 0, 1, 2, 3: each finds its own entry and hit bytes"""
    chain = ps.chain_addresses(pkg, 64)
    b = mas.Builder(pkg)
    for j, a in enumerate(chain):
        b.squawk(T0 + j, a, im.index_to_mode_a(100 + j))
        if j % 2 == 0:
            b.reply(T0 + 10, im.index_to_mode_a(100 + j), n=4)
    o = both(pkg, 64, [None], [b.step(), ("match", T0 + 1000, T0 + 1000)])[2][-1]
    assert o["hits"] == {(0, a): (1 - j % 2, 0) for j, a in enumerate(chain)}


# ---- delivery of the hits ----
@pytest.mark.parametrize("count", [0, 1, 1025])
def test_hits_rows_are_the_snapshots_rows(pkg, torch_cuda, count):
    steps = ([population(pkg, count)] if count else []) + [("match", T0 + 2000, T0 + 2000)]
    o = both(pkg, 2048, [None], steps)[2][-1]  # observe() holds row j of the hits to row j of the snapshot
    assert len(o["hits_raw"]) == count and list(o["hits_raw"]["addr"]) == sorted(o["hits_raw"]["addr"])
    assert not count or o["hits_raw"]["mode_a_hit"].any()


def test_hits_capacity_one_too_small_and_device_output(pkg, torch_cuda):
    t = pkg.capi.PositionTracker(capacity=256, receivers=[None, None], table=True, modeac=True)
    mas.run_library(t, 2, [population(pkg, 100, receivers=2), ("match", T0 + 2000, T0 + 2000)], every_step=False)
    want = t.modeac_hits()
    assert len(want) == 100 and want["mode_a_hit"].any() and want["mode_c_hit"].any()
    buf = np.full(99 * 16, 0xAA, dtype=np.uint8)
    n = C.c_size_t(0)
    assert t.f["modeac_hits"](t.h, buf.ctypes.data, 99, 0, C.byref(n)) == -errno.ENOSPC
    assert n.value == 100 and (buf == 0xAA).all()
    d = torch_cuda.full((101 * 16,), 0x55, dtype=torch_cuda.uint8, device="cuda")
    assert t.modeac_hits_device(d.data_ptr(), 101) == 100
    back = d.cpu().numpy()
    assert back[:1600].tobytes() == want.tobytes() and (back[1600:] == 0x55).all()
    dc = torch_cuda.full((4097 * 16,), 0x55, dtype=torch_cuda.uint8, device="cuda")
    t.modeac_codes_device(1, dc.data_ptr())
    back = dc.cpu().numpy()
    assert back[:65536].tobytes() == t.modeac_codes(1).tobytes() and (back[65536:] == 0x55).all()
    t.close()


# ---- trackers that do not match ----
def test_plain_and_enabled_trackers_deliver_todays_bytes(pkg, torch_cuda):
    """a table tracker without matching refuses the calls and skips Mode A/C records as before; one with matching, fed
    the same stream (its few Mode A/C records match nobody), delivers the same rows, NIC / Rc and snapshot; both are the
    twin's"""
    receivers, m, f, r = acs.mixed_stream(pkg)
    steps = [("update", m, f, r)]
    res = []
    for host, modeac in ((False, False), (False, True), (True, False)):
        t = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, host=host, table=True, modeac=modeac)
        if not modeac:
            for call in (lambda: t.modeac_match(T0, T0), lambda: t.modeac_codes(0), lambda: t.modeac_hits(4)):
                with pytest.raises(pkg.MsdError) as e:
                    call()
                assert e.value.code == -errno.EINVAL
        rows, nic, snaps = acs.run_library(t, steps, every_step=False)
        if modeac:
            t.modeac_match(int(m["sysTimestampMsg"][-1]), int(m["sysTimestampMsg"][-1]))
            assert not t.modeac_hits()["mode_a_hit"].any() and not t.modeac_hits()["mode_c_hit"].any()
            assert int(t.modeac_codes(0)["count"].sum() + t.modeac_codes(1)["count"].sum()) == int((m["msgtype"] == 32).sum())
            snaps = [t.snapshot()]
        res.append((rows.tobytes(), nic.tobytes(), snaps[-1].tobytes()))
        t.close()
    assert res[0] == res[2] and res[1] == res[2]
    bare = pkg.capi.PositionTracker(capacity=64)
    with pytest.raises(pkg.MsdError) as e:
        bare.modeac_enable()
    assert e.value.code == -errno.EINVAL
    bare.close()


# ---- end to end ----
def test_capture_to_matches(pkg, torch_cuda):
    """a generated capture with Mode S frames and Mode A/C replies through a context with mode_ac = 1, its records and
    fields (msd_collect_fields) handed to the tracker in device memory, and one match"""
    n = 8 * 131072 + 333
    iq = pkg.siggen.generate(pkg.siggen.make_cfg(seed=606, msgs_per_sec=5000, ac_per_sec=600, n_aircraft=80), n)
    d_iq = torch_cuda.from_numpy(iq).to("cuda:0")
    dem = pkg.Demodulator(nfix_crc=1, mode_ac=1, max_batch_samples=8 * 131072 + 131072, message_capacity=1 << 17, decode_fields=True)
    dem.launch_device(d_iq.data_ptr(), n, last=True)
    msgs, fields = dem.collect_fields()
    replies = int((msgs["msgtype"] == 32).sum())
    assert len(msgs) > 250 and replies > 10
    dm = torch_cuda.from_numpy(np.frombuffer(msgs.tobytes(), dtype=np.uint8).copy()).to("cuda:0")
    df = torch_cuda.from_numpy(np.frombuffer(fields.tobytes(), dtype=np.uint8).copy()).to("cuda:0")
    torch_cuda.cuda.synchronize()
    now = int(msgs["sysTimestampMsg"].max())
    gpu = pkg.capi.PositionTracker(capacity=1024, table=True, modeac=True)
    rows = gpu.update_device(dm.data_ptr(), df.data_ptr(), len(msgs))
    gpu.modeac_match(now, now)
    got = mas.observe(gpu, 1)
    gpu.close()
    twin = pkg.capi.PositionTracker(capacity=1024, host=True, table=True, modeac=True)
    want_rows = twin.update(msgs, fields)
    twin.modeac_match(now, now)
    want = mas.observe(twin, 1)
    twin.close()
    assert rows.tobytes() == want_rows.tobytes()
    assert int(got["codes"][0]["lastcount"].sum()) == replies  # one match: every count was copied, none is old enough to go
    assert int(got["codes"][0]["count"].sum()) == replies
    assert got["codes"][0].tobytes() == want["codes"][0].tobytes() and got["hits_raw"].tobytes() == want["hits_raw"].tobytes()
    assert got["snap_raw"].tobytes() == want["snap_raw"].tobytes() and len(got["snap_raw"]) > 10
