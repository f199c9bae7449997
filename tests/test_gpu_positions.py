"""The position tracker on the GPU (msd_pos_*, msd_pos_kernels.hip) against its host twin (libmsd_host.so), record by
record and bit by bit, the thirteen cpr_* counters and the live-aircraft count included.  Every stream keeps every
plausibility gate at least 1 m from its limit on the twin (asserted), a thousand times the 1e-3 m of the contract in
modes_hip.h, so the device's own sin / cos / acos / atan2 cannot decide a record differently.  min_gate_margin_m itself
is the device's own figure there and is only held to the same 1 m."""
import errno
import math

import numpy as np
import pytest

import pos_streams as ps

pytestmark = pytest.mark.gpu
COUNTERS = ("cpr_surface", "cpr_airborne", "cpr_global_ok", "cpr_global_bad", "cpr_global_skipped", "cpr_global_range_checks",
            "cpr_global_speed_checks", "cpr_local_ok", "cpr_local_aircraft_relative", "cpr_local_receiver_relative",
            "cpr_local_skipped", "cpr_local_range_checks", "cpr_local_speed_checks", "aircraft")


def both(pkg, receivers, fp, steps, capacity=1024, pieces=None):
    """steps through a GPU tracker and a twin of the same configuration; asserts equality and returns the GPU's rows"""
    outs = []
    for host in (False, True):
        t = pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, filter_persistence=fp, host=host)
        outs.append((ps.run_library(t, steps, pieces), t.stats()))
        t.close()
    (g, gst), (h, hst) = outs
    assert hst["min_gate_margin_m"] >= 1.0, hst["min_gate_margin_m"]
    assert g.tobytes() == h.tobytes(), [(i, g[i], h[i]) for i in range(len(g)) if g[i].tobytes() != h[i].tobytes()][:5]
    assert {k: gst[k] for k in COUNTERS} == {k: hst[k] for k in COUNTERS}
    assert gst["min_gate_margin_m"] >= 1.0
    assert math.isinf(gst["min_gate_margin_m"]) == math.isinf(hst["min_gate_margin_m"])
    return g, gst


@pytest.fixture(scope="module")
def mixed(pkg):
    return ps.mixed_stream(pkg)


def pair(b, t, addr, lat, lon, rx=0):
    return b.pos(t, addr, lat, lon, 0, rx=rx).pos(t + 400, addr, lat, lon, 1, rx=rx)


def test_one_record(pkg, torch_cuda):
    b = ps.Builder(pkg).pos(ps.T0, 0x4840D6, 52.25, 3.9, 0)
    g, st = both(pkg, [ps.HOME], 0, [b.step()])
    assert int(g["result"][0]) == -1 and st["aircraft"] == 1 and st["cpr_airborne"] == 1


def test_pair_in_one_call_and_over_two(pkg, torch_cuda):
    b = pair(ps.Builder(pkg), ps.T0, 0x4840D6, 52.25, 3.9)
    step = b.step()
    one, _ = both(pkg, [None], 0, [step])
    two, _ = both(pkg, [None], 0, [step], pieces=1)
    assert one.tobytes() == two.tobytes() and int(one["decoded"][1]) == 1 and int(one["relative"][1]) == 0
    assert abs(one["lat"][1] - 52.25) < 1e-4 and abs(one["lon"][1] - 3.9) < 1e-4


def test_65_aircraft_more_than_one_wavefront_of_walkers(pkg, torch_cuda):
    b = ps.Builder(pkg)
    for k in range(65):  # interleaved: every aircraft's two records are 65 apart in the stream
        b.pos(ps.T0 + k, 0x400000 + k, 40.0 + 0.1 * k, -3.0 + 0.05 * k, 0)
    for k in range(65):
        b.pos(ps.T0 + 500 + k, 0x400000 + k, 40.0 + 0.1 * k, -3.0 + 0.05 * k, 1)
    g, st = both(pkg, [None], 0, [b.step()])
    assert st["aircraft"] == 65 and st["cpr_global_ok"] == 65 and g["decoded"][65:].all() and not g["decoded"][:65].any()
    assert np.allclose(g["lat"][65:], 40.0 + 0.1 * np.arange(65), atol=1e-4)


def test_one_aircraft_300_records_is_a_serial_walk(pkg, torch_cuda):
    b = ps.Builder(pkg)
    for k in range(300):
        if k % 10 == 9:
            b.vel(ps.T0 + 500 * k, 0x4B1234, 300, 300)
        else:
            b.pos(ps.T0 + 500 * k, 0x4B1234, 47.0 + 5e-4 * k, 8.0 + 5e-4 * k, k & 1)
    g, st = both(pkg, [None], 0, [b.step()], capacity=64)
    assert st["aircraft"] == 1 and st["cpr_global_ok"] > 250


def test_colliding_addresses_and_receiver_keys(pkg, torch_cuda):
    """Two addresses with the same home slot in a 64-slot table, and one address on two receivers (different keys)."""
    home = {}
    a = 0x300000
    while True:  # at most 65 addresses until two share a home slot
        s = pkg.capi.pos_home_slot(0, a, 64)
        if s in home:
            break
        home[s] = a
        a += 1
    a0, a1 = home[s], a
    b = ps.Builder(pkg)
    pair(b, ps.T0, a0, 10.0, 10.0)
    pair(b, ps.T0, a1, -20.0, 30.0)
    pair(b, ps.T0, a0, 60.0, -100.0, rx=1)  # the same address heard by another receiver is another aircraft
    g, st = both(pkg, [None, None], 0, [b.step()], capacity=64)
    assert st["aircraft"] == 3 and [int(x) for x in g["result"]] == [-1, 0, -1, 0, -1, 0]
    assert np.allclose(g["lat"][[1, 3, 5]], [10.0, -20.0, 60.0], atol=1e-4)


def test_full_table_changes_nothing_and_expiry_frees_slots(pkg, torch_cuda):
    trackers = [pkg.capi.PositionTracker(capacity=64, receivers=[None], host=h) for h in (False, True)]
    b = ps.Builder(pkg)
    for k in range(62):
        pair(b, ps.T0 + k, 0x100 + k, 10.0 + 0.1 * k, 10.0)
    fill = b.step()
    for k in range(3):
        b.pos(ps.T0 + 1000, 0x900 + k, 10.0, 10.0, 1)
    b.pos(ps.T0 + 1000, 0x100, 10.0, 10.0, 0)  # a known aircraft in the same call: its state must not move either
    over = b.step()
    for k in range(64):
        pair(b, ps.T0 + 700000 + k, 0xA00 + k, -5.0, 20.0 + 0.1 * k)
    later = b.step()
    res = []
    for t in trackers:
        r = [t.update(*fill[1:])]
        before = t.stats()
        with pytest.raises(pkg.MsdError) as e:
            t.update(*over[1:])
        assert e.value.code == -errno.ENOSPC
        assert t.stats() == before
        r.append(t.update(over[1][3:], over[2][3:], over[3][3:]))  # the known aircraft alone: as if nothing had happened
        t.expire(ps.T0 + 700000)                                   # everyone is more than 10 minutes old
        assert t.stats()["aircraft"] == 0
        r.append(t.update(*later[1:]))                             # 64 new aircraft fit again
        assert t.stats()["aircraft"] == 64
        res.append((np.concatenate(r), t.stats()))
        t.close()
    assert res[0][0].tobytes() == res[1][0].tobytes()
    assert {k: res[0][1][k] for k in COUNTERS} == {k: res[1][1][k] for k in COUNTERS}
    assert res[0][1]["cpr_global_ok"] == 62 + 1 + 64  # the known aircraft's new even half pairs with its odd half


def test_expiry_scenario(pkg, torch_cuda):
    receivers, fp, steps = ps.scenarios(pkg)["expiry_and_ttl"]
    both(pkg, receivers, fp, steps, capacity=64)


@pytest.mark.parametrize("name", ["surface_windows", "global_failure", "receiver_relative", "speed_check", "backwards",
                                  "clock_from_zero", "type_and_source_mismatch", "refusals", "surface_speed_check",
                                  "surface_movement_codes", "global_max_range", "negative_max_range",
                                  "higher_source_skips_speed_check", "reliable_sides", "odd_latitude_alone_out_of_range"])
def test_scenarios(pkg, torch_cuda, name):
    receivers, fp, steps = ps.scenarios(pkg)[name]
    g, st = both(pkg, receivers, fp, steps)
    if name == "refusals" or name in ps.KNOWN:  # the device's own rows against the answers derived by hand
        ps.known(name, g, st)


def test_cutting_invariance(pkg, torch_cuda, mixed):
    receivers, m, f, r = mixed
    steps = [("update", m, f, r)]
    whole, st = both(pkg, receivers, 0, steps)
    assert all(st[k] > 0 for k in COUNTERS)
    for pieces in (1, 7, 64):
        t = pkg.capi.PositionTracker(capacity=1024, receivers=receivers)
        cut = ps.run_library(t, steps, pieces)
        cst = t.stats()
        t.close()
        assert cut.tobytes() == whole.tobytes(), pieces
        assert {k: cst[k] for k in COUNTERS} == {k: st[k] for k in COUNTERS}
        # the same device arithmetic, reduced over one walker at a time here and over dozens at once there
        assert np.float64(cst["min_gate_margin_m"]).tobytes() == np.float64(st["min_gate_margin_m"]).tobytes(), pieces


def test_device_records_and_bad_receiver_index(pkg, torch_cuda, mixed):
    """The records in device memory give what host records give; a receiver index out of range in a device array is
    -EINVAL with nothing changed."""
    import torch
    receivers, m, f, r = mixed
    t = pkg.capi.PositionTracker(capacity=1024, receivers=receivers)
    want = t.update(m, f, r)
    wst = t.stats()
    t.reset()
    dm = torch.from_numpy(m.view(np.uint8).copy()).cuda()
    df = torch.from_numpy(f.view(np.uint8).copy()).cuda()
    bad = r.copy()
    bad[1000] = 2
    dbad = torch.from_numpy(bad.view(np.int32)).cuda()
    with pytest.raises(pkg.MsdError) as e:
        t.update_device(dm.data_ptr(), df.data_ptr(), len(m), dbad.data_ptr())
    assert e.value.code == -errno.EINVAL and t.stats()["aircraft"] == 0 and t.stats()["cpr_airborne"] == 0
    dr = torch.from_numpy(r.view(np.int32).copy()).cuda()
    got = t.update_device(dm.data_ptr(), df.data_ptr(), len(m), dr.data_ptr())
    assert got.tobytes() == want.tobytes()
    assert {k: t.stats()[k] for k in COUNTERS} == {k: wst[k] for k in COUNTERS}
    t.close()
