"""The SBS output on the GPU (msd_pos_sbs_enable, msd_pos_update_sbs, msd_pos_sbs_wire) against the host twin, which
test_sbs_model.py holds equal to a second reading of net_io.c and to lines written out by hand, and whose arithmetic
tests/c/sbs_units.c holds against glibc.  Everything is compared by bytes -- the row of every record, the stream, its
ends --: the contract is the table's, equality wherever the msd_position rows are equal, and has no tolerance.  Beside the
rules (every scenario, the mixed stream with its expiries, cut into calls of 1, 63 and 257 records) this covers what
exists on the device only: the SBS instantiations of the two walks over the grouped order and the row they hand over,
rows into device memory, the ground-track table, and the text writer's tiles, runs and seams.
Every stream keeps every plausibility gate at least 1 m from its limit on the twin, and the tests assert it."""
import ctypes as C
import errno

import numpy as np
import pytest

import aircraft_streams as acs
import indep_sbs as isbs
import reduce_streams as rs
import sbs_streams as ss

pytestmark = pytest.mark.gpu


def tracker(pkg, host, receivers, capacity=1024, **kw):
    return pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, host=host, table=True, sbs=True, **kw)


def run(pkg, host, receivers, steps, capacity=1024, pieces=None, **kw):
    t = tracker(pkg, host, receivers, capacity, **kw)
    out = ss.run_library(t, steps, pieces)
    st = t.stats()
    t.close()
    if host:
        assert st["min_gate_margin_m"] >= 1.0, st["min_gate_margin_m"]
    return out


def same(got, want):
    assert got[0].tobytes() == want[0].tobytes(), "msd_position rows"
    assert got[1].tobytes() == want[1].tobytes(), "NIC / Rc"
    bad = [i for i in range(len(want[2])) if got[2][i].tobytes() != want[2][i].tobytes()]
    assert not bad, [(i, got[2][i], want[2][i]) for i in bad[:4]]


@pytest.fixture(scope="module")
def scen(pkg):
    return ss.scenarios(pkg)


@pytest.fixture(scope="module")
def mixed(pkg):
    receivers, steps = rs.mixed_steps(pkg)
    return receivers, steps, run(pkg, True, receivers, steps)


@pytest.fixture(scope="module")
def writers(pkg, torch_cuda):
    t = {h: tracker(pkg, h, [None], 64) for h in (False, True)}
    yield t
    for x in t.values():
        x.close()


ALL_FLAGS = [dict(verbatim=v, net_only=o, gnss=g) for v in (False, True) for o in (False, True) for g in (False, True)]


# ---- the rules ----
@pytest.mark.parametrize("name", ss.NAMES)
def test_scenario(pkg, torch_cuda, scen, writers, name):
    s = scen[name]
    m, f, r = ss.records(s["steps"])
    if s["rows"] is None:
        want = run(pkg, True, s["receivers"], s["steps"], s["capacity"])
        same(run(pkg, False, s["receivers"], s["steps"], s["capacity"]), want)
        for pieces in (1, 63, 257):
            same(run(pkg, False, s["receivers"], s["steps"], s["capacity"], pieces), want)
        trk = want[2]
    else:
        trk = s["rows"]
    for opts, lines in s["cases"]:
        twin, tends = writers[True].sbs_wire(m, f, trk, **opts)
        got, ends = writers[False].sbs_wire(m, f, trk, **opts)
        assert ss.split(twin, tends) == lines
        assert got == twin and (ends == tends).all()


def test_mixed_stream(pkg, torch_cuda, mixed, writers):
    receivers, steps, want = mixed
    same(run(pkg, False, receivers, steps), want)
    m, f, r = ss.records(steps)
    for k, flags in enumerate(ALL_FLAGS):
        kw = dict(flags, now_ms=ss.T0 + 9000, utc_offset_ms=(-1) ** k * 3600000 * k)
        twin, tends = writers[True].sbs_wire(m, f, want[2], **kw)
        got, ends = writers[False].sbs_wire(m, f, want[2], **kw)
        assert got == twin and (ends == tends).all()
    assert len(twin) > 100000


@pytest.mark.parametrize("pieces", [1, 63, 257])
def test_mixed_stream_cut_into_calls(pkg, torch_cuda, mixed, pieces):
    receivers, steps, want = mixed
    same(run(pkg, False, receivers, steps, pieces=pieces), want)


# ---- where the rows go, and which call feeds a record ----
def on_device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def test_rows_into_device_memory_and_the_writer_from_it(pkg, torch_cuda, mixed, writers):
    receivers, steps, want = mixed
    m, f, r = ss.records(steps)
    n = len(m)
    t = tracker(pkg, False, receivers)
    d_trk = torch_cuda.full((32 * n + 256,), 0xEE, dtype=torch_cuda.uint8, device="cuda")
    at = 0
    for s in steps:
        if s[0] == "expire":
            t.expire(s[1])
            continue
        k = len(s[1])
        dm, df, dr = on_device(torch_cuda, s[1]), on_device(torch_cuda, s[2]), on_device(torch_cuda, s[3])
        torch_cuda.cuda.synchronize()
        t.update_sbs_device(dm.data_ptr(), df.data_ptr(), k, d_trk.data_ptr() + 32 * at, dr.data_ptr())
        at += k
    back = d_trk.cpu().numpy()
    assert back[:32 * n].tobytes() == want[2].tobytes() and (back[32 * n:] == 0xEE).all()
    dm, df = on_device(torch_cuda, m), on_device(torch_cuda, f)
    torch_cuda.cuda.synchronize()
    kw = dict(now_ms=ss.T0, gnss=True)
    got, ends = t.sbs_wire(dm.data_ptr(), df.data_ptr(), d_trk.data_ptr(), n=n, on_device=True, **kw)
    twin, tends = writers[True].sbs_wire(m, f, want[2], **kw)
    assert got == twin and (ends == tends).all() and len(twin) > 100000
    t.close()


def test_every_update_call_on_one_tracker(pkg, torch_cuda, mixed):
    """update, update_nicrc, update_reduce and update_sbs in turn on a tracker that reduces too: the rows it delivers are
    the twin's, and so are the verdicts, whichever call fed the records in between"""
    receivers, steps, want = mixed
    verdicts = rs.run_library(pkg.capi.PositionTracker(capacity=1024, receivers=receivers, host=True, table=True, reduce_interval_ms=125), steps)[2]
    t = tracker(pkg, False, receivers, reduce_interval_ms=125)
    rows, fwd, calls = [], [], 0
    for s in steps:
        if s[0] == "expire":
            t.expire(s[1])
            continue
        _, m, f, r = s
        for i in range(0, len(m), 50):
            part = (m[i:i + 50], f[i:i + 50], r[i:i + 50])
            none, nof = np.zeros(len(part[0]), dtype=pkg.capi.SBS_TRACK_DTYPE), np.full(len(part[0]), 255, dtype=np.uint8)
            none["pad"] = 255
            if calls % 4 == 0:
                t.update(*part)
            elif calls % 4 == 1:
                t.update_nicrc(*part)
            elif calls % 4 == 2:
                nof = t.update_reduce(*part, nicrc=False)[2]
            else:
                _, _, nof, none = t.update_sbs(*part, nicrc=False, forward=calls % 8 == 3)
                nof = np.full(len(part[0]), 255, dtype=np.uint8) if nof is None else nof
            rows.append(none), fwd.append(nof)
            calls += 1
    t.close()
    rows, fwd = np.concatenate(rows), np.concatenate(fwd)
    seen = rows["pad"][:, 0] != 255
    assert seen.sum() > 300 and rows[seen].tobytes() == want[2][seen].tobytes()
    assert (fwd != 255).sum() > 400 and (fwd[fwd != 255] == verdicts[fwd != 255]).all()


# ---- shapes of the walk ----
def test_one_aircraft_is_a_serial_walk(pkg, torch_cuda):
    receivers, m, f, r = acs.wide_stream(pkg, aircraft=1, records=300, replies=True)
    steps = [("update", m, f, r)]
    want = run(pkg, True, receivers, steps, 64)
    assert np.count_nonzero(want[2]["flags"] & isbs.SEEN_TWICE) == 299 and np.count_nonzero(want[2]["flags"] & isbs.CPR_DECODED) > 50
    same(run(pkg, False, receivers, steps, 65536), want)


def test_more_walkers_than_a_wavefront(pkg, torch_cuda):
    receivers, m, f, r = acs.wide_stream(pkg, aircraft=65, records=65 * 12, replies=True)
    steps = [("update", m, f, r)]
    want = run(pkg, True, receivers, steps)
    assert np.count_nonzero(want[2]["flags"] & isbs.SEEN_TWICE) == 65 * 11
    same(run(pkg, False, receivers, steps), want)


# ---- the writer ----
def writer_records(pkg, n, seed=5):
    """n records with rows by hand for the stateless writer: every SBS type and some that write nothing, and of every
    field a random choice between absent, short and longest, so that the lines' lengths cover the whole range"""
    rng = np.random.default_rng(seed + n)
    m = np.zeros(n, dtype=pkg.capi.MESSAGE_DTYPE)
    f = np.zeros(n, dtype=pkg.capi.FIELDS_DTYPE)
    t = np.zeros(n, dtype=pkg.capi.SBS_TRACK_DTYPE)
    pick = lambda *a: rng.choice(np.array(a), n)  # noqa: E731
    m["msgtype"] = pick(0, 4, 5, 11, 16, 17, 17, 17, 18, 20, 21, 24)
    m["sysTimestampMsg"] = ss.T0 + rng.integers(0, 10 ** 10, n)
    m["correctedbits"] = pick(0, 0, 0, 0, 1, 2)
    f["metype"] = rng.integers(0, 24, n)
    f["addr"] = rng.integers(1, 1 << 24, n) | np.where(rng.uniform(size=n) < 0.05, 1 << 24, 0)
    f["callsign_valid"] = pick(0, 1)
    f["callsign"] = rng.choice(np.frombuffer(b"ABCXYZ019 ", dtype="S1"), (n, 8)).view("S8").reshape(n)
    f["altitude_baro_valid"], f["altitude_geom_valid"] = pick(0, 1), pick(0, 1)
    f["altitude_baro"], f["altitude_geom"] = pick(-1000, 0, 38000, 126700), pick(-(1 << 31), 5, 41025, (1 << 31) - 1)
    f["velocity_valid"], f["mesub"] = pick(0, 0, 1), pick(1, 2)
    scale = np.where(f["mesub"] == 2, 4, 1)
    f["ew_vel"], f["ns_vel"] = rng.integers(-1022, 1023, n) * scale, rng.integers(-1022, 1023, n) * scale
    f["heading_valid"], f["heading_type"], f["heading_raw"] = pick(0, 0, 1), pick(1, 1, 3, 4, 5), rng.integers(0, 2048, n)
    f["commb_format"] = np.where(np.isin(m["msgtype"], (20, 21)), pick(0, 8, 8, 9), 0)
    # a heading has the bits its message carries: 11 in BDS 5,0 / 6,0, 10 in ES type 19, 7 in a surface position
    f["heading_raw"] &= np.where(f["commb_format"] != 0, 2047, np.where(f["metype"] == 19, 1023, 127)).astype(np.uint16)
    f["baro_rate_valid"], f["geom_rate_valid"] = pick(0, 1), pick(0, 1)
    f["baro_rate"], f["geom_rate"] = pick(-32768, -64, 0, 4032), pick(-32768, 7, 32767)
    f["squawk_valid"], f["squawk"] = pick(0, 1), pick(0, 0x1200, 0x7500, 0x7600, 0x7700, 0x7777)
    f["alert_valid"], f["alert"], f["spi_valid"], f["spi"] = pick(0, 1), pick(0, 1), pick(0, 1), pick(0, 1)
    f["airground"] = pick(0, 1, 2, 3)
    t["flags"] = isbs.TRACKED | isbs.SEEN_TWICE | (rng.integers(0, 8, n) << 2)
    t["gs_selected"] = pick(0.0, 0.5, 1.5, 15.5, 16.5, 141.42136, 1446.7, 65535.0)
    t["geom_delta"] = pick(-275, 0, 250, 1 << 30)
    t["lat"] = np.where(rng.uniform(size=n) < 0.2, pick(-90.0, 90.0, -0.000001, 0.015625, -123.456785), rng.uniform(-90, 90, n))
    t["lon"] = np.where(rng.uniform(size=n) < 0.2, pick(-180.0, 180.0, -0.000004, 0.046875, -179.999995), rng.uniform(-180, 180, n))
    return m, f, t


PATTERNS = ("all", "none", "last_of_each_tile", "first_of_second_tile", "random")


def written(pattern, n):
    i = np.arange(n)
    if pattern == "all":
        return np.ones(n, dtype=bool)
    if pattern == "none":
        return np.zeros(n, dtype=bool)
    if pattern == "last_of_each_tile":
        return (i % 256 == 255) | (i == n - 1)
    if pattern == "first_of_second_tile":
        return i == 256
    return np.random.default_rng(n).uniform(size=n) < 0.4


@pytest.mark.parametrize("n", [255, 256, 257, 1025])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_writer_shapes(pkg, writers, n, pattern):
    m, f, t = writer_records(pkg, n)
    on = written(pattern, n)
    if pattern == "all":  # every record one that writes: an SBS type, an ICAO address, fewer than two repaired bits
        m["msgtype"], m["correctedbits"], f["addr"] = np.where(m["msgtype"] == 24, 5, m["msgtype"]), 0, f["addr"] & 0xFFFFFF
        f["metype"] = np.clip(f["metype"], 1, 19)
    else:  # the others are held back in three different ways: not tracked, a first message, two repaired bits
        i = np.arange(n)
        t["flags"] = np.where(on | (i % 3 != 0), t["flags"], 0)
        t["flags"] = np.where(on | (i % 3 != 1), t["flags"], t["flags"] & ~np.uint8(isbs.SEEN_TWICE))
        m["correctedbits"] = np.where(on, 0, np.where(i % 3 == 2, 2, m["correctedbits"]))
        m["msgtype"], f["addr"] = np.where(on, 17, m["msgtype"]), np.where(on, f["addr"] & 0xFFFFFF, f["addr"])
        f["metype"] = np.where(on, np.clip(f["metype"], 1, 19), f["metype"])
    for gnss in (False, True):
        kw = dict(gnss=gnss, now_ms=ss.T0 + 123, utc_offset_ms=-18000000)
        want, wends = isbs.stream(m, f, isbs.rows_of(t), **kw)
        twin, tends = writers[True].sbs_wire(m, f, t, **kw)
        got, ends = writers[False].sbs_wire(m, f, t, **kw)
        assert twin == want and (tends == wends).all()
        assert got == want and (ends == wends).all()
        lens = np.diff(np.concatenate([[0], wends]))
        assert ((lens > 0) == on).all() and lens.max() <= pkg.capi.SBS_MAX
        if pattern == "none":
            assert writers[False].sbs_needed == 0 and not ends.any()
        if pattern == "all" and gnss and n == 1025:
            # the whole range of lengths: from the 80 bytes of a line with every field empty up to long ones
            assert lens.min() <= 90 and lens.max() >= 135


def test_writer_longest_line(pkg, writers):
    """the line that the comment at MSD_SBS_MAX adds up, between shorter ones on either side of a tile seam"""
    m, f, t = writer_records(pkg, 600)
    for i in (0, 255, 256, 599):
        m["msgtype"][i], m["correctedbits"][i], m["sysTimestampMsg"][i] = 20, 0, ss.T0
        f["addr"][i], f["callsign_valid"][i], f["callsign"][i] = 0xFFFFFF, 1, b"WWWWWWWW"
        f["altitude_geom_valid"][i], f["altitude_geom"][i], f["geom_rate_valid"][i], f["geom_rate"][i] = 1, -(1 << 31), 1, -32768
        f["squawk_valid"][i], f["squawk"][i], f["alert_valid"][i], f["alert"][i], f["spi_valid"][i], f["spi"][i] = 1, 0x7700, 1, 1, 1, 1
        f["airground"][i], f["velocity_valid"][i] = 1, 0
        f["commb_format"][i], f["heading_valid"][i], f["heading_type"][i], f["heading_raw"][i] = 8, 1, 1, 2047
        t["flags"][i] = isbs.TRACKED | isbs.SEEN_TWICE | isbs.GS_VALID | isbs.CPR_DECODED
        t["gs_selected"][i], t["lat"][i], t["lon"][i] = 65535, -180.0, -180.0
    kw = dict(gnss=True, now_is_received=True)
    twin, tends = writers[True].sbs_wire(m, f, t, **kw)
    got, ends = writers[False].sbs_wire(m, f, t, **kw)
    assert got == twin and (ends == tends).all()
    lens = np.diff(np.concatenate([[0], ends]))
    assert lens.max() == pkg.capi.SBS_MAX == 147 and [int(lens[i]) for i in (0, 255, 256, 599)] == [147] * 4
    assert got[:147] == (b"MSG,5,1,1,FFFFFF,1,2020/09/13,12:26:40.000,2020/09/13,12:26:40.000,WWWWWWWW,-2147483648H,65535,360,"
                         b"-180.00000,-180.00000,-32768H,7700,-1,-1,-1,-1\r\n")


def test_writer_times_out_of_range(pkg, writers):
    """a record's own time cannot be refused: beyond year 9999 the year is printed modulo 10000, a negative sum as 0"""
    m, f, t = writer_records(pkg, 300)
    m["sysTimestampMsg"][::3] = 253402300800000 + np.arange(100) * 86400000 * 180
    m["sysTimestampMsg"][1::3] = np.arange(100) * 1000
    m["sysTimestampMsg"][2::3] = (1 << 63) - 1 - np.arange(100, dtype=np.uint64) * np.uint64(10 ** 15)
    m["sysTimestampMsg"][5] = (1 << 64) - 1
    m["msgtype"], m["correctedbits"], f["metype"], f["addr"] = 17, 0, 4, f["addr"] & 0xFFFFFF  # every record writes
    f["heading_valid"] = 0
    seen = b""
    for off in (-50000, 3600000):
        kw = dict(now_ms=ss.T0, utc_offset_ms=off, net_only=True)
        want, wends = isbs.stream(m, f, isbs.rows_of(t), **kw)
        twin, tends = writers[True].sbs_wire(m, f, t, **kw)
        got, ends = writers[False].sbs_wire(m, f, t, **kw)
        assert twin == want and got == want and (ends == wends).all() and (tends == wends).all()
        seen += want
    assert b",1970/01/01,00:00:00.000," in seen and b",0000/01/01,01:00:00.000," in seen


def test_writer_capacity_and_empty_call(pkg, writers):
    t = writers[False]
    n = 1025
    m, f, trk = writer_records(pkg, n)
    opt = pkg.capi.SbsOptions(now_ms=ss.T0, utc_offset_ms=0, flags=pkg.capi.SBS_NET_ONLY, reserved=0)
    want, _ = isbs.stream(m, f, isbs.rows_of(trk), net_only=True, now_ms=ss.T0)
    out = np.full(len(want) + 64, 0xAA, dtype=np.uint8)
    ends = np.full(n, 0xAAAAAAAA, dtype=np.uint32)
    need = C.c_size_t(0)
    args = (t.h, m.ctypes.data, f.ctypes.data, trk.ctypes.data, n, 0, C.byref(opt), out.ctypes.data)
    assert t.f["sbs_wire"](*args, len(want) - 1, C.byref(need), ends.ctypes.data) == -errno.ENOSPC
    assert need.value == len(want) and (out == 0xAA).all() and (ends == 0xAAAAAAAA).all()
    assert t.f["sbs_wire"](*args, len(want), C.byref(need), ends.ctypes.data) == 0
    assert need.value == len(want) and out[:len(want)].tobytes() == want and (out[len(want):] == 0xAA).all()
    need.value = 77
    assert t.f["sbs_wire"](t.h, None, None, None, 0, 0, C.byref(opt), None, 0, C.byref(need), None) == 0 and need.value == 0


# ---- machinery ----
def test_rolled_back_update_writes_no_row(pkg, torch_cuda, scen):
    s = scen["delivery"]
    m, f, r = ss.records(s["steps"])
    b = rs.Builder(pkg)
    for k in range(71):
        b.squawk5(rs.T0 + 600, 0x300000 + k)
    _, bm, bf, br = b.step()
    res = []
    for fail_first in (True, False):
        t = tracker(pkg, False, [None], 64)
        t.update_sbs(m[:1], f[:1], r[:1])
        if fail_first:  # 72 aircraft do not fit 64 slots: nothing changes, no row is written
            out = np.zeros(len(bm), dtype=pkg.capi.POSITION_DTYPE)
            trk = np.full(len(bm) * 32, 0xEE, dtype=np.uint8)
            rc = t.f["update_sbs"](t.h, bm.ctypes.data, bf.ctypes.data, br.ctypes.data, len(bm), 0, out.ctypes.data, None, None,
                                   trk.ctypes.data)
            assert rc == -errno.ENOSPC and (trk == 0xEE).all() and t.live() == 1
        res.append(t.update_sbs(bm[:40], bf[:40], br[:40])[3].tobytes() + t.update_sbs(m[1:], f[1:], r[1:])[3].tobytes())
        t.close()
    assert res[0] == res[1]


def test_reset_keeps_the_tracker_enabled(pkg, torch_cuda, scen, writers):
    s = scen["velocity_track"]
    m, f, r = ss.records(s["steps"])
    t = tracker(pkg, False, [None], 64)
    first = t.update_sbs(m, f, r)[3]
    again = t.update_sbs(m, f, r)[3]
    assert not first["flags"][0] & isbs.SEEN_TWICE and again["flags"][0] & isbs.SEEN_TWICE
    t.reset()
    assert t.update_sbs(m, f, r)[3].tobytes() == first.tobytes()
    opts, lines = s["cases"][0]
    got, ends = t.sbs_wire(m, f, first, **opts)  # the ground-track table is still there
    assert ss.split(got, ends) == lines
    t.close()


def test_a_tracker_that_never_enables_sbs(pkg, torch_cuda):
    """delivers what it delivered, whether or not another one writes SBS, and refuses the two new calls"""
    receivers, m, f, r = acs.mixed_stream(pkg)
    steps = [("update", m, f, r)]
    res = {}
    for key, host, sbs in (("twin", True, False), ("plain", False, False), ("sbs", False, True)):
        t = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, host=host, table=True, modeac=True,
                                     reduce_interval_ms=125, sbs=sbs)
        if sbs:  # fed through the new call
            rows, nic, _ = ss.run_library(t, steps)
            snaps = [t.snapshot()]
        else:
            rows, nic, snaps = acs.run_library(t, steps, every_step=False)
        t.modeac_match(acs.T0 + 5000, acs.T0 + 5000)
        res[key] = (rows.tobytes(), nic.tobytes(), snaps[-1].tobytes(), t.modeac_hits().tobytes(), t.modeac_codes(0).tobytes())
        if key == "plain":
            trk = np.zeros(5, dtype=pkg.capi.SBS_TRACK_DTYPE)
            for call in (lambda: t.update_sbs(m[:5], f[:5], r[:5]), lambda: t.sbs_wire(m[:5], f[:5], trk)):
                with pytest.raises(pkg.MsdError) as e:
                    call()
                assert e.value.code == -errno.EINVAL
        t.close()
    assert res["plain"] == res["twin"] and res["sbs"] == res["twin"]
