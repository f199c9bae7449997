"""Mode A/C matching on the CPU: the host twin (libmsd_host.so, msd_modeac_impl.h compiled for the host) against the second
reading of track.c / mode_ac.c in tests/indep_modeac.py -- every receiver's four arrays, every aircraft's hits, every
msd_aircraft member of every snapshot and every record's row --, on one small scenario per rule and on a 2000-record
mixed stream with a match every second; each scenario's decisive values against an expectation derived by hand; the
Gillham table both ways; and what the interface promises: an enabled tracker delivers what a plain one does, the calls
are refused where they do not apply, a rolled-back call counts nothing."""
import errno

import numpy as np
import pytest

import aircraft_streams as acs
import indep_modeac as im
import modeac_streams as mas
import pos_streams as ps

T0 = ps.T0


@pytest.fixture(scope="module")
def scen(pkg):
    return mas.scenarios(pkg)


def twin(pkg, receivers, steps, pieces=None, capacity=64, every_step=True):
    t = pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, host=True, table=True, modeac=True)
    out = mas.run_library(t, len(receivers), steps, pieces, every_step)
    st = t.stats()
    t.close()
    assert st["min_gate_margin_m"] >= 1.0
    return out


def same_as_model(pkg, receivers, steps, got):
    rows, nic, obs = got
    mrows, mnic, mobs = mas.run_model(pkg, receivers, steps)
    assert ps.rows_of(rows) == ps.rows_of_model(mrows)
    assert [(int(q["nic"]), int(q["rc"]), int(q["set"])) for q in nic] == mnic
    assert len(obs) == len(mobs)
    for k, (g, w) in enumerate(zip(obs, mobs)):
        for rx in range(len(receivers)):
            got_codes = [tuple(int(x) for x in c) for c in g["codes"][rx]]
            if got_codes != w["codes"][rx]:
                raise AssertionError((k, rx, [(i, a, b) for i, (a, b) in enumerate(zip(got_codes, w["codes"][rx])) if a != b][:6]))
        assert [(int(h["receiver"]), int(h["addr"]), int(h["mode_a_hit"]), int(h["mode_c_hit"])) for h in g["hits_raw"]] == w["hits"], k
        assert acs.differences(g["snap_raw"], w["snap"]) == [], k


def test_scenario_list_is_complete(scen):
    assert sorted(scen) == sorted(mas.NAMES)


@pytest.mark.parametrize("name", mas.NAMES)
def test_twin_equals_second_reading(pkg, scen, name):
    receivers, steps, _ = scen[name]
    same_as_model(pkg, receivers, steps, twin(pkg, receivers, steps))


@pytest.mark.parametrize("name", mas.NAMES)
def test_scenario_reaches_what_it_is_named_for(pkg, scen, name):
    receivers, steps, check = scen[name]
    check(twin(pkg, receivers, steps)[2])


@pytest.fixture(scope="module")
def mixed(pkg):
    receivers, steps, whole = mas.mixed_steps(pkg)
    return receivers, steps, whole, twin(pkg, receivers, steps, capacity=1024)


def test_mixed_stream_equals_second_reading(pkg, mixed):
    receivers, steps, (m, f, r), got = mixed
    same_as_model(pkg, receivers, steps, got)
    assert len(m) == 2000 and sum(1 for s in steps if s[0] == "match") >= 30
    replies = int((m["msgtype"] == 32).sum())
    assert replies >= 350
    hits = [o["hits_raw"] for o in got[2]]
    # the stream reaches both kinds of hit, ambiguous codes, matched and unmatched live codes and codes that age out
    assert any(h["mode_a_hit"].any() for h in hits) and any(h["mode_c_hit"].any() for h in hits)
    matches = np.concatenate([c["match"] for o in got[2] for c in o["codes"]])
    ages = np.concatenate([c["age"] for o in got[2] for c in o["codes"]])
    assert (matches == 0xFFFFFFFF).any() and ((matches != 0) & (matches != 0xFFFFFFFF)).any()
    assert (ages == 10).any() and (ages > 10).any() and (ages == 15).any()
    cleared = sum(int(c["count"].sum()) for c in got[2][-1]["codes"])
    assert 0 < cleared < replies  # some codes were heard too rarely and have been cleared


@pytest.mark.parametrize("pieces", [1, 7])
def test_cutting_does_not_matter(pkg, mixed, pieces):
    receivers, steps, _, want = mixed
    mas.same_bytes(twin(pkg, receivers, steps, pieces=pieces, capacity=1024), want)


def test_mode_c_to_a_inverts_a_to_c(pkg):
    """modeACInit: every index with a valid altitude maps back to itself, every other C in the table's range gives 0, and
    no two codes share a C (the reference's assert)."""
    seen = {}
    for i in range(4096):
        mode_a = im.index_to_mode_a(i)
        assert im.mode_a_to_index(mode_a) == i
        c = im.internal_mode_a_to_mode_c(mode_a)
        if c == im.INVALID_ALTITUDE:
            continue
        assert c not in seen, (hex(mode_a), hex(seen.get(c, 0)))
        seen[c] = mode_a
        assert pkg.capi.mode_c_to_a(c) == mode_a
    assert min(seen) == -12 and len(seen) == 1280
    for c in range(-14, 4084):
        assert pkg.capi.mode_c_to_a(c) == seen.get(c, 0) == im.mode_c_to_mode_a(c)
    assert pkg.capi.mode_c_to_a(-(1 << 31)) == 0 and pkg.capi.mode_c_to_a((1 << 31) - 1) == 0


def test_enabled_and_plain_twin_deliver_the_same(pkg, mixed):
    """rows, NIC / Rc and snapshot bytes of the mixed stream do not change with the matching enabled"""
    receivers, steps, _, want = mixed
    plain = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, host=True, table=True)
    rows, nic, snaps = acs.run_library(plain, [s for s in steps if s[0] != "match"], every_step=False)
    plain.close()
    assert rows.tobytes() == want[0].tobytes() and nic.tobytes() == want[1].tobytes()
    assert snaps[-1].tobytes() == want[2][-1]["snap_raw"].tobytes()


def test_calls_are_refused_where_they_do_not_apply(pkg):
    EINVAL = -errno.EINVAL

    def refused(call):
        with pytest.raises(pkg.MsdError) as e:
            call()
        return e.value.code

    bare = pkg.capi.PositionTracker(capacity=64, host=True)
    assert refused(bare.modeac_enable) == EINVAL
    bare.close()
    t = pkg.capi.PositionTracker(capacity=64, receivers=[None, None], host=True, table=True)
    for call in (lambda: t.modeac_match(T0, T0), lambda: t.modeac_codes(0), lambda: t.modeac_hits(4)):
        assert refused(call) == EINVAL
    t.modeac_enable()
    t.modeac_enable()  # a second call changes nothing
    assert refused(lambda: t.modeac_codes(2)) == EINVAL
    assert len(t.modeac_hits()) == 0 and not t.modeac_codes(1).view(np.uint32).any()
    t.close()


def test_rolled_back_call_counts_nothing_and_reset_keeps_the_tracker_enabled(pkg):
    b = mas.Builder(pkg)
    for k in range(60):
        b.squawk(T0 + k, 0x400000 + k, 0x1200)
    fill = b.step()
    for k in range(10):  # ten aircraft too many, replies in between
        b.squawk(T0 + 100, 0x700000 + k, 0x1200).reply(T0 + 100, 0x1200, n=2)
    _, m, f, r = b.step()
    t = pkg.capi.PositionTracker(capacity=64, host=True, table=True, modeac=True)
    mas.run_library(t, 1, [fill, b.reply(T0 + 90, 0x3300, n=3).step()])
    before = mas.observe(t, 1)
    with pytest.raises(pkg.MsdError) as e:
        t.update_nicrc(m, f, r)
    assert e.value.code == -errno.ENOSPC
    after = mas.observe(t, 1)
    assert after["codes"][0].tobytes() == before["codes"][0].tobytes() and int(after["codes"][0]["count"].sum()) == 3
    assert after["hits_raw"].tobytes() == before["hits_raw"].tobytes() and len(after["hits_raw"]) == 60
    t.update_nicrc(m[1::3], f[1::3], r[1::3])  # the replies alone fit
    assert int(t.modeac_codes(0)[mas.idx(0x1200)]["count"]) == 10
    t.modeac_match(T0 + 1000, T0 + 1000)
    assert int(t.modeac_hits()["mode_a_hit"].sum()) == 60
    t.reset()
    assert len(t.modeac_hits()) == 0 and not t.modeac_codes(0).view(np.uint32).any()
    mas.run_library(t, 1, [fill])  # still enabled: the aircraft come back without hits
    assert len(t.modeac_hits()) == 60 and not t.modeac_hits()["mode_a_hit"].any()
    t.close()


def test_struct_sizes(pkg):
    assert pkg.capi.MODEAC_CODE_DTYPE.itemsize == 16 and pkg.capi.MODEAC_HIT_DTYPE.itemsize == 16
    assert pkg.capi.AIRCRAFT_DTYPE.itemsize == 592
