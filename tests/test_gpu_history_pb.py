"""history_N.pb on the GPU: the device (msd_pos_history_pb, msd_history_kernels.hip) == the host object == the second
reading of tests/indep_history.py, stream and rows, on the tables of tests/history_streams.py and tests/pb_streams.py,
with receivers sized around the writer's 256-item workgroup (items are aircraft plus one head per receiver), with many
receivers of which most are empty, after an expiry has rebuilt the table, through the -ENOSPC / size / repeat rule and
without an array for the rows."""
import numpy as np
import pytest

import history_streams as hs
import indep_history as ih
import pb_streams as pbs

pytestmark = pytest.mark.gpu

MANY = [0] * 1024
for _r, _c in ((0, 3), (1, 1), (255, 2), (256, 1), (257, 4), (600, 255), (1023, 5)):
    MANY[_r] = _c


def trackers(pkg, receivers, capacity=1 << 12):
    return [pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, host=h, table=True) for h in (False, True)]


def three_ways(pkg, scenario, refuse=False, capacity=1 << 12):
    """the scenario's writes by the device, the host object and the second reading; the first two byte for byte, stream
    and rows, the third file by file -> the device's [(stream, rows)]"""
    receivers, steps, writes = scenario
    dev, host = trackers(pkg, receivers, capacity)
    model = pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, host=True, table=True)
    try:
        got = hs.run(dev, scenario, refuse=refuse)
        twin = hs.run(host, scenario)
        want = hs.run_model(pkg, model, scenario)
    finally:
        for t in (dev, host, model):
            t.close()
    assert len(got) == len(twin) == len(want) == len(writes)
    for (stream, rx), (t_stream, t_rx), (files, rows) in zip(got, twin, want):
        assert stream == t_stream
        assert rx.tobytes() == t_rx.tobytes()
        assert hs.split(stream, rx) == files and [int(n) for n in rx["aircraft"]] == rows
    return got


@pytest.mark.parametrize("name", sorted(hs.TABLES))
def test_the_rules_tables(pkg, torch_cuda, name):
    got = three_ways(pkg, hs.TABLES[name](pkg), refuse=name in ("selection", "expire", "nothing"))
    if name == "nothing":
        assert got[0][0] == b""  # the store kernel has nothing to run for


@pytest.mark.parametrize("name", sorted(pbs.TABLES))
def test_the_aircraft_pb_tables(pkg, torch_cuda, name):
    """one step's table each, written at aircraft.pb's own times"""
    receivers, steps, writes = pbs.TABLES[name](pkg)
    three_ways(pkg, (receivers, steps, [(after, now) for after, now, _ in writes]))


@pytest.mark.parametrize("live", [0, 1, hs.WT - 1, hs.WT, hs.WT + 1])
def test_one_receiver_around_the_workgroup(pkg, torch_cuda, live):
    """with the head the items are live + 1: 255 fills one workgroup, 256 and 257 reach into a second"""
    got = three_ways(pkg, hs.counts_table(pkg, [live]))
    assert int(got[0][1]["aircraft"][0]) == live


def test_every_third_aircraft_written(pkg, torch_cuda):
    """lengths of 0 between the written entries, over three workgroups and a seam inside a receiver"""
    counts = [300, 0, 1, 299]
    got = three_ways(pkg, hs.counts_table(pkg, counts, every=3), refuse=True)
    first = np.concatenate([[0], np.cumsum(counts)])
    assert [int(n) for n in got[0][1]["aircraft"]] == [len(range(-a % 3 + a, b, 3)) for a, b in zip(first[:-1], first[1:])]
    assert int(got[0][1]["aircraft"].sum()) == 200


def test_many_receivers_most_of_them_empty(pkg, torch_cuda):
    got = three_ways(pkg, hs.counts_table(pkg, MANY))
    stream, rx = got[0]
    assert [int(n) for n in rx["aircraft"]] == MANY
    head = int(rx["end"][2]) - int(rx["end"][1])
    assert head > 0 and (np.diff(rx["end"].astype(np.int64))[np.array(MANY[1:]) == 0] == head).all()


def test_without_rows(pkg, torch_cuda):
    sc = hs.TABLES["three"](pkg)
    dev, host = trackers(pkg, sc[0])
    try:
        for t in (dev, host):
            hs.feed(t, sc[1][0])
        now = sc[2][0][1]
        stream, rows = host.history_pb_stream(now)
        assert dev.history_pb_stream(now, rx=False) == (stream, None)
        assert dev.history_pb(now) == hs.split(stream, rows)
        assert [ih.read_file(f)["now"] for f in dev.history_pb(now)] == [now // 1000] * 3
    finally:
        dev.close()
        host.close()
