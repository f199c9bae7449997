"""history_N.pb past one round of the writer's scan: 65 793 aircraft in one receiver are 65 794 items, 258 workgroups and
two rounds of block_sums_scan (msd_block_scan_impl.h) through scan_kernel<2>; the GPU object against the host twin, byte
for byte, stream and rows -- the condition every dense-stream writer of the tracker is held to (tests/writer_scale.py)."""
import pytest

import aircraft_streams as acs
import indep_history as ih
import writer_scale as ws

pytestmark = pytest.mark.gpu
AIRCRAFT = ws.WT * ws.WT + ws.WT + 1


def run(pkg, stream, host):
    receivers, m, f, r = stream
    t = pkg.capi.PositionTracker(capacity=1 << 17, receivers=receivers, host=host, table=True)
    t.update_nicrc(m, f, r)
    out = t.history_pb_stream(int(m["sysTimestampMsg"][-1])), t.live()
    t.close()
    return out


def test_gpu_equals_twin_past_one_round(pkg, torch_cuda):
    assert AIRCRAFT == 65793 and -(-(AIRCRAFT + 1) // ws.WT) == 258 and ws.rounds(AIRCRAFT + 1) == 2
    stream = acs.wide_stream(pkg, aircraft=AIRCRAFT, records=4 * AIRCRAFT, receivers=1, replies=True)
    want, live = run(pkg, stream, True)
    # the shape, on the twin's output: everyone is live, both outcomes occur in thousands, and the addresses written are
    # spread over the whole ordered list, so entries lie behind the first round's 65 536 items
    d = ih.read_file(want[0])
    written = int(want[1]["aircraft"][0])
    assert live == AIRCRAFT and AIRCRAFT // 4 < written < 3 * AIRCRAFT // 4 and int(want[1]["end"][0]) == len(want[0])
    addrs = sorted(int(a) for a in set(stream[2]["addr"].tolist()))
    assert len(d["history"]) == written and d["history"][-1]["addr"] in addrs[ws.WT * ws.WT:]
    got, got_live = run(pkg, stream, False)
    assert got_live == live
    diff = ws.first_difference("history_pb", got, want)
    assert diff is None, diff
