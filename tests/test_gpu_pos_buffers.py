"""The position tracker's device memory (csrc/msd_devbuf.h, msd_pos.cpp): every buffer is an owning array that grows to
the largest call seen, the four writers share one output array and one skeleton, and closing the tracker returns all of
it.  Two things no other test holds: every writer and read-out on ONE tracker while the call sizes grow, shrink and grow
again -- against the host twin, by bytes, the contract has no margin --, and the free device memory across create /
destroy cycles."""
import errno

import numpy as np
import pytest

import aircraft_streams as acs

pytestmark = pytest.mark.gpu

ALL = dict(table=True, modeac=True, reduce_interval_ms=1000, sbs=True, pb=True, vrs=True)
CALLS = (3, 700, 1, 300)  # records per update: one workgroup of 256, three, one, two -- buffers larger than the call on the way down
AIRCRAFT = 300            # on two receivers: 150 each, past the writers' 128-item tile; all of them, past a workgroup


def refused(call, needed, want):
    """call() with a buffer one byte too short: -ENOSPC, and the size it would have taken"""
    with pytest.raises(Exception) as e:
        call()
    assert getattr(e.value, "code", None) == -errno.ENOSPC, e.value
    assert needed() == want


def test_every_writer_on_one_tracker_with_calls_that_grow_shrink_and_grow(pkg, torch_cuda):
    receivers, m, f, r = acs.wide_stream(pkg, aircraft=AIRCRAFT, records=sum(CALLS), receivers=2, skipped_every=17, replies=True)
    gpu, twin = (pkg.capi.PositionTracker(capacity=1024, receivers=receivers, host=h, **ALL) for h in (False, True))
    res = {t: {} for t in (gpu, twin)}

    def writers(t, mm, ff, rows, now):
        def reduce_wire():
            return t.reduce_wire(mm, rows[2])
        def sbs_wire():
            return t.sbs_wire(mm, ff, rows[3], now_ms=now, gnss=True)
        def aircraft_pb():
            return t.aircraft_pb_stream(now, messages_total=[7, 1 << 40])
        def vrs():
            return t.vrs_stream(now)
        def snapshot():
            return t.snapshot()
        def modeac_hits():
            return t.modeac_hits()
        return [reduce_wire, sbs_wire, aircraft_pb, vrs, snapshot, modeac_hits]

    at = 0
    for step, k in enumerate(CALLS):
        mm, ff, rr = m[at:at + k], f[at:at + k], r[at:at + k]
        at += k
        now = int(mm["sysTimestampMsg"][-1])
        for t in (gpu, twin):
            rows = t.update_sbs(mm, ff, rr, nicrc=True, forward=True)
            t.modeac_match(now, now)
            out = res[t]
            out["rows"] = rows
            calls = writers(t, mm, ff, rows, now)
            for j in range(len(calls)):
                call = calls[(j + step) % len(calls)]  # the order moves on by one each step
                if step == 1 and call.__name__ == "sbs_wire":
                    # a VRS write that is refused, then the SBS write into the output array it did not get to grow
                    need = len(t.vrs_stream(now)[0])
                    refused(lambda: t.vrs_stream(now, cap=need - 1), lambda: t.vrs_needed, need)
                if step == 3 and call.__name__ == "aircraft_pb":
                    # and a refused SBS write in front of a pb write
                    need = len(t.sbs_wire(mm, ff, rows[3], now_ms=now, gnss=True)[0])
                    assert need > 0
                    refused(lambda: t.sbs_wire(mm, ff, rows[3], now_ms=now, gnss=True, cap=need - 1), lambda: t.sbs_needed, need)
                out[call.__name__] = call()
        got, want = res[gpu], res[twin]
        if step == 1:  # the items of pb and VRS are past the store tile per receiver and past one workgroup together
            assert twin.live() == AIRCRAFT > 256 and np.bincount(want["snapshot"]["receiver"]).min() > 128
        for name in ("rows", "reduce_wire", "sbs_wire", "aircraft_pb", "vrs"):
            for a, b in zip(got[name], want[name]):
                assert (a == b) if isinstance(b, bytes) else (a.tobytes() == b.tobytes()), (step, name)
        # (the first call's three records deliver nothing yet: the record writers' store kernels run with no byte to write)
        assert all(len(want[name][0]) > 0 for name in ("reduce_wire", "sbs_wire", "aircraft_pb", "vrs")) == (step > 0)
        for name in ("snapshot", "modeac_hits"):
            assert got[name].tobytes() == want[name].tobytes() and len(want[name]) == twin.live(), (step, name)
    assert twin.stats()["min_gate_margin_m"] >= 1.0
    gpu.close(), twin.close()


def on_device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def test_create_destroy_cycles_return_the_device_memory(pkg, torch_cuda):
    """One cycle: a table tracker of 1 << 16 slots with all five features, one update of n = 1 << 16 device-resident
    records, each writer and read-out once, close.  After a warm-up cycle eight more must leave the free device memory
    where it was: the smallest call-sized buffer is n bytes = 64 KiB, so one buffer leaked per cycle costs at least
    8 x 64 KiB, and the bound is a fall of less than 512 KiB.
    Measured before the arrays owned their memory (hand-written release lists): a fall of 0 bytes over the eight cycles;
    with them: 0 bytes."""
    torch = torch_cuda
    n = 1 << 16
    receivers, m, f, r = acs.wide_stream(pkg, aircraft=4099, records=n, receivers=2, skipped_every=17, replies=True)
    dm, df, dr = on_device(torch, m), on_device(torch, f), on_device(torch, r)
    d_fwd = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_trk = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    now = int(m["sysTimestampMsg"][-1])

    def cycle():
        t = pkg.capi.PositionTracker(capacity=1 << 16, receivers=receivers, **ALL)
        t.update_sbs_device(dm.data_ptr(), df.data_ptr(), n, d_trk.data_ptr(), dr.data_ptr(), d_fwd.data_ptr())
        sizes = [len(t.reduce_wire(dm.data_ptr(), d_fwd.data_ptr(), n=n, on_device=True)[0]),
                 len(t.sbs_wire(dm.data_ptr(), df.data_ptr(), d_trk.data_ptr(), n=n, on_device=True, now_ms=now)[0]),
                 len(t.aircraft_pb_stream(now)[0]), len(t.vrs_stream(now)[0]), len(t.snapshot()), len(t.modeac_hits())]
        t.close()
        return sizes

    torch.cuda.synchronize()
    first = cycle()
    assert min(first) > 0 and first[4] == first[5] == 4099, first
    before = torch.cuda.mem_get_info()[0]
    for _ in range(8):
        assert cycle() == first
    fell = before - torch.cuda.mem_get_info()[0]
    print(f"free device memory fell by {fell} bytes over eight cycles")
    assert fell < 512 * 1024, fell
