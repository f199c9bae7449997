#!/usr/bin/env python3
"""What the SBS output costs.  On scripts/aircraft_rate.py's streams of squitters and replies at 1 000 and 100 000
aircraft (tests/aircraft_streams.wide_stream): lines and bytes per second of msd_pos_update_sbs + msd_pos_sbs_wire with
the records and the rows in device memory, and of the same two calls from and to host memory; records per second of
msd_pos_update_sbs alone beside msd_pos_update_reduce at the same sizes (the update it is set beside); the host twin on
one core; and the one-off cost of msd_pos_sbs_enable (the ground-track table, built on the host and uploaded).  Medians
of --repeat calls on a reset tracker, every call's time written down, so that the run-to-run spread is in the file.
Reported, not gated.  Not part of bench.py.  Writes profiles/sbs_rate.json.

--baseline OUT [--tree DIR]: only what exists without SBS -- msd_pos_update_reduce on a tracker that never enables SBS,
device-resident, at the same sizes -- from the tree at DIR (default: this one), written to OUT.  Run alternately from the
parent commit's tree and from this one in one session on one machine, the files go back in with
--parent-runs A.json B.json / --tree-runs C.json D.json: both lists are written as `sbs_not_enabled`, with whether this
tree's median lies inside the parent's own fastest-to-slowest spread."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1_000, 400_000), (100_000, 1_000_000))
CAPACITY = 1 << 18


def timed(call, reset, repeat):
    times = []
    for _ in range(repeat):
        reset()
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return times


def load(tree):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import __graft_entry__ as g
    import aircraft_streams as acs
    return g.load_package(), acs


def device_records(torch, m, f):
    dm = torch.from_numpy(m.view(np.uint8).copy()).cuda()
    df = torch.from_numpy(f.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return dm, df


def baseline(args):
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    pkg, acs = load(os.path.abspath(args.tree))
    cases = []
    for aircraft, records in SIZES:
        m, f = acs.wide_stream(pkg, aircraft, records, replies=True)[1:3]
        dm, df = device_records(torch, m, f)
        dv = torch.zeros(records, dtype=torch.uint8, device="cuda")
        gpu = pkg.capi.PositionTracker(capacity=CAPACITY, table=True, reduce_interval_ms=125)
        gpu.update_reduce_device(dm.data_ptr(), df.data_ptr(), records, dv.data_ptr())
        t = timed(lambda: gpu.update_reduce_device(dm.data_ptr(), df.data_ptr(), records, dv.data_ptr()), gpu.reset, args.repeat)
        gpu.close()
        cases.append(dict(live_aircraft=aircraft, records=records, gpu_update_reduce_call_ms=[round(x * 1e3, 3) for x in t]))
        print(json.dumps(cases[-1]), flush=True)
    with open(args.baseline, "w") as fh:
        json.dump({"tree": os.path.abspath(args.tree), "cases": cases}, fh, indent=1)
        fh.write("\n")


def not_enabled(parent_runs, tree_runs):
    rows = []
    read = lambda paths: [json.load(open(p))["cases"] for p in paths]  # noqa: E731
    parent, tree = read(parent_runs), read(tree_runs)
    for k, case in enumerate(tree[0]):
        p = [x for run in parent for x in run[k]["gpu_update_reduce_call_ms"]]
        t = [x for run in tree for x in run[k]["gpu_update_reduce_call_ms"]]
        med = float(np.median(t))
        rows.append(dict(live_aircraft=case["live_aircraft"], records=case["records"], call="msd_pos_update_reduce",
                         parent_call_ms=p, tree_call_ms=t, parent_median_ms=round(float(np.median(p)), 3), tree_median_ms=round(med, 3),
                         parent_spread_ms=[min(p), max(p)], within_parent_spread=bool(min(p) <= med <= max(p))))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent-runs", nargs="*", default=[])
    ap.add_argument("--tree-runs", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sbs_rate.json"))
    args = ap.parse_args()
    if args.baseline:
        return baseline(args)
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    pkg, acs = load(ROOT)
    capi = pkg.capi
    doc = {"what": "per second, median of %d calls on a reset tracker; see scripts/sbs_rate.py" % args.repeat, "cases": []}
    enable_ms = []
    for _ in range(args.repeat):
        t = capi.PositionTracker(capacity=64, table=True)
        t0 = time.perf_counter()
        t.sbs_enable()
        enable_ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        t.close()
    doc["sbs_enable_ms"] = enable_ms
    for aircraft, records in SIZES:
        m, f = acs.wide_stream(pkg, aircraft, records, replies=True)[1:3]
        dm, df = device_records(torch, m, f)
        dv = torch.zeros(records, dtype=torch.uint8, device="cuda")
        dt = torch.zeros(records * capi.SBS_TRACK_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        gpu = capi.PositionTracker(capacity=CAPACITY, table=True, reduce_interval_ms=125, sbs=True)
        twin = capi.PositionTracker(capacity=CAPACITY, host=True, table=True, sbs=True)
        rows = twin.update_sbs(m, f, nicrc=False)[3]
        gpu.update_sbs_device(dm.data_ptr(), df.data_ptr(), records, dt.data_ptr())
        assert dt.cpu().numpy().tobytes() == rows.tobytes(), "the GPU and the twin disagree"
        kw = dict(now_ms=1_600_000_000_000, utc_offset_ms=3600000)
        stream, ends = gpu.sbs_wire(dm.data_ptr(), df.data_ptr(), dt.data_ptr(), n=records, on_device=True, **kw)
        assert stream == twin.sbs_wire(m, f, rows, **kw)[0], "the streams disagree"
        nbytes, lines = len(stream), int(np.count_nonzero(np.diff(np.concatenate([[0], ends]))))
        case = dict(live_aircraft=aircraft, records=records, lines=lines, bytes=nbytes,
                    twin_min_gate_margin_m=twin.stats()["min_gate_margin_m"])

        def gpu_update():
            gpu.update_sbs_device(dm.data_ptr(), df.data_ptr(), records, dt.data_ptr())

        def gpu_both():
            gpu_update()
            gpu.sbs_wire(dm.data_ptr(), df.data_ptr(), dt.data_ptr(), n=records, on_device=True, cap=nbytes, **kw)

        def gpu_host():
            r = gpu.update_sbs(m, f, nicrc=False)[3]
            gpu.sbs_wire(m, f, r, cap=nbytes, **kw)

        def twin_both():
            r = twin.update_sbs(m, f, nicrc=False)[3]
            twin.sbs_wire(m, f, r, cap=nbytes, **kw)
        for key, call, reset in (
                ("gpu_update_reduce", lambda: gpu.update_reduce_device(dm.data_ptr(), df.data_ptr(), records, dv.data_ptr()), gpu.reset),
                ("gpu_update_sbs", gpu_update, gpu.reset), ("gpu_update_and_wire", gpu_both, gpu.reset),
                ("gpu_update_and_wire_host_memory", gpu_host, gpu.reset), ("twin_update_and_wire", twin_both, twin.reset)):
            t = timed(call, reset, args.repeat)
            med = float(np.median(t))
            case[key + "_records_per_s"] = round(records / med)
            if "wire" in key:
                case[key + "_lines_per_s"], case[key + "_bytes_per_s"] = round(lines / med), round(nbytes / med)
            case[key + "_call_ms"] = [round(x * 1e3, 3) for x in t]
        gpu.close()
        twin.close()
        print(json.dumps(case), flush=True)
        doc["cases"].append(case)
    if args.parent_runs and args.tree_runs:
        doc["sbs_not_enabled"] = not_enabled(args.parent_runs, args.tree_runs)
        for row in doc["sbs_not_enabled"]:
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_call_ms")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
