#!/usr/bin/env python3
"""What aircraft.pb costs.  A table of 1 000 and of 100 000 live aircraft (tests/aircraft_streams.wide_stream with replies,
four records per aircraft), on one receiver and spread over 1 024 receivers: files and bytes per second of
msd_pos_aircraft_pb -- every receiver's file in one call, into host memory -- against the host object on one core; the
one-off cost of msd_pos_pb_enable (the written state, the ground-track table built on the host and uploaded).  Medians of
--repeat calls, every call's time written down, so that the run-to-run spread is in the file.  The two streams are
compared before anything is timed.  Reported, not gated.  Not part of bench.py.  Writes profiles/aircraft_pb_rate.json.

--baseline OUT [--tree DIR]: only what exists without aircraft.pb -- msd_pos_update on a table tracker that never enables
it, device-resident records, at the same sizes -- from the tree at DIR (default: this one), written to OUT.  Run
alternately from the parent commit's tree and from this one in one session on one machine, the files go back in with
--parent-runs A.json B.json / --tree-runs C.json D.json: both lists are written as `pb_not_enabled`, with whether this
tree's median lies inside the parent's own fastest-to-slowest spread."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1_000, 1), (1_000, 1024), (100_000, 1), (100_000, 1024))
BASE_SIZES = ((1_000, 400_000), (100_000, 1_000_000))
CAPACITY = 1 << 18
NOW_MS = 1_600_000_000_000 + 30_000


def timed(call, repeat, reset=None):
    times = []
    for _ in range(repeat):
        if reset:
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


def baseline(args):
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    pkg, acs = load(os.path.abspath(args.tree))
    cases = []
    for aircraft, records in BASE_SIZES:
        m, f = acs.wide_stream(pkg, aircraft, records, replies=True)[1:3]
        dm = torch.from_numpy(m.view(np.uint8).copy()).cuda()
        df = torch.from_numpy(f.view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        gpu = pkg.capi.PositionTracker(capacity=CAPACITY, table=True)
        gpu.update_device(dm.data_ptr(), df.data_ptr(), records)
        t = timed(lambda: gpu.update_device(dm.data_ptr(), df.data_ptr(), records), args.repeat, gpu.reset)
        gpu.close()
        cases.append(dict(live_aircraft=aircraft, records=records, gpu_update_call_ms=[round(x * 1e3, 3) for x in t]))
        print(json.dumps(cases[-1]), flush=True)
    with open(args.baseline, "w") as fh:
        json.dump({"tree": os.path.abspath(args.tree), "cases": cases}, fh, indent=1)
        fh.write("\n")


def not_enabled(parent_runs, tree_runs):
    rows = []
    read = lambda paths: [json.load(open(p))["cases"] for p in paths]  # noqa: E731
    parent, tree = read(parent_runs), read(tree_runs)
    for k, case in enumerate(tree[0]):
        p = [x for run in parent for x in run[k]["gpu_update_call_ms"]]
        t = [x for run in tree for x in run[k]["gpu_update_call_ms"]]
        med = float(np.median(t))
        rows.append(dict(live_aircraft=case["live_aircraft"], records=case["records"], call="msd_pos_update",
                         parent_call_ms=p, tree_call_ms=t, parent_median_ms=round(float(np.median(p)), 3), tree_median_ms=round(med, 3),
                         parent_spread_ms=[min(p), max(p)], tree_spread_ms=[min(t), max(t)],
                         within_parent_spread=bool(min(p) <= med <= max(p))))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent-runs", nargs="*", default=[])
    ap.add_argument("--tree-runs", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aircraft_pb_rate.json"))
    args = ap.parse_args()
    if args.baseline:
        return baseline(args)
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    pkg, acs = load(ROOT)
    capi = pkg.capi
    doc = {"what": "per second, median of %d calls; see scripts/aircraft_pb_rate.py" % args.repeat, "cases": []}
    enable_ms = []
    for _ in range(args.repeat):
        t = capi.PositionTracker(capacity=CAPACITY, table=True)
        t0 = time.perf_counter()
        t.pb_enable()
        enable_ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        t.close()
    doc["pb_enable_ms"] = enable_ms
    for aircraft, receivers in SIZES:
        rx, m, f, r = acs.wide_stream(pkg, aircraft, 4 * aircraft, receivers=receivers, replies=True)
        total = np.arange(receivers, dtype=np.uint64) + 1
        gpu = capi.PositionTracker(capacity=CAPACITY, receivers=rx, table=True, pb=True)
        host = capi.PositionTracker(capacity=CAPACITY, receivers=rx, host=True, table=True, pb=True)
        gpu.update_nicrc(m, f, r)
        host.update_nicrc(m, f, r)
        stream, rows = gpu.aircraft_pb_stream(NOW_MS, total)
        hstream, hrows = host.aircraft_pb_stream(NOW_MS, total)
        assert host.pb_margin >= capi.PB_RSSI_MARGIN_ULPS, host.pb_margin
        assert stream == hstream and rows.tobytes() == hrows.tobytes(), "the GPU and the host object disagree"
        nbytes = len(stream)
        case = dict(live_aircraft=aircraft, receivers=receivers, files=receivers, aircraft_written=int(rows["aircraft"].sum()),
                    bytes=nbytes, host_min_rssi_margin_ulps=host.pb_margin)
        for key, obj in (("gpu", gpu), ("host_object", host)):
            t = timed(lambda: obj.aircraft_pb_stream(NOW_MS, total, cap=nbytes), args.repeat)
            med = float(np.median(t))
            case[key + "_files_per_s"], case[key + "_bytes_per_s"] = round(receivers / med), round(nbytes / med)
            case[key + "_aircraft_per_s"] = round(case["aircraft_written"] / med)
            case[key + "_call_ms"] = [round(x * 1e3, 3) for x in t]
        gpu.close()
        host.close()
        print(json.dumps(case), flush=True)
        doc["cases"].append(case)
    if args.parent_runs and args.tree_runs:
        doc["pb_not_enabled"] = not_enabled(args.parent_runs, args.tree_runs)
        for row in doc["pb_not_enabled"]:
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_call_ms")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
