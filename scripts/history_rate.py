#!/usr/bin/env python3
"""What history_N.pb costs.  A table of 1 000 and of 100 000 live aircraft (tests/aircraft_streams.wide_stream with replies,
four records per aircraft), on one receiver and spread over 1 024 receivers: the time of one msd_pos_history_pb call --
every receiver's file in one call, into host memory -- against the host object on one core, and against
msd_pos_aircraft_pb on the same table in the same process.  Medians of --repeat calls, every call's time written down, so
that the run-to-run spread is in the file.  The two streams and the rows are compared by bytes before anything is timed.
Reported, not gated.  Not part of bench.py.  Writes profiles/history_rate.json.

--baseline OUT [--tree DIR]: what must not have moved, from the tree at DIR (default: this one), written to OUT --
msd_pos_update (device-resident records) and msd_pos_aircraft_pb on a table tracker that never calls
msd_pos_history_pb.  Run alternately from the parent commit's tree and from this one, each run a process of its own, in
one session on one machine; the files go back in with --parent-runs A.json B.json / --tree-runs C.json D.json: both lists
are written as `unchanged_calls`, with whether this tree's median lies inside the parent's own fastest-to-slowest spread."""
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
        cases.append(dict(call="msd_pos_update", live_aircraft=aircraft, records=records, call_ms=[round(x * 1e3, 3) for x in t]))
        print(json.dumps(cases[-1]), flush=True)
    for aircraft, _ in BASE_SIZES:
        rx, m, f, r = acs.wide_stream(pkg, aircraft, 4 * aircraft, receivers=1, replies=True)
        gpu = pkg.capi.PositionTracker(capacity=CAPACITY, receivers=rx, table=True, pb=True)
        gpu.update_nicrc(m, f, r)
        stream, _ = gpu.aircraft_pb_stream(NOW_MS)
        t = timed(lambda: gpu.aircraft_pb_stream(NOW_MS, cap=len(stream)), args.repeat)
        gpu.close()
        cases.append(dict(call="msd_pos_aircraft_pb", live_aircraft=aircraft, bytes=len(stream), call_ms=[round(x * 1e3, 3) for x in t]))
        print(json.dumps(cases[-1]), flush=True)
    with open(args.baseline, "w") as fh:
        json.dump({"tree": os.path.abspath(args.tree), "cases": cases}, fh, indent=1)
        fh.write("\n")


def unchanged(parent_runs, tree_runs):
    rows = []
    read = lambda paths: [json.load(open(p))["cases"] for p in paths]  # noqa: E731
    parent, tree = read(parent_runs), read(tree_runs)
    for k, case in enumerate(tree[0]):
        p = [x for run in parent for x in run[k]["call_ms"]]
        t = [x for run in tree for x in run[k]["call_ms"]]
        med = float(np.median(t))
        rows.append(dict(call=case["call"], live_aircraft=case["live_aircraft"], parent_call_ms=p, tree_call_ms=t,
                         parent_median_ms=round(float(np.median(p)), 3), tree_median_ms=round(med, 3),
                         parent_spread_ms=[min(p), max(p)], tree_spread_ms=[min(t), max(t)],
                         within_parent_spread=bool(min(p) <= med <= max(p))))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent-runs", nargs="*", default=[])
    ap.add_argument("--tree-runs", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history_rate.json"))
    args = ap.parse_args()
    if args.baseline:
        return baseline(args)
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    pkg, acs = load(ROOT)
    capi = pkg.capi
    doc = {"what": "one msd_pos_history_pb call, median of %d; see scripts/history_rate.py" % args.repeat, "cases": []}
    for aircraft, receivers in SIZES:
        rx, m, f, r = acs.wide_stream(pkg, aircraft, 4 * aircraft, receivers=receivers, replies=True)
        now = int(m["sysTimestampMsg"].max()) + 1
        gpu = capi.PositionTracker(capacity=CAPACITY, receivers=rx, table=True, pb=True)
        host = capi.PositionTracker(capacity=CAPACITY, receivers=rx, host=True, table=True)
        gpu.update_nicrc(m, f, r)
        host.update_nicrc(m, f, r)
        t0 = time.perf_counter()
        stream, rows = gpu.history_pb_stream(now)  # the first call reserves the writer's scratch
        first_ms = (time.perf_counter() - t0) * 1e3
        hstream, hrows = host.history_pb_stream(now)
        assert stream == hstream and rows.tobytes() == hrows.tobytes(), "the GPU and the host object disagree"
        nbytes = len(stream)
        case = dict(live_aircraft=aircraft, receivers=receivers, aircraft_written=int(rows["aircraft"].sum()), bytes=nbytes,
                    first_call_with_size_query_ms=round(first_ms, 3))
        for key, obj in (("gpu", gpu), ("host_object", host)):
            t = timed(lambda: obj.history_pb_stream(now, cap=nbytes), args.repeat)
            med = float(np.median(t))
            case[key + "_median_ms"] = round(med * 1e3, 3)
            case[key + "_bytes_per_s"] = round(nbytes / med)
            case[key + "_call_ms"] = [round(x * 1e3, 3) for x in t]
        pb, _ = gpu.aircraft_pb_stream(now)
        t = timed(lambda: gpu.aircraft_pb_stream(now, cap=len(pb)), args.repeat)
        case["aircraft_pb_bytes"] = len(pb)
        case["aircraft_pb_median_ms"] = round(float(np.median(t)) * 1e3, 3)
        case["aircraft_pb_call_ms"] = [round(x * 1e3, 3) for x in t]
        print(json.dumps(case), flush=True)
        doc["cases"].append(case)
        gpu.close()
        host.close()
    if args.parent_runs and args.tree_runs:
        doc["unchanged_calls"] = unchanged(args.parent_runs, args.tree_runs)
        for row in doc["unchanged_calls"]:
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_call_ms")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
