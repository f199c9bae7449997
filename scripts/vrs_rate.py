#!/usr/bin/env python3
"""What the VRS output costs.  A table of 1 000 and of 100 000 live aircraft (tests/aircraft_streams.wide_stream with
replies, four records per aircraft), on one receiver and spread over 1 024 receivers, written whole (n_parts 1) and as
readsb sends it (part 0 of 8): the time of one msd_pos_vrs call -- every receiver's document in one call, into host memory
-- against the host object on one core.  Medians of --repeat calls, every call's time written down, so that the run-to-run
spread is in the file.  The two streams and the rows are compared by bytes before anything is timed.  Reported, not
gated.  Not part of bench.py.  Writes profiles/vrs_rate.json.

--baseline OUT [--tree DIR]: what must not have moved, from the tree at DIR (default: this one), written to OUT --
msd_pos_update on a table tracker that never enables VRS (device-resident records), and msd_pos_aircraft_pb on a tracker
that enables aircraft.pb and, where the tree has it, VRS as well.  Run alternately from the parent commit's tree and from
this one in one session on one machine; the files go back in with --parent-runs A.json B.json / --tree-runs C.json D.json:
both lists are written as `unchanged_calls`, with whether this tree's median lies inside the parent's own
fastest-to-slowest spread."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1_000, 1), (1_000, 1024), (100_000, 1), (100_000, 1024))
PARTS = ((0, 1), (0, 8))
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


def live_now(m):
    """a write time at which every aircraft of the stream was seen within the last five seconds"""
    return int(m["sysTimestampMsg"].max()) + 1


def recent(m, f, r, now):
    """one more all-call reply of every aircraft just before `now`, so that all of them are selected"""
    _, first = np.unique(f["addr"].astype(np.uint64) | (r.astype(np.uint64) << 32), return_index=True)
    m2, f2 = m[first].copy(), np.zeros(len(first), dtype=f.dtype)
    m2["sysTimestampMsg"], m2["msgtype"] = now - 1, 11
    f2["addr"], f2["source"] = f["addr"][first], 3  # SOURCE_MODE_S
    return np.concatenate([m, m2]), np.concatenate([f, f2]), np.concatenate([r, r[first]])


def baseline(args):
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    pkg, acs = load(os.path.abspath(args.tree))
    has_vrs = hasattr(pkg.capi.PositionTracker, "vrs_enable")
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
        if has_vrs:
            gpu.vrs_enable()
        gpu.update_nicrc(m, f, r)
        stream, _ = gpu.aircraft_pb_stream(NOW_MS)
        t = timed(lambda: gpu.aircraft_pb_stream(NOW_MS, cap=len(stream)), args.repeat)
        gpu.close()
        cases.append(dict(call="msd_pos_aircraft_pb", live_aircraft=aircraft, vrs_enabled=has_vrs, bytes=len(stream),
                          call_ms=[round(x * 1e3, 3) for x in t]))
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
        rows.append(dict(call=case["call"], live_aircraft=case["live_aircraft"], vrs_enabled=bool(case.get("vrs_enabled", False)),
                         parent_call_ms=p, tree_call_ms=t, parent_median_ms=round(float(np.median(p)), 3),
                         tree_median_ms=round(med, 3), parent_spread_ms=[min(p), max(p)], tree_spread_ms=[min(t), max(t)],
                         within_parent_spread=bool(min(p) <= med <= max(p))))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent-runs", nargs="*", default=[])
    ap.add_argument("--tree-runs", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vrs_rate.json"))
    args = ap.parse_args()
    if args.baseline:
        return baseline(args)
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    pkg, acs = load(ROOT)
    capi = pkg.capi
    doc = {"what": "one msd_pos_vrs call, median of %d; see scripts/vrs_rate.py" % args.repeat, "cases": []}
    enable_ms = []
    for _ in range(args.repeat):
        t = capi.PositionTracker(capacity=CAPACITY, table=True)
        t0 = time.perf_counter()
        t.vrs_enable()
        enable_ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        t.close()
    doc["vrs_enable_ms"] = enable_ms
    for aircraft, receivers in SIZES:
        rx, m, f, r = acs.wide_stream(pkg, aircraft, 4 * aircraft, receivers=receivers, replies=True)
        now = live_now(m)
        m, f, r = recent(m, f, r, now)
        gpu = capi.PositionTracker(capacity=CAPACITY, receivers=rx, table=True, vrs=True)
        host = capi.PositionTracker(capacity=CAPACITY, receivers=rx, host=True, table=True, vrs=True)
        gpu.update_nicrc(m, f, r)
        host.update_nicrc(m, f, r)
        for part, n_parts in PARTS:
            stream, rows = gpu.vrs_stream(now, part, n_parts)
            hstream, hrows = host.vrs_stream(now, part, n_parts)
            assert stream == hstream and rows.tobytes() == hrows.tobytes(), "the GPU and the host object disagree"
            nbytes = len(stream)
            case = dict(live_aircraft=aircraft, receivers=receivers, part=part, n_parts=n_parts,
                        aircraft_written=int(rows["aircraft"].sum()), bytes=nbytes)
            for key, obj in (("gpu", gpu), ("host_object", host)):
                t = timed(lambda: obj.vrs_stream(now, part, n_parts, cap=nbytes), args.repeat)
                med = float(np.median(t))
                case[key + "_median_ms"] = round(med * 1e3, 3)
                case[key + "_bytes_per_s"] = round(nbytes / med)
                case[key + "_call_ms"] = [round(x * 1e3, 3) for x in t]
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
