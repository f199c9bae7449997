#!/usr/bin/env python3
"""What the aircraft table costs.  On scripts/positions_rate.py's three streams (position squitters of 1, 1 000 and
100 000 aircraft) and on a stream that is half squitters and half DF4 / 5 / 11 / 20 / 21 replies at 1 000 and 100 000
aircraft (tests/aircraft_streams.wide_stream): records per second of msd_pos_update with device records on a tracker
without and with the table, of the host twin with the table on one core, and the time of one msd_pos_snapshot into host
memory.  Medians of --repeat calls, every call's time written down.  Reported, not gated.  Not part of bench.py.
Writes profiles/aircraft_table_rate.json.

--parent FILE: the positions_rate.json that the parent commit's scripts/positions_rate.py wrote on the same machine.
Its table-less rates are written beside this tree's, with whether this tree's median call time lies inside the parent's
own fastest-to-slowest spread: the table must not cost a tracker that has none anything."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import aircraft_streams as acs  # noqa: E402
import pos_streams as ps  # noqa: E402


def timed(call, reset, repeat):
    times = []
    for _ in range(repeat):
        reset()
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aircraft_table_rate.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    pkg = g.load_package()
    parent = json.load(open(args.parent))["cases"] if args.parent else []
    doc = {"what": "records per second, median of %d calls; see scripts/aircraft_rate.py" % args.repeat, "cases": []}
    cases = [("positions", a, n) for a, n in ((1, 20_000), (1_000, 400_000), (100_000, 1_000_000))]
    cases += [("squitters_and_replies", 1_000, 400_000), ("squitters_and_replies", 100_000, 1_000_000)]
    for kind, aircraft, records in cases:
        if kind == "positions":
            m, f = ps.wide_stream(pkg, aircraft, records)[1:3]
        else:
            m, f = acs.wide_stream(pkg, aircraft, records, replies=True)[1:3]
        cap = 1 << 18
        dm = torch.from_numpy(m.view(np.uint8).copy()).cuda()
        df = torch.from_numpy(f.view(np.uint8).copy()).cuda()
        case = dict(stream=kind, live_aircraft=aircraft, records=records)
        snaps = {}
        for table in (False, True):
            gpu = pkg.capi.PositionTracker(capacity=cap, table=table)
            twin = pkg.capi.PositionTracker(capacity=cap, host=True, table=table)
            want = twin.update(m, f)
            got = gpu.update_device(dm.data_ptr(), df.data_ptr(), records)
            assert got.tobytes() == want.tobytes(), "the GPU and the twin disagree"
            case["decoded"], case["twin_min_gate_margin_m"] = int(want["decoded"].sum()), twin.stats()["min_gate_margin_m"]
            t = timed(lambda: gpu.update_device(dm.data_ptr(), df.data_ptr(), records), gpu.reset, args.repeat)
            key = "gpu_table" if table else "gpu_no_table"
            case[key + "_records_per_s"] = round(records / float(np.median(t)))
            case[key + "_call_ms"] = [round(x * 1e3, 3) for x in t]
            if table:
                assert gpu.snapshot().tobytes() == twin.snapshot().tobytes(), "the snapshots disagree"
                h = timed(lambda: twin.update(m, f), twin.reset, args.repeat)
                case["twin_table_one_core_records_per_s"] = round(records / float(np.median(h)))
                case["twin_table_call_ms"] = [round(x * 1e3, 3) for x in h]
                s = timed(gpu.snapshot, lambda: None, args.repeat)
                case["gpu_snapshot_ms"] = [round(x * 1e3, 3) for x in s]
                case["gpu_snapshot_median_ms"] = round(float(np.median(s)) * 1e3, 3)
                case["snapshot_bytes"] = int(gpu.live()) * pkg.capi.AIRCRAFT_DTYPE.itemsize
            gpu.close()
            twin.close()
        case["table_cost"] = round(case["gpu_no_table_records_per_s"] / case["gpu_table_records_per_s"], 3)
        if kind == "positions":
            for p in parent:
                if p["live_aircraft"] == aircraft and p["records"] == records:
                    med = float(np.median(case["gpu_no_table_call_ms"]))
                    case["parent_gpu_call_ms"] = p["gpu_call_ms"]
                    case["parent_gpu_records_per_s"] = p["gpu_records_per_s"]
                    case["no_table_median_ms"] = round(med, 3)
                    case["no_table_median_within_parent_spread"] = bool(min(p["gpu_call_ms"]) <= med <= max(p["gpu_call_ms"]))
        print(json.dumps(case), flush=True)
        doc["cases"].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
