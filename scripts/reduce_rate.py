#!/usr/bin/env python3
"""What the reduced Beast output costs and what it saves.  On scripts/aircraft_rate.py's streams of squitters and replies
at 1 000 and 100 000 aircraft (tests/aircraft_streams.wide_stream), at the intervals 125 and 1000 ms: records per second
of msd_pos_update_reduce with the records and the verdicts in device memory, and of that call followed by
msd_pos_reduce_wire into host memory; the same two for the host twin on one core; and the share of the records and of the
bytes of the unreduced Beast feed that are forwarded.  Medians of --repeat calls on a reset tracker, every call's time
written down.  Reported, not gated.  Not part of bench.py.  Writes profiles/reduce_rate.json.

--parent-runs A.json B.json / --tree-runs C.json D.json: what scripts/aircraft_rate.py -- a tracker that never enables
reducing -- wrote from the parent commit and from this tree, run alternately in one session on one machine.  Both lists
go into the JSON as `reducing_not_enabled`, with whether each of this tree's medians lies inside the parent's own
fastest-to-slowest spread."""
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


def timed(call, reset, repeat):
    times = []
    for _ in range(repeat):
        reset()
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return times


def not_enabled(parent_runs, tree_runs):
    rows = []
    load = lambda paths: [json.load(open(p))["cases"] for p in paths]  # noqa: E731
    parent, tree = load(parent_runs), load(tree_runs)
    for k, case in enumerate(tree[0]):
        for key in ("gpu_no_table_call_ms", "gpu_table_call_ms"):
            p = [x for run in parent for x in run[k][key]]
            t = [x for run in tree for x in run[k][key]]
            med = float(np.median(t))
            rows.append(dict(stream=case["stream"], live_aircraft=case["live_aircraft"], records=case["records"], tracker=key[4:-8],
                             parent_call_ms=p, tree_call_ms=t, tree_median_ms=round(med, 3),
                             within_parent_spread=bool(min(p) <= med <= max(p))))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--parent-runs", nargs="*", default=[])
    ap.add_argument("--tree-runs", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduce_rate.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    pkg = g.load_package()
    doc = {"what": "records per second, median of %d calls; see scripts/reduce_rate.py" % args.repeat, "cases": []}
    for aircraft, records in ((1_000, 400_000), (100_000, 1_000_000)):
        m, f = acs.wide_stream(pkg, aircraft, records, replies=True)[1:3]
        dm = torch.from_numpy(m.view(np.uint8).copy()).cuda()
        df = torch.from_numpy(f.view(np.uint8).copy()).cuda()
        dv = torch.zeros(records, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for interval in (125, 1000):
            cap = 1 << 18
            gpu = pkg.capi.PositionTracker(capacity=cap, table=True, reduce_interval_ms=interval)
            twin = pkg.capi.PositionTracker(capacity=cap, host=True, table=True, reduce_interval_ms=interval)
            want = twin.update_reduce(m, f)
            gpu.update_reduce_device(dm.data_ptr(), df.data_ptr(), records, dv.data_ptr())
            verdicts = dv.cpu().numpy()
            assert verdicts.tobytes() == want[2].tobytes(), "the GPU and the twin disagree"
            stream, ends = gpu.reduce_wire(dm.data_ptr(), dv.data_ptr(), n=records, on_device=True)
            assert stream == twin.reduce_wire(m, verdicts)[0], "the streams disagree"
            feed = len(twin.reduce_wire(m, np.full(records, 3, dtype=np.uint8))[0])  # every record that Beast output sends
            cap_bytes = len(stream)
            case = dict(live_aircraft=aircraft, records=records, interval_ms=interval,
                        twin_min_gate_margin_m=twin.stats()["min_gate_margin_m"],
                        records_forwarded=int(np.count_nonzero(np.diff(np.concatenate([[0], ends])))),
                        verdicts_forward=int(np.count_nonzero(verdicts & 1)), bytes_forwarded=cap_bytes, bytes_of_the_feed=feed)
            case["share_of_records"] = round(case["records_forwarded"] / records, 4)
            case["share_of_bytes"] = round(cap_bytes / feed, 4)

            def gpu_update():
                gpu.update_reduce_device(dm.data_ptr(), df.data_ptr(), records, dv.data_ptr())

            def gpu_both():
                gpu_update()
                gpu.reduce_wire(dm.data_ptr(), dv.data_ptr(), n=records, on_device=True, cap=cap_bytes)

            def twin_both():
                v = twin.update_reduce(m, f)[2]
                twin.reduce_wire(m, v, cap=cap_bytes)
            for key, call, reset in (("gpu_update_reduce", gpu_update, gpu.reset), ("gpu_update_and_wire", gpu_both, gpu.reset),
                                     ("twin_update_reduce", lambda: twin.update_reduce(m, f), twin.reset),
                                     ("twin_update_and_wire", twin_both, twin.reset)):
                t = timed(call, reset, args.repeat)
                case[key + "_records_per_s"] = round(records / float(np.median(t)))
                case[key + "_call_ms"] = [round(x * 1e3, 3) for x in t]
            gpu.close()
            twin.close()
            print(json.dumps(case), flush=True)
            doc["cases"].append(case)
    if args.parent_runs and args.tree_runs:
        doc["reducing_not_enabled"] = not_enabled(args.parent_runs, args.tree_runs)
        for row in doc["reducing_not_enabled"]:
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_call_ms")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
