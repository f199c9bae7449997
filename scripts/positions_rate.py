#!/usr/bin/env python3
"""Records per second of msd_pos_update with device records at 1, 1 000 and 100 000 live aircraft, and of the host twin
(msd_pos_host_update, one core) on the same streams.  Not part of bench.py.  Writes profiles/positions_rate.json.

A stream is position squitters only, round robin over the aircraft, even and odd alternating, 0.5 s between two
positions of one aircraft, each aircraft flying straight at about 400 kt: nearly every record is a global decode with a
speed check.  One call takes the whole stream (`records` records); the median of `--repeat` calls on a tracker reset in
between is reported, and for the GPU also the rate of calls of 4096 records, which is closer to what a live feed hands
over at once."""
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
import pos_streams as ps  # noqa: E402


def stream(pkg, aircraft, records):
    return ps.wide_stream(pkg, aircraft, records)[1:3]


def median_rate(call, reset, n, repeat):
    times = []
    for _ in range(repeat):
        reset()
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return n / float(np.median(times)), [round(x * 1e3, 3) for x in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "positions_rate.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    pkg = g.load_package()
    doc = {"what": "records per second, median of %d calls; see scripts/positions_rate.py" % args.repeat, "cases": []}
    for aircraft, records in ((1, 20_000), (1_000, 400_000), (100_000, 1_000_000)):
        m, f = stream(pkg, aircraft, records)
        cap = 1 << 18
        gpu = pkg.capi.PositionTracker(capacity=cap)
        twin = pkg.capi.PositionTracker(capacity=cap, host=True)
        dm = torch.from_numpy(m.view(np.uint8).copy()).cuda()
        df = torch.from_numpy(f.view(np.uint8).copy()).cuda()
        want = twin.update(m, f)
        got = gpu.update_device(dm.data_ptr(), df.data_ptr(), records)
        assert got.tobytes() == want.tobytes(), "the GPU and the twin disagree"
        decoded = int(want["decoded"].sum())
        margin = twin.stats()["min_gate_margin_m"]
        g_rate, g_ms = median_rate(lambda: gpu.update_device(dm.data_ptr(), df.data_ptr(), records), gpu.reset, records, args.repeat)
        h_rate, h_ms = median_rate(lambda: twin.update(m, f), twin.reset, records, args.repeat)

        def chunks():
            for o in range(0, records, 4096):
                n = min(4096, records - o)
                gpu.update_device(dm.data_ptr() + 56 * o, df.data_ptr() + 140 * o, n)
        c_rate, c_ms = median_rate(chunks, gpu.reset, records, max(1, args.repeat // 2))
        case = dict(live_aircraft=aircraft, records=records, decoded=decoded, twin_min_gate_margin_m=margin,
                    gpu_records_per_s=round(g_rate), gpu_call_ms=g_ms, gpu_records_per_s_calls_of_4096=round(c_rate),
                    gpu_calls_of_4096_ms=c_ms, twin_one_core_records_per_s=round(h_rate), twin_call_ms=h_ms)
        print(json.dumps(case), flush=True)
        doc["cases"].append(case)
        gpu.close()
        twin.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
