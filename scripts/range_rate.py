#!/usr/bin/env python3
"""What the receiver range costs msd_pos_update, with device records at 1 000 and 100 000 live aircraft -- the workloads of
scripts/positions_rate.py, seen from one receiver with a location (every evaluated record then adds to the same receiver's
words: the contended case) and from 1 024 of them.  Not part of bench.py.  Writes profiles/range_rate.json.

Per workload, records per second (median of --repeat calls of the whole stream on a tracker reset in between, one warm-up
call first) of a tracker that never enables the range, of one that keeps distance and longest, and of one that keeps the
polar range too; and the range kernel's own time (events around it: msd_pos_range_measure, msd_pos.h) with and without the
per-wavefront reduction in front of its atomics.  --runs N repeats the not-enabled measurement N times in one process and
keeps every median: run on the parent commit (which has no range: the script then measures nothing else), that is the
run-to-run spread a tracker that never enables the range has to stay inside; --parent FILE ... copies such documents into
the output beside this commit's own figures (several: the parent's tree and this one run alternately in one session,
the parent's runs pooled), --own FILE ... pools this commit's earlier documents of the same session the same way."""
import argparse
import ctypes as C
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

WORKLOADS = ((1_000, 400_000), (100_000, 1_000_000))


def median_ms(call, reset, repeat):
    reset()
    call()  # warm-up: buffers grown, code loaded
    times = []
    for _ in range(repeat):
        reset()
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), [round(x, 3) for x in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent", nargs="*", default=[], help="documents this script wrote on the parent commit")
    ap.add_argument("--own", nargs="*", default=[], help="documents this script wrote on this commit earlier in the session")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_rate.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    pkg = g.load_package()
    has_range = hasattr(pkg.capi.PositionTracker, "range_enable")
    doc = {"what": "msd_pos_update with device records, ms per call of the whole stream and records per second; medians of "
                   "%d calls; see scripts/range_rate.py" % args.repeat,
           "device": torch.cuda.get_device_name(0), "has_range": has_range, "cases": []}
    for aircraft, records in WORKLOADS:
        for nrx in (1, 1024):
            receivers, m, f, r = ps.wide_stream(pkg, aircraft, records, receivers=nrx)
            receivers = [dict(lat=10.0 + 0.01 * k, lon=20.0 - 0.01 * k, latlon_valid=1) for k in range(nrx)]
            dm = torch.from_numpy(m.view(np.uint8).copy()).cuda()
            df = torch.from_numpy(f.view(np.uint8).copy()).cuda()
            dr = torch.from_numpy(r.copy()).cuda()
            torch.cuda.synchronize()
            case = dict(live_aircraft=aircraft, records=records, receivers=nrx)

            def measure(tracker):
                call = lambda: tracker.update_device(dm.data_ptr(), df.data_ptr(), records, dr.data_ptr())  # noqa: E731
                return median_ms(call, tracker.reset, args.repeat)

            plain = pkg.capi.PositionTracker(capacity=1 << 18, receivers=receivers)
            runs = [measure(plain) for _ in range(args.runs)]
            case["not_enabled_ms_per_run"] = [round(x[0], 3) for x in runs]
            case["not_enabled_ms"] = round(float(np.median([x[0] for x in runs])), 3)
            case["not_enabled_records_per_s"] = round(records / case["not_enabled_ms"] * 1e3)
            want = plain.update_device(dm.data_ptr(), df.data_ptr(), records, dr.data_ptr())
            plain.close()
            if has_range:
                for name, polar in (("distance_and_longest", False), ("with_polar_range", True)):
                    t = pkg.capi.PositionTracker(capacity=1 << 18, receivers=receivers, range=True, polar=polar)
                    ms, every = measure(t)
                    case[name + "_ms"], case[name + "_ms_each"] = round(ms, 3), every
                    case[name + "_records_per_s"] = round(records / ms * 1e3)
                    got = t.update_device(dm.data_ptr(), df.data_ptr(), records, dr.data_ptr())
                    assert got.tobytes() == want.tobytes(), "the range changed the positions"
                    if polar:
                        lib, kernel, rows = pkg.capi.lib(), {}, {}
                        lib.msd_pos_range_measure.argtypes = [C.c_void_p, C.c_int, C.c_int]
                        lib.msd_pos_range_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
                        for combine in (1, 0):
                            assert lib.msd_pos_range_measure(t.h, combine, 1) == 0
                            each = []
                            for _ in range(args.repeat + 1):
                                t.reset()
                                t.update_device(dm.data_ptr(), df.data_ptr(), records, dr.data_ptr())
                                ms = C.c_float(0)
                                assert lib.msd_pos_range_kernel_ms(t.h, C.byref(ms)) == 0
                                each.append(round(ms.value, 4))
                            kernel[combine] = each[1:]  # the first call is the warm-up
                            rows[combine] = t.range_read().tobytes() + t.range_distances().tobytes()
                        assert rows[0] == rows[1], "the reduction changed the result"
                        case["evaluated"] = int(t.range_read()["evaluated"].sum())
                        case["range_kernel_ms_reduced_per_wavefront"] = float(np.median(kernel[1]))
                        case["range_kernel_ms_one_atomic_per_lane"] = float(np.median(kernel[0]))
                        case["range_kernel_ms_each"] = {"reduced": kernel[1], "per_lane": kernel[0]}
                    t.close()
            print(json.dumps(case), flush=True)
            doc["cases"].append(case)

    def pooled(paths):
        docs = [json.load(open(p)) for p in paths]
        return [[x for d in docs for x in d["cases"][k]["not_enabled_ms_per_run"]] for k in range(len(doc["cases"]))]

    if args.own:
        for c, runs in zip(doc["cases"], pooled(args.own)):
            c["not_enabled_ms_per_run"] = runs + c["not_enabled_ms_per_run"]  # in the order they were measured
            c["not_enabled_ms"] = round(float(np.median(c["not_enabled_ms_per_run"])), 3)
            c["not_enabled_records_per_s"] = round(c["records"] / c["not_enabled_ms"] * 1e3)
    if args.parent:
        doc["parent_commit"] = []
        for c, runs in zip(doc["cases"], pooled(args.parent)):
            doc["parent_commit"].append(dict(live_aircraft=c["live_aircraft"], records=c["records"], receivers=c["receivers"],
                                             not_enabled_ms_per_run=runs, not_enabled_ms=round(float(np.median(runs)), 3)))
            c["parent_spread_ms"] = [min(runs), max(runs)]
            c["not_enabled_inside_parent_spread"] = bool(c["not_enabled_ms"] <= max(runs))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
