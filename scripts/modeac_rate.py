#!/usr/bin/env python3
"""What the Mode A/C matching costs.  Reported, not gated; not part of bench.py.  Writes profiles/modeac_rate.json.

update:  records per second of msd_pos_update with device records on a table tracker with the matching enabled, at 1 000
         and 100 000 aircraft (tests/aircraft_streams.wide_stream), with no replies and with every second record a
         Mode A/C reply spread over 1, 16 and 4096 codes (which leaves 500 and 50 000 of the aircraft), against the host
         twin on one core.  Codes and hits are compared
         with the twin's before anything is timed.
match:   the time of one msd_pos_modeac_match at 500 and 50 000 live aircraft on 1 and 1024 receivers, against the twin.
Medians of --repeat calls, every call's time written down.

--label NAME: the key the results are stored under, so that the same script can be run on two builds of the library
(MSD_LIBMODES_HIP=...): `combine` is the build as it is, `no_combine` one with -DMSD_MODEAC_COMBINE_ROUNDS=0, in which every
reply adds one to its word by itself.  A run merges into --out if that exists.
--unused-parent FILE.. --unused-this FILE..: outputs of scripts/aircraft_rate.py from one session, the parent commit's
and this tree's, run alternately (neither enables the matching): both lists of call times are written down, with whether
this tree's median lies inside the parent's fastest-to-slowest spread.  No GPU is needed for this step."""
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


def index_to_mode_a(i):
    return (i & 0o7) | ((i & 0o70) << 1) | ((i & 0o700) << 2) | ((i & 0o7000) << 3)


def stream(pkg, aircraft, records, receivers, codes):
    """wide_stream with every second record a reply on one of `codes` codes (0: no replies) -- with an even number of
    aircraft that leaves every second aircraft: the cases report the live count --; squawks for the aircraft"""
    rx, m, f, r = acs.wide_stream(pkg, aircraft, records, receivers)
    i = np.arange(records)
    f["squawk_valid"], f["squawk"] = 1, index_to_mode_a((i % aircraft) % 4096)
    if codes:
        m["msgtype"][1::2] = 32
        f["squawk"][1::2] = index_to_mode_a(((i[1::2] // 2) * 2654435761 >> 7) % codes)
    return rx, m, f, r


def ms(times):
    return [round(x * 1e3, 3) for x in times]


def same(gpu, twin, nrx):
    assert gpu.modeac_hits().tobytes() == twin.modeac_hits().tobytes(), "the hits disagree"
    for k in sorted({0, nrx // 2, nrx - 1}):
        assert gpu.modeac_codes(k).tobytes() == twin.modeac_codes(k).tobytes(), "the codes disagree"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--label", default="combine")
    ap.add_argument("--skip-match", action="store_true")
    ap.add_argument("--unused-parent", nargs="+", default=None)
    ap.add_argument("--unused-this", nargs="+", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modeac_rate.json"))
    args = ap.parse_args()
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc["what"] = "see scripts/modeac_rate.py; medians of %d calls" % args.repeat
    if args.unused_parent and args.unused_this:
        def calls(files):  # (stream, aircraft, records, tracker) -> the call times of all the files' runs
            out = {}
            for name in files:
                for c in json.load(open(name))["cases"]:
                    for key in ("gpu_no_table_call_ms", "gpu_table_call_ms"):
                        out.setdefault((c["stream"], c["live_aircraft"], c["records"], key[4:-8]), []).extend(c[key])
            return out

        parent, rows = calls(args.unused_parent), []
        for (kind, aircraft, records, tracker), t in calls(args.unused_this).items():
            p, med = parent[(kind, aircraft, records, tracker)], float(np.median(t))
            rows.append(dict(stream=kind, live_aircraft=aircraft, records=records, tracker=tracker, parent_call_ms=p,
                             this_call_ms=t, parent_median_ms=round(float(np.median(p)), 3), this_median_ms=round(med, 3),
                             within_parent_spread=bool(min(p) <= med <= max(p))))
        doc["matching_not_enabled"] = rows
    else:
        import torch
        assert torch.cuda.is_available(), "needs a GPU"
        pkg = g.load_package()
        out = dict(library=os.path.basename(os.path.dirname(pkg.capi.LIB_PATH)), update=[], match=[])
        for aircraft, records in ((1_000, 400_000), (100_000, 1_000_000)):
            for codes in (0, 1, 16, 4096):
                rx, m, f, r = stream(pkg, aircraft, records, 1, codes)
                dm = torch.from_numpy(m.view(np.uint8).copy()).cuda()
                df = torch.from_numpy(f.view(np.uint8).copy()).cuda()
                gpu = pkg.capi.PositionTracker(capacity=1 << 18, table=True, modeac=True)
                twin = pkg.capi.PositionTracker(capacity=1 << 18, host=True, table=True, modeac=True)
                want, got = twin.update(m, f), gpu.update_device(dm.data_ptr(), df.data_ptr(), records)
                assert got.tobytes() == want.tobytes(), "the GPU and the twin disagree"
                now = int(m["sysTimestampMsg"][-1])
                gpu.modeac_match(now, now), twin.modeac_match(now, now)
                same(gpu, twin, 1)
                t = timed(lambda: gpu.update_device(dm.data_ptr(), df.data_ptr(), records), gpu.reset, args.repeat)
                h = timed(lambda: twin.update(m, f), twin.reset, args.repeat)
                case = dict(live_aircraft=aircraft, records=records, replies=int((m["msgtype"] == 32).sum()), codes=codes,
                            gpu_records_per_s=round(records / float(np.median(t))), gpu_call_ms=ms(t),
                            twin_one_core_records_per_s=round(records / float(np.median(h))), twin_call_ms=ms(h))
                print(json.dumps(case), flush=True)
                out["update"].append(case)
                gpu.close(), twin.close()
        for aircraft in (() if args.skip_match else (1_000, 100_000)):
            for nrx in (1, 1024):
                rx, m, f, r = stream(pkg, aircraft, 4 * aircraft, nrx, 4096)
                gpu = pkg.capi.PositionTracker(capacity=1 << 18, receivers=rx, table=True, modeac=True)
                twin = pkg.capi.PositionTracker(capacity=1 << 18, receivers=rx, host=True, table=True, modeac=True)
                gpu.update(m, f, r), twin.update(m, f, r)
                now = int(m["sysTimestampMsg"][-1])
                gpu.modeac_match(now, now), twin.modeac_match(now, now)
                same(gpu, twin, nrx)
                t = timed(lambda: gpu.modeac_match(now, now), lambda: None, args.repeat)
                h = timed(lambda: twin.modeac_match(now, now), lambda: None, args.repeat)
                case = dict(live_aircraft=int(gpu.live()), receivers=nrx, gpu_match_median_ms=round(float(np.median(t)) * 1e3, 3),
                            gpu_match_ms=ms(t), twin_match_median_ms=round(float(np.median(h)) * 1e3, 3), twin_match_ms=ms(h))
                print(json.dumps(case), flush=True)
                out["match"].append(case)
                gpu.close(), twin.close()
        if args.skip_match:
            del out["match"]
        doc.setdefault("runs", {}).setdefault(args.label, []).append(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
