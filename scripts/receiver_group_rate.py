"""Call time of a receiver group (msd_group_*) against one Demodulator per receiver; writes
profiles/receiver_group_rate.json.

    python scripts/receiver_group_rate.py [--reps 5] [--out profiles/receiver_group_rate.json]

A K-entry call takes one 131072-sample UC8 buffer from each of K receivers.  Real time for one receiver is
131072 / 2.4e6 = 54.6 ms per buffer, so a call of time t sustains K * 54.6 ms / t receivers.  Messages are
not handed to Python (deliver=False); the counters are.  The kernel trace of the K = 1024 call is a separate run:
rocprofv3 --kernel-trace --stats -- python scripts/receiver_group_rate.py --only 1024 --reps 1
(profiles/receiver_group_k1024_kernel_stats.csv)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 131072


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "receiver_group_rate.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    import torch
    capi, siggen = pkg.capi, pkg.siggen
    base = siggen.generate(siggen.make_cfg(seed=17, msgs_per_sec=3000, n_aircraft=60), 64 * CHUNK)
    ks = [a.only] if a.only else [1, 16, 256, 1024]
    kmax = max(ks)
    host = np.empty(kmax * CHUNK * 2, dtype=np.uint8)
    for r in range(kmax):
        host[r * CHUNK * 2:(r + 1) * CHUNK * 2] = base[(r % 64) * CHUNK * 2:((r % 64) + 1) * CHUNK * 2]
    dev = torch.from_numpy(host).cuda()
    res = {"buffer_samples": CHUNK, "format": "uc8", "reps": a.reps, "group": {}}
    for k in ks:
        grp = capi.ReceiverGroup(k, fmt=capi.FMT_UC8)
        row = {}
        for where, iq in (("device", dev), ("host", host)):
            grp.submit(iq, list(range(k)), deliver=False)  # warm-up: arenas, threads, first-touch
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                grp.submit(iq, list(range(k)), deliver=False)
                ts.append(time.perf_counter() - t0)
            t = float(np.median(ts))
            row[where] = {"call_ms_median": t * 1e3, "call_ms_all": [x * 1e3 for x in ts],
                          "gsamples_per_s": k * CHUNK / t / 1e9, "receivers_real_time": k * (CHUNK / 2.4e6) / t}
        t = grp.timing()  # (the group keeps no kernel times: the rocprofv3 run has them)
        row["timing"] = {k: t[k] for k in ("hits", "tries", "reruns", "resolve_passes", "resolve_fallback")}
        res["group"][str(k)] = row
        grp.close()
        print(k, json.dumps({w: round(row[w]["call_ms_median"], 3) for w in ("device", "host")}), flush=True)
    if not a.only:
        res["separate_demodulators"] = {}
        for k in (16, 64):
            ds = [capi.Demodulator(fmt=capi.FMT_UC8, flags=0) for _ in range(k)]
            for i, d in enumerate(ds):  # warm-up
                d.submit_device(dev.data_ptr() + i * CHUNK * 2, CHUNK, last=False)
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for i, d in enumerate(ds):
                    d.launch_device(dev.data_ptr() + i * CHUNK * 2, CHUNK, last=False)
                for d in ds:
                    d.collect(copy=False)
                ts.append(time.perf_counter() - t0)
            t = float(np.median(ts))
            res["separate_demodulators"][str(k)] = {"round_ms_median": t * 1e3, "gsamples_per_s": k * CHUNK / t / 1e9}
            for d in ds:
                d.close()
            print("separate", k, round(t * 1e3, 3), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
