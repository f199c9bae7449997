"""Call time of AVR text input per receiver of a group (msd_group_accept_avr) against the only alternative there was,
one msd_accept_avr call per receiver on contexts of their own; writes profiles/group_avr_rate.json.

    python scripts/group_avr_rate.py [--receivers 1024] [--bytes 4096] [--reps 20] [--contexts 1024]

Workload: K = 1024 receivers, 4 KiB of AVR text each per round (what a live feeder delivers per poll), the raw output of
replayed captures cut at arbitrary byte positions, so every receiver carries a kept line from round to round.  Both ways
run in one process, alternating round by round, from host and from device memory, over the same bytes with the same
now_ms; no message is handed to Python (no sink), the counters are compared at the end.  --contexts below the number of
receivers makes the 1024 context calls of a round cycle over fewer contexts (still one small call per receiver; the
counters are then not compared).  --only 1 times a one-entry call, for the launch count.

The per-kernel table is a separate run:
    rocprofv3 --kernel-trace --stats -- python scripts/group_avr_rate.py --reps 3 --group-only --out /tmp/x.json
(profiles/group_avr_k1024_kernel_stats.csv); the same with --only 1 shows the same kernels, each launched as often:
the launches of a call do not depend on its number of entries."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 131072


def avr_stream(pkg, O, seed, nbytes):
    """at least nbytes of AVR lines: the oracle's replay of a generated capture, repeated"""
    iq = pkg.siggen.generate(pkg.siggen.make_cfg(seed=seed, msgs_per_sec=3000, n_aircraft=60), 4 * CHUNK)
    msgs, _ = O.Oracle(O.FMT_UC8, 58, 1, 0).replay(iq)
    one = b"".join(O.avr_line(m) for m in msgs)
    return (one * (nbytes // len(one) + 1))[:nbytes]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--receivers", type=int, default=1024)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--contexts", type=int, default=1024)
    ap.add_argument("--only", type=int, default=0, help="entries per group call (default: all receivers)")
    ap.add_argument("--group-only", action="store_true", help="no contexts (for the kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_avr_rate.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    pkg, O = g.load_package(), g.load_oracle()
    import torch
    capi = pkg.capi
    K, B = a.receivers, a.bytes
    n = a.only or K
    rounds = a.reps + 1  # one warm-up round: scratch, first touch
    streams = [avr_stream(pkg, O, 100 + s, rounds * B) for s in range(8)]
    host = np.empty((rounds, K, B), dtype=np.uint8)  # round-major: one contiguous array per call
    for r in range(K):
        host[:, r, :] = np.frombuffer(streams[r % 8], dtype=np.uint8).reshape(rounds, B)
    dev = torch.from_numpy(host).cuda()
    L = capi._group_lib()
    res = {"receivers": K, "entries_per_call": n, "bytes_per_entry": B, "reps": a.reps,
           "calls_timed": "group: one msd_group_accept_avr with no sink; contexts: one msd_accept_avr with no sink per "
                          "receiver, in turn; one round of each alternating, in one process"}
    for where in ("device", "host"):
        grp = capi.ReceiverGroup(K, fmt=capi.FMT_UC8)
        ctxs = [] if a.group_only else [capi.Demodulator(fmt=capi.FMT_UC8, nfix_crc=1) for _ in range(min(a.contexts, K))]
        ent = (capi.GroupAvrEntry * n)()
        tg, tc = [], []
        for k in range(rounds):
            base = k * K * B
            for i in range(n):
                ent[i] = capi.GroupAvrEntry(i, 0, base + i * B, B, 0, 1000 + k)
            ptr = dev.data_ptr() if where == "device" else host.ctypes.data
            t0 = time.perf_counter()
            rc = L.msd_group_accept_avr(grp._h, C.c_void_p(ptr), 1 if where == "device" else 0, ent, n, None, None)
            t1 = time.perf_counter()
            assert rc == 0, L.msd_group_last_error(grp._h)
            for i in range(n if ctxs else 0):
                rc = capi.lib().msd_accept_avr(ctxs[i % len(ctxs)]._h, C.c_void_p(ptr + base + i * B), B,
                                               1 if where == "device" else 0, 0, 1000 + k, None, None)
                assert rc == 0
            t2 = time.perf_counter()
            if k:  # (round 0 is the warm-up)
                tg.append(t1 - t0)
                tc.append(t2 - t1)
        row = {"group_call_ms_median": float(np.median(tg)) * 1e3, "group_call_ms_all": [x * 1e3 for x in tg],
               "group_mbytes_per_s": n * B / float(np.median(tg)) / 1e6}
        if ctxs:
            row.update({"contexts": len(ctxs), "context_round_ms_median": float(np.median(tc)) * 1e3,
                        "context_round_ms_all": [x * 1e3 for x in tc],
                        "context_mbytes_per_s": n * B / float(np.median(tc)) / 1e6})
            if len(ctxs) == K:  # the same bytes in the same calls: the same counters
                for i in (0, n // 2, n - 1):
                    gs, cs = grp.remote_stats(i), ctxs[i].remote_stats()
                    gs.pop("tile_rewalks"), cs.pop("tile_rewalks")
                    assert gs == cs, (i, gs, cs)
                    assert grp.avr_stats(i) == ctxs[i].avr_stats(), i
                row["counters_equal"] = True
        row["lines_receiver_0"], row["frames_receiver_0"] = grp.avr_stats(0)["lines"], grp.remote_stats(0)["frames"]
        res[where] = row
        print(where, json.dumps({k: round(v, 3) for k, v in row.items() if k.endswith("median")}), flush=True)
        for d in ctxs:
            d.close()
        grp.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
