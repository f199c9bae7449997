"""bench.py at N=1 with and without --full: a plain run prints the headline line and nothing it does not need; --full
adds the CPU baselines, the diffs against the oracle and the second reading, the PCIe-inclusive rate and the lone
capture (the replay tool's runs and the `also` workloads are left out here: they take minutes at full size)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVED = ("cpu_baseline", "message_set_diff_vs_oracle", "messages_checked", "message_set_diff_vs_second_reading",
         "pcie_inclusive", "single_capture_ms", "dropin_magbuf", "also")


def bench_line(*extra, samples):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--settle-seconds", "1", "--samples", str(samples)] + list(extra)
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"].startswith("int32")
    assert d["steps"] == 3 and d["warmup"] == 1 and d["messages_per_step"] > 1000
    assert abs(d["value"] - samples / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 1e-3
    assert d["roofline"]["launches_timed"] > 0
    return d


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone(torch_cuda):
    d = bench_line(samples=1 << 27)
    assert not [k for k in MOVED if k in d], [k for k in MOVED if k in d]


@pytest.mark.gpu
def test_full_run_adds_baselines_and_checks(torch_cuda):
    # 2^24 samples are one batch per pass, three launches in the timed region: with the default interval of one timed
    # launch in three, which of them it is depends on how many passes the (time-bound) settling took, and a timed launch
    # is only recognised behind another collect of the region -- launches_timed came out 0 in one run of three.  Every
    # launch timed: two of the three are always recognised.
    d = bench_line("--full", "--no-dropin", "--timing-interval", "1", samples=1 << 24)
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["value"] > 0
    assert d["cpu_baseline"]["two_threads_like_the_reference"]["messages"] > 0
    assert d["message_set_diff_vs_oracle"] == 0 and d["messages_checked"] == d["messages_per_step"]
    assert d["message_set_diff_vs_second_reading"]["diff"] == 0
    assert d["pcie_inclusive"]["value"] > 0 and d["single_capture_ms"]["value"] > 0
    assert "dropin_magbuf" not in d and "also" not in d       # --no-dropin; `also` only at the full 1 GiB
