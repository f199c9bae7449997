"""`msd_replay --match-modeac` needs the Mode A/C demodulator and the aircraft table: without --modeac or without
--aircraft the tool refuses before it opens anything (no GPU is touched)."""
import os
import subprocess

import pytest


def tool(pkg, *args):
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "msd_replay")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args", [
    ("--positions", "--aircraft", "--match-modeac"),                 # no --modeac
    ("--modeac", "--positions", "--match-modeac"),                   # no --aircraft
    ("--modeac", "--match-modeac"),                                  # neither --positions nor --aircraft
    ("--mode-ac", "--match-modeac", "--no-output"),
])
def test_match_modeac_is_refused_without_its_company(pkg, tmp_path, args):
    capture = tmp_path / "none.uc8"
    capture.write_bytes(b"\x7f" * 4096)
    res = tool(pkg, "--ifile", str(capture), "--iformat", "uc8", *args)
    assert res.returncode == 2 and res.stdout == ""
    assert "--match-modeac" in res.stderr and "--modeac" in res.stderr and "--aircraft" in res.stderr


def test_usage_names_the_option(pkg):
    res = tool(pkg, "--no-such-option")
    assert res.returncode == 2 and "--match-modeac" in res.stderr and "modeac-code SQUAWK,count,age,match" in res.stderr
