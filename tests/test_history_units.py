"""tests/c/history_units.c -- the history_N.pb encoder (msd_history_impl.h, what the device runs) and the host twin's
writer of one entry: every varint length, length == bytes written with guard bytes behind the destination, the longest
entry, the selection and altitude rules on random entries -- built as a stand-alone program with
-fsanitize=address,undefined and run on the CPU (scripts/sanitize.sh builds the same program)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 11 addresses x 15 altitudes x 5 x 5 coordinates and three more entries, 200 000 random entries with two rules each, the head
AT_LEAST = 11 * 15 * 25 + 3 + 3 * 200_000 + 7


def test_history_units_under_sanitizers(pkg, tmp_path):
    csrc = os.path.dirname(pkg.capi.LIB_PATH)
    exe = str(tmp_path / "history_units")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(csrc, "host"), os.path.join(ROOT, "tests", "c", "history_units.c"),
                           os.path.join(csrc, "host", "msd_pos_host.c"), "-o", exe, "-L" + csrc, "-lmodes_hip",
                           "-Wl,-rpath," + csrc, "-lpthread", "-lm"])
    out = subprocess.check_output([exe], text=True, stderr=subprocess.STDOUT)
    assert "history_units: ok, " in out and int(out.split("ok, ")[1].split()[0]) >= AT_LEAST, out
