"""tests/c/vrs_units.c -- the VRS writer's printing (msd_vrs_impl.h, what the device runs): %f, %.2f and %.0f against
snprintf, the JSON escaping of every byte value, whole objects against the host twin's writer with length == bytes written,
the longest object -- built as a stand-alone program with -fsanitize=address,undefined and run on the CPU
(scripts/sanitize.sh builds the same program)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 10 million %f, 2 x 65536 %.2f, the halves with their neighbours and 2 million random %.0f, 256 escapes, 200 001 objects
AT_LEAST = 10_000_000 + 2 * 65536 + 2_000_000 + 256 + 200_001


def test_vrs_units_under_sanitizers(pkg, tmp_path):
    csrc = os.path.dirname(pkg.capi.LIB_PATH)
    exe = str(tmp_path / "vrs_units")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(csrc, "host"), os.path.join(ROOT, "tests", "c", "vrs_units.c"),
                           os.path.join(csrc, "host", "msd_pos_host.c"), "-o", exe, "-L" + csrc, "-lmodes_hip",
                           "-Wl,-rpath," + csrc, "-lpthread", "-lm"])
    out = subprocess.check_output([exe], text=True, stderr=subprocess.STDOUT)
    assert "vrs_units: ok, " in out and int(out.split("ok, ")[1].split()[0]) >= AT_LEAST, out
