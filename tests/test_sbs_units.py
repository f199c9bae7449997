"""tests/c/sbs_units.c -- the SBS writer's arithmetic (msd_sbs_impl.h, what the device runs) against glibc's snprintf,
gmtime_r and atan2, and its lines against the host twin's -- built as a stand-alone program with
-fsanitize=address,undefined and run on the CPU (scripts/sanitize.sh builds the same program)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sbs_units_under_sanitizers(pkg, tmp_path):
    csrc = os.path.dirname(pkg.capi.LIB_PATH)
    exe = str(tmp_path / "sbs_units")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(csrc, "host"), os.path.join(ROOT, "tests", "c", "sbs_units.c"),
                           os.path.join(csrc, "host", "msd_pos_host.c"), "-o", exe, "-L" + csrc, "-lmodes_hip",
                           "-Wl,-rpath," + csrc, "-lpthread", "-lm"])
    out = subprocess.check_output([exe], text=True, stderr=subprocess.STDOUT)
    assert "sbs_units: ok, " in out and int(out.split("ok, ")[1].split()[0]) >= 10_000_000, out
