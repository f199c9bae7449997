"""tests/c/range_units.c -- the host object's receiver range (msd_pos_host_range_*, msd_pos_impl.h's per-record function)
through a 64-slot table with expiry, a refused call, reads into buffers of exactly the size needed and a reset -- built as
a stand-alone program with -fsanitize=address,undefined and run on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_range_units_under_sanitizers(pkg, tmp_path):
    csrc = os.path.dirname(pkg.capi.LIB_PATH)
    exe = str(tmp_path / "range_units")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(csrc, "host"), os.path.join(ROOT, "tests", "c", "range_units.c"),
                           os.path.join(csrc, "host", "msd_pos_host.c"), "-o", exe, "-L" + csrc, "-lmodes_hip",
                           "-Wl,-rpath," + csrc, "-lpthread", "-lm"])
    out = subprocess.check_output([exe], text=True, stderr=subprocess.STDOUT)
    assert "range_units: ok, " in out and int(out.split("ok, ")[1].split()[0]) >= 10_000, out
