"""tests/c/pb_units.c -- the aircraft.pb encoder (msd_pb_impl.h, what the device runs): varints, length == bytes written,
the longest entry, the truncating ground-track table against msd_aircraft_to_float -- built as a stand-alone program with
-fsanitize=address,undefined and run on the CPU (scripts/sanitize.sh builds the same program)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pb_units_under_sanitizers(pkg, tmp_path):
    csrc = os.path.dirname(pkg.capi.LIB_PATH)
    exe = str(tmp_path / "pb_units")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(csrc, "host"), os.path.join(ROOT, "tests", "c", "pb_units.c"),
                           os.path.join(csrc, "host", "msd_pos_host.c"), "-o", exe, "-L" + csrc, "-lmodes_hip",
                           "-Wl,-rpath," + csrc, "-lpthread", "-lm"])
    out = subprocess.check_output([exe], text=True, stderr=subprocess.STDOUT)
    assert "pb_units: ok, " in out and int(out.split("ok, ")[1].split()[0]) >= 8_000_000, out
