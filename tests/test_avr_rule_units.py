"""tests/c/avr_rule_units.cpp -- the AVR text input's line rule as the device runs it (msd_avr_impl.h: line_at over a
window's masks, put_record) against the host reader, msd_avr_reader_feed, one '\\n' at a time -- built as a stand-alone
program with -fsanitize=address,undefined and run on the CPU."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SAN = ["-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def cases_listed(span):
    """The newlines that tests/c/avr_rule_units.cpp compares, shape by shape as its main() lists them.  Its line() lays a
    newline, the text and a newline into the window: two comparisons, the first of them missing only where that newline
    lies in the look-back, under the first positions of the sweep.  Its lines() is line() at 4 places."""
    shortline = 1 + 14 + 1  # "*", 14 digits, ";"
    # a record line ending at every position of the span, and the newline in front of it
    positions = span + (span - (shortline + 1))
    # 4 / 14 / 28 digits; first digit at bit 0 / 1 / 36 / 37 / 63; "*" and "<"; all hex, first digit not, last digit not
    seams = 3 * 5 * 2 * 3 * 2
    guard = 2           # the longest line ending at the window's last byte
    length = 2 * 2 * 2  # two places; MSD_AVR_LINE_MAX and one more
    # rmin at LB, 77, LB - 1: discard off / on, r - REACH at rmin - 1, rmin, rmin + 1, one newline each;
    # rmin = 0: discard off / on, pieces of 2 and of 1 newline
    start = 3 * 2 * 3 * 1 + 2 * (2 + 1)
    calls = (5 * 2 * 3 + 2      # prefixes: five heads, 14 / 28 digits, short / right / long; an unknown and a bare one
             + 2 + 1            # Mode A/C off and on; missing ';'
             + 5 + 4            # NUL; white space
             + 2 + 2 * 2 + 5)   # non-hex payload digits; timestamps with keep_timestamp 0 / 1; signal digits
    return positions + seams + guard + length + start + calls * 4 * 2


def test_avr_rule_units_under_sanitizers(pkg, tmp_path):
    csrc = os.path.dirname(pkg.capi.LIB_PATH)
    inc = ["-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(csrc, "host")]
    wire, exe = str(tmp_path / "msd_wire.o"), str(tmp_path / "avr_rule_units")
    subprocess.check_call(["gcc", "-std=c11"] + SAN + inc +
                          ["-c", os.path.join(csrc, "host", "msd_wire.c"), "-o", wire])
    # (#pragma unroll in put_record is the device compiler's)
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-Wno-unknown-pragmas"] + inc +
                          [os.path.join(ROOT, "tests", "c", "avr_rule_units.cpp"), wire, "-o", exe, "-lm"])
    out = subprocess.check_output([exe], text=True, stderr=subprocess.STDOUT)
    assert "avr_rule_units: ok, " in out, out
    n = int(out.split("ok, ")[1].split()[0])
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    lib.msd_avr_span_bytes.restype = ctypes.c_uint32
    span = lib.msd_avr_span_bytes()
    assert n >= span and n == cases_listed(span), (out, cases_listed(span))
