#!/usr/bin/env python3
"""Which decisions of the shared tracker headers do the constructed streams never take both ways?

The device (msd_pos_kernels.hip and its neighbours) and the host twin (libmsd_host.so) compile the same headers --
msd_trk_impl.h, msd_pos_impl.h, msd_cpr_impl.h, msd_modeac_impl.h -- and the GPU tests hold the device to the twin's bytes
on the streams of tests/*_streams.py.  A rule no stream exercises is therefore checked by nobody.  This script measures it
on the CPU: it compiles host/msd_pos_host.c, the one translation unit of the twin that includes the four headers, with
-O0 --coverage in a temporary directory, links a libmsd_host.so there from it and the tree's other host objects, runs the
CPU model tests against that library (capi.py takes the directory from MSD_LIBMODES_HIP) and reads gcov -b.

Per header it prints every line with a branch outcome that was never taken, as file:line: source, and the two
percentages (lines executed, branches taken at least once).  Nothing is written inside the tree: the objects, the .gcda /
.gcov files and pytest's cache stay in the temporary directory.  The tree must be built (build() of __graft_entry__.py).

    python scripts/stream_coverage.py             the ten CPU modules of the tracker stack
    python scripts/stream_coverage.py -k random   passes further arguments to pytest
    python scripts/stream_coverage.py --writers   the device-only writers (msd_sbs / msd_vrs / msd_pb_impl.h) instead,
                                                  through tests/c/*_units.c and the records those programs make
    python scripts/stream_coverage.py --fields    the field decoder (msd_fields_impl.h, compiled three times for the device
                                                  and once for the host) instead: msd_fields.c alone, instrumented, fed the
                                                  constructed families of tests/field_cases.py through msd_decode_fields
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "readsb-protobuf_amd", "csrc")
HEADERS = ("msd_trk_impl.h", "msd_pos_impl.h", "msd_cpr_impl.h", "msd_modeac_impl.h")
WRITERS = {"sbs": "msd_sbs_impl.h", "vrs": "msd_vrs_impl.h", "pb": "msd_pb_impl.h"}
MODULES = ("test_aircraft_model", "test_positions_model", "test_range_model", "test_sbs_model", "test_vrs_model",
           "test_pb_model", "test_reduce_model", "test_modeac_model", "test_cpr_sweep", "test_cpr_reference")
OTHER_OBJECTS = ("msd_fifo.o", "msd_sdr_ifile.o", "msd_wire.o", "msd_converter.o", "msd_demod.o")
CFLAGS = ["-std=c11", "-O0", "-g", "--coverage", "-fPIC", "-ffp-contract=off", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
          "-I" + os.path.join(CSRC, "host")]


def run(cmd, **kw):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    return r.returncode, r.stdout


def must(cmd, **kw):
    code, out = run(cmd, **kw)
    if code:
        sys.exit("%s\n%s" % (" ".join(cmd), out))
    return out


def build_twin(tmp):
    """libmsd_host.so with an instrumented msd_pos_host.o, beside a copy of libmodes_hip.so (the twin links against it)"""
    for name in ("libmodes_hip.so",) + tuple(os.path.join("host", o) for o in OTHER_OBJECTS):
        if not os.path.exists(os.path.join(CSRC, name)):
            sys.exit("build the tree first: %s is missing" % name)
    shutil.copy(os.path.join(CSRC, "libmodes_hip.so"), tmp)
    if os.path.exists(os.path.join(CSRC, "libmsd_siggen.so")):
        shutil.copy(os.path.join(CSRC, "libmsd_siggen.so"), tmp)
    must(["gcc"] + CFLAGS + ["-c", os.path.join(CSRC, "host", "msd_pos_host.c"), "-o", "msd_pos_host.o"], cwd=tmp)
    must(["gcc", "-shared", "-fPIC", "--coverage", "-o", "libmsd_host.so", "msd_pos_host.o"] +
         [os.path.join(CSRC, "host", o) for o in OTHER_OBJECTS] + ["-L.", "-lmodes_hip", "-Wl,-rpath,$ORIGIN", "-lpthread", "-lm"],
         cwd=tmp)


def run_tests(tmp, extra):
    env = dict(os.environ, MSD_LIBMODES_HIP=os.path.join(tmp, "libmodes_hip.so"), PYTHONDONTWRITEBYTECODE="1")
    cmd = [sys.executable, "-m", "pytest", "-q", "-m", "not gpu", "-p", "no:cacheprovider", "-o", "cache_dir=" + os.path.join(tmp, "cache")]
    cmd += [os.path.join(ROOT, "tests", m + ".py") for m in MODULES] + extra
    code, out = run(cmd, cwd=ROOT, env=env)
    tail = out.strip().splitlines()[-1] if out.strip() else ""
    print("pytest: %s" % tail)
    if code:
        print(out[-4000:])
        print("(the figures below are of a run with failures)")


def gcov(tmp, gcda, wanted):
    """-> {header: (lines %, lines, branches taken %, branches, [(line, source)])}"""
    out = must(["gcov", "-b", "-c", gcda], cwd=tmp)
    res = {}
    for block in out.split("\n\n"):
        m = re.search(r"File '([^']+)'", block)
        if not m or os.path.basename(m.group(1)) not in wanted:
            continue
        name = os.path.basename(m.group(1))
        lines = re.search(r"Lines executed:([\d.]+)% of (\d+)", block)
        taken = re.search(r"Taken at least once:([\d.]+)% of (\d+)", block)
        res[name] = [float(lines.group(1)), int(lines.group(2)), float(taken.group(1)) if taken else 100.0,
                     int(taken.group(2)) if taken else 0, []]
    for name in res:
        cur, open_ = None, {}
        with open(os.path.join(tmp, name + ".gcov")) as fh:
            for ln in fh:
                m = re.match(r"\s*([^:]+):\s*(\d+):(.*)", ln)
                if m and not ln.startswith(("branch", "call", "function")):
                    cur = (int(m.group(2)), m.group(3).strip())
                elif ln.startswith("branch") and cur:
                    if "never executed" in ln or re.search(r"taken 0(\s|$)", ln):
                        open_.setdefault(cur, []).append(int(ln.split()[1]))
        res[name][4] = sorted((line, src, which) for (line, src), which in open_.items())
    return res


def report(res, order):
    for name in order:
        if name not in res:
            print("%s: not in the coverage data" % name)
            continue
        lp, ln, bp, bn, open_ = res[name]
        print("%s: lines executed %.1f %% of %d, branches taken at least once %.1f %% of %d, %d lines with an outcome never taken"
              % (name, lp, ln, bp, bn, len(open_)))
        for line, src, which in open_:  # gcov numbers a line's branches in the order of its conditions, two per condition
            print("%s:%d: %s   [branches never taken: %s]" % (name, line, src, ", ".join(map(str, which))))
        print()


def writers(tmp, extra):
    """The device-only writers: tests/c/{sbs,vrs,pb}_units.c compile msd_sbs / msd_vrs / msd_pb_impl.h for the host and hold
    them to the host object's writers on pseudo-random records of their own.  Each is built instrumented, with
    host/msd_pos_host.c as its tests build it, and run as it is."""
    shutil.copy(os.path.join(CSRC, "libmodes_hip.so"), tmp)
    for key, header in WRITERS.items():
        src = os.path.join(ROOT, "tests", "c", key + "_units.c")
        exe = os.path.join(tmp, key + "_units")
        must(["gcc"] + CFLAGS + [src, os.path.join(CSRC, "host", "msd_pos_host.c"), "-o", exe, "-L.", "-lmodes_hip",
                                 "-Wl,-rpath,$ORIGIN", "-lpthread", "-lm"], cwd=tmp)
        code, out = run([exe] + extra, cwd=tmp)
        print("%s_units: exit %d, %s" % (key, code, (out.strip().splitlines() or [""])[-1]))
        gcda = [f for f in os.listdir(tmp) if f.endswith(".gcda") and f.startswith(key + "_units-" + key)]
        if gcda:
            report(gcov(tmp, gcda[0], (header,)), (header,))
        else:
            print("%s: no coverage data among %s" % (header, sorted(f for f in os.listdir(tmp) if f.endswith(".gcda"))))


FIELDS_CHILD = """
import ctypes, sys
sys.path[:0] = [%(root)r, %(tests)r]
import numpy as np
import __graft_entry__ as g
import field_cases as fc
capi = g.load_package().capi
lib = ctypes.CDLL(%(lib)r)
lib.msd_decode_fields.restype = None
out = np.zeros(1, dtype=capi.FIELDS_DTYPE)
for letter in %(letters)r:
    records, note = fc.build(capi.MESSAGE_DTYPE, letter)
    records = np.ascontiguousarray(records)
    for i in range(len(records)):
        lib.msd_decode_fields(ctypes.c_void_p(records.ctypes.data + i * records.dtype.itemsize), None, ctypes.c_void_p(out.ctypes.data))
    if letter == "f":  # and once as the replies of one buffer, each with the one before as its carry
        carry = np.zeros(1, dtype=capi.FIELDS_DTYPE)
        for i in range(len(records)):
            lib.msd_decode_fields(ctypes.c_void_p(records.ctypes.data + i * records.dtype.itemsize),
                                  ctypes.c_void_p(carry.ctypes.data) if i else None, ctypes.c_void_p(out.ctypes.data))
            carry[:] = out
    print("family %%s: %%d records -- %%s" %% (letter, len(records), note["what"]))
"""


def fields(tmp, letters):
    """msd_fields.c alone, instrumented, as a library of its own; a child process sends the families' records through its
    msd_decode_fields (the coverage data is written when that process ends)"""
    must(["gcc"] + CFLAGS + ["-shared", os.path.join(CSRC, "msd_fields.c"), "-o", "libmsd_fields_cov.so", "-lpthread", "-lm"], cwd=tmp)
    child = FIELDS_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), lib=os.path.join(tmp, "libmsd_fields_cov.so"),
                                letters=letters or "abcdefg")
    code, out = run([sys.executable, "-c", child], cwd=tmp, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    print(out.strip())
    if code:
        sys.exit("the child that feeds the families failed (%d)" % code)
    gcda = [f for f in os.listdir(tmp) if f.endswith(".gcda")]
    if not gcda:
        sys.exit("the instrumented library wrote no coverage data")
    report(gcov(tmp, gcda[0], ("msd_fields_impl.h",)), ("msd_fields_impl.h",))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--writers", action="store_true")
    ap.add_argument("--fields", action="store_true")
    ap.add_argument("--families", default="", help="with --fields: the letters of the families to send (default: all)")
    args, extra = ap.parse_known_args()
    with tempfile.TemporaryDirectory(prefix="stream_coverage_") as tmp:
        if args.writers:
            writers(tmp, extra)
            return
        if args.fields:
            fields(tmp, args.families)
            return
        build_twin(tmp)
        run_tests(tmp, extra)
        gcda = [f for f in os.listdir(tmp) if f.endswith(".gcda")]
        if not gcda:
            sys.exit("the instrumented library wrote no coverage data: was it loaded?")
        report(gcov(tmp, gcda[0], HEADERS), HEADERS)


if __name__ == "__main__":
    main()
