#!/usr/bin/env python3
"""Regenerates tests/golden/reference_boundary.json and tests/golden/reference_fifo.json.

Both record what the reference itself says, so that the tests built on them run on a checkout that has no
reference tree beside it (no reference source is stored, only these outputs):
  reference_boundary.json  tests/c/boundary_layout_dump.c compiled against the reference's fifo.h / convert.h /
                           demod_2400.h: offset and size of every field of `struct mag_buf`, flag, format and
                           threshold values (tests/test_boundary.py)
  reference_fifo.json      what the reference's fifo.c (oracle/_ref/libref_fifo.so, made by build()) hands its
                           consumer on the two feeds of tests/test_host_fifo.py: per buffer the sample timestamp,
                           the valid length and a SHA-256 of the samples

Needs the reference tree where oracle/oracle.py looks for it; wherever it is there, the tests compare these records
with the live headers and library again.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
import __graft_entry__ as g  # noqa: E402


def main():
    import pathlib
    import tempfile

    import test_boundary
    import test_host_fifo

    O = g.load_oracle()
    ref = test_boundary.reference_headers(O)
    if ref is None or O.build_ref() is None:
        raise SystemExit("the reference tree is not there: nothing to record")
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        (tmp / "a").mkdir()
        (tmp / "b").mkdir()
        layout = test_boundary.dump_layout(tmp, ref)
        fifo = {"depth_one_feed": test_host_fifo.record(test_host_fifo.depth_one_feed(test_host_fifo.reference(O, tmp / "a"))),
                "three_queued_feed": test_host_fifo.record(test_host_fifo.three_queued_feed(test_host_fifo.reference(O, tmp / "b")))}
    for name, doc in (("reference_boundary.json", layout), ("reference_fifo.json", fifo)):
        with open(os.path.join(HERE, name), "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(name, "written")


if __name__ == "__main__":
    main()
