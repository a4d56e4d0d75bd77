#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Generate the count-alignments / ecdump fixture (``counts_cases.json``) in this directory by RUNNING THE REFERENCE.

Build-container only, like ``make_golden_gt.py``: imports the unmodified reference package from ``/root/reference`` with the
stand-ins of ``_standins/`` ahead of it, loads each ``.bin`` with its ``ecload``, calls ``count_alignments()``,
``count_unique_reads(ignore_haplotype=False)`` and ``count_unique_reads(ignore_haplotype=True)`` on what it returns, runs its
``ecdump`` under a log capture, and records data only:

  counts_cases.json    per case: the .bin, its shape (H, T), the three arrays (flattened; all their values, or the (flat index, value)
                       pairs of their non-zeros, whichever is shorter; every value the reference returned is a whole number,
                       recorded as int), the exception the counting raised instead (multisample files), and the (level, message)
                       lines of ecdump

    python tests/golden/make_golden_counts.py
"""
from __future__ import print_function

import json
import logging
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.join(HERE, "_standins"))

import numpy as np  # noqa: E402

from alntools import bin_utils, utils  # noqa: E402  (the reference)

GOLDEN = "<golden>"  # this directory, in the recorded messages

COUNTED = ["g1_edge.bin", "g1_edge_targets.bin", "g2_c1.bin", "g5_binwalk.bin", "gt_h8_in.bin", "gt_c1.out.bin"]
DUMP_ONLY = ["g4_multi_min0.bin"]


class _Capture(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.lines = []

    def emit(self, record):
        self.lines.append((record.levelname, record.getMessage()))


def record(a):
    """A whole-number array as data: {"dense": every value} or {"pairs": [flat index, value] of the non-zeros}, whichever is shorter."""
    a = np.asarray(a, dtype=np.float64).ravel()
    assert np.all(a == np.floor(a)), "the reference returned a fraction"
    dense = {"dense": [int(v) for v in a]}
    pairs = {"pairs": [[int(i), int(a[i])] for i in np.flatnonzero(a)]}
    return min(dense, pairs, key=lambda d: len(json.dumps(d, separators=(",", ":"))))


def dump_lines(path):
    cap = _Capture()
    log = utils.get_logger()
    log.addHandler(cap)
    log.setLevel(logging.DEBUG)
    try:
        bin_utils.ecdump(path)
    finally:
        log.removeHandler(cap)
    return [[lvl, m.replace(HERE, GOLDEN)] for lvl, m in cap.lines if lvl in ("INFO", "ERROR")]


def main():
    cases = []
    for name in COUNTED + DUMP_ONLY:
        path = os.path.join(HERE, name)
        case = {"bin": name, "ecdump": dump_lines(path), "aln": None, "uniq": None, "locus_uniq": None, "raises": None}
        apm = bin_utils.ecload(path)
        case["shape"] = [int(apm.num_haplotypes), int(apm.num_loci)]
        try:
            aln = apm.count_alignments()
            uniq = apm.count_unique_reads(ignore_haplotype=False)
            lu = apm.count_unique_reads(ignore_haplotype=True)
            assert np.asarray(aln).shape == tuple(case["shape"]) and np.asarray(lu).shape == (case["shape"][1],)
            case["aln"], case["uniq"], case["locus_uniq"] = record(aln), record(uniq), record(lu)
        except Exception as e:                                        # (multisample: the reference's counting raises)
            case["raises"] = type(e).__name__
        assert (case["raises"] is None) == (name in COUNTED), (name, case["raises"])
        cases.append(case)
        print(name, case["shape"], case["raises"], [list(case[k])[0] if case[k] is not None else None for k in ("aln", "uniq", "locus_uniq")])
    with open(os.path.join(HERE, "counts_cases.json"), "w") as f:          # (one case per line)
        f.write('{"golden":%s,"cases":[\n%s\n]}\n' % (json.dumps(GOLDEN), ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases)))


if __name__ == "__main__":
    main()
