#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Generate the ecbundle fixtures (``bundle_*``) in this directory by RUNNING THE REFERENCE.

Build-container only, like ``make_golden_counts.py``: imports the unmodified reference package from ``/root/reference`` with the
stand-ins of ``_standins/`` ahead of it, loads each ``.bin`` with its ``ecload``, reads the group file with its ``load_groups`` and
calls ``bundle(reset=True)`` on the result, and records data only:

  bundle_c1_mixed.grp.txt   a group file for g2_c1.bin with a transcript in two groups, transcripts in none, a transcript repeated on
                            one line and a group whose line has no transcript (written here, by hand-made rules)
  bundle_cases.json         every case: the .bin, the group file, the shape (G, H, E) of what the reference returned and the .npz that
                            holds it, or the name of the exception the reference raised instead
  bundle_<case>.npz         per haplotype h the CSC of the reference's E x G matrix: ``indptr`` (H x (G + 1)) and ``indices`` (the
                            haplotypes' row indices one after the other, ascending within a column; ``start`` (H + 1) cuts them);
                            every stored value is 1 after reset, which the script asserts instead of recording

    python tests/golden/make_golden_bundle.py
"""
from __future__ import print_function

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.join(HERE, "_standins"))

import numpy as np  # noqa: E402

from alntools import bin_utils  # noqa: E402  (the reference)

CASES = [("c1", "g2_c1.bin", "gt_c1.grp.txt"), ("h8", "gt_h8_in.bin", "gt_h8.grp.txt"), ("ms", "g4b_multi_min0.bin", "gt_ms.grp.txt"),
         ("c1_mixed", "g2_c1.bin", "bundle_c1_mixed.grp.txt"), ("err_tx", "g2_c1.bin", "gt_err_tx.grp.txt")]


def write_mixed(path, lname):
    """60 genes over the first 300 targets of g2_c1.bin, 5 each; every third gene also lists the first transcript of the gene before it
    (a transcript in two groups), every fourth lists its own first transcript twice, gene 17's line has no transcript (its five are then
    in no group), and targets 300 and up are in no group either."""
    with open(path, "w") as f:
        for g in range(60):
            tx = [lname[5 * g + k] for k in range(5)]
            if g % 3 == 2:
                tx.append(lname[5 * (g - 1)])
            if g % 4 == 1:
                tx.insert(2, tx[0])
            if g == 17:
                tx = []
            f.write("\t".join(["M%05d" % g] + tx) + "\n")


def main():
    cases = []
    for name, ec, grp in CASES:
        apm = bin_utils.ecload(os.path.join(HERE, ec))
        if name == "c1_mixed":
            write_mixed(os.path.join(HERE, grp), list(apm.lname))
        case = {"name": name, "ec": ec, "grp": grp, "shape": None, "npz": None, "raises": None}
        try:
            apm.load_groups(os.path.join(HERE, grp))
            out = apm.bundle(reset=True)
            G, H, E = (int(x) for x in out.shape)
            assert G == len(apm.gname) and H == apm.num_haplotypes and E == apm.num_reads
            ptr, idx = [], []
            for h in range(H):
                m = out.data[h].tocsc()
                m.sum_duplicates()
                m.sort_indices()
                assert m.shape == (E, G) and np.all(m.data == 1)
                ptr.append(m.indptr.astype(np.int32))
                idx.append(m.indices.astype(np.int32))
            start = np.cumsum([0] + [len(x) for x in idx]).astype(np.int64)
            case["shape"], case["npz"] = [G, H, E], "bundle_%s.npz" % name
            np.savez_compressed(os.path.join(HERE, case["npz"]), indptr=np.array(ptr), indices=np.concatenate(idx), start=start)
        except Exception as e:
            case["raises"] = type(e).__name__
        cases.append(case)
        print(name, case["shape"], case["raises"])
    with open(os.path.join(HERE, "bundle_cases.json"), "w") as f:          # (one case per line)
        f.write('{"cases":[\n%s\n]}\n' % ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases))


if __name__ == "__main__":
    main()
