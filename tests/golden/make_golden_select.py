#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Generate the ecselect fixtures (``select_*``) in this directory by RUNNING THE REFERENCE.

Build-container only, like ``make_golden_bundle.py``: imports the unmodified reference package from ``/root/reference`` with the
stand-ins of ``_standins/`` ahead of it, loads each ``.bin`` with its ``ecload`` and calls ``get_unique_reads`` on the result, with
``ignore_haplotype`` False and True, and records data only:

  select_cases.json     every case: the .bin, the shape (T, H, E) of what the reference loaded, the .npz that holds what it pulled and,
                        per ``ignore_haplotype``, the number of rows that kept an alignment
  select_<case>.npz     per pull p in ("allele", "locus"), per haplotype h the CSC of the reference's E x T matrix: ``<p>_indptr``
                        (H x (T + 1)) and ``<p>_indices`` (the haplotypes' row indices one after the other, ascending within a column;
                        ``<p>_start`` (H + 1) cuts them) -- every stored value is 1, which the script asserts instead of recording -- and
                        the count that came back: a dense vector ``<p>_count`` (E), or the CSC arrays ``<p>_count_indptr`` /
                        ``<p>_count_indices`` / ``<p>_count_data`` of an E x S matrix

    python tests/golden/make_golden_select.py
"""
from __future__ import print_function

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.join(HERE, "_standins"))

import numpy as np  # noqa: E402
from scipy.sparse import csc_matrix  # noqa: E402

from alntools import bin_utils  # noqa: E402  (the reference)

CASES = [("c1", "g2_c1.bin"), ("h8", "gt_h8_in.bin"), ("ms", "g4b_multi_min0.bin"), ("c1_gt", "gt_c1.out.bin"), ("ms_gt", "gt_ms.out.bin")]


def main():
    cases = []
    for name, ec in CASES:
        apm = bin_utils.ecload(os.path.join(HERE, ec))
        T, H, E = (int(x) for x in apm.shape)
        case = {"name": name, "ec": ec, "shape": [T, H, E], "npz": "select_%s.npz" % name, "rows": {}}
        arrays = {}
        for p, ignore in (("allele", False), ("locus", True)):
            out = apm.get_unique_reads(ignore_haplotype=ignore)
            assert tuple(int(x) for x in out.shape) == (T, H, E)
            ptr, idx, rows = [], [], np.zeros(E, dtype=bool)
            for h in range(H):
                m = out.data[h].tocsc()
                m.sum_duplicates()
                m.sort_indices()
                assert m.shape == (E, T) and np.all(m.data == 1)
                ptr.append(m.indptr.astype(np.int32))
                idx.append(m.indices.astype(np.int32))
                rows[m.indices] = True
            arrays[p + "_indptr"] = np.array(ptr)
            arrays[p + "_indices"] = np.concatenate(idx)
            arrays[p + "_start"] = np.cumsum([0] + [len(x) for x in idx]).astype(np.int64)
            case["rows"][p] = int(rows.sum())
            if type(out.count) == csc_matrix:
                c = out.count.copy()
                c.sort_indices()
                assert c.shape[0] == E
                arrays[p + "_count_indptr"], arrays[p + "_count_indices"] = c.indptr.astype(np.int32), c.indices.astype(np.int32)
                arrays[p + "_count_data"] = np.asarray(c.data).astype(np.int64)
                assert np.all(arrays[p + "_count_data"] == c.data)
            else:
                arrays[p + "_count"] = np.asarray(out.count).astype(np.int64)
                assert arrays[p + "_count"].shape == (E,) and np.all(arrays[p + "_count"] == out.count)
        np.savez_compressed(os.path.join(HERE, case["npz"]), **arrays)
        cases.append(case)
        print(name, case["shape"], case["rows"])
    with open(os.path.join(HERE, "select_cases.json"), "w") as f:          # (one case per line)
        f.write('{"cases":[\n%s\n]}\n' % ",\n".join(json.dumps(c, separators=(",", ":"), sort_keys=True) for c in cases))


if __name__ == "__main__":
    main()
