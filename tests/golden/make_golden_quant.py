#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Generate the ecquant fixtures (``quant_*``) in this directory by RUNNING THE REFERENCE.

Build-container only, like ``make_golden_select.py``: imports the unmodified reference package from ``/root/reference`` with the
stand-ins of ``_standins/`` ahead of it, loads each ``.bin`` with its ``ecload`` and applies the EM step with the reference's own calls --
``reset(); multiply(phi, axis=2); normalize_reads(axis=READ); sum(axis=READ)`` on a copy whose ``count`` is the dense weight vector w (of a
multisample file: its rows summed over all samples, or one column), the 0/0 entries that ``normalize_reads`` leaves read as 0 -- starting
from ``theta_0 = sum(axis=READ)`` of the reset matrix, and records data only:

  quant_cases.json     every case: the .bin, the sample (null = pooled), whether scale = 1 / length, the shape (T, H, E), the steps k that
                       were recorded, B (the most set bits in a row), L (the longest per-haplotype column) and the .npz
  quant_<case>.npz     ``w`` (E, int64) and per recorded k the pair ``theta_<k>`` / ``next_<k>`` (H x T float64): theta_k and the step's
                       result theta_{k+1}; ``scale`` (H x T) when the case has one.  k = 0 is recorded in every case, so ``theta_0`` -- the reference's
                       ``sum(axis=READ)`` of the reset matrix -- is in every file: it pins the checker's and the device's aln to the reference's.

    python tests/golden/make_golden_quant.py
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

# name, .bin, sample column (None = pooled), scale = 1 / length, the steps recorded
CASES = [("c1", "g2_c1.bin", None, False, (0, 1, 5, 20)), ("ms", "g4b_multi_min0.bin", None, False, (0, 1, 5, 20)),
         ("ms_s0", "g4b_multi_min0.bin", 0, False, (0, 1, 5, 20)), ("c1_gt", "gt_c1.out.bin", None, False, (0, 1, 5, 20)),
         ("h8", "gt_h8_in.bin", None, False, (0, 5)), ("c1_len", "g2_c1.bin", None, True, (0, 1, 5, 20))]
LIMIT = 970265          # bytes: no .npz larger than the largest fixture already here


def step(apm, w, phi):
    m = apm.copy()
    m.reset()
    m.multiply(phi, axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        m.normalize_reads(axis=m.Axis.READ)
    for h in range(m.num_haplotypes):
        d = m.data[h].data
        d[~np.isfinite(d)] = 0.0                      # the reference's 0/0 (a row none of whose targets has any abundance) read as 0
    m.count = w.astype(np.float64)
    return np.asarray(m.sum(axis=m.Axis.READ), dtype=np.float64)


def main():
    cases = []
    for name, ec, sample, use_len, ks in CASES:
        apm = bin_utils.ecload(os.path.join(HERE, ec))
        T, H, E = (int(x) for x in apm.shape)
        if type(apm.count) == csc_matrix:
            c = apm.count.tocsc()
            w = np.asarray(c.sum(axis=1)).ravel() if sample is None else np.asarray(c[:, sample].todense()).ravel()
        else:
            assert sample is None
            w = np.asarray(apm.count).ravel()
        assert w.shape == (E,) and np.all(w == np.round(w)) and np.all(w >= 0)
        w = w.astype(np.int64)
        base = apm.copy()
        base.reset()
        base.count = w.astype(np.float64)
        theta = np.asarray(base.sum(axis=base.Axis.READ), dtype=np.float64)              # theta_0 = aln
        assert theta.shape == (H, T)
        arrays = {"w": w}
        scale = None
        if use_len:
            lens = np.asarray(apm.lengths, dtype=np.float64).T[:H]
            assert lens.shape == (H, T) and np.all(lens[theta > 0] > 0)
            scale = np.zeros((H, T))
            np.divide(1.0, lens, out=scale, where=lens > 0)
            arrays["scale"] = scale
        bits = np.zeros(E, dtype=np.int64)
        L = 0
        for h in range(H):
            d = base.data[h].tocsc()
            d.eliminate_zeros()
            bits += np.bincount(d.indices, minlength=E)
            L = max(L, int(np.diff(d.indptr).max()))
        for k in range(max(ks) + 1):
            nxt = step(apm, w, theta if scale is None else theta * scale)
            if k in ks:
                arrays["theta_%d" % k], arrays["next_%d" % k] = theta, nxt
                for a in (theta, nxt):
                    assert np.all(np.isfinite(a)) and np.all(a >= 0) and np.all(a[a > 0] > 1e-200)
            theta = nxt
        case = {"name": name, "ec": ec, "sample": sample, "use_lengths": use_len, "shape": [T, H, E], "steps": list(ks), "B": int(bits.max()), "L": L,
                "npz": "quant_%s.npz" % name}
        path = os.path.join(HERE, case["npz"])
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) <= LIMIT, (name, os.path.getsize(path))
        cases.append(case)
        print(name, case["shape"], "B", case["B"], "L", L, os.path.getsize(path), "bytes")
    with open(os.path.join(HERE, "quant_cases.json"), "w") as f:          # (one case per line)
        f.write('{"cases":[\n%s\n]}\n' % ",\n".join(json.dumps(c, separators=(",", ":"), sort_keys=True) for c in cases))


if __name__ == "__main__":
    main()
