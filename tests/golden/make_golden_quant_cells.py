#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Generate the per-cell ecquant fixtures (``quant_cells*``) in this directory by RUNNING THE REFERENCE.

Build-container only, like ``make_golden_quant.py``, whose ``step`` this applies: imports the unmodified reference package from
``/root/reference`` with the stand-ins of ``_standins/`` ahead of it, loads ``g4b_multi_min0.bin`` with its ``ecload`` and, for four more of its
cells than ``quant_ms_s0`` (cell 0) covers -- the cell with the most entries, the first cell with a single entry and two drawn with a seed --
applies the EM step with ``count`` = that cell's column of N, starting from ``theta_0 = sum(axis=READ)`` of the reset matrix.  Data only:

  quant_cells_cases.json   every case: the .bin, the cell, its number of entries, the steps k that were recorded, the cell's B (the most set
                           bits in one of its rows) and L (its longest per-haplotype column), the .npz and the prefix of its arrays there
  quant_cells.npz          per case ``<prefix>w`` (E, int64: the cell's column) and per recorded k ``<prefix>theta_<k>`` / ``<prefix>next_<k>``
                           (H x T float64)

    python tests/golden/make_golden_quant_cells.py
"""
from __future__ import print_function

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_quant import LIMIT, bin_utils, step  # noqa: E402  (puts the reference and the stand-ins on the path)

import numpy as np  # noqa: E402

EC = "g4b_multi_min0.bin"
STEPS = (0, 1, 5)
SEED = 20261019


def main():
    apm = bin_utils.ecload(os.path.join(HERE, EC))
    T, H, E = (int(x) for x in apm.shape)
    N = apm.count.tocsc()
    S = N.shape[1]
    entries = np.array([int((N[:, c].data > 0).sum()) for c in range(S)])
    most, single = int(np.argmax(entries)), int(np.flatnonzero(entries == 1)[0])
    rng = np.random.RandomState(SEED)
    pool = [c for c in range(1, S) if c not in (most, single) and entries[c] > 1]
    cells = [most, single] + sorted(int(c) for c in rng.choice(pool, 2, replace=False))
    arrays, cases = {}, []
    for c in cells:
        w = np.asarray(N[:, c].todense()).ravel()
        assert w.shape == (E,) and np.all(w == np.round(w)) and np.all(w >= 0)
        w = w.astype(np.int64)
        base = apm.copy()
        base.reset()
        base.count = w.astype(np.float64)
        theta = np.asarray(base.sum(axis=base.Axis.READ), dtype=np.float64)              # theta_0 = the cell's aln
        rows = w > 0
        bits = np.zeros(E, dtype=np.int64)
        L = 0
        for h in range(H):
            d = base.data[h].tocsr()
            d.eliminate_zeros()
            bits += np.diff(d.indptr)
            L = max(L, int(np.diff(d[rows].tocsc().indptr).max()))
        pre = "c%d_" % c
        arrays[pre + "w"] = w
        for k in range(max(STEPS) + 1):
            nxt = step(apm, w, theta)
            if k in STEPS:
                arrays[pre + "theta_%d" % k], arrays[pre + "next_%d" % k] = theta, nxt
                for a in (theta, nxt):
                    assert np.all(np.isfinite(a)) and np.all(a >= 0) and np.all(a[a > 0] > 1e-200)
            theta = nxt
        cases.append({"name": "cell%d" % c, "ec": EC, "cell": c, "entries": int(entries[c]), "steps": list(STEPS), "B": int(bits[rows].max()), "L": L,
                      "npz": "quant_cells.npz", "prefix": pre})
        print(cases[-1])
    path = os.path.join(HERE, "quant_cells.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) <= LIMIT, os.path.getsize(path)
    with open(os.path.join(HERE, "quant_cells_cases.json"), "w") as f:          # (one case per line)
        f.write('{"cases":[\n%s\n]}\n' % ",\n".join(json.dumps(c, separators=(",", ":"), sort_keys=True) for c in cases))


if __name__ == "__main__":
    main()
