#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Generate the fixtures of ecquant's hierarchical models per cell (``quant_cell_models*``) in this directory by RUNNING THE REFERENCE.

Build-container only, like ``make_golden_quant_models.py``, whose ``Case`` this applies with ``w`` = one cell's column of N: the step of a
model is the product of the reference's own factors on the aligned entries, then its weighted sum over reads with ``count = w``.  Input:
``g4b_multi_min0.bin`` with the partition ``quant_model_ms.grp.txt`` (read, not rewritten); the cells are the five that ``quant_ms_s0`` and
``quant_cells_cases.json`` cover; every model's run starts from ``theta_0`` = the cell's aln, which is 0 outside the cell's support and
stays 0 there, so the reference's sums over a gene are sums over the support.  Data only:

  quant_cell_models_cases.json   one case per cell: the .bin, the group file, the cell, the models, the steps k, the cell's B, L, M (the most
                                 members of one gene within its support) and R (the most genes in one of its rows), the .npz and the prefix
  quant_cell_models.npz          per case ``<prefix>w`` (E, int64) and per model m and recorded k ``<prefix>m<m>_theta_<k>`` and
                                 ``<prefix>m<m>_theta_<k+1>`` (H x T float64): the pair of step k

The script asserts that in no recorded pair a row with a count above 0 holds a gene, allele or isoform with D = 0 and Phi > 0 (the share of
rows under the deviation is 0: the reference's rule and ecquant's are the same there), that every recorded value is finite and that each
file stays within LIMIT.

    python tests/golden/make_golden_quant_cell_models.py
"""
from __future__ import print_function

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_quant_models import LIMIT, MODELS, STEPS, Case, bin_utils  # noqa: E402  (puts the reference and the stand-ins on the path)

import numpy as np  # noqa: E402

EC = "g4b_multi_min0.bin"
GRP = "quant_model_ms.grp.txt"
CELLS = (0, 3, 157, 190, 219)


def genes(apm):
    """(gene[t], names, per gene its targets) of the partition in GRP: genes in file order, then the unlisted targets in target order."""
    lid = dict(zip(apm.lname, range(len(apm.lname))))
    gene = np.full(len(apm.lname), -1, dtype=np.int32)
    names = []
    with open(os.path.join(HERE, GRP)) as fh:
        for line in fh:
            item = line.rstrip().split("\t")
            assert len(item) > 1 and all(gene[lid[t]] < 0 for t in item[1:])
            gene[[lid[t] for t in item[1:]]] = len(names)
            names.append(item[0])
    for t in np.flatnonzero(gene < 0):
        gene[t] = len(names)
        names.append(apm.lname[t])
    return gene, names, [np.flatnonzero(gene == g).tolist() for g in range(len(names))]


def deviating(k, phi, rows):
    """Does any of ``rows`` hold a gene, allele or isoform with D = 0 and Phi > 0?  (``Case.deviating`` over the rows with a count alone.)"""
    phi_gh = phi.dot(k.conv)
    phi_g, phi_t = phi_gh.sum(axis=0), phi.sum(axis=0)
    row = np.concatenate([r for r, _ in k.coords])
    col = np.concatenate([c for _, c in k.coords])
    hap = np.concatenate([np.full(len(r), h) for h, (r, _) in enumerate(k.coords)])
    mine = rows[row]
    row, col, hap = row[mine].astype(np.int64), col[mine], hap[mine]
    v, g = phi[hap, col], k.gene[col]

    def lost(key, big):
        u, first, inv = np.unique(key, return_index=True, return_inverse=True)
        d = np.bincount(inv, weights=v, minlength=len(u))
        return bool(((d == 0) & (big[first] > 0)).any())
    seg = row * k.G + g
    return lost(seg, phi_g[g]) or lost(seg * k.H + hap, phi_gh[hap, g]) or lost(row * k.T + col, phi_t[col])


def main():
    apm = bin_utils.ecload(os.path.join(HERE, EC))
    T, H, E = (int(x) for x in apm.shape)
    N = apm.count.tocsc()
    gene, names, groups = genes(apm)
    assert np.array_equal(gene, np.load(os.path.join(HERE, "quant_model_ms.npz"))["gene"])
    arrays, cases = {}, []
    for c in CELLS:
        w = np.asarray(N[:, c].todense()).ravel()
        assert w.shape == (E,) and np.all(w == np.round(w)) and np.all(w >= 0)
        w = w.astype(np.int64)
        k = Case(apm, w, gene, names, groups)
        rows = w > 0
        theta0 = k.theta0()
        assert theta0.shape == (H, T)
        support = theta0.sum(axis=0) > 0
        pre = "c%d_" % c
        arrays[pre + "w"] = w
        for model in MODELS:
            theta = theta0
            for s in range(max(STEPS) + 1):
                nxt = k.step(model, theta, None)
                if s in STEPS:
                    assert not deviating(k, theta, rows), (c, model, s)
                    arrays["%sm%d_theta_%d" % (pre, model, s)], arrays["%sm%d_theta_%d" % (pre, model, s + 1)] = theta, nxt
                    for a in (theta, nxt):
                        assert np.all(np.isfinite(a)) and np.all(a >= 0) and not a[:, ~support].any()
                theta = nxt
        bits = np.zeros(E, dtype=np.int64)
        L = 0
        for h in range(H):
            d = k.base.data[h].tocsr()
            bits += np.diff(d.indptr)
            L = max(L, int(np.diff(d[rows].tocsc().indptr).max()))
        seg = np.unique(np.concatenate([r[rows[r]].astype(np.int64) * k.G + gene[cc[rows[r]]] for r, cc in k.coords]))
        cases.append({"name": "cell%d" % c, "ec": EC, "grp": GRP, "cell": c, "entries": int(rows.sum()), "steps": list(STEPS), "models": list(MODELS),
                      "B": int(bits[rows].max()), "L": L, "M": int(np.bincount(gene[support]).max()), "R": int(np.bincount(seg // k.G).max()),
                      "shape": [T, H, E], "G": k.G, "npz": "quant_cell_models.npz", "prefix": pre})
        print(cases[-1])
    path = os.path.join(HERE, "quant_cell_models.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) <= LIMIT, os.path.getsize(path)
    out = os.path.join(HERE, "quant_cell_models_cases.json")
    with open(out, "w") as f:          # (one case per line)
        f.write('{"cases":[\n%s\n]}\n' % ",\n".join(json.dumps(c, separators=(",", ":"), sort_keys=True) for c in cases))
    assert os.path.getsize(out) <= LIMIT
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
