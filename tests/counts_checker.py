# -*- coding: utf-8 -*-
"""numpy restatement of count-alignments (the reference's ``AlignmentPropertyMatrix.count_alignments`` and ``count_unique_reads``,
``AlignmentPropertyMatrix.py:429-448``, on CSR A and CSC N), the yardstick of the GPU kernels (``ecb_count_alignments``) at shapes the
reference is too slow for, and of the multisample weights the reference leaves undefined.  Test infrastructure: the package has no CPU
path for it.  It equals the reference's three arrays on every case of ``tests/golden/counts_cases.json`` (``test_count_alignments.py``)."""
import numpy as np


def weights(n_ecs, indptr_n, indices_n, data_n, sample=None):
    """w[e]: the sum of row e of N over all samples, or its entries in column ``sample``; an EC listed twice has its counts added."""
    indptr_n = np.asarray(indptr_n, dtype=np.int64)
    lo, hi = (0, int(indptr_n[-1])) if sample is None else (int(indptr_n[sample]), int(indptr_n[sample + 1]))
    w = np.zeros(n_ecs, dtype=np.int64)
    np.add.at(w, np.asarray(indices_n, dtype=np.int64)[lo:hi], np.asarray(data_n, dtype=np.int64)[lo:hi])
    return w


def _sum_at(idx, w, n):
    """Exact int64 sum of w per index (np.bincount adds in float64: exact while every sum stays below 2^53, which is checked)."""
    assert float(np.sum(w, dtype=np.float64)) < 2.0 ** 53
    return np.bincount(idx, weights=w.astype(np.float64), minlength=n).astype(np.int64)


def count(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, sample=None):
    """(aln[H, T], uniq[H, T], locus_uniq[T]), int64."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    data = np.asarray(data, dtype=np.int64)
    E = len(indptr) - 1
    w = weights(E, indptr_n, indices_n, data_n, sample)
    row = np.repeat(np.arange(E), np.diff(indptr))
    pop = np.zeros(len(data), dtype=np.int64)
    for h in range(n_haps):
        pop += (data >> h) & 1
    row_pop = np.bincount(row, weights=pop, minlength=E).astype(np.int64)
    row_nz = np.bincount(row, weights=(data != 0), minlength=E).astype(np.int64)
    wz = w[row]
    aln = np.zeros((n_haps, n_loci), dtype=np.int64)
    uniq = np.zeros((n_haps, n_loci), dtype=np.int64)
    one_bit = row_pop[row] == 1
    for h in range(n_haps):
        bit = ((data >> h) & 1) == 1
        aln[h] = _sum_at(indices[bit], wz[bit], n_loci)
        uniq[h] = _sum_at(indices[bit & one_bit], wz[bit & one_bit], n_loci)
    lone = (row_nz[row] == 1) & (data != 0)
    return aln, uniq, _sum_at(indices[lone], wz[lone], n_loci)


def golden_arrays(case):
    """The three dense arrays of one counted case of counts_cases.json."""
    H, T = case["shape"]
    out = []
    for key, shape in (("aln", (H, T)), ("uniq", (H, T)), ("locus_uniq", (T,))):
        a = np.zeros(int(np.prod(shape)), dtype=np.int64)
        if "dense" in case[key]:
            a[:] = case[key]["dense"]
        for i, v in case[key].get("pairs", ()):
            a[i] = v
        out.append(a.reshape(shape))
    return out
