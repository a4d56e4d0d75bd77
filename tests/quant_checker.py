# -*- coding: utf-8 -*-
"""numpy restatement of ecquant (``include/ecb_quant.h``): one EM step -- the reference's ``reset(); multiply(phi, axis=2);
normalize_reads(axis=READ); sum(axis=READ)`` with ``count = w`` (``AlignmentPropertyMatrix.py:277-384``), its 0/0 read as 0 -- and the run
that applies steps until ``delta <= tol * W`` or ``max_iters``.  float64 throughout, row-wise: the yardstick of the GPU kernels where the
reference is absent.  Test infrastructure: the package has no CPU path for it.  ``test_ecquant.py`` pins it to the step pairs recorded from
the reference (``tests/golden/quant_cases.json``)."""
import numpy as np

import counts_checker


class Problem(object):
    """What a step needs of an :class:`ECMatrices` (or of bare arrays), worked out once: the non-zeros expanded to one entry per set bit."""

    def __init__(self, indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, sample=None):
        indptr = np.asarray(indptr, dtype=np.int64)
        indices = np.asarray(indices, dtype=np.int64)
        data = np.asarray(data, dtype=np.int64)
        self.E, self.T, self.H, self.nnz = len(indptr) - 1, n_loci, n_haps, len(data)
        self.w = counts_checker.weights(self.E, indptr_n, indices_n, data_n, sample)
        row = np.repeat(np.arange(self.E), np.diff(indptr))
        rows, flat = [], []
        for h in range(n_haps):
            bit = ((data >> h) & 1) == 1
            rows.append(row[bit])
            flat.append(h * n_loci + indices[bit])
        self.bit_row = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)      # the row of every set bit ...
        self.bit_flat = np.concatenate(flat) if flat else np.zeros(0, dtype=np.int64)     # ... and its place h T + t in theta
        self.has_bit = np.bincount(self.bit_row, minlength=self.E) > 0
        self.W = int(self.w[self.has_bit].sum())
        #: B = the most set bits in a row, L = the longest per-haplotype column: the lengths of the two sums of a step
        self.B = int(np.bincount(self.bit_row, minlength=max(self.E, 1)).max()) if self.E else 0
        self.L = int(np.bincount(self.bit_flat, minlength=n_haps * n_loci).max())

    @classmethod
    def of(cls, m, sample=None):
        return cls(m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN, sample)

    def aln(self):
        """theta_0 when none is given: the alignment counts (exact integers)."""
        return np.bincount(self.bit_flat, weights=self.w[self.bit_row].astype(np.float64), minlength=self.H * self.T).reshape(self.H, self.T)

    def tolerance(self):
        """The relative bound of one step, entry by entry: (B + L + 4) 2^-52."""
        return (self.B + self.L + 4) * 2.0 ** -52


def step(p, theta, scale=None):
    """(theta', explained) of one step."""
    phi = np.asarray(theta, dtype=np.float64).reshape(-1)
    if scale is not None:
        phi = phi * np.asarray(scale, dtype=np.float64).reshape(-1)
    d = np.bincount(p.bit_row, weights=phi[p.bit_flat], minlength=p.E) if p.E else np.zeros(0)
    r = np.zeros(p.E)
    np.divide(p.w.astype(np.float64), d, out=r, where=d > 0)
    acc = np.bincount(p.bit_flat, weights=r[p.bit_row], minlength=p.H * p.T)
    return (phi * acc).reshape(p.H, p.T), int(p.w[d > 0].sum())


def delta(new, old):
    """The change of one step: the sum over (h, t) of |new - old| (math.fsum: the exact sum, rounded once)."""
    import math
    return math.fsum(np.abs(np.asarray(new) - np.asarray(old)).reshape(-1).tolist())


def run(p, scale=None, theta_in=None, max_iters=1000, tol=1e-6):
    """(theta, info) as ``ecb.quantify`` returns them."""
    theta = p.aln() if theta_in is None else np.array(theta_in, dtype=np.float64).reshape(p.H, p.T)
    info = {"n_iter": 0, "delta": 0.0, "explained": 0, "converged": False}
    if p.E == 0 or p.nnz == 0:                      # the empty inputs: theta = 0, no step, converged
        info["converged"] = True
        return np.zeros((p.H, p.T)), info
    stop = tol * float(p.W)
    while info["n_iter"] < max_iters:
        new, info["explained"] = step(p, theta, scale)
        info["delta"] = delta(new, theta)
        theta = new
        info["n_iter"] += 1
        if info["delta"] <= stop:
            info["converged"] = True
            break
    return theta, info


def agree(got, ref, bound):
    """Entry by entry |got - ref| <= bound * ref, and exactly the same entries 0.  Returns the worst relative difference."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    assert np.array_equal(got == 0, ref == 0), "different entries are 0"
    nz = ref != 0
    rel = np.abs(got[nz] - ref[nz]) / ref[nz]
    worst = float(rel.max()) if rel.size else 0.0
    assert worst <= bound, (worst, bound)
    return worst
