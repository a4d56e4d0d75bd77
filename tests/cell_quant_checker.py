# -*- coding: utf-8 -*-
"""numpy restatement of ecquant per cell (``include/ecb_quant_cells.h``): every cell of a multisample N as a problem of its own -- its rows
(the entries of its column with a count > 0, an EC listed twice being two rows), its support, W, B and L -- handed to ``quant_checker`` as a
:class:`quant_checker.Problem` over the cell's own rows.  Test infrastructure: the package has no CPU path for it.
``test_ecquant_cells.py`` pins it to the step pairs recorded from the reference (``quant_ms_s0.npz``, ``quant_cells_cases.json``)."""
import numpy as np

import quant_checker as qchk


class Cell(object):
    """Cell ``c``: ``rows`` (the indices into N of its entries with a count > 0), ``p`` (the :class:`quant_checker.Problem` of those rows: row k
    has the pattern of row ``e_k`` of A and the weight ``n_k``), ``support`` (ascending loci with a mask other than 0 in some row)."""

    def __init__(self, indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, c):
        indptr, indices, data = (np.asarray(a, dtype=np.int64) for a in (indptr, indices, data))
        indptr_n, indices_n, data_n = (np.asarray(a, dtype=np.int64) for a in (indptr_n, indices_n, data_n))
        j = np.arange(indptr_n[c], indptr_n[c + 1])
        self.c, self.rows = c, j[data_n[j] > 0]
        e = indices_n[self.rows]
        lens = indptr[e + 1] - indptr[e]
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        src = np.repeat(indptr[e] - rp[:-1], lens) + np.arange(rp[-1]) if len(e) else np.zeros(0, dtype=np.int64)
        R = len(e)
        self.p = qchk.Problem(rp, indices[src], data[src], n_loci, n_haps, [0, R], np.arange(R), data_n[self.rows])
        self.support = np.unique(indices[src][data[src] != 0]).astype(np.int64)
        self.row_len = lens
        #: the column lengths of the cell, per slot: the rows that hold a non-zero (mask other than 0) at the slot's locus
        self.col_len = np.bincount(indices[src][data[src] != 0], minlength=n_loci)[self.support]

    @property
    def W(self):
        return self.p.W

    def empty(self):
        return len(self.support) == 0

    def tolerance(self):
        return self.p.tolerance()

    def gather(self, dense):
        """A dense H x T table at the cell's slots: [n_slots, H]."""
        return np.ascontiguousarray(np.asarray(dense)[:, self.support].T)

    def scatter(self, slots):
        """[n_slots, H] -> H x T, 0 outside the support."""
        out = np.zeros((self.p.H, self.p.T))
        out[:, self.support] = np.asarray(slots).T
        return out

    def step(self, theta, scale=None):
        """(theta' H x T, explained) of one step from the dense ``theta``, which is read at the support alone."""
        t = np.zeros((self.p.H, self.p.T))
        t[:, self.support] = np.asarray(theta, dtype=np.float64)[:, self.support]
        return qchk.step(self.p, t, scale)

    def run(self, scale=None, theta_in=None, max_iters=1000, tol=1e-6):
        """(theta H x T, info) as ``quantify_cells`` reports the cell: a cell without a support, and every cell when no step is asked for, is
        converged."""
        if self.empty():
            return np.zeros((self.p.H, self.p.T)), {"n_iter": 0, "delta": 0.0, "explained": 0, "converged": True}
        if theta_in is not None:
            t = np.zeros((self.p.H, self.p.T))
            t[:, self.support] = np.asarray(theta_in, dtype=np.float64)[:, self.support]
            theta_in = t
        theta, info = qchk.run(self.p, scale, theta_in, max_iters, tol)
        if max_iters == 0:
            info["converged"] = True
        return theta, info


def cells(m, keep=None):
    """Every cell of an :class:`ECMatrices` (``keep``: None or per-cell flags; a cell that is not kept comes back as None)."""
    S = len(m.indptrN) - 1
    return [Cell(m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN, c)
            if keep is None or keep[c] else None for c in range(S)]


def expected_support(cs):
    """(cell_ptr int64 [S + 1], slot_locus int32) of a list of cells (None = not kept)."""
    n = [0 if c is None else len(c.support) for c in cs]
    ptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    loc = np.concatenate([c.support for c in cs if c is not None] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    return ptr, loc


def quantify_cells(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, cell_keep=None, scale=None, theta_in=None, max_iters=1000,
                   tol=1e-6, budget_bytes=0, device=0):
    """What ``ecb.quantify_cells`` returns for numpy arrays, from the checker: ``(cell_ptr, slot_locus, theta[n_slots, H], info)``."""
    S = len(indptr_n) - 1
    cs = [Cell(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, c) if cell_keep is None or cell_keep[c] else None for c in range(S)]
    ptr, loc = expected_support(cs)
    theta = np.zeros((len(loc), n_haps))
    info = {"n_iter": np.zeros(S, dtype=np.uint32), "delta": np.zeros(S), "explained": np.zeros(S, dtype=np.int64), "converged": np.ones(S, dtype=bool)}
    for c, cell in enumerate(cs):
        if cell is None:
            continue
        t, i = cell.run(scale, theta_in, max_iters, tol)
        theta[ptr[c]:ptr[c + 1]] = cell.gather(t)
        for k in info:
            info[k][c] = i[k]
    return ptr, loc, theta, info
