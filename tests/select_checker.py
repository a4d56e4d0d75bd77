# -*- coding: utf-8 -*-
"""numpy restatement of ``ecselect``'s six rules, the yardstick of the GPU path (``ecb_select``).  Test infrastructure: the package has no
CPU path for the selection."""
import numpy as np

from alntools_amd import bin_utils, ecb

#: the classes by the names the package gives them, in the order of their numbers: None (every row), "unique", "locus-unique", "multi"
CLASSES = (None,) + tuple(sorted((k for k in ecb.ROW_CLASSES if k not in (None, "all")), key=ecb.ROW_CLASSES.get))


def row_counts(m):
    """Per row of A: (bits, nz) -- the set bits over all its masks, and its non-zeros whose mask is not 0."""
    E = m.num_reads
    row = np.repeat(np.arange(E), np.diff(m.indptrA.astype(np.int64)))
    d = m.dataA.astype(np.int64)
    pop = np.zeros(len(d), dtype=np.int64)
    for h in range(31):
        pop += (d >> h) & 1
    bits = np.bincount(row, weights=pop, minlength=E).astype(np.int64)
    nz = np.bincount(row, weights=(d != 0), minlength=E).astype(np.int64)
    return bits, nz


def in_class(m, row_class):
    """Rule 1: the row flags."""
    bits, nz = row_counts(m)
    number = ecb.ROW_CLASSES.get(row_class, row_class)
    return (np.ones(m.num_reads, dtype=bool), bits == 1, nz == 1, nz >= 2)[number]


def named(m, samples=None):
    """Rule 2: names -> flags over the file's samples (None: all); a name that is not in the file is a KeyError naming it."""
    if samples is None:
        return np.ones(m.num_samples, dtype=bool)
    keep = np.zeros(m.num_samples, dtype=bool)
    for n in samples:
        if n not in m.sname:
            raise KeyError(n)
        keep[m.sname.index(n)] = True
    return keep


def select_flags(m, row_class=None, keep=None, mincount=None):
    """Rules 1 and 3 - 5 on flags: ``keep`` is a bool array over the samples (None: all named).  Returns (ECMatrices, the samples that
    stayed as a bool array, the rows that stayed as a bool array)."""
    E, S = m.num_reads, m.num_samples
    cls = in_class(m, row_class)
    ptr = m.indptrN.astype(np.int64)
    col = np.repeat(np.arange(S), np.diff(ptr))
    ec, cnt = m.indicesN.astype(np.int64), m.dataN.astype(np.int64)
    stay = np.ones(S, dtype=bool) if keep is None else np.asarray(keep, dtype=bool).copy()
    if mincount is not None:
        total = np.zeros(S, dtype=np.int64)
        np.add.at(total, col[cls[ec]], cnt[cls[ec]])
        stay &= total >= max(int(mincount), 1)
    ekeep = cls[ec] & stay[col] & (cnt > 0)
    rows = np.zeros(E, dtype=bool)
    rows[ec[ekeep]] = True
    newrow = np.cumsum(rows) - 1
    ipn = np.concatenate([[0], np.cumsum(np.bincount(col[ekeep], minlength=S)[stay])]) if S else np.zeros(1, dtype=np.int64)
    pa = m.indptrA.astype(np.int64)
    lens = np.diff(pa)
    nzkeep = np.repeat(rows, lens)
    ipa = np.concatenate([[0], np.cumsum(lens[rows])])
    out = bin_utils.ECMatrices(m.hname, m.lname, m.lengths, [s for s, k in zip(m.sname, stay) if k], ipa, m.indicesA[nzkeep], m.dataA[nzkeep],
                               ipn, newrow[ec[ekeep]], cnt[ekeep])
    return out, stay, rows


def select(m, row_class=None, samples=None, mincount=None):
    """The six rules on names: the selected ``ECMatrices`` (rule 6: targets, lengths and haplotypes copied, the samples the kept ones)."""
    return select_flags(m, row_class, None if samples is None else named(m, samples), mincount)[0]


def select_bytes(m, row_class=None, samples=None, mincount=None):
    return bin_utils.ecsave2_bytes(select(m, row_class, samples, mincount))
