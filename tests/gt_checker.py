# -*- coding: utf-8 -*-
"""numpy restatement of apply-genotypes' masking (the reference's ``APM.apply_genotypes`` + ``ecsave2`` on CSR A), the yardstick of
the GPU kernel (``ecb_apply_mask``).  Test infrastructure: the package has no CPU path for it."""
import numpy as np


def mask_csr(indptr, indices, data, mask):
    """A' = A & mask[locus], zeros dropped, every row kept."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    v = np.asarray(data, dtype=np.int64) & np.asarray(mask, dtype=np.int64)[indices]
    keep = v != 0
    csum = np.concatenate([[0], np.cumsum(keep)])
    return csum[indptr].astype(np.int32), indices[keep].astype(np.int32), v[keep].astype(np.int32)


def random_csr(rng, n_ecs, n_loci, n_haps, max_row=900, long_share=0.05):
    """Rows of 0 - 10 loci, a share of them up to ``max_row``; columns strictly ascending; masks non-zero below 2^H."""
    n_long = rng.random(n_ecs) < long_share
    lens = np.where(n_long, rng.integers(0, min(max_row, n_loci) + 1, n_ecs), rng.integers(0, min(10, n_loci) + 1, n_ecs))
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.empty(int(indptr[-1]), dtype=np.int32)
    for e in np.flatnonzero(lens):
        indices[indptr[e]:indptr[e + 1]] = np.sort(rng.choice(n_loci, size=int(lens[e]), replace=False))
    data = rng.integers(1, 1 << n_haps, size=len(indices), dtype=np.int64).astype(np.int32)
    return indptr, indices, data


def c3_csr(seed=3, n_ecs=3_700_000, n_loci=80_000, n_haps=8):
    """A config-3-sized CSR A (about 3.7 M ECs, 12 M non-zeros, 80 k loci, 8 haplotypes), built without a per-row loop: row lengths
    0 - 9 (mean 3.2), a few rows of 100 - 900 loci; columns by positive gaps, so strictly ascending; masks 1 .. 2^H - 1."""
    rng = np.random.default_rng(seed)
    lens = rng.choice(np.arange(10), size=n_ecs, p=[.01, .14, .2, .2, .17, .12, .08, .05, .02, .01])
    long_rows = rng.choice(n_ecs, size=200, replace=False)
    lens[long_rows] = rng.integers(100, 901, size=200)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(indptr[-1])
    row = np.repeat(np.arange(n_ecs), lens)
    gap = rng.integers(1, 60, size=nnz).astype(np.int64)
    gap[indptr[:-1][lens > 0]] = rng.integers(0, n_loci // 2, size=int((lens > 0).sum()))
    col = np.cumsum(gap)
    col -= np.repeat(col[indptr[:-1]] - gap[indptr[:-1]], lens)       # (each row's running sum restarts at its first gap)
    col %= n_loci
    # (a row whose sum wrapped past n_loci is re-sorted: a long row may then be out of order -- those rows are laid out again, sorted)
    bad = np.flatnonzero(np.diff(col) <= 0)
    bad = bad[row[bad] == row[bad + 1]]
    for e in np.unique(row[bad]):
        a, b = indptr[e], indptr[e + 1]
        col[a:b] = np.sort(rng.choice(n_loci, size=b - a, replace=False))
    data = rng.integers(1, 1 << n_haps, size=nnz)
    return indptr.astype(np.int32), col.astype(np.int32), data.astype(np.int32), n_loci, n_haps


def write_c3_files(d, seed=3):
    """The config-3-sized .bin and genotype / group files of the profile run (1 - 6 transcripts per gene, 5 % of the transcripts in no
    gene, 10 % of the genes not genotyped, half het and half hom)."""
    import os
    from alntools_amd import bin_utils
    indptr, indices, data, T, H = c3_csr(seed)
    rng = np.random.default_rng(seed + 1)
    E = len(indptr) - 1
    lname = ["ENSMUST%011d" % t for t in range(T)]
    hname = list("ABCDEFGH")[:H]
    m = bin_utils.ECMatrices(hname, lname, rng.integers(200, 5000, size=(T, H)), ["c3"], indptr, indices, data,
                             np.array([0, E], dtype=np.int32), np.arange(E, dtype=np.int32), rng.integers(1, 100, size=E).astype(np.int32))
    paths = [os.path.join(d, n) for n in ("c3.bin", "c3.gt.txt", "c3.grp.txt")]
    bin_utils.ecsave2(paths[0], m)
    with open(paths[2], "w") as grp, open(paths[1], "w") as gt:
        gt.write("#gene\tgenotype\n")
        t, g = 0, 0
        while t < T:
            k = int(rng.integers(1, 7))
            txs = [x for x in lname[t:t + k] if rng.random() >= 0.05]
            name = "ENSMUSG%011d" % g
            grp.write("\t".join([name] + txs) + "\n")
            if txs and rng.random() >= 0.1:
                a, b = rng.choice(hname, size=2)
                gt.write("{}\t{}\n".format(name, a + (b if rng.random() < 0.5 else a)))
            t, g = t + k, g + 1
    return paths
