# -*- coding: utf-8 -*-
"""numpy / scipy restatement of ecclusters (``include/ecb_components.h``): the connected components of the target-EC incidence of CSR A
weighted by CSC N, by ``scipy.sparse.csgraph.connected_components``.  Nothing here is taken from the library.  Test infrastructure: the
package has no CPU path for it.  ``tests/test_ecclusters.py`` holds it to a pure-Python union-find."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import counts_checker


def components(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, sample=None, min_count=1):
    """``(comp_of_locus int32 [T], comp_of_ec int32 [E], comp_loci int32 [C], comp_ecs int32 [C], comp_reads int64 [C], sizes)`` with
    ``sizes = (C, linking rows, loci of the largest component, components of two loci or more)``."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    data = np.asarray(data, dtype=np.int64)
    E, T = len(indptr) - 1, int(n_loci)
    w = counts_checker.weights(E, indptr_n, indices_n, data_n, sample)
    row = np.repeat(np.arange(E), np.diff(indptr))
    member = data != 0                                                  # a mask of 0 is no alignment
    n_members = np.bincount(row[member], minlength=E)
    links = (w >= min_count) & (n_members > 0)
    # the members of the linking rows, in storage order; each joined with the one after it in its row: a chain of edges per row
    use = member & links[row]
    r, t = row[use], indices[use]
    same = r[1:] == r[:-1]
    a, b = t[:-1][same], t[1:][same]
    graph = coo_matrix((np.ones(len(a), dtype=np.int8), (a, b)), shape=(T, T))
    _, label = connected_components(graph, directed=False)
    # renumbered by smallest member: the component of a locus = the number of components whose smallest locus lies at or below its own, less one
    smallest = np.full(label.max() + 1, T, dtype=np.int64)
    np.minimum.at(smallest, label, np.arange(T))
    rank = np.empty(len(smallest), dtype=np.int64)
    rank[np.argsort(smallest)] = np.arange(len(smallest))
    of_locus = rank[label]
    C = len(smallest)
    first = np.full(E, -1, dtype=np.int64)                              # a linking row's first member
    first[r[::-1]] = t[::-1]
    of_ec = np.where(links, of_locus[np.maximum(first, 0)], -1)
    loci = np.bincount(of_locus, minlength=C)
    ecs = np.bincount(of_ec[links], minlength=C)
    reads = np.zeros(C, dtype=np.int64)
    np.add.at(reads, of_ec[links], w[links])
    sizes = (C, int(links.sum()), int(loci.max()), int((loci >= 2).sum()))
    return of_locus.astype(np.int32), of_ec.astype(np.int32), loci.astype(np.int32), ecs.astype(np.int32), reads, sizes
