# -*- coding: utf-8 -*-
"""Input and timing of profiles/ecclusters_c3.txt: the config-3-sized ``.bin`` of ``tests/gt_checker.py:write_c3_files`` (3.7 M ECs,
12 M non-zeros, 80 000 loci, 8 haplotypes, seed 3) -- the file ``tools/count_c3.py`` counts.

    python tools/clusters_c3.py write DIR            the files
    python tools/clusters_c3.py one DIR components [MINCOUNT]   ecb_components_device once on device arrays (for a kernel trace of its own)
    python tools/clusters_c3.py one DIR count        ecb_count_alignments_device once on the same arrays: the yardstick -- both read A and N
                                                     once and share the checks
    python tools/clusters_c3.py time DIR [MINCOUNT]  both, warm, five calls each in one process (wall time of the call, waits included), the
                                                     result checked against tests/components_checker.py; the host entry; scipy's
                                                     connected_components on the host for the same matrix; then the same at a min_count that
                                                     breaks the giant component up
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _load(d):
    from alntools_amd import bin_utils
    return bin_utils.ecload(os.path.join(d, "c3.bin"))


def _dev(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in arrays]


def one(d, which, min_count=1):
    import torch
    from alntools_amd import ecb, ecb_components
    m = _load(d)
    A, N = _dev((m.indptrA, m.indicesA, m.dataA)), _dev((m.indptrN, m.indicesN, m.dataN))
    torch.cuda.synchronize()
    if which == "components":
        ecb_components.components(*A, m.num_loci, m.num_haplotypes, *N, min_count=min_count)
    else:
        ecb.count_alignments(*A, m.num_loci, m.num_haplotypes, *N)
    torch.cuda.synchronize()


def _wall(f, n=5):
    import torch
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def timed(d, min_counts=(1, 90)):
    import components_checker as cc
    from alntools_amd import ecb, ecb_components
    m = _load(d)
    T, H = m.num_loci, m.num_haplotypes
    host = (m.indptrA, m.indicesA, m.dataA)
    Nh = (m.indptrN, m.indicesN, m.dataN)
    A, N = _dev(host), _dev(Nh)
    fmt = lambda ts: " / ".join("%.3f" % t for t in ts)   # noqa: E731
    nnz = len(host[1])
    print("config 3: %d ECs, %d non-zeros, %d loci" % (len(host[0]) - 1, nnz, T))
    ecb.count_alignments(*A, T, H, *N)
    c = _wall(lambda: ecb.count_alignments(*A, T, H, *N))
    print("ecb_count_alignments_device  ms: %s   (min %.3f: %.1f ps per non-zero)" % (fmt(c), min(c), min(c) * 1e9 / nnz))
    for mc in min_counts:
        got = ecb_components.components(*A, T, H, *N, min_count=mc)
        t0 = time.perf_counter()
        exp = cc.components(*host, T, H, *Nh, min_count=mc)
        t1 = time.perf_counter()
        same = all(np.array_equal(g.cpu().numpy(), e) for g, e in zip(got[:5], exp[:5])) and tuple(got[5]) == tuple(exp[5])
        print("min_count %d: sizes %r; equals tests/components_checker.py: %s (the checker: %.2f s)" % (mc, got[5], same, t1 - t0))
        k = _wall(lambda: ecb_components.components(*A, T, H, *N, min_count=mc))
        print("  ecb_components_device  ms: %s   (min %.3f: %.1f ps per non-zero; %.2f x count-alignments)" % (fmt(k), min(k), min(k) * 1e9 / nnz, min(k) / min(c)))
        h = _wall(lambda: ecb_components.components(*host, T, H, *Nh, min_count=mc), 3)
        print("  ecb_components (host arrays: device buffers, copies in and out)  ms: %s" % fmt(h))
    # scipy alone, on the matrix the checker hands it at min_count 1: a chain of edges per row
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    ip, ix = host[0].astype(np.int64), host[1].astype(np.int64)
    row = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    same = row[1:] == row[:-1]
    g = coo_matrix((np.ones(int(same.sum()), dtype=np.int8), (ix[:-1][same], ix[1:][same])), shape=(T, T))
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        connected_components(g, directed=False)
        ts.append((time.perf_counter() - t0) * 1e3)
    print("scipy.sparse.csgraph.connected_components on the host, %d edges given as a COO matrix  ms: %s" % (g.nnz, fmt(ts)))


if __name__ == "__main__":
    if sys.argv[1] == "write":
        import gt_checker
        os.makedirs(sys.argv[2], exist_ok=True)
        print(gt_checker.write_c3_files(sys.argv[2]))
    elif sys.argv[1] == "one":
        one(sys.argv[2], sys.argv[3], *(int(a) for a in sys.argv[4:5]))
    else:
        timed(sys.argv[2], *([tuple(int(a) for a in sys.argv[3:])] if len(sys.argv) > 3 else []))
