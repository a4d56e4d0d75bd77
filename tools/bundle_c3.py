# -*- coding: utf-8 -*-
"""Input and timing of profiles/bundle_c3.txt: the config-3-sized matrix of ``tests/gt_checker.py:c3_csr`` (3.7 M ECs, 12 M non-zeros,
80 000 loci, 8 haplotypes, seed 3) bundled by a synthetic grouping of 1 - 6 consecutive isoforms per gene, 5 % of the transcripts in no gene.

    python tools/bundle_c3.py one bundle     ecb_bundle_device once on device arrays (for a kernel trace of its own)
    python tools/bundle_c3.py one gene       the same with every transcript in ONE gene: every row is one run of equal (row, group) keys
    python tools/bundle_c3.py one combine    ecb_combine_device of the same matrix as one part with a one-to-one permuting target map: the
                                             yardstick -- it sorts the same number of pairs and shares every later step (with ECB_LIB
                                             naming a build of the commit before, code this feature did not touch)
    python tools/bundle_c3.py time           all three, warm, wall time of the call (waits included), the ordinary bundle three times over
                                             for the run-to-run spread; the small cases checked against tests/bundle_checker.py first
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def grouping(T, seed=4):
    """(n_groups, map_ptr, map_idx): genes of 1 - 6 consecutive transcripts, 5 % of the transcripts in no gene."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 7, size=T)
    ends = np.cumsum(sizes)
    G = int(np.searchsorted(ends, T, side="left")) + 1
    gene = np.searchsorted(ends, np.arange(T), side="right")
    member = rng.random(T) >= 0.05
    ptr = np.concatenate([[0], np.cumsum(member)]).astype(np.int32)
    return G, ptr, gene[member].astype(np.int32)


def one_gene(T):
    return 1, np.arange(T + 1, dtype=np.int32), np.zeros(T, dtype=np.int32)


def _dev(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in arrays]


def _inputs():
    import gt_checker
    ip, ix, da, T, H = gt_checker.c3_csr(3)
    E = len(ip) - 1
    rng = np.random.default_rng(5)
    N = (np.array([0, E], dtype=np.int32), np.arange(E, dtype=np.int32), rng.integers(1, 100, size=E).astype(np.int32))
    return (ip, ix, da), N, T, H


def _calls():
    import torch
    from alntools_amd import ecb
    host, Nh, T, H = _inputs()
    A, N = _dev(host), _dev(Nh)
    calls = {}
    for name, (G, ptr, idx) in (("bundle", grouping(T)), ("gene", one_gene(T))):
        if hasattr(ecb.load(), "ecb_bundle_device"):
            mp, mi = _dev((ptr, idx))
            calls[name] = (lambda G=G, mp=mp, mi=mi: ecb.bundle(*A, *N, T, H, G, mp, mi), int(np.diff(ptr)[host[1]].sum()))
    perm = np.random.default_rng(6).permutation(T)
    part = dict(indptrA=A[0], indicesA=A[1], dataA=A[2], indptrN=N[0], indicesN=N[1], dataN=N[2], n_loci=T, target_map=perm, sample_map=np.array([0]))
    calls["combine"] = (lambda: ecb.combine([part], T, H, 1), len(host[1]))
    torch.cuda.synchronize()
    return calls, len(host[0]) - 1, len(host[1])


def _wall(f, n):
    import torch
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out, r


def check_small():
    import bundle_checker
    import ec_merge_checker
    from alntools_amd import bin_utils, ecb
    rng = np.random.default_rng(7)
    m = ec_merge_checker.random_bin(rng, 2000, ["t%d" % t for t in range(500)], list("ABCDEFGH"), ["s"], max_row=400)
    ok = True
    for G, ptr, idx in (grouping(500), one_gene(500)):
        groups = [[] for _ in range(G)]
        for t in range(500):
            for g in idx[ptr[t]:ptr[t + 1]]:
                groups[g].append(t)
        names = ["g%d" % g for g in range(G)]
        out = ecb.bundle(m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN, 500, 8, G, ptr, idx)
        got = bin_utils.ECMatrices(m.hname, names, bundle_checker.group_lengths(m, groups), m.sname, *out)
        ok &= bin_utils.ecsave2_bytes(got) == bundle_checker.bundle_bytes(m, names, groups)
    print("small cases equal tests/bundle_checker.py:", ok)


def timed():
    check_small()
    calls, E, nnz = _calls()
    print("config 3: %d ECs, %d non-zeros" % (E, nnz))
    fmt = lambda ts: " / ".join("%.2f" % t for t in ts)   # noqa: E731
    for f, _ in calls.values():
        f()
    for rep in range(3):
        ts, r = _wall(calls["bundle"][0], 3)
        X = calls["bundle"][1]
        print("ecb_bundle_device, 1 - 6 isoforms per gene, run %d  ms: %s   (min %.2f: %.2f ns per expanded pair; %d pairs -> %d ECs, %d non-zeros)"
              % (rep + 1, fmt(ts), min(ts), min(ts) * 1e6 / X, X, len(r[0]) - 1, len(r[1])))
    ts, r = _wall(calls["gene"][0], 3)
    X = calls["gene"][1]
    print("ecb_bundle_device, every transcript in one gene  ms: %s   (min %.2f: %.2f ns per expanded pair; %d pairs -> %d ECs, %d non-zeros)"
          % (fmt(ts), min(ts), min(ts) * 1e6 / X, X, len(r[0]) - 1, len(r[1])))
    ts, r = _wall(calls["combine"][0], 3)
    print("ecb_combine_device, one part, permuting target map  ms: %s   (min %.2f; %d pairs -> %d ECs)" % (fmt(ts), min(ts), nnz, len(r[0]) - 1))


if __name__ == "__main__":
    if sys.argv[1] == "one":
        _calls()[0][sys.argv[2]][0]()
        import torch
        torch.cuda.synchronize()
    else:
        timed()
