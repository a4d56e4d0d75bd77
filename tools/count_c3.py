# -*- coding: utf-8 -*-
"""Input and timing of profiles/count_alignments_c3.txt: the config-3-sized ``.bin`` of ``tests/gt_checker.py:write_c3_files`` (3.7 M ECs,
13 M non-zeros, 80 000 loci, 8 haplotypes, seed 3).

    python tools/count_c3.py write DIR          the files
    python tools/count_c3.py one DIR count      ecb_count_alignments_device once on device arrays (for a kernel trace of its own)
    python tools/count_c3.py one DIR transpose  ecb_csr_to_hapcsc_device once on the same arrays: the yardstick, code the feature did not touch
    python tools/count_c3.py time DIR           both, warm, five calls each in one process (wall time of the call, waits included), the result
                                                checked against tests/counts_checker.py; then the skewed matrix -- every row also holds
                                                locus 0 -- and the time per non-zero of both
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def skewed(ip, ix, da):
    """The same rows, each also holding locus 0 (mask 1 where it is new)."""
    ip = ip.astype(np.int64)
    lens = np.diff(ip)
    has0 = np.zeros(len(lens), dtype=bool)
    first = ip[:-1][lens > 0]
    has0[lens > 0] = ix[first] == 0
    add = (~has0).astype(np.int64)
    ip2 = np.concatenate([[0], np.cumsum(lens + add)])
    ix2 = np.zeros(int(ip2[-1]), dtype=np.int32)
    da2 = np.ones(int(ip2[-1]), dtype=np.int32)
    row = np.repeat(np.arange(len(lens)), lens)
    dst = np.arange(len(ix)) - ip[row] + ip2[row] + add[row]
    ix2[dst], da2[dst] = ix, da
    return ip2.astype(np.int32), ix2, da2


def _load(d):
    from alntools_amd import bin_utils
    return bin_utils.ecload(os.path.join(d, "c3.bin"))


def _dev(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in arrays]


def one(d, which):
    import torch
    from alntools_amd import ecb
    m = _load(d)
    A, N = _dev((m.indptrA, m.indicesA, m.dataA)), _dev((m.indptrN, m.indicesN, m.dataN))
    torch.cuda.synchronize()
    if which == "count":
        ecb.count_alignments(*A, m.num_loci, m.num_haplotypes, *N)
    else:
        ecb.csr_to_hapcsc(*A, m.num_loci, m.num_haplotypes)
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


def timed(d):
    import counts_checker
    from alntools_amd import ecb
    m = _load(d)
    T, H = m.num_loci, m.num_haplotypes
    host = (m.indptrA, m.indicesA, m.dataA)
    Nh = (m.indptrN, m.indicesN, m.dataN)
    A, N = _dev(host), _dev(Nh)
    got = ecb.count_alignments(*A, T, H, *N)
    exp = counts_checker.count(*host, T, H, *Nh)
    print("equals tests/counts_checker.py:", all(np.array_equal(g.cpu().numpy(), e) for g, e in zip(got, exp)))
    ecb.csr_to_hapcsc(*A, T, H)
    fmt = lambda ts: " / ".join("%.3f" % t for t in ts)   # noqa: E731
    c = _wall(lambda: ecb.count_alignments(*A, T, H, *N))
    t = _wall(lambda: ecb.csr_to_hapcsc(*A, T, H))
    nnz = len(host[1])
    print("config 3: %d ECs, %d non-zeros, %d set bits" % (len(host[0]) - 1, nnz, int(sum(((host[2] >> h) & 1).sum() for h in range(H)))))
    print("ecb_count_alignments_device  ms: %s   (min %.3f: %.1f ps per non-zero)" % (fmt(c), min(c), min(c) * 1e9 / nnz))
    print("ecb_csr_to_hapcsc_device     ms: %s   (min %.3f)" % (fmt(t), min(t)))
    h = _wall(lambda: ecb.count_alignments(*host, T, H, *Nh), 3)
    print("ecb_count_alignments (host arrays: device buffers, copies in and out)  ms: %s" % fmt(h))
    sk = skewed(*host)
    S = _dev(sk)
    got = ecb.count_alignments(*S, T, H, *N)
    exp = counts_checker.count(*sk, T, H, *Nh)
    print("skewed equals tests/counts_checker.py:", all(np.array_equal(g.cpu().numpy(), e) for g, e in zip(got, exp)))
    s = _wall(lambda: ecb.count_alignments(*S, T, H, *N))
    print("skewed (every row also holds locus 0): %d non-zeros  ms: %s   (min %.3f: %.1f ps per non-zero)" % (len(sk[1]), fmt(s), min(s), min(s) * 1e9 / len(sk[1])))


if __name__ == "__main__":
    if sys.argv[1] == "write":
        import gt_checker
        os.makedirs(sys.argv[2], exist_ok=True)
        print(gt_checker.write_c3_files(sys.argv[2]))
    elif sys.argv[1] == "one":
        one(sys.argv[2], sys.argv[3])
    else:
        timed(sys.argv[2])
