# -*- coding: utf-8 -*-
"""Plain-Python restatement of ``ecmerge``'s contract (dicts keyed by the set of (target name, haplotype mask) pairs), the yardstick of
the GPU path (``ecb_combine``) and of ``bin_utils.plan_merge``.  Test infrastructure: the package has no CPU path for the merge."""
import numpy as np

from alntools_amd import bin_utils


def merge(ms):
    """``ECMatrices`` in input order -> the merged ``ECMatrices``.  Same haplotypes assumed (the caller's refusal)."""
    m0 = ms[0]
    H = m0.num_haplotypes
    same_targets = all(m.lname == m0.lname for m in ms)
    lname, lens, tpos = [], [], {}
    if same_targets:
        lname = list(m0.lname)
        lens = [list(r) for r in np.asarray(m0.lengths).astype(np.int64).reshape(-1, H)]
    else:
        for m in ms:
            for t, r in zip(m.lname, np.asarray(m.lengths).astype(np.int64).reshape(-1, H)):
                if t not in tpos:
                    tpos[t] = len(lname)
                    lname.append(t)
                    lens.append(list(r))
    sname, spos = [], {}
    for m in ms:
        for s in m.sname:
            if s not in spos:
                spos[s] = len(sname)
                sname.append(s)
    ec_id, keys, counts = {}, [], {}
    for m in ms:
        ecs = []
        for e in range(m.num_reads):
            a, b = int(m.indptrA[e]), int(m.indptrA[e + 1])
            cols = [int(c) if same_targets else tpos[m.lname[int(c)]] for c in m.indicesA[a:b]]
            key = tuple(sorted(zip(cols, (int(d) for d in m.dataA[a:b]))))
            if key not in ec_id:
                ec_id[key] = len(keys)
                keys.append(key)
            ecs.append(ec_id[key])
        for s in range(m.num_samples):
            os_ = spos[m.sname[s]]
            for q in range(int(m.indptrN[s]), int(m.indptrN[s + 1])):
                k = (os_, ecs[int(m.indicesN[q])])
                counts[k] = counts.get(k, 0) + int(m.dataN[q])
    indptrA = np.cumsum([0] + [len(k) for k in keys])
    indicesA = [c for k in keys for c, _ in k]
    dataA = [d for k in keys for _, d in k]
    nz = sorted(k for k, v in counts.items() if v != 0)
    indptrN = np.searchsorted(np.array([s for s, _ in nz], dtype=np.int64), np.arange(len(sname) + 1))
    return bin_utils.ECMatrices(m0.hname, lname, np.array(lens, dtype=np.int64).reshape(len(lname), H), sname, indptrA, indicesA, dataA,
                                indptrN, [e for _, e in nz], [counts[k] for k in nz])


def merge_bytes(ms):
    return bin_utils.ecsave2_bytes(merge(ms))


def random_bin(rng, n_ecs, lname, hname, sname, max_row=1300, long_share=0.02, dup_share=0.2, empty_share=0.05, zero_share=0.1):
    """A random ``ECMatrices``: rows of every length (a share up to ``max_row`` pairs), empty rows, repeated rows, several samples, and
    rows that no sample counts."""
    T, H = len(lname), len(hname)
    lens = np.where(rng.random(n_ecs) < long_share, rng.integers(0, min(max_row, T) + 1, n_ecs), rng.integers(1, min(8, T) + 1, n_ecs))
    lens[rng.random(n_ecs) < empty_share] = 0
    rows = []
    for e in range(n_ecs):
        if rows and rng.random() < dup_share:
            rows.append(rows[int(rng.integers(0, len(rows)))])
            continue
        cols = np.sort(rng.choice(T, size=int(lens[e]), replace=False))
        rows.append((cols, rng.integers(1, 1 << H, size=len(cols))))
    indptrA = np.cumsum([0] + [len(r[0]) for r in rows])
    indicesA = np.concatenate([r[0] for r in rows] + [np.zeros(0, np.int64)])
    dataA = np.concatenate([r[1] for r in rows] + [np.zeros(0, np.int64)])
    ip, ix, dx = [0], [], []
    for _ in sname:
        cnt = rng.integers(0, 50, size=n_ecs)
        cnt[rng.random(n_ecs) < zero_share] = 0
        rows_n = np.flatnonzero(cnt)
        ix.append(rows_n)
        dx.append(cnt[rows_n])
        ip.append(ip[-1] + len(rows_n))
    lengths = rng.integers(100, 5000, size=(T, H))
    return bin_utils.ECMatrices(hname, lname, lengths, sname, indptrA, indicesA, dataA, ip,
                                np.concatenate(ix + [np.zeros(0, np.int64)]), np.concatenate(dx + [np.zeros(0, np.int64)]))


def permute_targets(m, rng):
    """The same ECs under a shuffled target list (columns renumbered, each row re-sorted)."""
    perm = rng.permutation(m.num_loci)                     # new position of old column c: perm[c]
    lname = [None] * m.num_loci
    lengths = np.zeros_like(np.asarray(m.lengths))
    for c, p in enumerate(perm):
        lname[p] = m.lname[c]
        lengths[p] = m.lengths[c]
    ix, dx = np.array(m.indicesA, dtype=np.int64).copy(), np.array(m.dataA, dtype=np.int64).copy()
    for e in range(m.num_reads):
        a, b = int(m.indptrA[e]), int(m.indptrA[e + 1])
        c = perm[m.indicesA[a:b]]
        o = np.argsort(c)
        ix[a:b], dx[a:b] = c[o], m.dataA[a:b][o]
    return bin_utils.ECMatrices(m.hname, lname, lengths, m.sname, m.indptrA, ix, dx, m.indptrN, m.indicesN, m.dataN)
